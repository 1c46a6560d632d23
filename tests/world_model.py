"""A model of what include/och_gpu.h promises for a resident world (och_world_*), a generator of
random operation lists over it, and the driver that walks an implementation through such a list and
compares every answer with the model, bit for bit.

A helper module, not a test file: tests/test_world_walk_host.py walks a stand-in made of the host
paths (and asserts the quotas that keep the walks from being vacuous), tests/test_gpu_world_walk.py
walks ort.World.

The model is written from the header, not from the kernels:
  cells        {(x, y, z): id}; a stroke applies in order, last wins, id 0 removes, out of range ignored.
  box          exact at create; grown by the box of a stroke's surviving (last-wins) in-range records
               with id != 0; restored by a checkout; made exact by tighten; left alone by a compaction.
  snapshots    handle -> (cells, box); handles 1, 2, ... never reused.
  strokes      +1 per stroke of n > 0 records (also when all are out of range), +0 for n = 0 or a refusal.
  generation   +1 per compaction.
  held / used  the (height, content) of every node the store holds in this generation, through a
               Python hash-cons; used = 1 + len(held).  At create: what the root reaches.  After an
               admitted stroke: plus, for every unique in-range key k and height h, the non-empty node
               of the new tree at k >> 3 (h + 1).  After a compaction: what the current root and every
               live snapshot's root reach.
  capacity     a stroke is refused, everything unchanged, exactly when used + the sum over h = 1..depth
               of |{k >> 3 h}| over its unique in-range keys > capacity.
  pools        the cells and box at a pool's last flush (at make_pool: the world's then).
  fill_box     ("world: regions") every voxel of the clipped box becomes id.  Counts are closed forms of
               the clipped box in Python integers: per axis and height the aligned intervals that meet it
               and the ones inside it; cells[H] = prod meeting - prod inside, cubes[h] = inside(h) -
               8 inside(h + 1).  Nothing inside the tree: strokes + 1, stats all 0.  A height with cubes +
               cells >= 2^31: INVALID.  used + sum cells + T > capacity (T = the greatest height with a
               cube for id != 0, else 0): REFUSED.  Otherwise held gains the non-empty node of the new
               tree at every straddling cell and, for id != 0, the uniform subtrees of heights 1..T; the
               box grows by the clipped box for id != 0.
  restore_box  inside the clipped box the snapshot's content.  The two trees are walked from the root;
               front = the straddling cells visited whose two nodes differ, cubes = the inside children
               whose two words differ, cells = the visited cells with such a cube beneath them.  Handle
               0, equal roots, a box outside the tree, or no differing cube: strokes + 1 and nothing
               else, whatever the capacity.  Otherwise REFUSED when used + front > capacity; else held
               gains the new non-empty nodes at the `cells` cells and the box grows by the clipped box
               inside the snapshot's box.  The whole tree: the snapshot's root, cubes = 1, no id.

The generator consults only the model, so a seed gives the same operation list on every backend.
"""
import collections
import itertools
import types

import numpy as np

from test_pool_diff_host import expected_pairs, morton_keys, truth_of_lists
from test_pool_read_host import scatter
from test_voxel_builder import ODD_IDS, ORIGIN, check_pool, corner_records, expected_pool

SKY = 0xFFFEBF00
NOTHING = {"n": 0, "pairs": 0, "box_lo": (0, 0, 0), "box_hi": (0, 0, 0)}
REFUSED = "refused"
INVALID = "invalid"
REGION_LIMIT = 1 << 31            # a height of a box stroke holds fewer cubes + cells than this
FILL_VOXELS = 1 << 15             # the generator's fills with id != 0 stay at or below this many voxels
NO_REGION = {"cubes": 0, "cells": 0, "new_ids": 0, "lo": (0, 0, 0), "hi": (0, 0, 0)}
DIFF_FIRST_SIZE = 1024            # the diff buffers' first size, in pairs of one level


def exact_box(cells):
    if not cells:
        return None
    c = np.array(list(cells), np.int64)
    return tuple(int(v) for v in c.min(0)), tuple(int(v) + 1 for v in c.max(0))


def box_union(a, b):
    if a is None or b is None:
        return a or b
    return tuple(min(p, q) for p, q in zip(a[0], b[0])), tuple(max(p, q) for p, q in zip(a[1], b[1]))


def clip_box(lo, hi, depth):
    """The box clipped to the tree as ((x, y, z), (x, y, z)) of Python integers, None where nothing is left."""
    lo = tuple(max(int(v), 0) for v in lo)
    hi = tuple(min(int(v), 1 << depth) for v in hi)
    return (lo, hi) if all(l < h for l, h in zip(lo, hi)) else None


def box_counts(box, depth):
    """(cubes per height, cells per height, the greatest height with a cube) of a clipped box, from closed
    forms: per axis at height h, the aligned intervals of length 2^h that meet [lo, hi) and the ones inside it."""
    inside, cells = [], []
    for h in range(depth + 1):
        meet = ins = 1
        for l, u in zip(*box):
            meet *= ((u - 1) >> h) - (l >> h) + 1
            ins *= max(0, (u >> h) - ((l + (1 << h) - 1) >> h))
        inside.append(ins)
        cells.append(meet - ins)
    inside.append(0)
    cubes = [inside[h] - 8 * inside[h + 1] for h in range(depth + 1)]
    return cubes, cells, max(h for h in range(depth + 1) if cubes[h])


def in_box(c, box):
    return all(l <= v < u for v, l, u in zip(c, *box))


def box_inside(a, b):
    """Box a (or None: no voxels) lies inside box b."""
    return a is None or (b is not None and all(p >= q for p, q in zip(a[0], b[0])) and all(p <= q for p, q in zip(a[1], b[1])))


def box_meet(a, b):
    if a is None or b is None:
        return None
    lo, hi = tuple(max(p, q) for p, q in zip(a[0], b[0])), tuple(min(p, q) for p, q in zip(a[1], b[1]))
    return (lo, hi) if all(l < h for l, h in zip(lo, hi)) else None


def coords_of(keys, levels):
    """Morton keys (x bit 0, y bit 1, z bit 2 per level) of `levels` levels as an (n, 3) int64 array."""
    k = np.asarray(keys, np.int64).reshape(-1)
    out = np.zeros((len(k), 3), np.int64)
    for i in range(levels):
        for a in range(3):
            out[:, a] |= ((k >> (3 * i + a)) & 1) << i
    return out


def records_of(cells):
    return np.array([(x, y, z, v) for (x, y, z), v in cells.items()], np.int64).reshape(-1, 4)


def in_range(records, depth):
    c = np.asarray(records, np.int64).reshape(-1, 4)[:, :3]
    return ((c >= 0) & (c < 1 << depth)).all(1)


class State:
    """A content: cells, its hash-consed tree (per height {position: node}, root) and a loose box."""

    def __init__(self, cells, levels, root, box):
        self.cells, self.levels, self.root, self.box = cells, levels, root, box

    def nodes(self):
        return {v for level in self.levels for v in level.values()}


class Model:
    def __init__(self, depth, base_records, capacity=None):
        self.depth, self.cons, self.rows = depth, {}, {0: (0,) * 8}
        cells = self._apply({}, base_records)
        self.now = self._state(cells, exact_box(cells))
        self.held = self.now.nodes()
        self.capacity = capacity if capacity is not None else 2 * len(self.held) + 64 * depth
        self.snapshots, self.next_snapshot = {}, 1
        self.strokes = self.generation = 0
        self.version = 0              # +1 whenever the current content may have changed

    # -- the tree
    def _apply(self, cells, records):
        cells, dim = dict(cells), 1 << self.depth
        for x, y, z, v in np.asarray(records, np.int64).reshape(-1, 4).tolist():
            if 0 <= x < dim and 0 <= y < dim and 0 <= z < dim:
                if v:
                    cells[(x, y, z)] = v
                else:
                    cells.pop((x, y, z), None)
        return cells

    def _keys(self, coords):
        c = np.asarray(coords, np.int64).reshape(-1, 3)
        return morton_keys(c[:, 0], c[:, 1], c[:, 2], self.depth)

    def _intern(self, h, row):
        node = self.cons.setdefault((h, row), len(self.cons) + 1)
        self.rows[node] = row
        return node

    def _state(self, cells, box):
        cur = dict(zip(self._keys(list(cells)).tolist(), cells.values()))
        levels = []
        for h in range(self.depth):
            rows = {}
            for key, w in cur.items():
                rows.setdefault(key >> 3, [0] * 8)[key & 7] = w
            cur = {pk: self._intern(h, tuple(row)) for pk, row in rows.items()}
            levels.append(cur)
        return State(cells, levels, cur.get(0, 0), box)

    # -- what info() must say
    @property
    def used(self):
        return 1 + len(self.held)

    @property
    def cells(self):
        return self.now.cells

    def info(self):
        lo, hi = self.now.box or ((0, 0, 0), (0, 0, 0))
        return {"capacity": self.capacity, "used": self.used, "strokes": self.strokes, "generation": self.generation,
                "depth": self.depth, "box_lo": lo, "box_hi": hi}

    # -- strokes
    def stroke_keys(self, records):
        rec = np.asarray(records, np.int64).reshape(-1, 4)
        rec = rec[in_range(rec, self.depth)]
        return np.unique(self._keys(rec[:, :3]))

    def stroke_need(self, records):
        keys = self.stroke_keys(records)
        return sum(len(np.unique(keys >> np.uint64(3 * h))) for h in range(1, self.depth + 1)) if len(keys) else 0

    def edit(self, records):
        """None for n = 0, REFUSED, or "outside" / "stroke"."""
        rec = np.asarray(records, np.int64).reshape(-1, 4)
        if not len(rec):
            return None
        keys = self.stroke_keys(rec)
        if not len(keys):
            self.strokes += 1
            return "outside"
        if self.used + self.stroke_need(rec) > self.capacity:
            return REFUSED
        last, dim = {}, 1 << self.depth
        for x, y, z, v in rec.tolist():
            if 0 <= x < dim and 0 <= y < dim and 0 <= z < dim:
                last[(x, y, z)] = v
        grown = exact_box({c: v for c, v in last.items() if v})      # the surviving records with id != 0
        self.now = self._state(self._apply(self.now.cells, rec), box_union(self.now.box, grown))
        for h, level in enumerate(self.now.levels):
            for pk in np.unique(keys >> np.uint64(3 * (h + 1))).tolist():
                if pk in level:
                    self.held.add(level[pk])
        self.strokes += 1
        self.version += 1
        return "stroke"

    # -- box strokes
    def _straddling(self, state, box):
        """The non-empty nodes of `state` at the cells that straddle the box, found by classifying the
        positions of its sparse levels."""
        out = set()
        lo, hi = np.array(box[0], np.int64), np.array(box[1], np.int64)
        for h, level in enumerate(state.levels):
            if not level:
                continue
            keys = list(level)
            c = coords_of(keys, self.depth - h - 1) << (h + 1)
            e = c + (1 << (h + 1))
            meets = ((c < hi) & (e > lo)).all(1)
            inside = ((c >= lo) & (e <= hi)).all(1)
            out.update(level[keys[i]] for i in np.nonzero(meets & ~inside)[0].tolist())
        return out

    def fill_plan(self, lo, hi, id):
        """(clipped box or None, cubes, cells, T, need, INVALID / REFUSED / None) of a fill, nothing changed."""
        box = clip_box(lo, hi, self.depth)
        if box is None:
            return None, [], [], 0, 0, None
        cubes, cells, top = box_counts(box, self.depth)
        T = top if id else 0
        need = sum(cells) + T
        what = None
        if any(a + b >= REGION_LIMIT for a, b in zip(cubes, cells)):
            what = INVALID
        elif self.used + need > self.capacity:
            what = REFUSED
        return box, cubes, cells, T, need, what

    def fill_box(self, lo, hi, id):
        """("outside" / INVALID / REFUSED / "fill", the stats or None)."""
        box, cubes, cells, T, need, what = self.fill_plan(lo, hi, id)
        if box is None:
            self.strokes += 1
            return "outside", dict(NO_REGION)
        if what:
            return what, None
        new = {c: v for c, v in self.now.cells.items() if not in_box(c, box)}
        if id:
            assert np.prod([u - l for l, u in zip(*box)], dtype=object) <= 2 * FILL_VOXELS, box
            (x0, y0, z0), (x1, y1, z1) = box
            new.update(((x, y, z), id) for x in range(x0, x1) for y in range(y0, y1) for z in range(z0, z1))
        self.now = self._state(new, box_union(self.now.box, box) if id else self.now.box)
        before = len(self.held)
        self.held |= self._straddling(self.now, box)
        uniform = id
        for h in range(T):
            uniform = self._intern(h, (uniform,) * 8)
            self.held.add(uniform)
        self.strokes += 1
        self.version += 1
        return "fill", {"cubes": sum(cubes), "cells": sum(cells), "new_ids": len(self.held) - before, "lo": box[0], "hi": box[1]}

    def restore_plan(self, s, box):
        """(front, cubes, the cells with a differing cube beneath them as (height, key)) of the walk of the
        current tree and snapshot s's from the root, for a clipped box that is not the whole tree."""
        lo, hi = box
        rows_of, count, cells = self.rows, [0, 0], []

        def visit(H, key, o, na, nb):
            count[0] += 1
            ra, rb, half, found = rows_of[na], rows_of[nb], 1 << (H - 1), False
            for k in range(8):
                if ra[k] == rb[k]:
                    continue
                c = (o[0] + (k & 1) * half, o[1] + ((k >> 1) & 1) * half, o[2] + ((k >> 2) & 1) * half)
                if any(c[a] >= hi[a] or c[a] + half <= lo[a] for a in range(3)):
                    continue
                if all(lo[a] <= c[a] and c[a] + half <= hi[a] for a in range(3)):
                    count[1] += 1
                    found = True
                elif visit(H - 1, key << 3 | k, c, ra[k], rb[k]):
                    found = True
            if found:
                cells.append((H, key))
            return found

        visit(self.depth, 0, (0, 0, 0), self.now.root, self.state(s).root)
        return count[0], count[1], cells

    def restore_box(self, s, lo, hi):
        """("nothing" / "whole" / "no_effect" / REFUSED / "restore", the stats or None)."""
        snap, box = self.state(s), clip_box(lo, hi, self.depth)
        st = dict(NO_REGION) if box is None else dict(NO_REGION, lo=box[0], hi=box[1])
        if box is None or snap.root == self.now.root:
            self.strokes += 1
            return "nothing", st
        grown = box_union(self.now.box, box_meet(box, snap.box))
        if box == ((0, 0, 0), (1 << self.depth,) * 3):
            self.now = State(snap.cells, snap.levels, snap.root, grown)
            self.strokes += 1
            self.version += 1
            return "whole", dict(st, cubes=1)
        front, cubes, cells = self.restore_plan(s, box)
        if not cubes:                  # the two states differ outside the box only: no id, no refusal, the box stays
            self.strokes += 1
            return "no_effect", st
        if self.used + front > self.capacity:
            return REFUSED, None
        new = {c: v for c, v in self.now.cells.items() if not in_box(c, box)}
        new.update((c, v) for c, v in snap.cells.items() if in_box(c, box))
        self.now = self._state(new, grown)
        before = len(self.held)
        for H, key in cells:
            node = self.now.levels[H - 1].get(key)
            if node:
                self.held.add(node)
        self.strokes += 1
        self.version += 1
        return "restore", dict(st, cubes=cubes, cells=len(cells), new_ids=len(self.held) - before)

    # -- history
    def snapshot(self):
        s = self.next_snapshot
        self.next_snapshot += 1
        self.snapshots[s] = (self.now, self.generation)
        return s

    def state(self, s):
        return self.now if s == 0 else self.snapshots[s][0]

    def checkout(self, s):
        if s:
            self.now = self.snapshots[s][0]
            self.version += 1

    def release(self, s):
        del self.snapshots[s]

    def compact(self):
        self.held = self.now.nodes().union(*(st.nodes() for st, _ in self.snapshots.values()))
        self.generation += 1

    def tighten(self):
        self.now = State(self.now.cells, self.now.levels, self.now.root, exact_box(self.now.cells))
        return self.now.box or ((0, 0, 0), (0, 0, 0))

    def diff(self, a, b):
        """(records, stats with pairs) of the voxels that differ between states a and b, ids under b."""
        ca, cb = self.state(a).cells, self.state(b).cells
        coords = [c for c in set(ca) | set(cb) if ca.get(c, 0) != cb.get(c, 0)]
        rec, st, keys = truth_of_lists(self.depth, np.array(coords, np.int64).reshape(-1, 3), [cb.get(c, 0) for c in coords])
        st = dict(st, pairs=expected_pairs(keys, self.depth) if len(keys) else 0)
        return rec, st, (len(np.unique(keys >> np.uint64(3))) if len(keys) else 0)


# ------------------------------------------------------------ the generator

class Generator:
    """next() gives one operation, a dict with "op" and its arguments, from the model's state and the
    seed alone.  `pending` holds what must follow directly (a retry after a compaction, the stroke
    after a checkout): that is how the quotas of tests/test_world_walk_host.py are met on purpose."""

    def __init__(self, model, seed, big=False):
        self.m, self.rng, self.big = model, np.random.default_rng(seed), big
        self.pending = collections.deque()
        self.step = 0
        self.pools = 0
        self.deep = model.depth > 8
        self.dim = 1 << model.depth
        self.script = ([(8, "big"), (15, "u8"), (20, "set_remove"), (40, "big")] if big else
                       [(15, "u8"), (20, "set_remove"), (25, "empty"), (35, "checkout_compact"), (50, "empty_now"),
                        (62, "checkout_compact")])
        # the box strokes' sequences: the capacity ones in every walk, of the others every second one
        regions = ["r_checkout", "r_whole", "r_across", "r_empty", "r_untouched", "r_uniform", "r_outside", "r_checkout"]
        regions = [name for i, name in enumerate(regions) if (i + seed) % 2 == 0]
        regions += ["r_pin_fill", "r_pin_restore", "r_refuse_fill", "r_refuse_restore"]
        self.script += [(self.script[-1][0] + 3 + 5 * i, name) for i, name in enumerate(regions)]

    # -- coordinates and strokes
    def coords(self, n):
        if self.deep:
            corners = corner_records(self.m.depth)[:, :3].astype(np.int64)
            return corners[self.rng.integers(0, len(corners), n)] + self.rng.integers(-5, 6, (n, 3))
        return self.rng.integers(0, self.dim, (n, 3))

    def ids(self, n, odd=0.1):
        ids = self.rng.integers(1, 6, n).astype(np.int64)
        pick = self.rng.random(n) < odd
        ids[pick] = np.array(ODD_IDS + [255, 256, 300], np.int64)[self.rng.integers(0, len(ODD_IDS) + 3, int(pick.sum()))]
        return ids

    def box(self, side):
        size = self.rng.integers(1, side + 1, 3)
        if self.deep:
            lo = self.coords(1)[0]
        else:
            lo = self.rng.integers(-1, max(self.dim - 1, 1), 3)
        return lo, lo + size

    @staticmethod
    def box_list(lo, hi, id):
        z, y, x = np.mgrid[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        return np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(x.size, id, np.int64)], 1).astype(np.int64)

    def stroke(self, kind=None):
        m, rng = self.m, self.rng
        side = 2 if m.depth == 1 else min(8, self.dim)
        kinds = ["scatter"] * 5 + ["fill"] * 3 + ["cut"] * 2 + ["rewrite", "empty_list", "outside", "set_remove", "dups"]
        kind = kind or kinds[rng.integers(0, len(kinds))]
        if kind in ("rewrite", "remove_all") and not m.cells:
            kind = "scatter"
        outside = self.outside_the_box() if kind == "set_remove" else None
        if kind == "set_remove" and outside is None:
            kind = "scatter"
        if kind == "scatter":
            n = min(1 + int(rng.exponential(12)), 120, 2 * self.dim ** 2)
            rec = np.concatenate([self.coords(n), self.ids(n)[:, None]], 1)
            rec[rng.random(n) < 0.15, 3] = 0
            out = rng.random(n) < 0.05
            rec[out, rng.integers(0, 3)] = np.array([-1, self.dim, 1 << 40])[rng.integers(0, 3)]
        elif kind == "dups":
            n = int(rng.integers(2, 40))
            c = self.coords(max(1, n // 4))
            rec = np.concatenate([c[rng.integers(0, len(c), n)], self.ids(n)[:, None]], 1)
            rec[rng.random(n) < 0.3, 3] = 0
        elif kind in ("fill", "cut"):
            lo, hi = self.box(side)
            rec = self.box_list(lo, hi, 0 if kind == "cut" else int(self.ids(1, odd=0.2)[0]))
        elif kind == "rewrite":
            keys = list(m.cells)
            pick = rng.permutation(len(keys))[:max(1, len(keys) // 3)]
            rec = np.array([keys[i] + (m.cells[keys[i]],) for i in pick], np.int64)
        elif kind == "remove_all":
            rec = records_of(m.cells) * np.array([1, 1, 1, 0], np.int64)
        elif kind == "empty_list":
            rec = np.zeros((0, 4), np.int64)
        elif kind == "outside":
            n = int(rng.integers(1, 20))
            rec = np.concatenate([self.coords(n), self.ids(n)[:, None]], 1)
            rec[:, rng.integers(0, 3)] = np.array([-1, self.dim, 1 << 33])[rng.integers(0, 3, n)]
        elif kind == "set_remove":
            # the two readings of "records with id != 0" differ: a coordinate outside the box, set then removed
            # between them up to three present voxels get new ids: inside the box, so only c could grow it
            keys = list(m.cells)
            keep = np.array([keys[i] for i in rng.permutation(len(keys))[:3]], np.int64).reshape(-1, 3)
            rec = np.concatenate([np.concatenate([[outside], keep, [outside]]),
                                  np.array([7] + [1, 2, 3][:len(keep)] + [0], np.int64)[:, None]], 1)
        elif kind == "small_new":
            # a few voxels with an id nothing else uses: the content does change
            rec = np.concatenate([rng.integers(0, self.dim, (5, 3)), np.full((5, 1), 1000 + self.step, np.int64)], 1)
        elif kind == "big_fill":
            lo = rng.integers(0, self.dim - 26, 3)
            rec = self.box_list(lo, lo + rng.integers(23, 27, 3), int(rng.integers(1, 6)))
        elif kind == "big_cut":
            lo, hi = m.now.box
            rec = self.box_list(np.array(lo), np.array(hi), 0)
        return {"op": "edit", "records": rec.astype(np.int64).reshape(-1, 4), "device": bool(rng.random() < 0.45), "kind": kind}

    def outside_the_box(self):
        """A coordinate inside the tree and outside the current box; None where the box is the whole tree."""
        box = self.m.now.box
        for _ in range(50):
            c = np.clip(self.coords(1)[0], 0, self.dim - 1)
            if box is None or not all(box[0][a] <= c[a] < box[1][a] for a in range(3)):
                return c
        for c in ((0, 0, 0), (self.dim - 1,) * 3):
            if not all(box[0][a] <= c[a] < box[1][a] for a in range(3)):
                return np.array(c, np.int64)
        return None

    # -- box strokes
    def some_cell(self, states=None):
        """A coordinate: mostly a voxel of the current state or of a snapshot, else anywhere."""
        states = [self.m.now] + [st for st, _ in self.m.snapshots.values()] if states is None else states
        states = [st for st in states if st.cells]
        if states and self.rng.random() < 0.85:
            cells = states[self.rng.integers(0, len(states))].cells
            return np.array(next(itertools.islice(cells, int(self.rng.integers(0, min(len(cells), 64))), None)), np.int64)
        return np.clip(self.coords(1)[0], 0, self.dim - 1)

    def aligned_box(self, centre, kmax, side_max):
        """A box near `centre` whose faces are multiples of 2^k plus or minus a few voxels, k in 0..kmax,
        of side at most about side_max.  Gives (lo, hi, k)."""
        rng = self.rng
        k = int(rng.integers(0, kmax + 1))
        while k and (1 << k) > side_max:
            k -= 1
        most = max(1, min(3, side_max >> k))
        size = rng.integers(1, most + 1, 3) << k
        lo = ((np.asarray(centre, np.int64) >> k) - rng.integers(0, most, 3)) << k
        hi = lo + size
        jitter = lambda: np.where(rng.random(3) < 0.6, 0, rng.integers(-2, 4, 3))
        lo, hi = lo + jitter(), hi + jitter()
        return lo, np.maximum(hi, lo + 1), k

    def region_box(self, fill, centre=None, kinds=True):
        """(lo, hi) for a box stroke: fill = True keeps the clipped box at or below FILL_VOXELS voxels."""
        rng, m = self.rng, self.m
        kind = ["aligned"] * 12 + ["overhang", "empty", "outside", "whole"]
        kind = kind[rng.integers(0, len(kind))] if kinds and centre is None else "aligned"
        if kind == "whole" and (not fill or m.depth <= 5):
            return (0, 0, 0), (self.dim,) * 3
        if kind == "outside":
            return (self.dim, 0, -4), (self.dim + 4, 4, 0)
        side_max = 16 if fill else max(self.dim >> 1, 1)
        for _ in range(20):
            lo, hi, _k = self.aligned_box(self.some_cell() if centre is None else centre, m.depth, side_max)
            if kind == "overhang":
                a = rng.integers(0, 3)
                lo[a], hi[a] = (-3, max(hi[a] - lo[a], 1)) if rng.random() < 0.5 else (self.dim - max(hi[a] - lo[a], 1), self.dim + 5)
            if kind == "empty":
                a = rng.integers(0, 3)
                hi[a] = lo[a] - rng.integers(0, 2)
                break
            box = clip_box(lo, hi, m.depth)
            if box is None or not fill or int(np.prod([u - l for l, u in zip(*box)], dtype=object)) <= FILL_VOXELS:
                break
            side_max = max(side_max >> 1, 1)
        return tuple(int(v) for v in lo), tuple(int(v) for v in hi)

    def fill_box_op(self, id=None, centre=None, over=0.15):
        """Budget-aware: mostly a box that the capacity admits, some on purpose over it."""
        m, rng = self.m, self.rng
        if id is None:
            id = 0 if rng.random() < 0.5 else int(self.ids(1, odd=0.2)[0])
        want_over = rng.random() < over
        for _ in range(12):
            lo, hi = self.region_box(bool(id), centre)
            what = m.fill_plan(lo, hi, id)[5]
            if what is None or (what == REFUSED and want_over) or (what == INVALID and rng.random() < 0.1):
                break
        else:
            c = self.some_cell() if centre is None else np.asarray(centre, np.int64)
            lo, hi = tuple(int(v) for v in c), tuple(int(v) + 1 for v in c)
        return {"op": "fill_box", "lo": lo, "hi": hi, "id": id}

    def restore_box_op(self, s=None, centre=None):
        if s is None:
            s = self.handle(zero=0.05, other_than=0)
        lo, hi = self.region_box(False, centre)
        return {"op": "restore_box", "s": s, "lo": lo, "hi": hi}

    def box_with_need(self, need_of, accept, centres, tries=400):
        """A box for which accept(need_of(lo, hi)) holds, or None: the scripted refusals and pinned bounds."""
        for _ in range(tries):
            lo, hi, _k = self.aligned_box(centres[self.rng.integers(0, len(centres))], self.m.depth, max(self.dim >> 1, 1))
            lo, hi = tuple(int(v) for v in lo), tuple(int(v) for v in hi)
            need = need_of(lo, hi)
            if need is not None and accept(need):
                return lo, hi
        return None

    def clear_need(self, lo, hi):
        box, _, _, _, need, what = self.m.fill_plan(lo, hi, 0)
        whole = box == ((0, 0, 0), (self.dim,) * 3)
        return None if box is None or whole or what == INVALID else need

    def restore_need(self, s):
        def need(lo, hi):
            box = clip_box(lo, hi, self.m.depth)
            if box is None or box == ((0, 0, 0), (self.dim,) * 3) or self.m.state(s).root == self.m.now.root:
                return None
            front, cubes, _ = self.m.restore_plan(s, box)
            return front if cubes else None
        return need

    def centres(self, state=None):
        cells = list((state or self.m.now).cells)
        return [np.array(c, np.int64) for c in cells[:200]] or [np.array((0, 0, 0), np.int64)]

    def used_after_compaction(self):
        m = self.m
        return 1 + len(m.now.nodes().union(*(st.nodes() for st, _ in m.snapshots.values())))

    def pin_ops(self, kind):
        """Two strokes that pin the capacity bound from both sides: used + need == capacity + 1, refused, then
        used + need == capacity, admitted.  kind "fill" (a clear) or "restore" (from the newest snapshot)."""
        m = self.m
        free = m.capacity - m.used
        if kind == "fill":
            need_of, centres, make = self.clear_need, self.centres(), lambda b: {"op": "fill_box", "lo": b[0], "hi": b[1], "id": 0}
        else:
            if not m.snapshots:
                return []
            s = max(m.snapshots)
            need_of, centres = self.restore_need(s), self.centres(m.state(s))
            make = lambda b: {"op": "restore_box", "s": s, "lo": b[0], "hi": b[1]}
        over = self.box_with_need(need_of, lambda n: n == free + 1, centres)
        exact = self.box_with_need(need_of, lambda n: n == free, centres)
        return [dict(make(b), pin=True) for b in (over, exact) if b is not None]

    def refuse_ops(self, kind):
        """A stroke that the capacity refuses now and admits after a compaction, if the store holds enough
        abandoned rows for one; the generator's compact-and-retry does the rest."""
        m = self.m
        free, free_then = m.capacity - m.used, m.capacity - self.used_after_compaction()
        if kind == "fill":
            need_of, centres, make = self.clear_need, self.centres(), lambda b: {"op": "fill_box", "lo": b[0], "hi": b[1], "id": 0}
        else:
            if not m.snapshots:
                return []
            s = max(m.snapshots)
            need_of, centres = self.restore_need(s), self.centres(m.state(s))
            make = lambda b: {"op": "restore_box", "s": s, "lo": b[0], "hi": b[1]}
        box = self.box_with_need(need_of, lambda n: free < n <= free_then, centres) if free_then > free else None
        return [make(box)] if box is not None else []

    # -- the other operations
    def handle(self, zero=0.2, other_than=None):
        """A live handle or 0 (the current state); other_than = a handle: mostly a state with another root
        than that one's, since a checkout of, or a diff against, equal content is answered on the host."""
        live = sorted(self.m.snapshots)
        if other_than is not None and self.rng.random() < 0.8:
            differing = [s for s in [0] + live if self.m.state(s).root != self.m.state(other_than).root]
            if differing:
                return differing[self.rng.integers(0, len(differing))]
        if not live or self.rng.random() < zero:
            return 0
        return live[self.rng.integers(0, len(live))]

    def diff_op(self, a=None, b=None):
        a = self.handle() if a is None else a
        b = self.handle(other_than=a) if b is None else b
        form = ["host", "device", "device", "summary"][self.rng.integers(0, 4)]
        return {"op": "diff", "a": a, "b": b, "form": form}

    def read_box_op(self):
        rng, m = self.rng, self.m
        kind = ["inside", "overhang", "empty", "inside", "overhang"][rng.integers(0, 5)]
        if self.deep or m.depth > 5:
            centre = np.array(list(m.cells)[rng.integers(0, len(m.cells))] if m.cells else self.coords(1)[0], np.int64)
            lo, hi = centre - rng.integers(0, 6, 3), centre + rng.integers(1, 7, 3)
            if kind == "overhang":
                corner = np.array([0, self.dim][rng.integers(0, 2)])
                lo, hi = corner - rng.integers(1, 5, 3), corner + rng.integers(1, 5, 3)
            elif kind == "inside":
                lo, hi = np.clip(lo, 0, self.dim), np.clip(hi, 0, self.dim)
        elif kind == "overhang":
            lo, hi = -rng.integers(1, 4, 3), self.dim + rng.integers(1, 4, 3)
        else:
            lo = rng.integers(0, self.dim, 3)
            hi = np.minimum(lo + rng.integers(1, self.dim + 1, 3), self.dim)
        if kind == "empty":
            hi, a = hi.copy(), rng.integers(0, 3)
            hi[a] = lo[a]
        hi = np.maximum(hi, lo)
        return {"op": "read_box", "lo": tuple(int(v) for v in lo), "hi": tuple(int(v) for v in hi), "kind": kind,
                "dtype": [np.uint8, np.uint32][rng.integers(0, 2)], "device": bool(rng.random() < 0.45)}

    # -- sequences that the quotas of tests/test_world_walk_host.py need, each begun at the first free
    # step at or after its own; a method gives the first operation and queues the rest (None: not now)
    def script_big(self):
        # snapshots A, B, C around a small stroke and one of more than 1024 leaf-level parents: the diff of
        # the large one, then the small one right after it in the kept buffers; again after a compaction
        self.pending.extend([self.stroke("small_new"), {"op": "snapshot"}, self.stroke("big_fill"), {"op": "snapshot"},
                             {"op": "big_diff"}, {"op": "small_diff"}, {"op": "compact"}, {"op": "big_diff"},
                             {"op": "small_diff"}, self.stroke("big_cut")])
        return {"op": "snapshot"}

    def script_u8(self):
        # an id that a u8 grid cannot hold, then a u8 read of a box around it
        fill = self.stroke("fill")
        rec = fill["records"]
        rec[:, 3] = 300 + self.step
        lo, hi = rec[:, :3].min(0) - 1, rec[:, :3].max(0) + 2
        self.pending.append({"op": "read_box", "lo": tuple(int(v) for v in lo), "hi": tuple(int(v) for v in hi),
                             "kind": "overhang", "dtype": np.uint8, "device": bool(self.rng.random() < 0.5)})
        return fill

    def script_set_remove(self):
        return self.stroke("set_remove")

    def script_empty(self):
        # everything removed with a snapshot live (a diff with an empty side), then an empty world without one
        self.pending.extend([self.stroke("remove_all"), {"op": "diff_last"}, {"op": "release_all"}, {"op": "compact"},
                             {"op": "tighten"}, self.stroke("scatter"), {"op": "snapshot"}])
        return {"op": "snapshot"}

    def script_empty_now(self):
        # the current state empty, a snapshot's not: a compaction, then back
        self.pending.extend([self.stroke("remove_all"), {"op": "diff_last"}, {"op": "compact"}, {"op": "tighten"},
                             {"op": "checkout_last"}, {"op": "tighten"}])
        return {"op": "snapshot"}

    def script_checkout_compact(self):
        # a checkout that changes the root directly before a compaction: the host's root against the new store's head
        s = self.handle(zero=0.0, other_than=0)
        if self.m.state(s).root == self.m.now.root:
            return None
        self.pending.append({"op": "compact"})
        return {"op": "checkout", "s": s}

    # -- the box strokes' sequences
    def with_pool(self, ops):
        """The operations behind a make_pool where the walk has no pool yet: they flush and check pool 0."""
        if not self.pools:
            self.pools += 1
            ops = [{"op": "make_pool"}] + ops
        self.pending.extend(ops[1:])
        return ops[0]

    def whole(self):
        return {"lo": (0, 0, 0), "hi": (self.dim,) * 3}

    def script_r_checkout(self):
        # a checkout that changes the root, then a box stroke: the head's root word is behind the host's
        s = self.handle(zero=0.0, other_than=0)
        if self.m.state(s).root == self.m.now.root:
            return None
        centre = self.some_cell([self.m.state(s)])
        follow = self.fill_box_op(id=[0, 3][self.step % 2], centre=centre, over=0) if self.rng.random() < 0.7 else \
            self.restore_box_op(s=self.handle(zero=0.0, other_than=s), centre=centre)
        self.pending.append(follow)
        return {"op": "checkout", "s": s}

    def script_r_whole(self):
        # the root changes on the host alone (a whole-tree clear, a whole-tree restore): a record stroke, a
        # flush without new ids, a compaction with the snapshot live and a tighten right after such a change
        clear, back = dict(self.whole(), op="fill_box", id=0), dict(self.whole(), op="restore_box", s="last")
        flush, check = {"op": "flush", "pool": 0}, {"op": "check_pool", "pool": 0}
        return self.with_pool([{"op": "snapshot"}, clear, self.stroke("small_new"), flush, check, back, dict(flush), dict(check),
                               self.stroke("small_new"), dict(back), {"op": "compact"}, {"op": "tighten"}])

    def script_r_across(self):
        # a restore from a snapshot whose ids a compaction has renumbered since
        stroke = self.stroke("small_new")
        c = stroke["records"][0, :3]
        self.pending.extend([stroke, {"op": "compact"},
                             {"op": "restore_box", "s": "last", "lo": tuple(int(v) - 1 for v in c), "hi": tuple(int(v) + 2 for v in c)}])
        return {"op": "snapshot"}

    def script_r_empty(self):
        # an empty current state under a restore from a snapshot with voxels, then the reverse
        if not self.m.cells:
            return None
        lo, hi = self.region_box(False, centre=self.some_cell([self.m.now]))
        self.pending.extend([dict(self.whole(), op="fill_box", id=0), {"op": "snapshot"},
                             {"op": "restore_box", "s": "prev", "lo": lo, "hi": hi}, {"op": "restore_box", "s": "last", "lo": lo, "hi": hi}])
        return {"op": "snapshot"}

    def script_r_untouched(self):
        # the roots differ, and every difference lies outside the box
        stroke = self.stroke("small_new")
        touched = [tuple(c) for c in stroke["records"][:, :3].tolist()]
        for _ in range(40):
            lo, hi = self.region_box(False, kinds=False)
            box = clip_box(lo, hi, self.m.depth)
            if box is not None and box != ((0, 0, 0), (self.dim,) * 3) and not any(in_box(c, box) for c in touched):
                self.pending.extend([stroke, {"op": "restore_box", "s": "last", "lo": lo, "hi": hi}])
                return {"op": "snapshot"}
        return None

    def script_r_uniform(self):
        # a fill whose uniform subtrees the store holds already, and the same fill after a compaction
        if self.m.depth < 2:
            return None
        T = min(2, self.m.depth - 1)
        fills = []
        for c in (self.rng.integers(0, 1 << (self.m.depth - T), (3, 3)) << T).tolist():
            fills.append({"op": "fill_box", "lo": tuple(c), "hi": tuple(v + (1 << T) for v in c), "id": 2000 + self.step})
        self.pending.extend(fills[1:2] + [{"op": "compact"}] + fills[2:])
        return fills[0]

    def script_r_outside(self):
        # a restore that brings voxels back outside the tightened box, then a frame: the pool's cull box
        if not self.m.cells:
            return None
        c = self.some_cell([self.m.now])
        half = self.dim >> 1
        lo = tuple(int(v >= half) * half for v in c)
        lo, hi = (lo[0], 0, 0), (lo[0] + half, self.dim, self.dim)       # the half of the tree, along x, that holds c
        return self.with_pool([{"op": "snapshot"}, {"op": "fill_box", "lo": lo, "hi": hi, "id": 0}, {"op": "tighten"},
                               {"op": "restore_box", "s": "last", "lo": tuple(int(v) - 1 for v in c), "hi": tuple(int(v) + 2 for v in c)},
                               {"op": "flush", "pool": 0}, {"op": "check_pool", "pool": 0}])

    def script_r_pin_fill(self):
        self.pending.append({"op": "pin", "kind": "fill"})
        return {"op": "compact"}

    def script_r_pin_restore(self):
        if not self.m.cells:
            return None
        self.pending.extend([dict(self.whole(), op="fill_box", id=0), {"op": "pin", "kind": "restore"}])
        return {"op": "snapshot"}

    def script_r_refuse_fill(self):
        return {"op": "refuse", "kind": "fill"}

    def script_r_refuse_restore(self):
        self.pending.extend([self.stroke("scatter"), self.stroke("scatter"), {"op": "refuse", "kind": "restore"}])
        return {"op": "snapshot"}

    def next(self):
        self.step += 1
        if self.pending:
            return self.pending.popleft()
        m, rng = self.m, self.rng
        if self.script and self.step >= self.script[0][0]:
            first = getattr(self, "script_" + self.script.pop(0)[1])()
            if first is not None:
                return first
        table = [("edit", 30), ("snapshot", 8), ("checkout", 10), ("release", 3), ("compact", 5), ("tighten", 6),
                 ("make_pool", 3), ("flush", 6), ("check_pool", 5), ("diff", 10), ("at", 3), ("read_box", 6),
                 ("download", 2), ("revert_by_diff", 3), ("fill_box", 8), ("restore_box", 7)]
        names, weights = zip(*table)
        op = names[rng.choice(len(names), p=np.array(weights) / sum(weights))]
        if op == "edit":
            return self.stroke()
        if op == "checkout":
            s = self.handle(zero=0.1, other_than=0)
            follow = rng.integers(0, 5)
            if follow == 4:
                self.pending.append(self.fill_box_op(over=0) if rng.random() < 0.5 else self.restore_box_op())
            elif follow == 0:
                self.pending.append(self.stroke("scatter"))
            elif follow == 1:
                self.pending.append({"op": "compact"})
            elif follow == 2:
                self.pending.append({"op": "tighten"})
            return {"op": "checkout", "s": s}
        if op == "release":
            if not m.snapshots:
                return {"op": "snapshot"}
            return {"op": "release", "s": self.handle(zero=0.0)}
        if op == "make_pool":
            if self.pools >= 2:
                return {"op": "flush", "pool": int(rng.integers(0, self.pools))}
            self.pools += 1
            return {"op": "make_pool"}
        if op in ("flush", "check_pool"):
            if not self.pools:
                self.pools += 1
                return {"op": "make_pool"}
            return {"op": op, "pool": int(rng.integers(0, self.pools))}
        if op == "fill_box":
            return self.fill_box_op()
        if op == "restore_box":
            return self.restore_box_op()
        if op == "diff":
            return self.diff_op()
        if op == "at":
            return {"op": "at", "device": bool(rng.random() < 0.5), "seed": int(rng.integers(0, 1 << 30))}
        if op == "read_box":
            return self.read_box_op()
        if op == "revert_by_diff":
            s = self.handle(zero=0.0)
            if not s or m.used + m.stroke_need(m.diff(0, s)[0].astype(np.int64)) > m.capacity:
                return {"op": "snapshot"}
            return {"op": "revert_by_diff", "s": s}
        return {"op": op}

    def refused(self, op):
        """The header's advice after a refusal: compact and retry (once; the retry may be refused again)."""
        if not op.get("retry") and not op.get("pin"):
            self.pending.appendleft(dict(op, retry=True))
            self.pending.appendleft({"op": "compact"})


# ------------------------------------------------------------ the driver

def to_u32(records):
    """Records of any width as uint32, a coordinate outside uint32 as one outside any tree (World.edit's rule)."""
    wide = np.asarray(records, np.int64).reshape(-1, 4).copy()
    outside = ((wide[:, :3] < 0) | (wide[:, :3] > 0xFFFFFFFF)).any(axis=1)
    wide[outside, :3] = 0xFFFFFFFF
    return wide.astype(np.uint32)


class Walk:
    """One walk of `world` (ort.World or a stand-in with its methods) beside a Model.

    world.has_store  False for a stand-in without a store: `used`, `capacity`, the loose box, refusals
                     and pools are the model's alone there, and a diff's `pairs` is not compared.
    tally            a Counter of what the walk met, from the model alone (the quotas)."""

    def __init__(self, ort, world, model, seed, big=False, O=None, on_gpu=False, tally=None):
        self.ort, self.world, self.m, self.O, self.on_gpu = ort, world, model, O, on_gpu
        self.gen = Generator(model, seed, big)
        self.has_store = getattr(world, "has_store", True)
        self.tally = tally if tally is not None else collections.Counter()
        self.pools = []                # [the pool or None, {"cells", "strokes", "generation"}]
        self.roots = {}                # (generation, model root) <-> the implementation's root
        self.last = None               # the operation before this one
        self.last_diff_parents = None
        self.compacted_since_tighten, self.tightened_at = True, None
        self.trail = []                # the tags of the operations so far: what the sequences' quotas look at
        self.uniform_fills = {}        # (id, T) of a fill's uniform subtrees -> the generation it ran in
        self.seed = seed
        self.check_info()
        self.check_content()

    # -- checks
    def check_info(self):
        info, want = self.world.info(), self.m.info()
        for k, v in want.items():
            if k in info:
                assert info[k] == v, (k, info[k], v, self.last)
        assert (info["root"] == 0) == (not self.m.cells), (info["root"], len(self.m.cells))
        if self.has_store:
            # inside a generation two roots are equal exactly when their contents are
            for key in ((self.m.generation, "model", self.m.now.root), (self.m.generation, "world", info["root"])):
                other = info["root"] if key[1] == "model" else self.m.now.root
                assert self.roots.setdefault(key, other) == other, (key, other, self.last)

    def check_content(self):
        m = self.m
        rec = records_of(m.cells)
        check_pool(self.world.download(), m.depth, rec)
        self.check_at(self.seed, False)

    def check_at(self, seed, device):
        from test_gpu_world_read import expected_ids, probe_coordinates
        coords = probe_coordinates(self.m.depth, self.m.cells, seed)
        want = expected_ids(self.m.cells, coords)
        if device and self.on_gpu:
            import torch
            got = self.world.at(torch.from_numpy(coords.astype(np.int32)).cuda()).cpu().numpy().view(np.uint32)
        else:
            got = self.world.at(coords)
        assert got.dtype == np.uint32 and np.array_equal(got, want)

    def check_diff(self, a, b, form):
        rec, st, parents = self.m.diff(a, b)
        if form == "device" and self.on_gpu:
            got, got_st = self.world.diff(a, b, device=True)
            got = got.cpu().numpy().view(np.uint32)
        elif form == "summary":
            got, got_st = self.world.diff(a, b, records=False)
            assert got is None
        else:
            got, got_st = self.world.diff(a, b)
        if got is not None:
            assert got.shape == rec.shape and got.tobytes() == rec.tobytes(), (a, b, form)
        if not self.has_store:
            got_st = dict(got_st, pairs=st["pairs"])
        assert got_st == st, (got_st, st, a, b, form)
        return rec, st, parents

    # -- one operation
    def run(self, steps):
        try:
            for _ in range(steps):
                op = self.gen.next()
                changed = getattr(self, "do_" + op["op"])(op)
                self.check_info()
                self.trail.append(op.get("tags", ()))
                self.count_sequences()
                if changed:
                    self.check_content()
                self.last = op
        finally:
            for pool, _ in self.pools:
                if pool is not None:
                    pool.close()

    SEQUENCES = {"region_after_checkout": ("checkout_moved", "region"),
                 "seq_whole_clear": ("whole_clear", "stroke", "flush0", "check_pool0"),
                 "seq_whole_restore": ("whole_restore", "flush0", "check_pool0"),
                 "seq_whole_restore_compact": ("whole_restore", "compact_snapshots", "tighten"),
                 "seq_restore_outside_box": ("restore_outside_box", "flush0", "check_pool0")}

    def count_sequences(self):
        for name, tags in self.SEQUENCES.items():
            n = len(tags)
            self.tally[name] += len(self.trail) >= n and all(tag in had for tag, had in zip(tags, self.trail[-n:]))

    def after_checkout(self):
        """The operation before this one was a checkout that changed the root (checkout(0) and a checkout of
        the current content change nothing: the next stroke has no root to upload first)."""
        return self.last is not None and self.last.get("moved", False)

    def do_edit(self, op):
        m, t, rec = self.m, self.tally, op["records"]
        before = m.info()
        what = m.edit(rec)
        t["edit"] += 1
        t["edit_device"] += op["device"]
        if what == REFUSED:
            t["refused"] += 1
            t["refused_again"] += bool(op.get("retry"))
            self.gen.refused(op)
            if self.has_store:
                import pytest
                with pytest.raises(self.ort.OchError, match="CAPACITY") as e:
                    self.world.edit(to_u32(rec))
                assert e.value.status == -6 and m.info() == before
            return True                 # everything unchanged: the content is checked
        if what == "stroke":
            t["admitted"] += 1
            op["tags"] = ("stroke",)
            named = rec[in_range(rec, m.depth) & (rec[:, 3] != 0)]       # the other reading: every record with id != 0
            lo, hi = before["box_lo"], before["box_hi"]
            if (lo, hi) != ((0, 0, 0), (0, 0, 0)) and len(named):
                loose = (tuple(min(p, int(q)) for p, q in zip(lo, named[:, :3].min(0))),
                         tuple(max(p, int(q) + 1) for p, q in zip(hi, named[:, :3].max(0))))
                t["box_readings_differ"] += loose != (m.info()["box_lo"], m.info()["box_hi"])
            t["stroke_after_checkout"] += self.after_checkout()
            t["no_change"] += op["kind"] == "rewrite"
            t["emptying"] += not m.cells
        t["outside"] += what == "outside"
        if op["device"] and self.on_gpu:
            import torch
            self.world.edit(torch.from_numpy(to_u32(rec).view(np.int32)).cuda())
        else:
            self.world.edit(rec if self.seed % 2 else to_u32(rec))
        return True

    # -- box strokes
    def check_region(self, got, want):
        if not self.has_store:         # a stand-in says what it can: never new_ids
            want = {k: want[k] for k in got}
        assert got == want, (got, want, self.last)

    def region_refused(self, op, what, before, call):
        """The model refused the stroke: the world does, with everything unchanged."""
        import pytest
        t = self.tally
        t["region_refused"] += what == REFUSED
        t["region_invalid"] += what == INVALID
        t["region_refused_again"] += what == REFUSED and bool(op.get("retry"))
        if what == REFUSED:
            self.gen.refused(op)
        if self.has_store:
            with pytest.raises(self.ort.OchError, match="CAPACITY" if what == REFUSED else "INVALID") as e:
                call()
            assert e.value.status == (-6 if what == REFUSED else -1)
        assert self.m.info() == before
        return True                    # everything unchanged: info and the content are checked

    def alignments(self, st):
        """The alignments k <= 4 of the clipped box's faces that lie inside the tree: c a multiple of 2^k and no more."""
        faces = [c for c in st["lo"] + st["hi"] if 0 < c < 1 << self.m.depth]
        return {k for k in ((c & -c).bit_length() - 1 for c in faces) if k <= 4}

    def do_fill_box(self, op):
        m, t, lo, hi, id = self.m, self.tally, op["lo"], op["hi"], op["id"]
        before, cells, root, used = m.info(), m.cells, m.now.root, m.used
        box, _, _, T, need, _ = m.fill_plan(lo, hi, id)
        uniform, held = id, T > 0
        for h in range(T):             # the uniform subtrees of heights 1..T: does the store hold them all?
            uniform = m.cons.get((h, (uniform,) * 8))
            held = held and uniform in m.held
        what, st = m.fill_box(lo, hi, id)
        kind = "fill" if id else "clear"
        t["fill_box"] += 1
        if what in (REFUSED, INVALID):
            t["bound_refused_" + kind] += bool(op.get("pin")) and what == REFUSED and used + need == m.capacity + 1
            return self.region_refused(op, what, before, lambda: self.world.fill_box(lo, hi, id))
        self.check_region(self.world.fill_box(lo, hi, id), st)
        changed = m.cells != cells
        t[kind + "_change"] += changed
        for k in self.alignments(st) if changed else ():
            t[f"{kind}_k{k}"] += 1
        t["retry_admitted_" + kind] += bool(op.get("retry")) and what == "fill"
        t["bound_admitted_" + kind] += bool(op.get("pin")) and what == "fill" and used + need == m.capacity
        if T > 0:
            t["fill_uniform_held"] += held and self.uniform_fills.get((id, T)) == m.generation
            t["fill_uniform_after_compaction"] += self.uniform_fills.get((id, T), m.generation) < m.generation
            self.uniform_fills[id, T] = m.generation
        host_only = what == "fill" and not id and box == ((0, 0, 0), (1 << m.depth,) * 3)
        op["tags"] = ("whole_clear",) if host_only and root else ("region",) if what == "fill" and not host_only else ()
        return True

    def do_restore_box(self, op):
        m, t, lo, hi = self.m, self.tally, op["lo"], op["hi"]
        if isinstance(op["s"], str):
            op["s"] = sorted(m.snapshots)[{"last": -1, "prev": -2}[op["s"]]]
        s = op["s"]
        before, cells, state, used = m.info(), m.cells, m.now, m.used
        need = self.gen.restore_need(s)(lo, hi)
        what, st = m.restore_box(s, lo, hi)
        t["restore_box"] += 1
        if what == REFUSED:
            t["bound_refused_restore"] += bool(op.get("pin")) and used + need == m.capacity + 1
            return self.region_refused(op, what, before, lambda: self.world.restore_box(s, lo, hi))
        self.check_region(self.world.restore_box(s, lo, hi), st)
        changed = m.cells != cells
        t["restore_change"] += changed
        for k in self.alignments(st) if changed else ():
            t[f"restore_k{k}"] += 1
        t["restore_old"] += bool(changed and s and m.snapshots[s][1] < m.generation)
        t["restore_into_empty"] += changed and not cells
        t["restore_from_empty"] += bool(changed and not m.state(s).cells)
        t["restore_no_effect"] += what == "no_effect"
        t["retry_admitted_restore"] += bool(op.get("retry")) and what == "restore"
        t["bound_admitted_restore"] += bool(op.get("pin")) and what == "restore" and used + need == m.capacity
        outside = changed and not box_inside(exact_box(m.cells), state.box)
        op["tags"] = ((("whole_restore",) if what == "whole" else ("region",) if what == "restore" else ())
                      + (("restore_outside_box",) if outside else ()))
        return True

    def do_pin(self, op):
        ops = self.gen.pin_ops(op["kind"])
        self.gen.pending.extendleft(reversed(ops))
        return False

    def do_refuse(self, op):
        self.gen.pending.extendleft(reversed(self.gen.refuse_ops(op["kind"])))
        return False

    def do_snapshot(self, op):
        assert self.world.snapshot() == self.m.snapshot()
        return False

    def do_checkout(self, op):
        root = self.m.now.root
        self.m.checkout(op["s"])
        self.world.checkout(op["s"])
        op["moved"] = self.m.now.root != root
        op["tags"] = ("checkout_moved",) if op["moved"] else ()
        self.tally["checkout_calls"] += 1
        self.tally["checkout"] += op["moved"]
        return True

    def do_checkout_last(self, op):
        op["s"] = max(self.m.snapshots)
        return self.do_checkout(op)

    def do_release(self, op):
        self.m.release(op["s"])
        self.world.release(op["s"])
        assert self.world.snapshots() == sorted(self.m.snapshots)
        return False

    def do_release_all(self, op):
        for s in sorted(self.m.snapshots):
            self.do_release({"s": s})
        return False

    def do_compact(self, op):
        m, t = self.m, self.tally
        t["compact"] += 1
        op["tags"] = ("compact_snapshots",) if m.snapshots else ()
        t["compact_snapshots"] += bool(m.snapshots)
        t["compact_empty_now"] += bool(m.snapshots) and not m.cells and any(st.cells for st, _ in m.snapshots.values())
        t["compact_empty"] += not m.snapshots and not m.cells
        t["compact_after_checkout"] += self.after_checkout()
        m.compact()
        self.world.compact()
        self.compacted_since_tighten = True
        assert self.world.snapshots() == sorted(m.snapshots)
        return True

    def do_tighten(self, op):
        m, t = self.m, self.tally
        t["tighten"] += 1
        op["tags"] = ("tighten",)
        t["tighten_after_checkout"] += self.after_checkout()
        t["tighten_first"] += self.compacted_since_tighten
        t["tighten_incremental"] += not self.compacted_since_tighten and self.tightened_at != m.strokes
        self.compacted_since_tighten, self.tightened_at = False, m.strokes
        assert self.world.tighten() == m.tighten()
        return True

    def do_make_pool(self, op):
        self.tally["make_pool"] += 1
        pool = self.world.make_pool() if self.has_store else None
        self.pools.append([pool, None])
        self.publish(len(self.pools) - 1)
        return False

    def publish(self, i):
        self.pools[i][1] = {"cells": self.m.cells, "strokes": self.m.strokes, "generation": self.m.generation}

    def do_flush(self, op):
        pool, shown = self.pools[op["pool"]]
        self.tally["flush"] += 1
        op["tags"] = (f"flush{op['pool']}",)
        self.tally["flush_whole"] += shown["generation"] != self.m.generation
        if pool is not None:
            self.world.flush(pool)
        self.publish(op["pool"])
        return False

    def do_check_pool(self, op):
        pool, shown = self.pools[op["pool"]]
        self.tally["check_pool"] += 1
        op["tags"] = (f"check_pool{op['pool']}",)
        self.tally["check_pool_behind"] += self.m.strokes - shown["strokes"] >= 2
        if pool is None:
            return False
        from test_gpu_world import H, VIEW, W, check_traces, oracle_frame, random_rays
        ort, depth = self.ort, self.m.depth
        nodes, root = expected_pool(depth, records_of(shown["cells"]))
        pool.set_palette(ort.VoxelData().get_colours())
        if not root:
            for layout in (0, 1):
                pool.set_option("layout", layout)
                assert np.all(pool.render(ort.camera(tuple(ORIGIN), *VIEW, W, H)) == SKY), layout
            return False
        tree = types.SimpleNamespace(nodes=nodes, root=root, depth=depth)
        want = oracle_frame(ort, self.O, tree)
        for layout in (0, 1):
            pool.set_option("layout", layout)
            assert np.array_equal(pool.render(ort.camera(tuple(ORIGIN), *VIEW, W, H)), want), layout
        check_traces(ort, self.O, pool, tree, *random_rays(self.seed, 1024))
        return False

    def do_diff(self, op):
        a, b, m, t = op["a"], op["b"], self.m, self.tally
        rec, st, parents = self.check_diff(a, b, op["form"])
        walked = m.state(a).root != m.state(b).root      # equal roots are answered without a launch
        assert walked == (parents > 0)
        t["diff_calls"] += 1
        t["diff_device"] += op["form"] == "device"
        t["diff"] += walked
        t["diff_empty_side"] += (not m.state(a).cells) != (not m.state(b).cells)
        t["diff_across_compaction"] += bool(walked and a and b and max(m.snapshots[a][1], m.snapshots[b][1]) < m.generation)
        t["diff_big"] += parents > DIFF_FIRST_SIZE
        t["diff_small_after_big"] += (self.last is not None and self.last["op"] in ("diff", "big_diff", "small_diff")
                                      and (self.last_diff_parents or 0) > DIFF_FIRST_SIZE >= parents > 0)
        self.last_diff_parents = parents
        return False

    def do_big_diff(self, op):
        live = sorted(self.m.snapshots)
        return self.do_diff({"a": live[-2], "b": live[-1], "form": ["host", "device", "summary"][self.m.strokes % 3]})

    def do_small_diff(self, op):
        live = sorted(self.m.snapshots)
        return self.do_diff({"a": live[-3], "b": live[-2], "form": "device"})

    def do_diff_last(self, op):
        return self.do_diff({"a": max(self.m.snapshots), "b": 0, "form": "device"})

    def do_at(self, op):
        self.tally["at"] += 1
        self.tally["at_device"] += op["device"]
        self.check_at(op["seed"], op["device"])
        return False

    def do_read_box(self, op):
        import pytest
        m, t, lo, hi, dtype = self.m, self.tally, op["lo"], op["hi"], op["dtype"]
        want = scatter(m.cells, lo, hi, np.uint32)
        t["read_box"] += 1
        t["read_box_device"] += op["device"]
        t["read_box_overhang"] += any(l < 0 for l in lo) or any(h > 1 << m.depth for h in hi)
        device = op["device"] and self.on_gpu
        if dtype == np.uint8 and want.size and int(want.max()) > 255:
            t["read_box_u8_refused"] += 1
            # the world names the largest id above 255, the host path one of them
            names = str(int(want.max())) if self.has_store else "|".join(str(v) for v in np.unique(want[want > 255]).tolist())
            with pytest.raises(self.ort.OchError, match=f"INVALID.* ({names}) ") as e:
                self.world.read_box(lo, hi, dtype, device=device)
            assert e.value.status == -1
            return False
        got = self.world.read_box(lo, hi, dtype, device=device)
        if device:
            got = got.cpu().numpy().view(dtype)
        assert got.dtype == dtype and got.shape == want.shape and np.array_equal(got, want.astype(dtype)), (lo, hi, dtype)
        return False

    def do_download(self, op):
        self.check_content()
        return False

    def do_revert_by_diff(self, op):
        s, m = op["s"], self.m
        self.tally["revert_by_diff"] += 1
        rec, _, _ = self.check_diff(0, s, "host")
        got = self.world.diff(0, s)[0]
        what = m.edit(rec.astype(np.int64))
        assert what in (None, "stroke")
        self.world.edit(got)
        self.tally["edit"] += what is not None
        self.tally["admitted"] += what is not None
        assert m.cells == m.state(s).cells
        empty, st = self.world.diff(0, s)
        if not self.has_store:
            st = dict(st, pairs=0)
        assert empty.shape == (0, 4) and st == NOTHING
        return True
