"""The random walks of tests/world_model.py against a stand-in made of the host paths alone, and the
quotas that keep the walks from being vacuous.

HostWorld has World's methods but no store: a stroke is ort.edit_voxels(use_gpu=False) with a random
thread count, at() is NodePool.at behind a range check, read_box() NodePool.read_box, diff()
NodePool.diff of two pools, tighten() ort.occupied_box, fill_box() the editor over ort.box_records,
a clear of any size the tree's diff against an empty pool filtered to the box and applied, restore_box()
its diff against the snapshot's tree likewise; their stats come from och_box_cubes' counts and, for a
restore at depth <= 5, from differing() over the two dense grids.  The driver skips `used`, the loose box,
refusals and pools for it (the model still meets them: the operation list is the GPU's).  That
proves model, generator and driver against a second implementation before a GPU is involved, and
gives the host editor its first randomised chains.

The quotas are counted from the model alone, over all seeds of WALKS together.  Only instances that
reach the code they are named for count: a checkout counts when it changes the root (checkout(0) or
of the current content uploads nothing later), a diff when its two roots differ (equal roots return
before any launch), a smaller diff after a large one when it is not empty."""
import collections
import time

import numpy as np
import pytest

from test_voxel_builder import corner_records
from world_model import Model, Walk

# (seed, depth, capacity, steps): capacity an integer = that many `depth` rows above what the base
# needs, None = the default, "roomy" = 40 000 ids (the two strokes of more than 1024 leaf-level
# parents need some 2 000 rows each).  Depths 1 and 2: the root is, or sits directly on, a leaf-level
# node; 6: the smallest at which one stroke can exceed 1024 leaf-level parents; 16 and 21: a few
# hundred cells clustered around corner_records; the second depth-21 walk has room for the box strokes' cells.
# After its `steps` operations every walk runs REGION_STEPS more: the room that the box strokes' sequences need.
WALKS = [(101, 1, 8, 80), (102, 2, 20, 80), (103, 3, 30, 90), (104, 4, 30, 90), (105, 5, None, 90), (106, 5, 40, 100),
         (107, 6, "roomy", 70), (108, 6, 100, 80), (109, 16, 20, 80), (110, 21, 16, 80), (111, 21, 2000, 80)]
REGION_STEPS = 50


def base_records(seed, depth):
    rng = np.random.default_rng(seed)
    dim = 1 << depth
    if depth > 8:
        corners = corner_records(depth).astype(np.int64)
        c = corners[rng.integers(0, len(corners), 250), :3] + rng.integers(-5, 6, (250, 3))
        c = c[((c >= 0) & (c < dim)).all(1)]
        return np.concatenate([corners, np.concatenate([c, rng.integers(1, 6, (len(c), 1))], 1)])
    n = {1: 3, 2: 20, 3: 100, 4: 300, 5: 500, 6: 1500}[depth]
    return np.concatenate([rng.integers(0, dim, (n, 3)), rng.integers(1, 6, (n, 1))], 1).astype(np.int64)


def make_model(seed, depth, capacity):
    base = base_records(seed, depth)
    model = Model(depth, base, None)
    if capacity == "roomy":
        model.capacity = 40_000
    elif capacity is not None:
        model.capacity = model.used + capacity * depth
    return model, base


class HostWorld:
    has_store = False

    def __init__(self, ort, depth, base, seed):
        self.ort, self.depth, self.rng = ort, depth, np.random.default_rng(seed)
        self.tree = ort.build_voxels(base, depth=depth, use_gpu=False)
        self.saved, self.next_snapshot, self.strokes, self.generation = {}, 1, 0, 0

    def info(self):
        return {"root": self.tree.root, "depth": self.depth, "strokes": self.strokes, "generation": self.generation}

    def edit(self, records):
        if len(records):
            self.tree = self.ort.edit_voxels(self.tree, records, use_gpu=False, threads=int(self.rng.integers(1, 6)))
            self.strokes += 1

    def download(self):
        return self.tree

    def at(self, coords):
        dim = 1 << self.depth
        return np.array([self.tree.at(x, y, z) if 0 <= x < dim and 0 <= y < dim and 0 <= z < dim else 0
                         for x, y, z in np.asarray(coords).tolist()], np.uint32)

    def read_box(self, lo, hi, dtype=np.uint8, device=False):
        return self.tree.read_box(lo, hi, dtype)

    def tighten(self):
        return self.ort.occupied_box(self.tree.nodes, self.tree.root, self.depth)

    def compact(self):
        self.generation += 1

    def snapshot(self):
        self.saved[self.next_snapshot] = self.tree
        self.next_snapshot += 1
        return self.next_snapshot - 1

    def _state(self, s):
        return self.saved[s] if s else self.tree

    def checkout(self, s):
        self.tree = self._state(s)

    def release(self, s):
        del self.saved[s]

    def snapshots(self):
        return sorted(self.saved)

    def diff(self, a, b=0, device=False, records=True):
        return self._state(a).diff(self._state(b), records=records)

    # -- box strokes: the record editor, with the records a diff of two pools gives where the box is large
    def _clipped(self, lo, hi):
        lo, hi = np.maximum(np.asarray(lo, np.int64), 0), np.minimum(np.asarray(hi, np.int64), 1 << self.depth)
        return (lo, hi) if (lo < hi).all() else None

    def _become(self, other, box):
        """Inside the box the voxels of `other`: its diff against the current tree, filtered to the box, applied."""
        rec, _ = self.tree.diff(other)
        c = rec[:, :3].astype(np.int64)
        rec = rec[((c >= box[0]) & (c < box[1])).all(1)]
        if len(rec):
            self.tree = self.ort.edit_voxels(self.tree, rec, use_gpu=False, threads=int(self.rng.integers(1, 6)))

    def _counts(self, lo, hi):
        """och_box_cubes' two totals, counts only (the cubes of a large box are too many to list)."""
        import ctypes as C
        cubes, cells, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
        assert self.ort.load().och_box_cubes((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), self.depth, None, None, 0, cubes, cells,
                                             C.byref(n)) == 0
        assert sum(cubes) == n.value
        return int(n.value), int(sum(cells))

    def fill_box(self, lo, hi, id):
        self.strokes += 1
        box = self._clipped(lo, hi)
        if box is None:
            return {"cubes": 0, "cells": 0, "lo": (0, 0, 0), "hi": (0, 0, 0)}
        if id:
            self.tree = self.ort.edit_voxels(self.tree, self.ort.box_records(box[0], box[1], id), use_gpu=False,
                                             threads=int(self.rng.integers(1, 6)))
        else:
            self._become(self.ort.build_voxels(np.zeros((0, 4), np.uint32), depth=self.depth, use_gpu=False), box)
        cubes, cells = self._counts(box[0].tolist(), box[1].tolist())
        return {"cubes": cubes, "cells": cells, "lo": tuple(box[0].tolist()), "hi": tuple(box[1].tolist())}

    def restore_box(self, s, lo, hi):
        from test_gpu_world_region import differing, whole_grid
        self.strokes += 1
        box = self._clipped(lo, hi)
        if box is None:
            return {"cubes": 0, "cells": 0, "lo": (0, 0, 0), "hi": (0, 0, 0)}
        out = {"lo": tuple(box[0].tolist()), "hi": tuple(box[1].tolist())}
        snap = self._state(s)
        if self.depth <= 5:            # the counts from the two dense grids
            a, b = whole_grid(self.tree), whole_grid(snap)
            cubes, cells = differing(self.depth, box[0], box[1], a, b)
            out.update(cubes=cubes, cells=cells)
        self._become(snap, box)
        return out


@pytest.fixture(scope="module")
def tallies():
    """seed -> the Counter of its walk, filled by test_walk_host."""
    return {}


@pytest.mark.parametrize("seed,depth,capacity,steps", WALKS)
def test_walk_host(ort, tallies, seed, depth, capacity, steps):
    model, base = make_model(seed, depth, capacity)
    t0, tally = time.perf_counter(), collections.Counter()
    Walk(ort, HostWorld(ort, depth, base, seed), model, seed, big=capacity == "roomy", tally=tally).run(steps + REGION_STEPS)
    tallies[seed] = tally
    print(f"walk {seed} depth {depth}: {steps + REGION_STEPS} operations in {time.perf_counter() - t0:.1f} s")


# quota -> (the tally's key, the least count); a third of each kind with a device form is counted below
QUOTAS = {"admitted strokes": ("admitted", 150), "refused strokes": ("refused", 5),
          "still refused after the compaction": ("refused_again", 1), "compactions": ("compact", 10),
          "compactions with live snapshots": ("compact_snapshots", 4),
          "... while the current state is empty and a snapshot's is not": ("compact_empty_now", 1),
          "compactions of an empty world without a snapshot": ("compact_empty", 1), "checkouts": ("checkout", 20),
          "checkout then stroke": ("stroke_after_checkout", 5), "checkout then compaction": ("compact_after_checkout", 3),
          "checkout then tighten": ("tighten_after_checkout", 3), "diffs": ("diff", 20),
          "diffs with an empty side": ("diff_empty_side", 3),
          "diffs of snapshots from before a compaction": ("diff_across_compaction", 3),
          "diffs of more than 1024 leaf-level parents": ("diff_big", 3),
          "a smaller diff right after one of those": ("diff_small_after_big", 1), "tightens": ("tighten", 10),
          "tightens first after a compaction": ("tighten_first", 3), "incremental tightens": ("tighten_incremental", 3),
          "flushes": ("flush", 10), "flushes rewriting a pool whole": ("flush_whole", 3),
          "check_pool two strokes behind": ("check_pool_behind", 3), "read_box calls": ("read_box", 10),
          "overhanging read_box calls": ("read_box_overhang", 3), "u8 refusals": ("read_box_u8_refused", 2),
          "revert_by_diff": ("revert_by_diff", 3), "no-change strokes": ("no_change", 1),
          "all-out-of-range strokes": ("outside", 1), "emptying strokes": ("emptying", 1),
          "strokes where the two readings of the box rule differ": ("box_readings_differ", 1),
          # box strokes (fill_box, restore_box)
          "fills that change the content": ("fill_change", 3), "clears that change the content": ("clear_change", 3),
          "restores that change the content": ("restore_change", 3),
          "restores from a snapshot older than the current generation": ("restore_old", 3),
          "box strokes directly after a root-changing checkout": ("region_after_checkout", 3),
          "refused box strokes": ("region_refused", 3),
          "a whole-tree clear, then a record stroke, flush and check_pool": ("seq_whole_clear", 1),
          "a whole-tree restore, then flush and check_pool": ("seq_whole_restore", 1),
          "a whole-tree restore, then a compaction with live snapshots, then tighten": ("seq_whole_restore_compact", 1),
          "a restore into an empty world": ("restore_into_empty", 1), "a restore from an empty snapshot": ("restore_from_empty", 1),
          "a restore of a box that holds no difference": ("restore_no_effect", 1),
          "a fill whose uniform subtrees the store holds": ("fill_uniform_held", 1),
          "the same fill after a compaction": ("fill_uniform_after_compaction", 1),
          "a restore outside the tightened box, then flush and check_pool": ("seq_restore_outside_box", 1),
          "a fill refused, and admitted after the compaction": ("retry_admitted_clear", 1),
          "a restore refused, and admitted after the compaction": ("retry_admitted_restore", 1),
          "a fill refused at used + need == capacity + 1": ("bound_refused_clear", 1),
          "a fill admitted at used + need == capacity": ("bound_admitted_clear", 1),
          "a restore refused at used + need == capacity + 1": ("bound_refused_restore", 1),
          "a restore admitted at used + need == capacity": ("bound_admitted_restore", 1)}
QUOTAS.update({f"a {kind} that changes the content with a face aligned to 2^{k} and no more": (f"{kind}_k{k}", 1)
               for kind in ("fill", "clear", "restore") for k in range(5)})


def test_quotas(ort, tallies):
    """The walks meet what they are for.  A seed whose walk has not run in this session (a partial
    selection) is walked here, so the result does not depend on which tests ran before."""
    tally = collections.Counter()
    for seed, depth, capacity, steps in WALKS:
        if seed not in tallies:
            model, base = make_model(seed, depth, capacity)
            tallies[seed] = collections.Counter()
            Walk(ort, HostWorld(ort, depth, base, seed), model, seed, big=capacity == "roomy", tally=tallies[seed]).run(steps + REGION_STEPS)
        tally.update(tallies[seed])
    print(dict(tally))
    short = {name: (tally[key], least) for name, (key, least) in QUOTAS.items() if tally[key] < least}
    for kind, calls in (("edit", "edit"), ("diff", "diff_calls"), ("at", "at"), ("read_box", "read_box")):
        if 3 * tally[kind + "_device"] < tally[calls]:
            short[kind + " in its device form"] = (tally[kind + "_device"], tally[calls])
    assert not short, short
