"""The model, generator and driver of tests/world_model.py with the sphere strokes of a resident world
(och_world_fill_sphere, och_world_restore_sphere) added, written from include/och_gpu.h ("world: regions").

A helper module, not a test file: tests/test_world_sphere_walk_host.py walks the host stand-in and asserts
the quotas, tests/test_gpu_world_sphere_walk.py walks ort.World.

  ball            voxel (x, y, z) is in it iff the squares of 2x+1-c2x, 2y+1-c2y, 2z+1-c2z sum to at most
                  d^2; an aligned cube is classified per axis in Python integers (classify, shared with
                  tests/test_sphere_cubes_host.py); the axis box is ceil((c2 - d - 1) / 2) ..
                  floor((c2 + d - 1) / 2) + 1 clipped to the tree.
  fill_sphere     the counts come from a top-down recursion over the classifier.  No cube (an empty axis
                  box, a root cell outside the ball): strokes + 1, stats 0 but the clipped axis box,
                  never refused, the box left alone.  used + sum cells + T > capacity (T = the greatest
                  height with a cube for id != 0, else 0): REFUSED.  Otherwise held gains the non-empty
                  node of the new tree at every straddling cell and, for id != 0, the uniform subtrees
                  of heights 1..T; the box grows by the clipped axis box for id != 0.  A ball over the
                  whole tree is one cube of height depth and no cell.
  restore_sphere  Model.restore_box with the ball's classifier: front = the straddling cells visited whose
                  two nodes differ, cubes = the inside children whose two words differ, cells = the visited
                  cells with such a cube beneath them; no differing cube: strokes + 1 and nothing else;
                  REFUSED when used + front > capacity; the box grows by the clipped axis box inside the
                  snapshot's box; the whole tree: the snapshot's root, cubes = 1, no id.

The generator mixes sphere strokes into every other operation of Generator.next(), box strokes included,
and adds sequences of its own: whole-tree strokes of each kind and capacity bounds pinned from both sides."""
import numpy as np

from test_sphere_cubes_host import classify
from world_model import FILL_VOXELS, NO_REGION, REFUSED, Generator, Model, State, Walk, box_meet, box_union, exact_box

FILL_DIAMETER = 22                # a filled ball stays far below FILL_VOXELS voxels: the driver probes every content


def axis_box(c2, d, depth):
    """The ball's axis box clipped to the tree, None where nothing is left."""
    n = 1 << depth
    lo = tuple(min(max(-((d + 1 - c) // 2), 0), n) for c in c2)
    hi = tuple(min(max((c + d - 1) // 2 + 1, 0), n) for c in c2)
    return (lo, hi) if all(l < h for l, h in zip(lo, hi)) else None


def in_ball(c, c2, d):
    return sum((2 * v + 1 - m) ** 2 for v, m in zip(c, c2)) <= d * d


def ball_voxels(c2, d, box):
    """The ball's voxels inside the clipped axis box, as tuples of Python integers."""
    (x0, y0, z0), (x1, y1, z1) = box
    off = [(2 * np.arange(l, u, dtype=np.int64) + 1 - m) ** 2 for l, u, m in zip(box[0], box[1], c2)]
    x, y, z = np.nonzero(off[0][:, None, None] + off[1][None, :, None] + off[2][None, None, :] <= d * d)
    return list(zip((x + x0).tolist(), (y + y0).tolist(), (z + z0).tolist()))


def child(o, k, half):
    return (o[0] + (k & 1) * half, o[1] + ((k >> 1) & 1) * half, o[2] + ((k >> 2) & 1) * half)


class SphereModel(Model):
    def ball_walk(self, c2, d):
        """(cubes per height, the straddling cells as (height, key)) of the walk from the root cell."""
        cubes, cells = [0] * (self.depth + 1), []

        def visit(H, key, o):
            c = classify(c2, d, o, H)
            if c == 2:
                cubes[H] += 1
            elif c == 1:
                cells.append((H, key))
                for k in range(8):
                    visit(H - 1, key << 3 | k, child(o, k, 1 << (H - 1)))

        visit(self.depth, 0, (0, 0, 0))
        return cubes, cells

    def fill_sphere_plan(self, c2, d, id):
        """(clipped axis box or None, cubes per height, straddling cells, T, need, REFUSED / None), nothing changed."""
        box = axis_box(c2, d, self.depth)
        if box is None:
            return None, [], [], 0, 0, None
        cubes, cells = self.ball_walk(c2, d)
        T = max((h for h in range(self.depth + 1) if cubes[h]), default=0) if id else 0
        need = len(cells) + T
        return box, cubes, cells, T, need, REFUSED if sum(cubes) and self.used + need > self.capacity else None

    def fill_sphere(self, c2, d, id):
        """("nothing" / REFUSED / "fill", the stats or None)."""
        box, cubes, cells, T, need, what = self.fill_sphere_plan(c2, d, id)
        st = dict(NO_REGION) if box is None else dict(NO_REGION, lo=box[0], hi=box[1])
        if not sum(cubes):
            self.strokes += 1
            return "nothing", st
        if what:
            return what, None
        new = {c: v for c, v in self.now.cells.items() if not in_ball(c, c2, d)}
        if id:
            voxels = ball_voxels(c2, d, box)
            assert len(voxels) <= FILL_VOXELS, (c2, d)
            new.update((c, id) for c in voxels)
        self.now = self._state(new, box_union(self.now.box, box) if id else self.now.box)
        before = len(self.held)
        for H, key in cells:
            node = self.now.levels[H - 1].get(key)
            if node:
                self.held.add(node)
        uniform = id
        for h in range(T):
            uniform = self._intern(h, (uniform,) * 8)
            self.held.add(uniform)
        self.strokes += 1
        self.version += 1
        return "fill", dict(st, cubes=sum(cubes), cells=len(cells), new_ids=len(self.held) - before)

    def restore_sphere_plan(self, s, c2, d):
        """Model.restore_plan for a ball that straddles the root cell."""
        rows_of, count, cells = self.rows, [0, 0], []

        def visit(H, key, o, na, nb):
            count[0] += 1
            ra, rb, half, found = rows_of[na], rows_of[nb], 1 << (H - 1), False
            for k in range(8):
                if ra[k] == rb[k]:
                    continue
                c = child(o, k, half)
                cls = classify(c2, d, c, H - 1)
                if cls == 2:
                    count[1] += 1
                    found = True
                elif cls == 1 and visit(H - 1, key << 3 | k, c, ra[k], rb[k]):
                    found = True
            if found:
                cells.append((H, key))
            return found

        visit(self.depth, 0, (0, 0, 0), self.now.root, self.state(s).root)
        return count[0], count[1], cells

    def restore_sphere_need(self, s, c2, d):
        """The ids a restore may take (its front), None where it is answered without a walk or finds no cube."""
        box = axis_box(c2, d, self.depth)
        if box is None or classify(c2, d, (0, 0, 0), self.depth) != 1 or self.state(s).root == self.now.root:
            return None
        front, cubes, _ = self.restore_sphere_plan(s, c2, d)
        return front if cubes else None

    def restore_sphere(self, s, c2, d):
        """("nothing" / "whole" / "no_effect" / REFUSED / "restore", the stats or None)."""
        snap, box = self.state(s), axis_box(c2, d, self.depth)
        st = dict(NO_REGION) if box is None else dict(NO_REGION, lo=box[0], hi=box[1])
        root = classify(c2, d, (0, 0, 0), self.depth) if box else 0
        if root == 0 or snap.root == self.now.root:
            self.strokes += 1
            return "nothing", st
        grown = box_union(self.now.box, box_meet(box, snap.box))
        if root == 2:
            self.now = State(snap.cells, snap.levels, snap.root, grown)
            self.strokes += 1
            self.version += 1
            return "whole", dict(st, cubes=1)
        front, cubes, cells = self.restore_sphere_plan(s, c2, d)
        if not cubes:
            self.strokes += 1
            return "no_effect", st
        if self.used + front > self.capacity:
            return REFUSED, None
        new = {c: v for c, v in self.now.cells.items() if not in_ball(c, c2, d)}
        new.update((c, v) for c, v in snap.cells.items() if in_ball(c, c2, d))
        self.now = self._state(new, grown)
        before = len(self.held)
        for H, key in cells:
            node = self.now.levels[H - 1].get(key)
            if node:
                self.held.add(node)
        self.strokes += 1
        self.version += 1
        return "restore", dict(st, cubes=cubes, cells=len(cells), new_ids=len(self.held) - before)


class SphereGenerator(Generator):
    SPHERES = 0.3                     # of the operations that nothing queued

    def __init__(self, model, seed, big=False):
        super().__init__(model, seed, big)
        # the sphere strokes' sequences, between the others'
        names = ["s_checkout", "s_whole", "s_pin_fill", "s_pin_restore", "s_refuse_fill", "s_untouched", "s_refuse_restore", "s_checkout"]
        self.script = sorted(self.script + [(12 + 14 * i, name) for i, name in enumerate(names)], key=lambda e: e[0])

    def region_box(self, fill, centre=None, kinds=True):
        lo, hi = super().region_box(fill, centre, kinds)
        return lo, tuple(max(l, h) for l, h in zip(lo, hi))          # an empty box: World.fill_box takes hi >= lo

    # -- balls
    def ball(self, fill, centre=None, kinds=True):
        """(centre2, diameter): centres of every parity, near voxels, on the tree's faces and corners and off
        them; diameters from 0 to overhanging and whole-tree; fill = True keeps the ball below FILL_VOXELS voxels."""
        rng, m = self.rng, self.m
        kind = ["near"] * 10 + ["face", "corner", "zero", "outside", "far", "whole", "overhang"]
        kind = kind[rng.integers(0, len(kind))] if kinds and centre is None else "near"
        most = min(FILL_DIAMETER, 2 * self.dim) if fill or self.deep else min(2 * self.dim, 96)
        c = np.asarray(self.some_cell() if centre is None else centre, np.int64)
        c2 = 2 * c + rng.integers(0, 2, 3) + np.where(rng.random(3) < 0.5, 0, rng.integers(-6, 7, 3))
        d = int(rng.integers(1, 8)) if rng.random() < 0.5 else int(rng.integers(1, most + 1))
        if kind == "whole" and (not fill or m.depth <= 4):
            c2, d = np.full(3, self.dim) + rng.integers(-1, 2, 3), 2 * self.dim
        elif kind == "far":                 # the argument range's end: the tree is wholly inside or wholly outside
            c2, d = (np.array([1 << 24, -(1 << 24), 0]), 1 << 24) if fill or rng.random() < 0.5 else (np.zeros(3, np.int64), 1 << 24)
        elif kind == "outside":
            c2, d = np.array([2 * self.dim + 9, self.dim, -3]), int(rng.integers(0, 8))
        elif kind == "face":
            c2[rng.integers(0, 3)] = [0, 2 * self.dim][rng.integers(0, 2)]
        elif kind == "corner":
            c2 = np.array([0, 2 * self.dim])[rng.integers(0, 2, 3)]
        elif kind == "zero":
            d = 0
        elif kind == "overhang":
            a = rng.integers(0, 3)
            c2[a] = [-3, 2 * self.dim + 2][rng.integers(0, 2)]
            d = max(d, 7)
        return tuple(int(v) for v in c2), int(d)

    def fill_sphere_op(self, id=None, centre=None, over=0.15):
        """Budget-aware, as fill_box_op: mostly a ball that the capacity admits, some on purpose over it."""
        m, rng = self.m, self.rng
        if id is None:
            id = 0 if rng.random() < 0.5 else int(self.ids(1, odd=0.2)[0])
        want_over = rng.random() < over
        for _ in range(12):
            c2, d = self.ball(bool(id), centre)
            what = m.fill_sphere_plan(c2, d, id)[5]
            if what is None or want_over:
                break
        else:
            c = self.some_cell() if centre is None else np.asarray(centre, np.int64)
            c2, d = tuple(int(2 * v + 1) for v in c), 0
        return {"op": "fill_sphere", "c2": c2, "d": d, "id": id}

    def restore_sphere_op(self, s=None, centre=None):
        if s is None:
            s = self.handle(zero=0.05, other_than=0)
        if centre is None and self.rng.random() < 0.6:   # mostly around a voxel that differs: the restore has something to do
            a, b = self.m.state(s).cells, self.m.cells
            differ = [c for c in a.keys() | b.keys() if a.get(c, 0) != b.get(c, 0)][:64]
            if differ:
                centre = differ[self.rng.integers(0, len(differ))]
        c2, d = self.ball(False, centre)
        return {"op": "restore_sphere", "s": s, "c2": c2, "d": d}

    def ball_with_need(self, need_of, accept, centres, tries=300):
        for _ in range(tries):
            c2, d = self.ball(True, centre=centres[self.rng.integers(0, len(centres))], kinds=False)   # small: the search walks each
            need = need_of(c2, d)
            if need is not None and accept(need):
                return c2, d
        return None

    def ball_with_exact_need(self, need_of, target, centres, most, tries=16):
        """A ball whose need is exactly `target`: per centre, the diameter at which the need, which mostly grows
        with it, first reaches the target, and its neighbours."""
        if target > 40 * most * most:                  # more cells than a ball of this size straddles
            return None
        short = 0
        for _ in range(tries):
            c = np.asarray(centres[self.rng.integers(0, len(centres))], np.int64)
            c2 = tuple(int(v) for v in 2 * c + self.rng.integers(0, 2, 3))
            lo, hi = 0, most
            while lo < hi:
                mid = (lo + hi) // 2
                need = need_of(c2, mid)
                lo, hi = (lo, mid) if need is not None and need >= target else (mid + 1, hi)
            for d in (lo, lo + 1, lo - 1, lo + 2):
                if 0 <= d <= most and need_of(c2, d) == target:
                    return c2, d
            short += lo == most and (need_of(c2, most) or 0) < target
            if short == 2:                             # out of a small ball's reach
                return None
        return None

    def clear_sphere_need(self, c2, d):
        box, cubes, _, _, need, _ = self.m.fill_sphere_plan(c2, d, 0)
        return need if box is not None and sum(cubes) and not cubes[self.m.depth] else None

    def pin_ops(self, kind, again=0):
        if not kind.startswith("sphere"):
            return super().pin_ops(kind)
        m = self.m
        free = m.capacity - m.used
        if kind == "sphere_fill":
            need_of, centres = self.clear_sphere_need, self.centres()
            make = lambda b: {"op": "fill_sphere", "c2": b[0], "d": b[1], "id": 0}
        else:
            if not m.snapshots:
                return []
            s = max(m.snapshots)
            need_of, centres = (lambda c2, d: m.restore_sphere_need(s, c2, d)), self.centres(m.state(s))
            make = lambda b: {"op": "restore_sphere", "s": s, "c2": b[0], "d": b[1]}
        # a clear's walk follows the whole surface, a restore's only what differs: that one may be large
        most = min(FILL_DIAMETER, 2 * self.dim) if kind == "sphere_fill" or self.deep else 2 * self.dim
        tries = 16 if kind == "sphere_fill" or self.deep else 120
        over = self.ball_with_exact_need(need_of, free + 1, centres, most, tries)
        exact = self.ball_with_exact_need(need_of, free, centres, most, tries)
        if (over is None or exact is None) and again < 2 and free > 4 * m.depth:
            # out of a ball's reach, mostly: a record stroke of fresh voxels takes ids first, then the pin again
            reach = max([need_of(tuple(int(2 * v + 1) for v in c), d) or 0 for c in centres[:6] for d in (most // 4, most // 2)] + [2 * m.depth])
            want = free - min(reach, free // 2)
            pool = np.concatenate([self.coords(min(4 * want, 20000)), np.full((min(4 * want, 20000), 1), 5000 + self.step, np.int64)], 1)
            lo, hi = 1, len(pool)                      # the longest prefix of the pool whose stroke the budget admits
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if m.stroke_need(pool[:mid]) <= want else (lo, mid - 1)
            rec = pool[:lo]
            stroke = {"op": "edit", "records": rec.astype(np.int64), "device": False, "kind": "filler"}
            return [stroke, {"op": "pin", "kind": kind, "again": again + 1}]
        return [dict(make(b), pin=True) for b in (over, exact) if b is not None]

    def refuse_ops(self, kind):
        if not kind.startswith("sphere"):
            return super().refuse_ops(kind)
        m = self.m
        free, free_then = m.capacity - m.used, m.capacity - self.used_after_compaction()
        if kind == "sphere_fill":
            need_of, centres = self.clear_sphere_need, self.centres()
            make = lambda b: {"op": "fill_sphere", "c2": b[0], "d": b[1], "id": 0}
        else:
            if not m.snapshots:
                return []
            s = max(m.snapshots)
            need_of, centres = (lambda c2, d: m.restore_sphere_need(s, c2, d)), self.centres(m.state(s))
            make = lambda b: {"op": "restore_sphere", "s": s, "c2": b[0], "d": b[1]}
        ball = self.ball_with_need(need_of, lambda n: free < n <= free_then, centres) if free_then > free else None
        return [make(ball)] if ball is not None else []

    # -- sequences
    def script_s_checkout(self):
        # a checkout that changes the root, then a sphere stroke: the head's root word is behind the host's
        s = self.handle(zero=0.0, other_than=0)
        if self.m.state(s).root == self.m.now.root:
            return None
        centre = self.some_cell([self.m.state(s)])
        follow = self.fill_sphere_op(id=[0, 3][self.step % 2], centre=centre, over=0) if self.rng.random() < 0.6 else \
            self.restore_sphere_op(s=self.handle(zero=0.0, other_than=s), centre=centre)
        self.pending.append(follow)
        return {"op": "checkout", "s": s}

    def script_s_refuse_fill(self):
        return {"op": "refuse", "kind": "sphere_fill"}

    def script_s_refuse_restore(self):
        self.pending.extend([self.stroke("scatter"), self.stroke("scatter"), {"op": "refuse", "kind": "sphere_restore"}])
        return {"op": "snapshot"}

    def whole_ball(self):
        return {"c2": (self.dim,) * 3, "d": 2 * self.dim}

    def script_s_whole(self):
        # a whole-tree fill where a record list of it is small, a whole-tree clear and a whole-tree restore:
        # the root changes on the host alone, then a stroke, a flush and a frame
        fill = [dict(self.whole_ball(), op="fill_sphere", id=7)] if self.m.depth <= 4 else []
        clear, back = dict(self.whole_ball(), op="fill_sphere", id=0), dict(self.whole_ball(), op="restore_sphere", s="last")
        flush, check = {"op": "flush", "pool": 0}, {"op": "check_pool", "pool": 0}
        return self.with_pool([{"op": "snapshot"}] + fill + [clear, self.stroke("small_new"), flush, check, back, dict(flush), dict(check)])

    def script_s_pin_fill(self):
        self.pending.append({"op": "pin", "kind": "sphere_fill"})
        return {"op": "compact"}

    def script_s_pin_restore(self):
        if not self.m.cells:
            return None
        self.pending.extend([dict(self.whole_ball(), op="fill_sphere", id=0), {"op": "pin", "kind": "sphere_restore"}])
        return {"op": "snapshot"}

    def script_s_untouched(self):
        # the roots differ, and every difference lies outside the ball
        stroke = self.stroke("small_new")
        touched = [tuple(c) for c in stroke["records"][:, :3].tolist()]
        for _ in range(40):
            c2, d = self.ball(False, kinds=False)
            if classify(c2, d, (0, 0, 0), self.m.depth) == 1 and not any(in_ball(c, c2, d) for c in touched):
                self.pending.extend([stroke, {"op": "restore_sphere", "s": "last", "c2": c2, "d": d}])
                return {"op": "snapshot"}
        return None

    def next(self):
        due = self.script and self.step + 1 >= self.script[0][0]
        if not self.pending and not due and self.rng.random() < self.SPHERES:
            self.step += 1
            return self.fill_sphere_op() if self.rng.random() < 0.55 else self.restore_sphere_op()
        return super().next()


class SphereWalk(Walk):
    def __init__(self, ort, world, model, seed, big=False, O=None, on_gpu=False, tally=None):
        super().__init__(ort, world, model, seed, big, O, on_gpu, tally)
        self.gen = SphereGenerator(model, seed, big)

    def do_pin(self, op):
        if not op["kind"].startswith("sphere"):
            return super().do_pin(op)
        self.gen.pending.extendleft(reversed(self.gen.pin_ops(op["kind"], op.get("again", 0))))
        return False

    def do_fill_sphere(self, op):
        m, t, c2, d, id = self.m, self.tally, op["c2"], op["d"], op["id"]
        before, cells, root, used = m.info(), m.cells, m.now.root, m.used
        need = m.fill_sphere_plan(c2, d, id)[4]
        what, st = m.fill_sphere(c2, d, id)
        kind = "fill" if id else "clear"
        t["fill_sphere"] += 1
        if what == REFUSED:
            t["sphere_refused"] += 1
            t["sphere_bound_refused_clear"] += bool(op.get("pin")) and used + need == m.capacity + 1
            return self.region_refused(op, what, before, lambda: self.world.fill_sphere(c2, d, id))
        self.check_region(self.world.fill_sphere(c2, d, id), st)
        whole = what == "fill" and st["cubes"] == 1 and st["cells"] == 0 and st["hi"] == (1 << m.depth,) * 3
        t["sphere_" + kind] += what == "fill"
        t["sphere_" + kind + "_change"] += m.cells != cells
        t["sphere_whole_" + kind] += whole
        t["sphere_no_effect"] += what == "nothing"
        t["sphere_nothing_in_a_box"] += what == "nothing" and st["hi"] != (0, 0, 0)
        t["sphere_retry_admitted"] += bool(op.get("retry")) and what == "fill"
        t["sphere_bound_admitted_clear"] += bool(op.get("pin")) and what == "fill" and used + need == m.capacity
        t["sphere_after_checkout"] += what == "fill" and self.after_checkout()
        host_only = whole and not id
        op["tags"] = ("whole_clear",) if host_only and root else ("region",) if what == "fill" and not host_only else ()
        return True

    def do_restore_sphere(self, op):
        m, t, c2, d = self.m, self.tally, op["c2"], op["d"]
        if isinstance(op["s"], str):
            op["s"] = sorted(m.snapshots)[{"last": -1, "prev": -2}[op["s"]]]
        s = op["s"]
        before, cells, used = m.info(), m.cells, m.used
        need = m.restore_sphere_need(s, c2, d)
        what, st = m.restore_sphere(s, c2, d)
        t["restore_sphere"] += 1
        if what == REFUSED:
            t["sphere_refused"] += 1
            t["sphere_bound_refused_restore"] += bool(op.get("pin")) and used + need == m.capacity + 1
            return self.region_refused(op, what, before, lambda: self.world.restore_sphere(s, c2, d))
        self.check_region(self.world.restore_sphere(s, c2, d), st)
        t["sphere_restore_change"] += m.cells != cells
        t["sphere_whole_restore"] += what == "whole"
        t["sphere_no_effect"] += what in ("nothing", "no_effect")
        t["sphere_restore_untouched"] += what == "no_effect"
        t["sphere_retry_admitted"] += bool(op.get("retry")) and what == "restore"
        t["sphere_bound_admitted_restore"] += bool(op.get("pin")) and what == "restore" and used + need == m.capacity
        t["sphere_after_checkout"] += what == "restore" and self.after_checkout()
        op["tags"] = ("whole_restore",) if what == "whole" else ("region",) if what == "restore" else ()
        return True
