"""Sphere strokes of a resident world on the GPU (World.fill_sphere, World.restore_sphere): a fill or clear
leaves the world as edit(sphere_records(...)) would, download for download; a restore leaves the
snapshot's content inside the ball and the current content outside it; a fill costs what
ort.sphere_cubes counts, a restore what differs.

The truth never comes from the code under test: the CPU path ort.edit_voxels(pool,
ort.sphere_records(...), use_gpu=False), or a numpy composition of dense grids (the ball is the
inequality of include/och_gpu.h over a grid, test_sphere_cubes_host.ball_grid) built with
build_voxels(use_gpu=False).  Store ids differ from run to run: only downloads, grids, stats and frames
are compared."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_world import BRUSH_POS, BRUSH_VIEW, check_frame, oracle_frame
from test_gpu_world_region import EMPTY, IDS, case, check_reads, empty_world, same_content, terrain, whole_grid  # noqa: F401
from test_sphere_cubes_host import ball_grid, classify
from test_voxel_builder import CASES, random_records, same_build

pytestmark = pytest.mark.gpu

SMALL = sorted(name for name, (depth, _) in CASES.items() if depth <= 5) + ["empty_d4"]
# what och_world_fill_sphere and och_world_restore_sphere start with, at most (och_world_region.h)
FILL_CUBES, FILL_FRONT, RESTORE_CUBES, RESTORE_FRONT = 1 << 17, 1 << 15, 1 << 16, 1 << 14


def axis_box(c2, d, depth):
    """The ball's axis box clipped to the tree, all 0 where that is empty."""
    n = 1 << depth
    lo = [min(max(-((d + 1 - c) // 2), 0), n) for c in c2]
    hi = [min(max((c + d - 1) // 2 + 1, 0), n) for c in c2]
    return (tuple(lo), tuple(hi)) if all(l < h for l, h in zip(lo, hi)) else ((0, 0, 0), (0, 0, 0))


def balls_of(depth, seed):
    """Seeded balls of every kind: centres of every parity, on and off the tree's faces, diameters from 0 to
    overhanging and whole-tree; diameters stay at or below 40 so that a record list of each is small."""
    n, rng = 1 << depth, np.random.default_rng(seed)
    mid = rng.integers(n // 2, 3 * n // 2 + 1, 3)
    p = rng.integers(0, n, 3)
    on_face = rng.integers(2, 2 * n - 1, 3)
    on_face[rng.integers(0, 3)] = 0
    out = [
        ("interior", mid, int(rng.integers(2, max(n // 2, 3)))),
        ("interior, odd", mid | 1, int(rng.integers(2, max(n // 2, 3))) | 1),
        ("mixed parity", (mid & ~1) + np.array([0, 1, 0]), min(n, 9)),
        ("on a face", on_face, min(n, 12)),
        ("on a corner", np.array([2 * n, 0, 2 * n]), min(n + 1, 17)),
        ("overhang", np.array([-3, n, 2 * n + 2]), min(2 * n, 40)),
        ("one voxel", 2 * p + 1, 0),
        ("eight voxels", 2 * p, 2),
        ("no voxel", 2 * p + np.array([1, 0, 1]), 0),
        ("outside", np.array([2 * n + 9, n, n]), 7),
    ]
    if depth <= 4:
        out += [("whole", np.full(3, n), 2 * n), ("whole, off centre", np.array([n + 1, n - 1, n]), 40)]
    return [(kind, tuple(int(v) for v in c2), int(d)) for kind, c2, d in out]


def truth_fill(ort, tree, c2, d, id):
    return ort.edit_voxels(tree, ort.sphere_records(c2, d, id), use_gpu=False)


def check_stats(ort, st, c2, d, depth):
    keys, heights, cubes, cells = ort.sphere_cubes(c2, d, depth)
    assert (st["cubes"], st["cells"]) == (len(keys), int(cells.sum())), (st, c2, d)
    assert (st["lo"], st["hi"]) == axis_box(c2, d, depth), (st, c2, d)
    return keys, heights, cubes, cells


def differing(depth, c2, d, a, b):
    """(cubes, cells) of a restore from the grids: the maximal cubes inside the ball whose content differs
    and the straddling cells whose content inside the ball differs."""
    differ = (a != b) & ball_grid(c2, d, depth)
    out = [0, 0]

    def visit(o, H):
        s = 1 << H
        c = classify(c2, d, o, H)
        if not c or not differ[o[2]:o[2] + s, o[1]:o[1] + s, o[0]:o[0] + s].any():
            return
        if c == 2:
            out[0] += 1
            return
        out[1] += 1
        for k in range(8):
            visit((o[0] + (k & 1) * s // 2, o[1] + ((k >> 1) & 1) * s // 2, o[2] + ((k >> 2) & 1) * s // 2), H - 1)

    visit((0, 0, 0), depth)
    return tuple(out)


# ------------------------------------------------------------ 1. a fill equals the record stroke

@pytest.mark.parametrize("name", SMALL)
def test_fill_equals_the_record_stroke(ort, gpu_device, name):
    depth, rec = case(name)
    truth = ort.build_voxels(rec, depth=depth)
    shift = len(name)
    with ort.World(truth, capacity=200_000) as world:
        for i, (kind, c2, d) in enumerate(balls_of(depth, shift)):
            for id in (IDS[(i + shift) % 4], IDS[(i + shift + 1) % 4]):
                before = world.info()
                st = world.fill_sphere(c2, d, id)
                truth = truth_fill(ort, truth, c2, d, id)
                info = world.info()
                assert info["strokes"] == before["strokes"] + 1 and st["new_ids"] == info["used"] - before["used"], (kind, id)
                keys, heights, _, _ = check_stats(ort, st, c2, d, depth)
                if not len(keys):                                     # no voxel of the ball in the tree: nothing but strokes
                    assert {**info, "strokes": 0} == {**before, "strokes": 0}, kind
                if kind.startswith("whole"):
                    assert st["cubes"] == 1 and st["cells"] == 0 and st["new_ids"] <= depth
                lo, hi = axis_box(c2, d, depth)
                check_reads(world, truth, lo, hi, i)
                same_build(world.download(), truth)
                if truth.root:
                    tlo, thi = ort.occupied_box(truth.nodes, truth.root, depth)
                    assert all(a <= b for a, b in zip(info["box_lo"], tlo)) and all(a >= b for a, b in zip(info["box_hi"], thi))
                if id and len(keys):                                  # the box grows by the clipped axis box
                    assert all(a <= b for a, b in zip(info["box_lo"], lo)) and all(a >= b for a, b in zip(info["box_hi"], hi))
                if not id:
                    assert (info["box_lo"], info["box_hi"]) == (before["box_lo"], before["box_hi"])
                # the store finds every row the fill made: the record stroke of the same ball needs no id
                world.edit(ort.sphere_records(c2, d, id))
                assert world.info()["used"] == info["used"] and world.info()["root"] == info["root"], (kind, id)


def test_null_stats_through_the_raw_call(ort, gpu_device):
    with empty_world(ort, 4) as world:
        c2 = (C.c_int32 * 3)(15, 17, 16)
        assert ort.load().och_world_fill_sphere(world._h, c2, 9, 5, None) == 0
        same_build(world.download(), truth_fill(ort, ort.build_voxels(EMPTY, depth=4), (15, 17, 16), 9, 5))
        s = world.snapshot()
        world.fill_sphere((8, 8, 8), 6, 0)
        assert ort.load().och_world_restore_sphere(world._h, s, c2, 9, None) == 0
        same_build(world.download(), truth_fill(ort, ort.build_voxels(EMPTY, depth=4), (15, 17, 16), 9, 5))


# ------------------------------------------------------------ 2. restore

@pytest.mark.parametrize("depth", [3, 4, 5])
def test_restore_is_the_composition(ort, gpu_device, depth):
    n = 1 << depth
    base = ort.build_voxels(random_records(depth, 40 * n, depth), depth=depth)
    stroke_a = random_records(depth + 50, 10 * n, depth, ids=(8, 12), remove=0.4)
    stroke_a[:, :3] = stroke_a[:, :3] % np.array([n, n, n // 2], np.uint32)          # the top half stays untouched
    fill_c2, fill_d = (n // 2 + 1, n, n // 2), n // 2 + 1
    with ort.World(base, capacity=200_000) as world:
        s = world.snapshot()
        old = whole_grid(base)
        world.edit(stroke_a)
        world.fill_sphere(fill_c2, fill_d, 77)
        after = world.snapshot()
        now = whole_grid(truth_fill(ort, ort.edit_voxels(base, stroke_a, use_gpu=False), fill_c2, fill_d, 77))
        assert (now[3 * n // 4:] == old[3 * n // 4:]).all() and (now != old).sum() > n
        for i, (kind, c2, d) in enumerate(balls_of(depth, 7 + depth)):
            if i == 3:
                world.compact()                                       # the handles survive it
            world.checkout(after)
            before = world.info()
            st = world.restore_sphere(s, c2, d)
            ball = ball_grid(c2, d, depth)
            want = np.where(ball, old, now)
            assert np.array_equal(world.read_box((0, 0, 0), (n, n, n), np.uint32), want), kind
            same_build(world.download(), ort.build_voxels(want, use_gpu=False))
            assert (st["cubes"], st["cells"]) == differing(depth, c2, d, old, now) or kind.startswith("whole"), (kind, c2, d, st)
            assert st["new_ids"] == world.info()["used"] - before["used"]
            assert (st["lo"], st["hi"]) == axis_box(c2, d, depth)
            rec, _ = world.diff(s)
            xyz = rec[:, :3].astype(np.int64)
            assert not ball[xyz[:, 2], xyz[:, 1], xyz[:, 0]].any(), kind  # nothing of the ball differs from s any more
            if kind.startswith("whole"):
                root = world.info()["root"]
                world.checkout(s)                                     # the snapshot's root itself (a compaction renumbers)
                assert world.info()["root"] == root and st["cubes"] == 1 and st["cells"] == 0 and st["new_ids"] == 0
            if st["cubes"] == 0:
                info = world.info()
                assert {**info, "strokes": 0} == {**before, "strokes": 0} and info["strokes"] == before["strokes"] + 1
        # a ball the strokes never touched, and the current state as the snapshot: nothing but strokes
        world.checkout(after)
        before = world.info()
        st = world.restore_sphere(s, (n, n, 2 * n - n // 4), n // 4)
        assert (st["cubes"], st["cells"], st["new_ids"]) == (0, 0, 0)
        assert world.restore_sphere(0, (n, n, n), 2 * n)["cubes"] == 0
        info = world.info()
        assert {**info, "strokes": 0} == {**before, "strokes": 0} and info["strokes"] == before["strokes"] + 2
        # a restore is a stroke like any other: strokes go on from it
        world.restore_sphere(s, (n // 2, n // 2, n // 2), n // 2)
        world.fill_sphere((5, 5, 5), 3, 5)
        want = np.where(ball_grid((n // 2, n // 2, n // 2), n // 2, depth), old, now)
        want[ball_grid((5, 5, 5), 3, depth)] = 5
        same_build(world.download(), ort.build_voxels(want, use_gpu=False))


# ------------------------------------------------------------ 3. strokes that outgrow their first buffers

BIG_DEPTH, BIG_C2, BIG_D = 8, (255, 257, 256), 253


@pytest.fixture(scope="module")
def big_ball():
    ball = ball_grid(BIG_C2, BIG_D, BIG_DEPTH)
    ball.setflags(write=False)
    return ball


def device_grid(world, n):
    return world.read_box((0, 0, 0), (n, n, n), np.uint8, device=True).cpu().numpy()


def test_fill_outgrows_its_first_walk(ort, gpu_device, big_ball):
    """A fill's walk launches each level with a bound of its frontier, at most 2^15 cells, and room for at
    most 2^17 cubes; this ball's frontier at height 1 and its cubes exceed both, so the host finds the
    level that was cut short in the walk's totals and walks again with more."""
    n = 1 << BIG_DEPTH
    keys, heights, cubes, cells = ort.sphere_cubes(BIG_C2, BIG_D, BIG_DEPTH)
    assert (len(keys), int(cells[1])) == (198_422, 37_702)
    assert len(keys) > FILL_CUBES and int(cells[1]) > FILL_FRONT and int(cubes[1:].sum()) <= FILL_CUBES
    with empty_world(ort, BIG_DEPTH, capacity=400_000) as world:
        st = world.fill_sphere(BIG_C2, BIG_D, 3)
        print("fill", st, cubes.tolist(), cells.tolist())
        check_stats(ort, st, BIG_C2, BIG_D, BIG_DEPTH)
        assert st["new_ids"] <= st["cells"] + int(heights.max())
        grid = np.where(big_ball, 3, 0).astype(np.uint8)
        assert np.array_equal(device_grid(world, n), grid)
        # small strokes in the grown buffers, then the large one again: every row is in the store already
        for c2, d, id in (((40, 41, 43), 9, 7), ((255, 257, 256), 11, 0), ((500, 300, 21), 30, 0xFE)):
            check_stats(ort, world.fill_sphere(c2, d, id), c2, d, BIG_DEPTH)
            grid[ball_grid(c2, d, BIG_DEPTH)] = id
        assert np.array_equal(device_grid(world, n), grid)
        world.fill_sphere((n, n, n), 2 * n, 0)
        assert world.info()["root"] == 0
        again = world.fill_sphere(BIG_C2, BIG_D, 3)
        assert (again["cubes"], again["cells"], again["new_ids"]) == (st["cubes"], st["cells"], 0)
        assert np.array_equal(device_grid(world, n), np.where(big_ball, 3, 0))


def test_restore_outgrows_its_buffers(ort, gpu_device, big_ball):
    """The same ball restored over a world that differs from the snapshot everywhere inside it: the
    restore's exact-sized walk outgrows its first 2^16 cubes and 2^14 cells and starts over."""
    n = 1 << BIG_DEPTH
    keys, heights, cubes, cells = ort.sphere_cubes(BIG_C2, BIG_D, BIG_DEPTH)
    assert len(keys) > RESTORE_CUBES and int(cells[1]) > RESTORE_FRONT
    with empty_world(ort, BIG_DEPTH, capacity=400_000) as world:
        s = world.snapshot()
        assert world.fill_sphere((n, n, n), 2 * n, 9)["cubes"] == 1
        st = world.restore_sphere(s, BIG_C2, BIG_D)
        assert (st["cubes"], st["cells"]) == (len(keys), int(cells.sum()))
        grid = np.where(big_ball, 0, 9).astype(np.uint8)
        assert np.array_equal(device_grid(world, n), grid)
        nines = world.snapshot()
        st = world.restore_sphere(nines, (100, 101, 103), 6)        # a small one in the grown buffers
        small = ball_grid((100, 101, 103), 6, BIG_DEPTH)
        assert small.sum() > 8 and (st["cubes"], st["cells"]) == differing(BIG_DEPTH, (100, 101, 103), 6, grid, np.where(small, 9, grid))
        assert np.array_equal(device_grid(world, n), np.where(small & big_ball, 9, grid))


def test_depth_7_download(ort, gpu_device):
    depth, c2, d = 7, (127, 129, 128), 125
    keys, heights, cubes, cells = ort.sphere_cubes(c2, d, depth)
    assert (len(keys), int(cells.sum())) == (47_680, 13_957)
    base = ort.build_voxels(random_records(77, 20_000, depth), depth=depth)
    ball = ball_grid(c2, d, depth)
    with ort.World(base, capacity=200_000) as world:
        s = world.snapshot()
        check_stats(ort, world.fill_sphere(c2, d, 6), c2, d, depth)
        same_content(world, np.where(ball, 6, whole_grid(base)).astype(np.uint32), ort=ort)
        check_stats(ort, world.fill_sphere(c2, d, 0), c2, d, depth)
        cut = np.where(ball, 0, whole_grid(base)).astype(np.uint32)
        same_content(world, cut, ort=ort)
        st = world.restore_sphere(s, c2, d)
        assert (st["cubes"], st["cells"]) == differing(depth, c2, d, cut, whole_grid(base))
        same_build(world.download(), base)


# ------------------------------------------------------------ 4. wavefront and workgroup edges

# A count or emit thread is one child of one cell: a wavefront holds 8 cells, a workgroup 32.
EDGES = [(7, (33, 33, 33), 3), (8, (32, 32, 32), 2), (9, (31, 33, 30), 4), (32, (32, 32, 32), 9), (256, (32, 26, 42), 21),
         (259, (31, 33, 30), 21)]


@pytest.mark.parametrize("front,c2,d", EDGES)
def test_wave_and_block_edges(ort, gpu_device, front, c2, d):
    depth = 5
    assert int(ort.sphere_cubes(c2, d, depth)[3][1]) == front        # the frontier at height 1
    base = ort.build_voxels(random_records(front, 6000, depth), depth=depth)
    with ort.World(base, capacity=100_000) as world:
        s = world.snapshot()
        truth = base
        for id in (3, 0):
            check_stats(ort, world.fill_sphere(c2, d, id), c2, d, depth)
            truth = truth_fill(ort, truth, c2, d, id)
            same_build(world.download(), truth)
        st = world.restore_sphere(s, c2, d)
        assert (st["cubes"], st["cells"]) == differing(depth, c2, d, whole_grid(truth), whole_grid(base))
        same_build(world.download(), base)


# ------------------------------------------------------------ 5. capacity

@pytest.mark.parametrize("id", [4, 0])
def test_capacity(ort, gpu_device, id):
    depth, c2, d = 5, (27, 31, 24), 21
    base = ort.build_voxels(random_records(11, 3000, depth), depth=depth)
    keys, heights, cubes, cells = ort.sphere_cubes(c2, d, depth)
    bound = base.n_nodes + 1 + int(cells.sum()) + (int(heights.max()) if id else 0)  # used + cells + T
    with ort.World(base, capacity=bound - 1) as world:
        before = world.info()
        assert before["used"] == base.n_nodes + 1
        with pytest.raises(ort.OchError, match="CAPACITY") as e:
            world.fill_sphere(c2, d, id)
        assert e.value.status == -6 and world.info() == before
        same_build(world.download(), base)
        st = world.fill_sphere((2 * (1 << depth) + 9, 3, 3), 5, id)  # nothing of it in the tree: never refused
        assert st["cubes"] == 0 and world.info()["used"] == before["used"]
        world.fill_sphere((1, 1, 1), 0, 0)                            # still a world: a small stroke fits
    with ort.World(base, capacity=bound) as world:
        world.fill_sphere(c2, d, id)
        assert world.info()["used"] <= bound
        same_build(world.download(), truth_fill(ort, base, c2, d, id))


def test_restore_capacity(ort, gpu_device):
    depth, c2, d = 4, (13, 14, 12), 11
    base = ort.build_voxels(random_records(12, 800, depth), depth=depth)
    with ort.World(base, capacity=base.n_nodes + 1 + 30) as world:
        s = world.snapshot()
        world.fill_sphere((16, 16, 16), 32, 0)                        # the whole tree: no id
        assert world.info()["used"] == base.n_nodes + 1 and world.info()["root"] == 0
        before = world.info()
        with pytest.raises(ort.OchError, match="CAPACITY"):
            world.restore_sphere(s, c2, d)                            # its frontier alone is more than 30 cells
        assert world.info() == before and world.download().root == 0
        world.restore_sphere(s, (16, 16, 16), 32)
        same_build(world.download(), base)


# ------------------------------------------------------------ 6. frames

def test_frames_follow_fills(ort, O, terrain):
    base, lo = terrain
    c2 = tuple(int(v) for v in 2 * (lo + 20))
    chain = base
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool:
        frames = [oracle_frame(ort, O, base, BRUSH_POS, BRUSH_VIEW)]
        s = world.snapshot()
        for id in (1, 0):
            chain = truth_fill(ort, chain, c2, 40, id)
            world.fill_sphere(c2, 40, id)
            world.flush(pool)
            check_frame(ort, O, pool, chain, BRUSH_POS, BRUSH_VIEW)
            frames.append(oracle_frame(ort, O, chain, BRUSH_POS, BRUSH_VIEW))
            assert (frames[-1] != frames[-2]).sum() > 10                # the ball shows in the 64 x 36 frame
        same_build(world.download(), chain)
        world.restore_sphere(s, c2, 40)
        world.flush(pool)
        want = ort.edit_voxels(base, EMPTY, use_gpu=False)              # the terrain as the voxel builders report it
        same_build(world.download(), want)
        check_frame(ort, O, pool, want, BRUSH_POS, BRUSH_VIEW)


# ------------------------------------------------------------ 7. guards

def test_guards(ort, gpu_device):
    depth = 4
    base = ort.build_voxels(random_records(3, 500, depth), depth=depth)
    with ort.World(base, capacity=10_000) as world:
        s = world.snapshot()
        before = world.info()
        with pytest.raises(ort.OchError, match="INVALID") as e:
            world.restore_sphere(99, (8, 8, 8), 4)
        assert e.value.status == -1 and "snapshot" in str(e.value)
        for c2, d in (((0.5, 0, 0), 4), ((0, 0, 0), 4.0), ((0, 0), 4), ((3, 3, 3), -1), (((1 << 24) + 1, 0, 0), 4),
                      ((0, -(1 << 24) - 1, 0), 4), ((0, 0, 0), (1 << 24) + 1), ((0, True, 0), 4), ((0, 0, 0), True)):
            with pytest.raises(ValueError):
                world.fill_sphere(c2, d, 1)
            with pytest.raises(ValueError):
                world.restore_sphere(0, c2, d)
        for id in (-1, 1 << 32, 1.0, True):
            with pytest.raises(ValueError):
                world.fill_sphere((8, 8, 8), 4, id)
        with pytest.raises(ValueError):
            world.restore_sphere("1", (8, 8, 8), 4)
        # the raw call refuses the argument range itself
        lib = ort.load()
        assert lib.och_world_fill_sphere(world._h, (C.c_int32 * 3)((1 << 24) + 1, 0, 0), 4, 1, None) == -1
        assert lib.och_world_fill_sphere(world._h, (C.c_int32 * 3)(0, 0, 0), (1 << 24) + 1, 1, None) == -1
        assert lib.och_world_restore_sphere(world._h, s, (C.c_int32 * 3)(0, 0, -(1 << 24) - 1), 4, None) == -1
        assert lib.och_world_fill_sphere(world._h, None, 4, 1, None) == -1
        assert world.info() == before
        # the range's ends are admitted: a ball far larger than the tree covers it or misses it
        assert world.fill_sphere((1 << 24, 1 << 24, 1 << 24), 1 << 24, 1)["cubes"] == 0
        assert world.fill_sphere((-(1 << 24), 0, 0), 1 << 24, 1)["cubes"] == 0
        same_build(world.download(), base)
        assert world.fill_sphere((0, 0, 0), 1 << 24, 2)["cubes"] == 1
        same_build(world.download(), ort.build_voxels(np.full((16, 16, 16), 2, np.uint32), use_gpu=False))
    for call in (lambda: world.fill_sphere((0.5, 0, 0), 4, 1), lambda: world.restore_sphere(None, (8, 8, 8), 4)):
        with pytest.raises(ValueError, match="closed"):
            call()
