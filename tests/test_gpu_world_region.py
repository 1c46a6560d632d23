"""Box-shaped strokes of a resident world on the GPU (World.fill_box, World.restore_box): a fill or clear
leaves the world as edit(box_records(...)) would, download for download; a restore leaves the snapshot's
content inside the box and the current content outside it; both cost what ort.box_cubes counts.

The truth never comes from the code under test: the CPU path ort.edit_voxels(pool, ort.box_records(lo, hi,
id), use_gpu=False), or a numpy composition of dense grids built with build_voxels(use_gpu=False).
Store ids differ from run to run (claim order): only downloads, grids, stats and frames are compared."""
import numpy as np
import pytest

from test_gpu_world import BRUSH_POS, BRUSH_VIEW, check_frame, oracle_frame
from test_voxel_builder import CASES, random_records, same_build

pytestmark = pytest.mark.gpu

IDS = [1, 0, 255, 0xFFFFFFFF]
SMALL = sorted(name for name, (depth, _) in CASES.items() if depth <= 5) + ["n257_d7", "empty_d4", "empty_d5"]
EMPTY = np.zeros((0, 4), np.uint32)


def case(name):
    return (int(name[-1]), EMPTY) if name.startswith("empty") else CASES[name]


def empty_world(ort, depth, capacity=20_000):
    return ort.World((np.zeros((0, 8), np.uint32), 0, depth), capacity=capacity)


def clip(lo, hi, depth):
    lo = np.maximum(np.asarray(lo, np.int64), 0)
    hi = np.minimum(np.asarray(hi, np.int64), 1 << depth)
    return (lo, hi) if (lo < hi).all() else (np.zeros(3, np.int64), np.zeros(3, np.int64))


def boxes_of(depth, seed):
    """Seeded boxes of every kind the issue names; sides stay at or below 40 so that a record list of each fits."""
    n, rng = 1 << depth, np.random.default_rng(seed)
    q = max(n // 4, 1)
    side = lambda: rng.integers(1, min(n, 40) + 1, 3)
    interior = rng.integers(0, q + 1, 3) + 1 if n > 2 else np.zeros(3, np.int64)
    face = rng.integers(0, n // 2 + 1, 3)
    face[rng.integers(0, 3)] = 0
    p = rng.integers(0, n, 3)
    cube = rng.integers(0, 2, 3) * (n // 2)
    out = [
        ("interior", interior, np.minimum(interior + side(), n - 1)),
        ("face", face, np.minimum(face + side(), n)),
        ("overhang", np.array([-3, n // 2 - 1, -1]), np.array([n // 2 + 1, n + 5, min(n, 3)])),
        ("one voxel", p, p + 1),
        ("aligned cube", cube, cube + n // 2),
        ("empty", p, p * np.array([1, 1, 1]) + np.array([3, 0, 2])),
        ("outside", np.array([n, 0, 0]), np.array([n + 4, 4, 4])),
    ]
    if depth <= 5:
        out += [("whole", np.zeros(3, np.int64), np.full(3, n)), ("whole and more", np.full(3, -2), np.full(3, n + 1))]
    return [(kind, tuple(int(v) for v in lo), tuple(int(v) for v in np.maximum(hi, lo))) for kind, lo, hi in out]


def truth_fill(ort, tree, lo, hi, id):
    return ort.edit_voxels(tree, ort.box_records(lo, hi, id), use_gpu=False)


def whole_grid(pool):
    return pool.read_box((0, 0, 0), (1 << pool.depth,) * 3, np.uint32)


def check_reads(world, truth, lo, hi, seed):
    """at and read_box before any flush, around the box and over the whole tree where that is small."""
    n = 1 << truth.depth
    if truth.depth <= 5:
        rlo, rhi = (-1, 0, -2), (n + 1, n, n + 2)
    else:
        rlo, rhi = tuple(max(v - 2, -1) for v in lo), tuple(min(v + 2, n + 1) for v in hi)
    want = truth.read_box(rlo, rhi, np.uint32)
    assert np.array_equal(world.read_box(rlo, rhi, np.uint32), want)
    rng = np.random.default_rng(seed)
    coords = np.concatenate([rng.integers(-1, n + 1, (64, 3)), rng.integers(np.array(rlo), np.maximum(rhi, np.array(rlo) + 1), (64, 3))])
    inside = ((coords >= 0) & (coords < n)).all(1)
    want_at = np.zeros(len(coords), np.uint32)
    whole = truth.read_box((0, 0, 0), (n,) * 3, np.uint32) if truth.depth <= 5 else None
    for i in np.nonzero(inside)[0]:
        x, y, z = (int(v) for v in coords[i])
        want_at[i] = whole[z, y, x] if whole is not None else truth.at(x, y, z)
    assert np.array_equal(world.at(coords), want_at)


def check_stats(ort, st, lo, hi, depth):
    keys, heights, cubes, cells = ort.box_cubes(lo, hi, depth)
    clo, chi = clip(lo, hi, depth)
    assert (st["cubes"], st["cells"]) == (len(keys), int(cells.sum())), (st, lo, hi)
    assert st["lo"] == tuple(clo.tolist()) and st["hi"] == tuple(chi.tolist())


# ------------------------------------------------------------ 1. a fill equals the record stroke

@pytest.mark.parametrize("name", SMALL)
def test_fill_equals_the_record_stroke(ort, gpu_device, name):
    depth, rec = case(name)
    truth = ort.build_voxels(rec, depth=depth)
    shift = len(name)
    with ort.World(truth, capacity=200_000) as world:
        for i, (kind, lo, hi) in enumerate(boxes_of(depth, shift)):
            for id in (IDS[(i + shift) % 4], IDS[(i + shift + 1) % 4]):
                strokes, used = world.info()["strokes"], world.info()["used"]
                st = world.fill_box(lo, hi, id)
                truth = truth_fill(ort, truth, lo, hi, id)
                info = world.info()
                assert info["strokes"] == strokes + 1 and st["new_ids"] == info["used"] - used, (kind, id)
                check_stats(ort, st, lo, hi, depth)
                check_reads(world, truth, lo, hi, i)
                same_build(world.download(), truth)
                if truth.root:
                    tlo, thi = ort.occupied_box(truth.nodes, truth.root, depth)
                    assert all(a <= b for a, b in zip(info["box_lo"], tlo)) and all(a >= b for a, b in zip(info["box_hi"], thi))
                # the store finds every row the fill made: the record stroke of the same box needs no id
                world.edit(ort.box_records(lo, hi, id))
                assert world.info()["used"] == info["used"] and world.info()["root"] == info["root"], (kind, id)


def test_fill_with_a_null_stats_pointer(ort, gpu_device):
    import ctypes as C
    with empty_world(ort, 4) as world:
        lo, hi = (C.c_int32 * 3)(1, 2, 3), (C.c_int32 * 3)(9, 9, 9)
        assert ort.load().och_world_fill_box(world._h, lo, hi, 5, None) == 0
        same_build(world.download(), truth_fill(ort, ort.build_voxels(EMPTY, depth=4), (1, 2, 3), (9, 9, 9), 5))
        s = world.snapshot()
        world.fill_box((0, 0, 0), (4, 4, 4), 0)
        assert ort.load().och_world_restore_box(world._h, s, lo, hi, None) == 0


# ------------------------------------------------------------ 2. wavefront and workgroup edges

EDGES = [(4, 63, (4, 5, 9), (13, 13, 13)), (4, 64, (5, 8, 6), (13, 15, 15)), (4, 65, (5, 4, 3), (13, 14, 12)),
         (5, 255, (6, 13, 4), (23, 21, 25)), (5, 256, (1, 3, 15), (31, 17, 17)), (5, 257, (4, 5, 1), (17, 29, 9))]


@pytest.mark.parametrize("depth,front,lo,hi", EDGES)
def test_wave_and_block_edges(ort, gpu_device, depth, front, lo, hi):
    assert int(ort.box_cubes(lo, hi, depth)[3][1]) == front           # the frontier at height 1
    base = ort.build_voxels(random_records(front, 6000, depth), depth=depth)
    with ort.World(base, capacity=100_000) as world:
        s = world.snapshot()
        truth = base
        for id in (3, 0):
            st = world.fill_box(lo, hi, id)
            check_stats(ort, st, lo, hi, depth)
            truth = truth_fill(ort, truth, lo, hi, id)
            same_build(world.download(), truth)
        world.fill_box((0, 0, 0), (2, 2, 2), 9)                       # something outside the box stays
        truth = truth_fill(ort, truth, (0, 0, 0), (2, 2, 2), 9)
        st = world.restore_box(s, lo, hi)
        want = whole_grid(truth)
        before = whole_grid(base)
        want[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = before[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        same_build(world.download(), ort.build_voxels(want, use_gpu=False))
        assert st["cubes"] > 0 and st["cells"] > 0


# ------------------------------------------------------------ 3. restore

def differing(depth, lo, hi, a, b):
    """(cubes, cells) of a restore from the grids: the maximal cubes inside the box whose content differs
    and the straddling cells whose content inside the box differs."""
    lo, hi = clip(lo, hi, depth)
    differ = a != b
    out = [0, 0]

    def visit(o, H):
        s = 1 << H
        if any(o[i] >= hi[i] or o[i] + s <= lo[i] for i in range(3)):
            return
        clo = [max(o[i], int(lo[i])) for i in range(3)]
        chi = [min(o[i] + s, int(hi[i])) for i in range(3)]
        if not differ[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]].any():
            return
        if all(lo[i] <= o[i] and o[i] + s <= hi[i] for i in range(3)):
            out[0] += 1
            return
        out[1] += 1
        for k in range(8):
            visit((o[0] + (k & 1) * s // 2, o[1] + ((k >> 1) & 1) * s // 2, o[2] + ((k >> 2) & 1) * s // 2), H - 1)

    if (lo < hi).all():
        visit((0, 0, 0), depth)
    return tuple(out)


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_restore_is_the_composition(ort, gpu_device, depth):
    n = 1 << depth
    base = ort.build_voxels(random_records(depth, 40 * n, depth), depth=depth)
    stroke_a = random_records(depth + 50, 10 * n, depth, ids=(8, 12), remove=0.4)
    stroke_a[:, :3] = stroke_a[:, :3] % np.array([n, n, n // 2], np.uint32)          # the top half stays untouched
    fill_lo, fill_hi = (1, n // 4, 0), (n // 2 + 1, n // 2 + 3, n // 2)
    with ort.World(base, capacity=200_000) as world:
        s = world.snapshot()
        old, old_root = whole_grid(base), world.info()["root"]
        world.edit(stroke_a)
        world.fill_box(fill_lo, fill_hi, 77)
        after = world.snapshot()
        now = whole_grid(truth_fill(ort, ort.edit_voxels(base, stroke_a, use_gpu=False), fill_lo, fill_hi, 77))
        assert (now[n // 2:] == old[n // 2:]).all() and (now != old).sum() > n
        for kind, lo, hi in boxes_of(depth, 7 + depth):
            world.checkout(after)
            used, root = world.info()["used"], world.info()["root"]
            st = world.restore_box(s, lo, hi)
            clo, chi = clip(lo, hi, depth)
            want = now.copy()
            want[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]] = old[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]]
            assert np.array_equal(world.read_box((0, 0, 0), (n, n, n), np.uint32), want), kind
            same_build(world.download(), ort.build_voxels(want, use_gpu=False))
            assert (st["cubes"], st["cells"]) == differing(depth, lo, hi, old, now), (kind, lo, hi, st)
            assert st["new_ids"] == world.info()["used"] - used
            assert st["lo"] == tuple(clo.tolist()) and st["hi"] == tuple(chi.tolist())
            rec, _ = world.diff(s)
            inside = ((rec[:, :3].astype(np.int64) >= clo) & (rec[:, :3].astype(np.int64) < chi)).all(1)
            assert not inside.any(), kind                           # nothing of the box differs from s any more
            if kind.startswith("whole"):
                assert world.info()["root"] == old_root and st["cubes"] == 1 and st["cells"] == 0
            if st["cubes"] == 0:
                assert world.info()["root"] == root and st["new_ids"] == 0
        # a box the strokes never touched: no id, no cube, no cell, the same root
        world.checkout(after)
        before = world.info()
        st = world.restore_box(s, (1, 2, n // 2), (n - 1, n, n - 1))
        assert (st["cubes"], st["cells"], st["new_ids"]) == (0, 0, 0)
        info = world.info()
        assert (info["root"], info["used"], info["strokes"]) == (before["root"], before["used"], before["strokes"] + 1)
        # the current state as the snapshot changes nothing either
        assert world.restore_box(0, (0, 0, 0), (n, n, n))["cubes"] == 0 and world.info()["root"] == before["root"]
        # a restore is a stroke like any other: strokes go on from it
        world.restore_box(s, (0, 0, 0), (n // 2, n // 2, n // 2))
        world.fill_box((1, 1, 1), (3, 3, 3), 5)
        want = now.copy()
        want[:n // 2, :n // 2, :n // 2] = old[:n // 2, :n // 2, :n // 2]
        want[1:3, 1:3, 1:3] = 5
        same_build(world.download(), ort.build_voxels(want, use_gpu=False))


# ------------------------------------------------------------ 3b. a restore that outgrows its buffers

# och_world_restore_box starts with room for min(the box's cubes, 2^16) cubes and a frontier of min(the
# widest level, 2^14) cells; a level that outgrows either ends the walk, which starts over from the roots
# with larger buffers.  BIG is the smallest cube-shaped box with odd faces that does both: every count
# below is recomputed from the box by the closed forms of tests/world_model.py, held to ort.box_cubes.
BIG_DEPTH, BIG_LO, BIG_HI = 7, (1, 1, 1), (127, 127, 127)
FIRST_CUBES, FIRST_FRONT = 1 << 16, 1 << 14


def closed_forms(ort, lo, hi, depth):
    """(cubes per height, cells per height) of the box, in Python integers, held to ort.box_cubes."""
    from world_model import box_counts, clip_box
    cubes, cells, _ = box_counts(clip_box(lo, hi, depth), depth)
    _, _, want_cubes, want_cells = ort.box_cubes(lo, hi, depth)
    assert cubes == [int(v) for v in want_cubes] and cells == [int(v) for v in want_cells]
    return cubes, cells


def box_of(grid, lo, hi):
    return grid[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]


@pytest.fixture(scope="module")
def big(ort):
    """The depth-7 base (some 20 000 voxels with ids 1..5), its dense grid, and the composition that the large
    restore must leave: the base inside BIG, a shell of 9 outside it.  Built once, on the CPU, and never written to."""
    n = 1 << BIG_DEPTH
    base = ort.build_voxels(random_records(77, 20_000, BIG_DEPTH), depth=BIG_DEPTH)
    old = whole_grid(base)
    shell = np.full((n, n, n), 9, np.uint32)
    box_of(shell, BIG_LO, BIG_HI)[...] = box_of(old, BIG_LO, BIG_HI)
    for a in (old, shell):
        a.setflags(write=False)
    return base, old, shell, ort.build_voxels(shell, use_gpu=False)


def same_content(world, grid, tree=None, ort=None):
    n = grid.shape[0]
    assert np.array_equal(world.read_box((0, 0, 0), (n, n, n), np.uint32), grid)
    same_build(world.download(), tree if tree is not None else ort.build_voxels(grid, use_gpu=False))   # the CPU builder


def small_restore(world, ort, frm, grid, frm_grid):
    """A restore of a few cubes, (9, 9, 9)..(12, 12, 12): its stats against the dense grids, the new grid."""
    lo, hi = (9, 9, 9), (12, 12, 12)
    st = world.restore_box(frm, lo, hi)
    assert (st["cubes"], st["cells"]) == differing(BIG_DEPTH, lo, hi, grid, frm_grid) and st["cubes"] > 1
    grid = grid.copy()
    box_of(grid, lo, hi)[...] = box_of(frm_grid, lo, hi)
    return st, grid


def test_restore_outgrows_its_buffers(ort, gpu_device, big):
    base, old, shell, shell_tree = big
    n = 1 << BIG_DEPTH
    cubes, cells = closed_forms(ort, BIG_LO, BIG_HI, BIG_DEPTH)
    # two restarts: the frontier at height 1 outgrows its first size while the cubes above height 0 still
    # fit, then, in the second walk, the cubes of height 0 outgrow theirs
    assert cells[1] > FIRST_FRONT and sum(cubes[1:]) <= FIRST_CUBES < sum(cubes) and max(cells[2:]) <= FIRST_FRONT
    nines = np.full((n, n, n), 9, np.uint32)
    with ort.World(base, capacity=200_000) as world:
        s = world.snapshot()
        assert world.fill_box((0, 0, 0), (n, n, n), 9)["cubes"] == 1     # every cell now differs from s
        filled = world.snapshot()
        st = world.restore_box(s, BIG_LO, BIG_HI)
        print("restore", st, "closed forms", sum(cubes), sum(cells), cubes, cells)
        assert (st["cubes"], st["cells"], st["lo"], st["hi"]) == (sum(cubes), sum(cells), BIG_LO, BIG_HI)
        same_content(world, shell, shell_tree)
        # the grown buffers are kept: a small restore, a fill, and the large restore once more without a restart
        small_st, grid = small_restore(world, ort, filled, shell, nines)
        same_content(world, grid, ort=ort)
        small_tree = world.download()
        lo, hi = (30, 31, 32), (50, 41, 45)
        check_stats(ort, world.fill_box(lo, hi, 4), lo, hi, BIG_DEPTH)
        box_of(grid, lo, hi)[...] = 4
        same_content(world, grid, ort=ort)
        world.checkout(filled)
        again = world.restore_box(s, BIG_LO, BIG_HI)
        assert {k: again[k] for k in ("cubes", "cells", "lo", "hi")} == {k: st[k] for k in ("cubes", "cells", "lo", "hi")}
        assert again["new_ids"] == 0                                     # the store holds every row of the first time
        same_content(world, shell, shell_tree)
        # pruned counts across many workgroups: only a thin slab inside the box differs from s
        world.checkout(s)
        lo, hi = (5, 5, 1), (120, 121, 3)                             # against the box's lower face, where its cubes are small
        world.fill_box(lo, hi, 9)
        now = old.copy()
        box_of(now, lo, hi)[...] = 9
        st = world.restore_box(s, BIG_LO, BIG_HI)
        want = differing(BIG_DEPTH, BIG_LO, BIG_HI, now, old)
        print("slab", st, want)
        assert (st["cubes"], st["cells"]) == want and want[0] > 10_000
        same_content(world, old, base)
    # the same small restore where nothing has grown: the same stats and download
    with ort.World(shell_tree, capacity=200_000) as world:
        a = world.snapshot()
        world.fill_box((0, 0, 0), (n, n, n), 9)
        filled = world.snapshot()
        world.checkout(a)
        fresh_st, fresh_grid = small_restore(world, ort, filled, shell, nines)
        assert {k: fresh_st[k] for k in ("cubes", "cells", "lo", "hi")} == {k: small_st[k] for k in ("cubes", "cells", "lo", "hi")}
        same_build(world.download(), small_tree)


def test_restore_outgrows_its_frontier_alone(ort, gpu_device, big):
    """BIG again, in a fresh world, where the state differs from the snapshot in one voxel of each of the
    64^3 - 62^3 = 23 816 cells of height 1 that straddle it (cells[1] of its closed forms): the frontier at
    height 1 outgrows its 2^14 cells, one restart, while the differing cubes, one of height 0 per cell, stay
    below 2^16."""
    base, old, _, _ = big
    cubes, cells = closed_forms(ort, BIG_LO, BIG_HI, BIG_DEPTH)
    c = np.stack(np.meshgrid(*[np.arange(64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    c = c[((c == 0) | (c == 63)).any(1)]                                 # the cells of height 1 that straddle BIG
    assert len(c) == cells[1] and FIRST_FRONT < len(c) <= FIRST_CUBES
    voxels = np.clip(2 * c, BIG_LO[0], BIG_HI[0] - 1)                    # one voxel of each, inside the box
    rec = np.concatenate([voxels, np.full((len(voxels), 1), 9)], 1).astype(np.uint32)
    now = old.copy()
    now[voxels[:, 2], voxels[:, 1], voxels[:, 0]] = 9
    with ort.World(base, capacity=200_000) as world:
        s = world.snapshot()
        world.edit(rec)
        assert np.array_equal(world.read_box((0, 0, 0), now.shape[::-1], np.uint32), now)
        st = world.restore_box(s, BIG_LO, BIG_HI)
        print("frontier alone", st, cells)
        assert (st["cubes"], st["cells"]) == (len(c), sum(cells)) == differing(BIG_DEPTH, BIG_LO, BIG_HI, now, old)
        same_content(world, old, base)


# ------------------------------------------------------------ 4. shallow and deep

@pytest.mark.parametrize("depth", [1, 2])
def test_shallow(ort, gpu_device, depth):
    n = 1 << depth
    base = ort.build_voxels(random_records(depth, 3 * n, depth), depth=depth)
    rng = np.random.default_rng(depth)
    with ort.World(base, capacity=10_000) as world:
        truth, s = base, world.snapshot()
        old = whole_grid(base)
        for i in range(24):
            lo = rng.integers(-1, n, 3)
            hi = lo + rng.integers(0, n + 2, 3)
            lo, hi = tuple(int(v) for v in lo), tuple(int(v) for v in hi)
            if i % 4 == 3:
                world.restore_box(s, lo, hi)
                clo, chi = clip(lo, hi, depth)
                grid = whole_grid(truth)
                grid[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]] = old[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]]
                truth = ort.build_voxels(grid, use_gpu=False)
            else:
                id = IDS[i % 4] if i % 4 != 1 else 0
                check_stats(ort, world.fill_box(lo, hi, id), lo, hi, depth)
                truth = truth_fill(ort, truth, lo, hi, id)
            same_build(world.download(), truth)


def test_deep(ort, gpu_device):
    """Depth 21, a 3-voxel world and the box of side 2^20 + 1 that straddles the centre: no record list
    could express it (2^60 voxels).  Its faces are odd on every axis, so a fill of it would rebuild 3 * 2^38
    cells, one per 2 x 2 x 2 block its faces cut: och_world_fill_box refuses it by the 2^31 rule, whatever
    the world holds.  The restore prunes by ids and does it in a handful of cells: that, then a fill and a
    clear of the aligned cube of side 2^20 in its middle, with at() on a handful of coordinates, are the
    check; the expected ids come from replaying the strokes per coordinate in Python."""
    depth, half = 21, 1 << 20
    lo, hi = (half // 2,) * 3, (half // 2 + half + 1,) * 3
    mid_lo, mid_hi = (half // 2,) * 3, (half // 2 + half,) * 3
    inside_a, inside_b, outside = (half, half + 1, half + 2), (lo[0], hi[1] - 1, half), (hi[0], half, half)
    first = {inside_a: 3, inside_b: 4, outside: 5}
    second = {inside_a: 0, inside_b: 9, outside: 6, (half + 7, half, half): 8, (half, half, hi[2]): 2}
    probe = list(first) + list(second)[3:] + [lo, (hi[0] - 1,) * 3, (lo[0] - 1, half, half), (0, 0, 0), (2 * half - 1,) * 3,
                                              mid_lo, (mid_hi[0] - 1,) * 3, (half, mid_hi[1], half), (half - 1, half, half + 12345)]
    within = lambda p, a, b: all(l <= c < u for c, l, u in zip(p, a, b))
    ops = []

    def expected():
        out = []
        for p in probe:
            v = first.get(p, 0)
            for op in ops:
                v = op(p, v)
            out.append(v)
        return out

    records = lambda d: np.array([p + (v,) for p, v in d.items()], np.uint32)
    base = ort.build_voxels(records(first), depth=depth)
    with ort.World(base, capacity=10_000) as world:
        s = world.snapshot()
        assert world.at(np.array(probe)).tolist() == expected()
        before = world.info()
        with pytest.raises(ort.OchError, match="INVALID") as e:
            world.fill_box(lo, hi, 1)
        assert e.value.status == -1 and "2^31" in str(e.value) and world.info() == before
        world.edit(records(second))
        ops.append(lambda p, v: second.get(p, v))
        assert world.at(np.array(probe)).tolist() == expected()
        st = world.restore_box(s, lo, hi)
        ops.append(lambda p, v: first.get(p, 0) if within(p, lo, hi) else v)
        got = world.at(np.array(probe)).tolist()
        assert got == expected() and got[:5] == [3, 4, 6, 0, 2]           # inside as the snapshot, outside as now
        assert 0 < st["cubes"] <= 3 and 0 < st["cells"] <= 3 * depth and st["new_ids"] <= st["cells"]
        assert st["lo"] == lo and st["hi"] == hi
        for id in (7, 0):
            keys, heights, cubes, cells = ort.box_cubes(mid_lo, mid_hi, depth)
            assert heights.tolist() == [19] * 8
            st = world.fill_box(mid_lo, mid_hi, id)
            ops.append(lambda p, v, id=id: id if within(p, mid_lo, mid_hi) else v)
            assert (st["cubes"], st["cells"]) == (8, int(cells.sum())) and st["new_ids"] <= st["cells"] + (19 if id else 0)
            assert world.at(np.array(probe)).tolist() == expected()
        left = {p: v for p, v in zip(probe, expected()) if v}
        assert len(left) == 3
        same_build(world.download(), ort.build_voxels(records(left), depth=depth))


# ------------------------------------------------------------ 5. capacity

@pytest.mark.parametrize("id", [4, 0])
def test_capacity(ort, gpu_device, id):
    depth, lo, hi = 5, (3, 5, 2), (21, 30, 19)
    base = ort.build_voxels(random_records(11, 3000, depth), depth=depth)
    keys, heights, cubes, cells = ort.box_cubes(lo, hi, depth)
    top = int(heights.max())
    bound = base.n_nodes + 1 + int(cells.sum()) + (top if id else 0)  # used + cells + T
    with ort.World(base, capacity=bound - 1) as world:
        assert world.info()["used"] == base.n_nodes + 1
        before = world.info()
        with pytest.raises(ort.OchError, match="CAPACITY") as e:
            world.fill_box(lo, hi, id)
        assert e.value.status == -6
        assert world.info() == before
        same_build(world.download(), base)
        world.fill_box((0, 0, 0), (1, 1, 1), 0)                       # still a world: a small stroke fits
    with ort.World(base, capacity=bound) as world:
        world.fill_box(lo, hi, id)
        assert world.info()["used"] <= bound
        same_build(world.download(), truth_fill(ort, base, lo, hi, id))


def test_restore_capacity(ort, gpu_device):
    depth, lo, hi = 4, (1, 1, 1), (12, 13, 11)
    base = ort.build_voxels(random_records(12, 800, depth), depth=depth)
    with ort.World(base, capacity=base.n_nodes + 1 + 40) as world:
        s = world.snapshot()
        world.fill_box((0, 0, 0), (16, 16, 16), 0)                    # the whole tree: no id
        assert world.info()["used"] == base.n_nodes + 1 and world.info()["root"] == 0
        before = world.info()
        with pytest.raises(ort.OchError, match="CAPACITY"):
            world.restore_box(s, lo, hi)                              # its frontier alone is more than 40 cells
        assert world.info() == before and world.download().root == 0
        world.restore_box(s, (0, 0, 0), (16, 16, 16))
        same_build(world.download(), base)


# ------------------------------------------------------------ 6. history and pools

@pytest.fixture(scope="module")
def terrain(ort, gpu_device):
    base = ort.build_terrain(8, use_gpu=True)
    top = max(z for z in range(256) if base.at(128, 128, z))
    return base, np.array([108, 108, top - 20])


def test_frames_follow_fills(ort, O, terrain):
    base, lo = terrain
    chain = base
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool:
        frames = [oracle_frame(ort, O, base, BRUSH_POS, BRUSH_VIEW)]
        s = world.snapshot()
        for id in (1, 0):
            chain = truth_fill(ort, chain, lo, lo + 40, id)
            world.fill_box(lo, lo + 40, id)
            world.flush(pool)
            check_frame(ort, O, pool, chain, BRUSH_POS, BRUSH_VIEW)
            frames.append(oracle_frame(ort, O, chain, BRUSH_POS, BRUSH_VIEW))
            assert (frames[-1] != frames[-2]).sum() > 50
        same_build(world.download(), chain)
        assert world.tighten() == ort.occupied_box(chain.nodes, chain.root, chain.depth)       # exact after a clear
        world.restore_box(s, lo + 10, lo + 30)
        world.flush(pool)
        back = ort.box_records(lo + 10, lo + 30, 0)                   # x fastest, then y, then z: read_box's order
        back[:, 3] = base.read_box(lo + 10, lo + 30, np.uint32).reshape(-1)
        want = ort.edit_voxels(chain, back, use_gpu=False)
        same_build(world.download(), want)
        check_frame(ort, O, pool, want, BRUSH_POS, BRUSH_VIEW)


def test_undo_stack_and_compaction(ort, gpu_device):
    depth = 5
    base = ort.build_voxels(random_records(31, 4000, depth), depth=depth)
    boxes = [((2, 3, 4), (20, 21, 19), 6), ((0, 0, 0), (32, 32, 7), 0), ((9, 9, 9), (10, 30, 31), 0xFFFFFFFF)]
    with ort.World(base, capacity=100_000) as world:
        undo = ort.UndoStack(world)
        states = [base]
        for lo, hi, id in boxes:
            world.fill_box(lo, hi, id)
            undo.push()
            states.append(truth_fill(ort, states[-1], lo, hi, id))
        for want in reversed(states[:-1]):
            assert undo.undo()
            same_build(world.download(), want)
        assert not undo.undo()
        for want in states[1:]:
            assert undo.redo()
            same_build(world.download(), want)
        used = world.info()["used"]
        world.compact()                                               # every state of the stack is live
        assert world.info()["used"] <= used and world.info()["generation"] == 1
        same_build(world.download(), states[-1])
        # handles survive the compaction: a region of the first state comes back in the new store
        st = world.restore_box(undo.entries[0], (0, 0, 0), (16, 32, 32))
        grid = whole_grid(states[-1])
        grid[:, :, :16] = whole_grid(base)[:, :, :16]
        same_build(world.download(), ort.build_voxels(grid, use_gpu=False))
        assert st["cubes"] > 0
        world.fill_box((0, 0, 0), (32, 32, 32), 2)                    # after a compaction the uniform rows are new again
        same_build(world.download(), ort.build_voxels(np.full((32, 32, 32), 2, np.uint32), use_gpu=False))


# ------------------------------------------------------------ 7. guards

def test_guards(ort, gpu_device):
    depth = 4
    base = ort.build_voxels(random_records(3, 500, depth), depth=depth)
    with ort.World(base, capacity=10_000) as world, ort.World(base, capacity=10_000) as other:
        s = world.snapshot()
        theirs = [other.snapshot() for _ in range(3)][-1]             # handle 3: this world has only 1
        before = world.info()
        for bad in (theirs, 99):
            with pytest.raises(ort.OchError, match="INVALID") as e:
                world.restore_box(bad, (0, 0, 0), (4, 4, 4))
            assert e.value.status == -1 and "snapshot" in str(e.value)
        world.release(s)
        with pytest.raises(ort.OchError, match="INVALID"):
            world.restore_box(s, (0, 0, 0), (4, 4, 4))
        for lo, hi in (((0.5, 0, 0), (4, 4, 4)), ((0, 0, 0), (4, 2.0, 4)), ((0, 0), (4, 4)), ((3, 3, 3), (4, 2, 4)),
                       ((0, 0, 0), (1 << 31, 1, 1))):
            with pytest.raises(ValueError):
                world.fill_box(lo, hi, 1)
            with pytest.raises(ValueError):
                world.restore_box(0, lo, hi)
        for id in (-1, 1 << 32, 1.0, True):
            with pytest.raises(ValueError):
                world.fill_box((0, 0, 0), (4, 4, 4), id)
        with pytest.raises(ValueError):
            world.restore_box("1", (0, 0, 0), (4, 4, 4))
        assert world.info() == before
        same_build(world.download(), base)
    for call in (lambda: world.fill_box((0, 0, 0), (4, 4, 4), 1), lambda: world.restore_box(0, (0, 0, 0), (4, 4, 4))):
        with pytest.raises(ValueError, match="closed"):
            call()
