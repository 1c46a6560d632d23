"""Conditional strokes of a resident world on the GPU (World.paint_box, World.paint_sphere): inside the
shape a voxel v becomes id where pred(v) holds and stays otherwise, as edit(select_records(...)) of the
pre-stroke grid would leave the world, download for download, at the cost tests/world_paint_model.py
counts from the header's definitions.

The truth never comes from the code under test: whole_grid of the CPU pool, a numpy np.where with the
ball's inequality (test_sphere_cubes_host.ball_grid) or a box slice and the predicate, then
build_voxels(use_gpu=False); or edit_voxels(tree, select_records(...), use_gpu=False).  Store ids differ
from run to run: only downloads, grids, stats and frames are compared."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_world import BRUSH_POS, BRUSH_VIEW, check_frame, oracle_of
from test_gpu_world_region import EMPTY, boxes_of, case, clip, empty_world, terrain, whole_grid  # noqa: F401
from test_gpu_world_sphere import BIG_C2, BIG_D, BIG_DEPTH, EDGES, SMALL, axis_box, balls_of, big_ball, device_grid  # noqa: F401
from test_pool_diff_host import check_equal, truth_of_lists
from test_sphere_cubes_host import ball_grid
from test_voxel_builder import random_records, same_build
from world_paint_model import WHEN_IS, WHEN_IS_NOT, ball_classifier, box_classifier, paint_counts, paint_detail, painted, pred

pytestmark = pytest.mark.gpu


def box_grid(lo, hi, depth):
    n = 1 << depth
    clo, chi = clip(lo, hi, depth)
    mask = np.zeros((n, n, n), bool)
    mask[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]] = True
    return mask


def shape_of(kind, a, b, depth):
    """(mask, classifier, clipped axis box) of a ball (centre2, diameter) or a box (lo, hi)."""
    if kind == "ball":
        return ball_grid(a, b, depth), ball_classifier(a, b), axis_box(a, b, depth)
    clo, chi = clip(a, b, depth)
    return box_grid(a, b, depth), box_classifier(a, b), (tuple(clo.tolist()), tuple(chi.tolist()))


def paint(world, kind, a, b, id, when, match):
    return world.paint_sphere(a, b, id, when, match) if kind == "ball" else world.paint_box(a, b, id, when, match)


def absent_id(grid):
    have = set(np.unique(grid).tolist())
    return next(v for v in range(2, 1000) if v not in have)


def stroke_and_check(ort, world, grid, kind, a, b, id, when, match, label=""):
    """One stroke held to everything the header promises; returns (the grid after it, the stats)."""
    depth = world.depth
    mask, classify, (lo, hi) = shape_of(kind, a, b, depth)
    cubes, cells, nodes, T = paint_counts(grid, classify, when, match, id)
    before = world.info()
    st = paint(world, kind, a, b, id, when, match)
    info = world.info()
    what = (label, kind, a, b, id, when, match, st)
    assert (st["cubes"], st["cells"], st["nodes"]) == (cubes, cells, nodes), (what, (cubes, cells, nodes, T))
    assert (st["lo"], st["hi"]) == (lo, hi), what
    assert info["strokes"] == before["strokes"] + 1 and st["new_ids"] == info["used"] - before["used"], what
    assert st["new_ids"] <= cells + nodes + T, what
    after = painted(grid, mask, when, match, id)
    if not cubes:
        assert {**info, "strokes": 0} == {**before, "strokes": 0} and np.array_equal(after, grid), what
    if pred(when, match, 0) and id and cubes:                          # the box grows by the clipped (axis) box
        assert all(p <= q for p, q in zip(info["box_lo"], lo)) and all(p >= q for p, q in zip(info["box_hi"], hi)), what
    else:
        assert (info["box_lo"], info["box_hi"]) == (before["box_lo"], before["box_hi"]), what
    same_build(world.download(), ort.build_voxels(after, use_gpu=False))
    # the store finds every row the stroke made: the record stroke needs no id and leaves the root where it is
    rec = ort.select_records(grid, (0, 0, 0), id, when, match, mask=mask)
    world.edit(rec)
    assert world.info()["used"] == info["used"] and world.info()["root"] == info["root"], what
    return after, st


def uses_of(grid, rng):
    """The five named uses, match and id from the grid's own ids and one it does not hold."""
    have = [v for v in np.unique(grid).tolist() if v] or [1]
    new = absent_id(grid)
    m, n = int(rng.choice(have)), int(rng.choice(have + [new]))
    return [(WHEN_IS_NOT, 0, n), (WHEN_IS, 0, int(rng.choice(have))), (WHEN_IS, m, new), (WHEN_IS, m, 0), (WHEN_IS_NOT, m, 0),
            (WHEN_IS, new, 5)]


# ------------------------------------------------------------ 1. a paint equals the record stroke

@pytest.mark.parametrize("name", SMALL)
def test_paint_equals_the_record_stroke(ort, gpu_device, name):
    depth, rec = case(name)
    tree = ort.build_voxels(rec, depth=depth)
    grid = whole_grid(tree)
    shift, rng = len(name), np.random.default_rng(len(name))
    shapes = [("ball", k, c2, d) for k, c2, d in balls_of(depth, shift)] + [("box", k, lo, hi) for k, lo, hi in boxes_of(depth, shift)]
    with ort.World(tree, capacity=200_000) as world:
        for i, (kind, label, a, b) in enumerate(shapes):
            uses = uses_of(grid, rng)
            for u in (i + shift, i + shift + 2):
                when, match, id = uses[u % 6]
                grid, st = stroke_and_check(ort, world, grid, kind, a, b, id, when, match, label)
                if label.startswith("whole") and st["cubes"]:
                    assert (st["cubes"], st["cells"]) == (1, 0)
            if i % 4 == 3:                                             # keep the world from emptying out
                extra = random_records(i + shift, 30, depth, ids=(1, 4))
                world.edit(extra)
                tree = ort.edit_voxels(ort.build_voxels(grid, use_gpu=False), extra, use_gpu=False)
                grid = whole_grid(tree)


def test_null_stats_and_guards(ort, gpu_device):
    base = ort.build_voxels(random_records(3, 500, 4), depth=4)
    grid = whole_grid(base)
    with ort.World(base, capacity=10_000) as world:
        lib = ort.load()
        lo, hi, c2 = (C.c_int32 * 3)(1, 2, 3), (C.c_int32 * 3)(9, 9, 9), (C.c_int32 * 3)(15, 17, 16)
        assert lib.och_world_paint_box(world._h, lo, hi, WHEN_IS_NOT, 0, 9, None) == 0
        grid = painted(grid, box_grid((1, 2, 3), (9, 9, 9), 4), WHEN_IS_NOT, 0, 9)
        assert lib.och_world_paint_sphere(world._h, c2, 9, WHEN_IS, 0, 8, None) == 0
        grid = painted(grid, ball_grid((15, 17, 16), 9, 4), WHEN_IS, 0, 8)
        same_build(world.download(), ort.build_voxels(grid, use_gpu=False))
        before = world.info()
        for when in (2, -1):
            assert lib.och_world_paint_box(world._h, lo, hi, when, 0, 9, None) == -1
            assert lib.och_world_paint_sphere(world._h, c2, 9, when, 0, 9, None) == -1
        assert lib.och_world_paint_sphere(world._h, (C.c_int32 * 3)((1 << 24) + 1, 0, 0), 4, 0, 0, 1, None) == -1
        assert lib.och_world_paint_sphere(world._h, c2, (1 << 24) + 1, 0, 0, 1, None) == -1
        assert lib.och_world_paint_box(world._h, None, hi, 0, 0, 1, None) == -1
        for bad in (dict(id=-1), dict(id=1.0), dict(id=True), dict(match=1 << 32), dict(match=2.0), dict(when=2), dict(when=True),
                    dict(when=None)):
            with pytest.raises(ValueError):
                world.paint_box((0, 0, 0), (4, 4, 4), **{"id": 1, **bad})
            with pytest.raises(ValueError):
                world.paint_sphere((8, 8, 8), 4, **{"id": 1, **bad})
        for c2_, d in (((0.5, 0, 0), 4), ((0, 0), 4), ((3, 3, 3), -1), (((1 << 24) + 1, 0, 0), 4), ((0, 0, 0), True)):
            with pytest.raises(ValueError):
                world.paint_sphere(c2_, d, 1)
        assert world.info() == before
        # the defaults paint: the solid voxels, nothing else
        world.paint_sphere((16, 16, 16), 40, 6)
        same_build(world.download(), ort.build_voxels(np.where(grid != 0, 6, 0).astype(np.uint32), use_gpu=False))
    with pytest.raises(ValueError, match="closed"):
        world.paint_box((0, 0, 0), (4, 4, 4), 1)


# ------------------------------------------------------------ 2. memoisation is real

def test_tiles_are_mapped_once(ort, gpu_device):
    """One 4^3 block of random ids tiled over a depth-5 world: under the ball there are hundreds of cubes
    and a handful of distinct nodes, and the stroke maps the handful."""
    depth, c2, d = 5, (32, 32, 32), 29
    tile = np.random.default_rng(2).integers(1, 6, (4, 4, 4)).astype(np.uint32)
    grid = np.tile(tile, (8, 8, 8))
    detail = paint_detail(grid, ball_classifier(c2, d), WHEN_IS_NOT, 0, 9)
    nodes = sum(detail["nodes_per_height"])
    assert nodes * 4 <= detail["cubes"] and sum(detail["cubes_per_height"][1:]) > 4 * nodes, detail
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=50_000) as world:
        grid, st = stroke_and_check(ort, world, grid, "ball", c2, d, 9, WHEN_IS_NOT, 0)
        assert st["nodes"] == nodes
        grid, st = stroke_and_check(ort, world, grid, "ball", c2, d, 2, WHEN_IS, 9)
        assert st["nodes"] * 4 <= st["cubes"]


# ------------------------------------------------------------ 3. many rows collapse to one

def test_every_row_collapses_to_one(ort, gpu_device):
    depth, n = 4, 16
    grid = np.random.default_rng(4).integers(1, 201, (n, n, n)).astype(np.uint32)
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=20_000) as world:
        st = world.paint_box((0, 0, 0), (n, n, n), 7)                  # 512 different height-1 rows, one mapped row
        assert (st["cubes"], st["cells"]) == (1, 0) and st["nodes"] == paint_counts(grid, box_classifier((0,) * 3, (n,) * 3), 1, 0, 7)[2]
        assert st["new_ids"] <= depth
        same_build(world.download(), ort.build_voxels(np.full((n, n, n), 7, np.uint32), use_gpu=False))
        st = world.paint_box((0, 0, 0), (n, n, n), 0, WHEN_IS, 7)
        assert (st["cubes"], st["nodes"], st["new_ids"]) == (1, depth, 0)
        assert world.info()["root"] == 0 and world.download().root == 0


# ------------------------------------------------------------ 4. subtrees vanish

def test_an_erased_material_takes_its_subtrees_along(ort, gpu_device):
    depth, n, m = 5, 32, 4
    rng = np.random.default_rng(6)
    grid = (rng.integers(1, 6, (n, n, n)) * (rng.random((n, n, n)) < 0.2)).astype(np.uint32)
    grid[8:16, 16:24, 0:8] = m                                         # one aligned 8^3 cube of m alone
    base = ort.build_voxels(grid, use_gpu=False)
    assert (grid == m).sum() > 600
    with ort.World(base, capacity=100_000) as world:
        for kind, a, b in (("ball", (17, 37, 23), 31), ("box", (0, 0, 0), (n, n, n))):
            grid, st = stroke_and_check(ort, world, grid, kind, a, b, 0, WHEN_IS, m)
        assert not (grid == m).any() and not world.read_box((0, 16, 8), (8, 24, 16), np.uint32).any()
        assert world.at(np.array([[3, 19, 11]]))[0] == 0
        # the cube's parent lost a child: its height-3 position is empty in the download
        tree = world.download()
        assert tree.n_nodes < base.n_nodes and not tree.read_box((0, 16, 8), (8, 24, 16)).any()


# ------------------------------------------------------------ 5. fill-under

def test_fill_under_keeps_what_is_there(ort, gpu_device):
    depth, n = 5, 32
    rng = np.random.default_rng(8)
    grid = np.zeros((n, n, n), np.uint32)
    grid[:n // 2] = rng.integers(0, 4, (n // 2, n, n)) * (rng.random((n // 2, n, n)) < 0.5)
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=100_000) as world:
        for kind, a, b in (("ball", (31, 33, 30), 27), ("box", (3, 1, 6), (30, 31, 29))):
            T = paint_counts(grid, shape_of(kind, a, b, depth)[1], WHEN_IS, 0, 9)[3]
            assert T >= 2                                              # empty cubes of height 2 and more turn uniform
            old = grid
            grid, st = stroke_and_check(ort, world, grid, kind, a, b, 9, WHEN_IS, 0)
            assert (grid[old != 0] == old[old != 0]).all() and (grid == 9).sum() > 1000
            again = paint(world, kind, a, b, 9, WHEN_IS, 0)
            assert again["new_ids"] == 0 and (again["cubes"], again["cells"]) != (0, 0)
            same_build(world.download(), ort.build_voxels(grid, use_gpu=False))


# ------------------------------------------------------------ 6. wavefront and workgroup edges

@pytest.mark.parametrize("front,c2,d", EDGES)
def test_frontier_edges(ort, gpu_device, front, c2, d):
    """The balls whose fill has a frontier of `front` cells at height 1, on a solid world: every cell is open."""
    depth, n = 5, 32
    assert int(ort.sphere_cubes(c2, d, depth)[3][1]) == front
    grid = np.random.default_rng(front).integers(1, 5, (n, n, n)).astype(np.uint32)
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=200_000) as world:
        grid, st = stroke_and_check(ort, world, grid, "ball", c2, d, 6, WHEN_IS, 2)
        grid, st = stroke_and_check(ort, world, grid, "ball", c2, d, 0, WHEN_IS_NOT, 6)
        keys, _, _, cells = ort.sphere_cubes(c2, d, depth)
        assert st["cells"] == int(cells.sum())                         # a solid world: the fill's frontier


@pytest.mark.parametrize("count", [7, 8, 9, 32, 33, 257])
def test_node_list_edges(ort, gpu_device, count):
    """`count` distinct height-1 nodes under the box: a gather thread is one child of one node, eight
    nodes a wavefront, 32 a workgroup."""
    depth, n = 5, 32
    grid = np.zeros((n, n, n), np.uint32)
    for j in range(count):                                             # block j of the 13^3 inside the box holds one voxel, id j + 1
        bx, by, bz = 1 + j % 13, 1 + j // 13 % 13, 1 + j // 169
        grid[2 * bz, 2 * by, 2 * bx] = j + 1
    lo, hi = (1, 1, 1), (31, 31, 31)
    detail = paint_detail(grid, box_classifier(lo, hi), WHEN_IS_NOT, 0, 300)
    assert detail["nodes_per_height"][1] == count
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=50_000) as world:
        grid, st = stroke_and_check(ort, world, grid, "box", lo, hi, 300, WHEN_IS_NOT, 0)
        assert st["nodes"] == sum(detail["nodes_per_height"])
        grid, st = stroke_and_check(ort, world, grid, "box", lo, hi, 301, WHEN_IS, 0)
        grid, st = stroke_and_check(ort, world, grid, "box", lo, hi, 0, WHEN_IS, 300)


# ------------------------------------------------------------ 7. outgrowing the first buffers

def test_paint_outgrows_its_first_buffers(ort, gpu_device, big_ball):
    """Depth 8: the ball of 198 422 cubes and 37 702 cells at height 1 over random voxels, three in ten
    solid, so that most of them are open: the walk's first 2^16 cubes and 2^14 cells and the map's first
    2^16 nodes all fall short, and each starts over with more."""
    n = 1 << BIG_DEPTH
    rng = np.random.default_rng(31)
    grid = (rng.integers(1, 6, (n, n, n), dtype=np.uint8) * (rng.random((n, n, n), dtype=np.float32) < 0.3)).astype(np.uint8)
    base = ort.build_voxels(grid, use_gpu=True)
    with ort.World(base, capacity=base.n_nodes + 1 + 2_000_000) as world:
        st = world.paint_sphere(BIG_C2, BIG_D, 3)
        print("paint", st)
        assert st["cubes"] > 1 << 16 and st["cells"] > 1 << 15 and st["nodes"] > 1 << 16
        assert st["new_ids"] <= st["cells"] + st["nodes"]
        want = np.where(big_ball & (grid != 0), 3, grid).astype(np.uint8)
        assert np.array_equal(device_grid(world, n), want)
        # a small stroke in the grown buffers
        small = ball_grid((100, 101, 103), 9, BIG_DEPTH)
        st = world.paint_sphere((100, 101, 103), 9, 7, WHEN_IS, 0)
        want = np.where(small & (want == 0), 7, want).astype(np.uint8)
        assert np.array_equal(device_grid(world, n), want) and 0 < st["cubes"] < 1000


# ------------------------------------------------------------ 8. capacity

@pytest.mark.parametrize("when,match,id", [(WHEN_IS_NOT, 0, 6), (WHEN_IS, 0, 6), (WHEN_IS, 2, 0)])
def test_capacity(ort, gpu_device, when, match, id):
    depth, c2, d = 5, (27, 31, 24), 21
    base = ort.build_voxels(random_records(11, 6000, depth), depth=depth)
    grid = whole_grid(base)
    cubes, cells, nodes, T = paint_counts(grid, ball_classifier(c2, d), when, match, id)
    assert cubes and nodes and (T > 0) == (when == WHEN_IS and match == 0)
    bound = base.n_nodes + 1 + cells + nodes + T
    with ort.World(base, capacity=bound - 1) as world:
        before = world.info()
        assert before["used"] == base.n_nodes + 1
        with pytest.raises(ort.OchError, match="CAPACITY") as e:
            world.paint_sphere(c2, d, id, when, match)
        assert e.value.status == -6 and world.info() == before
        same_build(world.download(), base)
    with ort.World(base, capacity=bound) as world:
        st = world.paint_sphere(c2, d, id, when, match)
        assert (st["cubes"], st["cells"], st["nodes"]) == (cubes, cells, nodes) and world.info()["used"] <= bound
        same_build(world.download(), ort.build_voxels(painted(grid, ball_grid(c2, d, depth), when, match, id), use_gpu=False))
    with ort.World(base, capacity=base.n_nodes + 1) as world:          # a full world: a stroke without a cube is never refused
        before = world.info()
        z, y, x = (int(v) for v in np.argwhere(grid)[0])                # one solid voxel: its cells are open, it is not
        st = world.paint_sphere((2 * x + 1, 2 * y + 1, 2 * z + 1), 0, 5, WHEN_IS, absent_id(grid))
        assert st["cubes"] == 0 and st["cells"] == depth and st["new_ids"] == 0
        assert world.paint_box((40, 0, 0), (44, 4, 4), 5)["cells"] == 0
        assert {**world.info(), "strokes": 0} == {**before, "strokes": 0} and world.info()["strokes"] == before["strokes"] + 2


# ------------------------------------------------------------ 9. history

def test_history(ort, gpu_device):
    depth, c2, d = 5, (30, 33, 29), 23
    base = ort.build_voxels(random_records(13, 5000, depth), depth=depth)
    grid = whole_grid(base)
    new = absent_id(grid)
    ball = ball_grid(c2, d, depth)
    with ort.World(base, capacity=100_000) as world:
        s = world.snapshot()
        world.paint_sphere(c2, d, new)
        z, y, x = np.nonzero(ball & (grid != 0))
        assert len(x) > 100
        rec = ort.select_records(grid, (0, 0, 0), new, WHEN_IS_NOT, 0, mask=ball)
        assert sorted(map(tuple, rec[:, :3].tolist())) == sorted(zip(x.tolist(), y.tolist(), z.tolist()))
        check_equal(world.diff(s), truth_of_lists(depth, rec[:, :3], rec[:, 3]))
        world.compact()
        after = painted(grid, ball, WHEN_IS_NOT, 0, new)
        same_build(world.download(), ort.build_voxels(after, use_gpu=False))
        st = world.paint_box((2, 3, 4), (20, 21, 22), 0, WHEN_IS, new)   # a stroke on the compacted store
        after = painted(after, box_grid((2, 3, 4), (20, 21, 22), depth), WHEN_IS, new, 0)
        assert st["cubes"] == paint_counts(painted(grid, ball, WHEN_IS_NOT, 0, new), box_classifier((2, 3, 4), (20, 21, 22)), WHEN_IS, new, 0)[0]
        same_build(world.download(), ort.build_voxels(after, use_gpu=False))
        world.restore_sphere(s, (32, 32, 32), 64)
        same_build(world.download(), base)
        world.paint_sphere(c2, d, new)
        world.restore_sphere(s, c2, d)
        same_build(world.download(), base)


# ------------------------------------------------------------ 10. frames

def test_frames_follow_a_paint(ort, O, terrain):
    base, lo = terrain
    centre = lo + 20
    c2 = tuple(int(v) for v in 2 * centre)
    blo, bhi = axis_box(c2, 40, base.depth)
    box = base.read_box(blo, bhi, np.uint32)
    g = [2 * np.arange(blo[a], bhi[a], dtype=np.int64) + 1 - c2[a] for a in range(3)]
    ball = g[2][:, None, None] ** 2 + g[1][None, :, None] ** 2 + g[0][None, None, :] ** 2 <= 40 * 40
    id = 1 if np.bincount(box[ball & (box != 0)]).argmax() != 1 else 2
    truth = ort.edit_voxels(base, ort.select_records(box, blo, id, WHEN_IS_NOT, 0, mask=ball), use_gpu=False)

    def hits(tree):
        ref, rcp = oracle_of(ort, O, tree)
        from test_gpu_world import H, W
        return O.trace_batch(ref, rcp, np.asarray(BRUSH_POS, np.float32), O.raygen(*BRUSH_VIEW, W, H))["voxel"]
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool:
        st = world.paint_sphere(c2, 40, id)
        assert st["cubes"] > 0
        world.flush(pool)
        check_frame(ort, O, pool, truth, BRUSH_POS, BRUSH_VIEW)
        same_build(world.download(), truth)
    plain, painted_hits = hits(base), hits(truth)
    assert (plain != painted_hits).sum() > 10                          # the paint shows
    assert np.array_equal(plain == 0, painted_hits == 0) and (plain == 0).sum() == (painted_hits == 0).sum()   # the silhouette stays


# ------------------------------------------------------------ 11. a short seeded random walk

def test_random_walk(ort, gpu_device):
    depth, n = 4, 16
    rng = np.random.default_rng(11)
    grid = whole_grid(ort.build_voxels(random_records(5, 600, depth), depth=depth))
    saved = []
    with ort.World(ort.build_voxels(grid, use_gpu=False), capacity=60_000) as world:
        for step in range(60):
            op = int(rng.integers(0, 9))
            c2, d = tuple(int(v) for v in rng.integers(0, 2 * n, 3)), int(rng.integers(0, n + 8))
            lo = rng.integers(-2, n, 3)
            hi = tuple(int(v) for v in lo + rng.integers(0, n, 3))
            lo = tuple(int(v) for v in lo)
            id, when, match = int(rng.integers(0, 5)), int(rng.integers(0, 2)), int(rng.integers(0, 5))
            if op <= 1:
                world.paint_sphere(c2, d, id, when, match)
                grid = painted(grid, ball_grid(c2, d, depth), when, match, id)
            elif op <= 3:
                world.paint_box(lo, hi, id, when, match)
                grid = painted(grid, box_grid(lo, hi, depth), when, match, id)
            elif op == 4:
                rec = random_records(step, 40, depth, ids=(1, 5), dup=0.0)
                world.edit(rec)
                grid[rec[:, 2], rec[:, 1], rec[:, 0]] = rec[:, 3]
            elif op == 5:
                if step % 2:
                    world.fill_sphere(c2, d, id)
                    grid = np.where(ball_grid(c2, d, depth), np.uint32(id), grid)
                else:
                    world.fill_box(lo, hi, id)
                    grid = np.where(box_grid(lo, hi, depth), np.uint32(id), grid)
            elif op == 6:
                saved.append((world.snapshot(), grid.copy()))
            elif op == 7 and saved:
                s, then = saved[int(rng.integers(0, len(saved)))]
                if step % 3 == 0:
                    world.checkout(s)
                    grid = then.copy()
                elif step % 3 == 1:
                    world.restore_sphere(s, c2, d)
                    grid = np.where(ball_grid(c2, d, depth), then, grid)
                else:
                    world.restore_box(s, lo, hi)
                    grid = np.where(box_grid(lo, hi, depth), then, grid)
            elif op == 8:
                world.compact()
            if step % 5 == 4:
                same_build(world.download(), ort.build_voxels(grid.astype(np.uint32), use_gpu=False))
        same_build(world.download(), ort.build_voxels(grid.astype(np.uint32), use_gpu=False))
