"""Conditional strokes (och_world_paint_box, och_world_paint_sphere) without a GPU: the counting model the
GPU tests hold the stroke to, on grids small enough to work by hand; ort.select_records against a plain
loop; the Python side's guards; the raw entries' refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from test_world_host import closed_world
from world_paint_model import WHEN_IS, WHEN_IS_NOT, ball_classifier, box_classifier, paint_counts, painted


def grid_of(depth, voxels):
    g = np.zeros((1 << depth,) * 3, np.uint32)
    for x, y, z, v in voxels:
        g[z, y, x] = v
    return g


def test_two_cubes_share_one_node():
    """Depth 2.  Two height-1 blocks of equal content, both inside the box [0,4) x [0,2) x [0,2): the root
    cell straddles (1 cell), its children 0 and 1 are cubes (2), the other six lie outside, and the two
    cubes' words are one node of the DAG (1 node)."""
    g = np.zeros((4, 4, 4), np.uint32)
    g[0:2, 0:2, 0:2] = 5
    g[0:2, 0:2, 2:4] = 5
    g[3, 3, 3] = 1                                                       # outside the box: only keeps the root busy
    box = box_classifier((0, 0, 0), (4, 2, 2))
    assert paint_counts(g, box, WHEN_IS_NOT, 0, 9) == (2, 1, 1, 0)       # paint: nodes < cubes
    assert paint_counts(g, box, WHEN_IS, 0, 9) == (2, 1, 1, 1)           # fill-under: a node is always open; T = 1
    assert paint_counts(g, box, WHEN_IS, 5, 0) == (2, 1, 1, 0)           # erase 5: pred(0) does not hold
    g[1, 1, 3] = 6                                                       # the second block differs now
    assert paint_counts(g, box, WHEN_IS_NOT, 0, 9) == (2, 1, 2, 0)


def test_an_empty_open_cell():
    """Depth 3, one voxel at (7, 7, 7), the box [0, 3)^3.  The root cell straddles.  Of its children only
    child 0, [0, 4)^3, meets the box: it is empty and straddles, so it is open iff pred(0).  Fill-under:
    it is a cell; its child [0, 2)^3 is a cube of height 1, the other seven children straddle (7 cells)
    and hold the remaining 27 - 8 = 19 voxels of the box, all empty, all open: 20 cubes, 1 + 1 + 7 cells,
    no node, T = 1.  Paint: the empty cell is dropped, the root cell alone was expanded."""
    g = grid_of(3, [(7, 7, 7, 3)])
    box = box_classifier((0, 0, 0), (3, 3, 3))
    assert paint_counts(g, box, WHEN_IS, 0, 7) == (20, 9, 0, 1)
    assert paint_counts(g, box, WHEN_IS, 0, 0) == (20, 9, 0, 0)          # id 0: no uniform subtree
    assert paint_counts(g, box, WHEN_IS_NOT, 0, 7) == (0, 1, 0, 0)
    assert paint_counts(np.zeros((8, 8, 8), np.uint32), box, WHEN_IS_NOT, 0, 7) == (0, 0, 0, 0)   # the root cell is not open
    assert paint_counts(np.zeros((8, 8, 8), np.uint32), box, WHEN_IS, 0, 7) == (20, 9, 0, 1)


def test_a_shape_over_the_tree_is_one_cube():
    """Depth 3, voxel 1 at (0, 0, 0) and at (4, 0, 0): the two height-2 blocks that hold them are equal, and
    so are their height-1 blocks: three distinct nodes under the root cube, the root included."""
    g = grid_of(3, [(0, 0, 0, 1), (4, 0, 0, 1)])
    whole = box_classifier((-1, 0, 0), (8, 9, 8))
    assert paint_counts(g, whole, WHEN_IS, 1, 2) == (1, 0, 3, 0)
    assert paint_counts(g, whole, WHEN_IS_NOT, 1, 0) == (1, 0, 3, 0)
    assert paint_counts(g, whole, WHEN_IS_NOT, 1, 4) == (1, 0, 3, 3)     # the empty voxels turn into 4: T = depth
    g[0, 0, 5] = 2                                                       # (5, 0, 0): the second height-1 and height-2 blocks differ
    assert paint_counts(g, whole, WHEN_IS, 1, 2) == (1, 0, 5, 0)
    assert paint_counts(np.zeros((8, 8, 8), np.uint32), whole, WHEN_IS, 0, 2) == (1, 0, 0, 3)
    assert paint_counts(np.zeros((8, 8, 8), np.uint32), whole, WHEN_IS, 2, 3) == (0, 0, 0, 0)
    assert paint_counts(g, box_classifier((3, 3, 3), (6, 3, 5)), WHEN_IS, 0, 2) == (0, 0, 0, 0)   # an empty box


def test_a_voxel_is_open_by_its_own_id():
    """Depth 2, the box [1, 3)^3: eight voxels, one in each height-1 block, every block straddles.  The
    voxels hold ids 1..8; replace 3 by 9 touches one of them."""
    g = np.zeros((4, 4, 4), np.uint32)
    g[1:3, 1:3, 1:3] = np.arange(1, 9, dtype=np.uint32).reshape(2, 2, 2)
    box = box_classifier((1, 1, 1), (3, 3, 3))
    assert paint_counts(g, box, WHEN_IS, 3, 9) == (1, 9, 0, 0)
    assert paint_counts(g, box, WHEN_IS_NOT, 3, 9) == (7, 9, 0, 0)
    assert paint_counts(g, box, WHEN_IS_NOT, 0, 9) == (8, 9, 0, 0)
    assert paint_counts(g, box, WHEN_IS, 0, 9) == (0, 9, 0, 0)


@pytest.mark.parametrize("depth", [3, 4])
def test_full_and_empty_worlds_count_as_the_fill(ort, depth):
    """Where every cube is open the walk is the fill's: a solid world painted, an empty world filled under."""
    n = 1 << depth
    solid, empty = np.full((n, n, n), 4, np.uint32), np.zeros((n, n, n), np.uint32)
    rng = np.random.default_rng(depth)
    for _ in range(6):
        lo = rng.integers(-2, n, 3)
        hi = lo + rng.integers(1, n + 2, 3)
        keys, heights, cubes, cells = ort.box_cubes(lo, hi, depth)
        want = (len(keys), int(cells.sum()))
        box = box_classifier(lo, hi)
        assert paint_counts(solid, box, WHEN_IS_NOT, 0, 2)[:2] == want
        got = paint_counts(empty, box, WHEN_IS, 0, 2)
        assert got == (*want, 0, int(heights.max()) if len(keys) else 0)
        c2, d = tuple(int(v) for v in rng.integers(0, 2 * n, 3)), int(rng.integers(0, 2 * n))
        keys, heights, cubes, cells = ort.sphere_cubes(c2, d, depth)
        got = paint_counts(solid, ball_classifier(c2, d), WHEN_IS_NOT, 0, 2)
        assert got[:2] == (len(keys), int(cells.sum())) and got[3] == 0
        # a solid world of one id: one node a height, down from the greatest cube
        assert got[2] == (int(heights.max()) if len(keys) else 0)


def test_painted_is_the_predicate():
    g = np.arange(64, dtype=np.uint32).reshape(4, 4, 4) % 5
    mask = np.zeros((4, 4, 4), bool)
    mask[1:, :3, 2:] = True
    out = painted(g, mask, WHEN_IS, 3, 9)
    for z, y, x in np.ndindex(4, 4, 4):
        assert out[z, y, x] == (9 if mask[z, y, x] and g[z, y, x] == 3 else g[z, y, x])
    out = painted(g, mask, WHEN_IS_NOT, 0, 7)
    assert ((out == 7) == (mask & (g != 0)) | (g == 7)).all() and (out[~mask] == g[~mask]).all()


def test_select_records_against_a_loop(ort):
    rng = np.random.default_rng(3)
    grid = rng.integers(0, 4, (3, 5, 4)).astype(np.uint32)
    grid[0, 0, 0] = 0xFFFFFFFF
    mask = rng.random(grid.shape) < 0.6
    origin = (7, -2, 100)
    for when, match, id, m in ((ort.WHEN_IS, 0, 9, None), (ort.WHEN_IS_NOT, 0, 9, mask), (ort.WHEN_IS, 2, 0, mask),
                               (ort.WHEN_IS_NOT, 2, 0xFFFFFFFF, None), (ort.WHEN_IS, 0xFFFFFFFF, 1, None)):
        want = []
        for z in range(3):
            for y in range(5):
                for x in range(4):
                    v = int(grid[z, y, x])
                    if (m is None or m[z, y, x]) and ((v == match) if when == ort.WHEN_IS else (v != match)):
                        want.append(((x + origin[0]) & 0xFFFFFFFF, (y + origin[1]) & 0xFFFFFFFF, z + origin[2], id))
        got = ort.select_records(grid, origin, id, when, match, mask=m)
        assert got.dtype == np.uint32 and got.shape == (len(want), 4)
        assert sorted(map(tuple, got.tolist())) == sorted(want)
    for dtype in (np.uint8, np.int32):
        assert np.array_equal(ort.select_records((grid % 4).astype(dtype), (0, 0, 0), 1, ort.WHEN_IS, 3),
                              ort.select_records(grid % 4, (0, 0, 0), 1, ort.WHEN_IS, 3))
    assert ort.select_records(np.zeros((0, 2, 2), np.uint8), (0, 0, 0), 1, 0, 0).shape == (0, 4)
    for bad in (dict(when=2), dict(when=True), dict(when=0.0), dict(id=-1), dict(id=1.0), dict(id=True), dict(match=1 << 32),
                dict(match=None), dict(grid=np.zeros((2, 2), np.uint8)), dict(grid=np.zeros((2, 2, 2), np.float32)),
                dict(mask=np.zeros((2, 2, 3), bool)), dict(mask=np.zeros((2, 2, 2), np.uint8)), dict(origin=(0, 0))):
        args = dict(grid=np.zeros((2, 2, 2), np.uint8), origin=(0, 0, 0), id=1, when=0, match=0, mask=None)
        args.update(bad)
        with pytest.raises(ValueError):
            ort.select_records(**args)


def test_python_guards(ort):
    from octree_ray_tracing_amd._marshal import u32_arg, when_arg
    assert (ort.WHEN_IS, ort.WHEN_IS_NOT) == (0, 1)
    assert when_arg(np.int64(1), "w") == 1 and u32_arg(np.uint32(0xFFFFFFFF), "w", "id") == 0xFFFFFFFF
    for bad in (2, -1, True, 1.0, "is", None):
        with pytest.raises(ValueError, match="when"):
            when_arg(bad, "World.paint_box")
    for bad in (-1, 1 << 32, 1.0, True, "3", None):
        with pytest.raises(ValueError, match="match"):
            u32_arg(bad, "World.paint_sphere", "match")
    w = closed_world(ort)
    for call in (lambda: w.paint_box((0, 0, 0), (2, 2, 2), 1), lambda: w.paint_sphere((4, 4, 4), 3, 1, ort.WHEN_IS, 2),
                 lambda: w.paint_box((0, 0, 0), (2, 2, 2), 1.5), lambda: w.paint_sphere((4, 4, 4), 3, 1, when=7)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_raw_entries_refuse_without_a_world(ort):
    from octree_ray_tracing_amd._lib import PaintStats
    lib, st = ort.load(), PaintStats()
    lo, hi, c2 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)(8, 8, 8)
    assert C.sizeof(PaintStats) == 56
    assert {"och_world_paint_box", "och_world_paint_sphere"} <= set(ort._lib.exported_symbols())
    assert lib.och_world_paint_box(None, lo, hi, 0, 0, 1, C.byref(st)) == -1 and b"NULL" in lib.och_last_error()
    assert lib.och_world_paint_sphere(None, c2, 5, 1, 0, 1, C.byref(st)) == -1 and b"NULL" in lib.och_last_error()
    assert lib.och_world_paint_box(None, None, hi, 0, 0, 1, None) == -1 and b"lo or hi" in lib.och_last_error()
    assert lib.och_world_paint_sphere(None, None, 5, 0, 0, 1, None) == -1 and b"centre2" in lib.och_last_error()
    for when in (2, -1):
        assert lib.och_world_paint_box(None, lo, hi, when, 0, 1, None) == -1 and b"when" in lib.och_last_error()
        assert lib.och_world_paint_sphere(None, c2, 5, when, 0, 1, None) == -1 and b"when" in lib.och_last_error()
