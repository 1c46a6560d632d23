"""och_box_cubes (ort.box_cubes) on the host: the maximal aligned cubes of a box, which a resident world's
region strokes (World.fill_box / restore_box, test_gpu_world_region.py) write as single child words, and
the cells that straddle the box, whose rows they rebuild.

The truth is independent of the code under test: the cubes painted into a numpy grid cover the box
exactly once, no cube's parent lies inside the box, the order is ascending height then ascending Morton
key, and the per-height counts equal the closed forms of the issue and a plain recursive Python walk."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_pool_diff_host import last_error, status

INVALID, CAPACITY = -1, -6


def clip(lo, hi, depth):
    lo = np.maximum(np.asarray(lo, np.int64), 0)
    hi = np.minimum(np.asarray(hi, np.int64), 1 << depth)
    return (lo, hi) if (lo < hi).all() else (np.zeros(3, np.int64), np.zeros(3, np.int64))


def closed_forms(lo, hi, depth):
    """(cubes per height, cells per height), heights 0 .. depth, from the per-axis counts."""
    lo, hi = clip(lo, hi, depth)
    if (lo == hi).all():
        return [0] * (depth + 1), [0] * (depth + 1)
    touch, inside = [], []
    for H in range(depth + 2):
        s = 1 << H
        touch.append(int(np.prod([-(-int(h) // s) - int(l) // s for l, h in zip(lo, hi)])))
        inside.append(int(np.prod([max(0, int(h) // s - -(-int(l) // s)) for l, h in zip(lo, hi)])))
    return ([inside[h] - 8 * inside[h + 1] for h in range(depth + 1)],
            [touch[H] - inside[H] for H in range(depth + 1)])


def recursive_walk(lo, hi, depth):
    """The same two lists from a plain top-down recursion over the tree's cells."""
    lo, hi = clip(lo, hi, depth)
    cubes, cells = [0] * (depth + 1), [0] * (depth + 1)

    def visit(o, H):
        s = 1 << H
        if any(o[a] >= hi[a] or o[a] + s <= lo[a] for a in range(3)):
            return
        if all(lo[a] <= o[a] and o[a] + s <= hi[a] for a in range(3)):
            cubes[H] += 1
            return
        cells[H] += 1
        for k in range(8):
            visit((o[0] + (k & 1) * s // 2, o[1] + ((k >> 1) & 1) * s // 2, o[2] + ((k >> 2) & 1) * s // 2), H - 1)

    if (lo < hi).all():
        visit((0, 0, 0), depth)
    return cubes, cells


def corner(key, levels):
    x = y = z = 0
    for l in range(levels):
        d = (int(key) >> (3 * l)) & 7
        x |= (d & 1) << l
        y |= ((d >> 1) & 1) << l
        z |= ((d >> 2) & 1) << l
    return x, y, z


def check_box(ort, lo, hi, depth, walk=True):
    keys, heights, cubes, cells = ort.box_cubes(lo, hi, depth)
    clo, chi = clip(lo, hi, depth)
    want_cubes, want_cells = closed_forms(lo, hi, depth)
    assert cubes.tolist() == want_cubes and cells.tolist() == want_cells, (lo, hi, depth)
    if walk:
        assert recursive_walk(lo, hi, depth) == (want_cubes, want_cells), (lo, hi, depth)
    assert keys.dtype == np.uint64 and heights.dtype == np.uint8 and len(keys) == len(heights) == sum(want_cubes)
    assert np.bincount(heights, minlength=depth + 1).tolist() == want_cubes
    # ascending height, ascending Morton key within a height
    order = heights.astype(np.uint64) << np.uint64(56) | keys
    assert (order[1:] > order[:-1]).all(), (lo, hi, depth)
    side = 1 << depth
    paint = np.zeros((side,) * 3, np.uint8)
    for key, h in zip(keys.tolist(), heights.tolist()):
        assert key >> (3 * (depth - h)) == 0
        s = 1 << h
        x, y, z = (c * s for c in corner(key, depth - h))
        paint[z:z + s, y:y + s, x:x + s] += 1
        # maximal: the parent cube does not lie inside the box
        if h < depth:
            p = 2 * s
            px, py, pz = x // p * p, y // p * p, z // p * p
            assert not all(l <= c and c + p <= u for c, l, u in zip((px, py, pz), clo, chi)), (lo, hi, key, h)
    want = np.zeros_like(paint)
    want[clo[2]:chi[2], clo[1]:chi[1], clo[0]:chi[0]] = 1
    assert np.array_equal(paint, want), (lo, hi, depth)


def test_every_box_of_a_depth_3_tree(ort):
    spans = [(l, h) for l in range(9) for h in range(l + 1, 9)]
    assert len(spans) == 36
    for (x0, x1), (y0, y1), (z0, z1) in itertools.product(spans, repeat=3):
        check_box(ort, (x0, y0, z0), (x1, y1, z1), 3, walk=False)
    for (x0, x1), (y0, y1), (z0, z1) in itertools.product(spans[::5], repeat=3):
        check_box(ort, (x0, y0, z0), (x1, y1, z1), 3)


@pytest.mark.parametrize("depth", [4, 5])
def test_random_boxes(ort, depth):
    rng = np.random.default_rng(100 + depth)
    side = 1 << depth
    kinds = {"overhang": 0, "empty": 0, "inside": 0}
    for i in range(2000):
        lo = rng.integers(-side // 4, side + side // 8, 3)
        hi = lo + rng.integers(0, side + side // 4, 3) if i % 7 else lo + rng.integers(0, 3, 3)
        clo, chi = clip(lo, hi, depth)
        kinds["empty" if (clo == chi).all() else "overhang" if (lo < 0).any() or (hi > side).any() else "inside"] += 1
        check_box(ort, lo, hi, depth, walk=i % 10 == 0)
    assert min(kinds.values()) > 20, kinds


def test_known_answers(ort):
    keys, heights, cubes, cells = ort.box_cubes((1980, 2080, 880), (2020, 2120, 920), 12)
    assert cubes.tolist() == [0, 0, 200, 36, 8] + [0] * 8 and len(keys) == 244
    assert cells.tolist() == [0, 0, 0, 50, 28, 12, 8, 2, 1, 1, 1, 1, 1] and int(cells.sum()) == 105
    assert recursive_walk((1980, 2080, 880), (2020, 2120, 920), 12) == (cubes.tolist(), cells.tolist())
    keys, heights, cubes, cells = ort.box_cubes((1, 1, 1), (7, 7, 7), 3)
    assert cubes.tolist() == [152, 8, 0, 0] and cells.tolist() == [0, 56, 8, 1]
    # the whole tree is one cube at height depth; a box outside it is nothing
    keys, heights, cubes, cells = ort.box_cubes((-5, 0, -1), (9, 8, 100), 3)
    assert keys.tolist() == [0] and heights.tolist() == [3] and cubes.tolist() == [0, 0, 0, 1] and not cells.any()
    keys, heights, cubes, cells = ort.box_cubes((8, 0, 0), (12, 8, 8), 3)
    assert len(keys) == 0 and not cubes.any() and not cells.any()
    # depth 21: the closed forms alone, no list
    n = C.c_uint64()
    lo, hi = (C.c_int32 * 3)(1, 1, 1), (C.c_int32 * 3)(*[(1 << 21) - 1] * 3)
    per_h, per_c = (C.c_uint64 * 22)(), (C.c_uint64 * 22)()
    assert status(ort, "och_box_cubes", lo, hi, 21, None, None, 0, per_h, per_c, C.byref(n)) == 0
    want_cubes, want_cells = closed_forms((1, 1, 1), [(1 << 21) - 1] * 3, 21)
    assert list(per_h)[:22] == want_cubes and list(per_c)[:22] == want_cells and n.value == sum(want_cubes)


def test_refusals(ort):
    lo, hi = (C.c_int32 * 3)(1, 1, 1), (C.c_int32 * 3)(7, 7, 7)
    n = C.c_uint64(77)
    keys, heights = np.zeros(160, np.uint64), np.zeros(160, np.uint8)
    args = (keys.ctypes.data, heights.ctypes.data)
    for depth in (0, 22, -1):
        assert status(ort, "och_box_cubes", lo, hi, depth, None, None, 0, None, None, C.byref(n)) == INVALID
        assert "depth" in last_error(ort)
    assert status(ort, "och_box_cubes", None, hi, 3, None, None, 0, None, None, C.byref(n)) == INVALID
    assert status(ort, "och_box_cubes", lo, None, 3, None, None, 0, None, None, C.byref(n)) == INVALID
    assert status(ort, "och_box_cubes", lo, hi, 3, None, None, 0, None, None, None) == INVALID
    assert status(ort, "och_box_cubes", lo, hi, 3, keys.ctypes.data, None, 160, None, None, C.byref(n)) == INVALID
    assert n.value == 77 and not keys.any()
    assert status(ort, "och_box_cubes", lo, hi, 3, *args, 159, None, None, C.byref(n)) == CAPACITY
    assert n.value == 160 and not keys.any() and not heights.any() and "160" in last_error(ort)
    assert status(ort, "och_box_cubes", lo, hi, 3, *args, 160, None, None, C.byref(n)) == 0 and n.value == 160
    assert np.array_equal(keys, ort.box_cubes((1, 1, 1), (7, 7, 7), 3)[0])
    with pytest.raises(ValueError):
        ort.box_cubes((1, 1, 1), (7, 0, 7), 3)
    with pytest.raises(ValueError):
        ort.box_cubes((1.5, 1, 1), (7, 7, 7), 3)


def test_region_entries_refuse_without_a_device(ort):
    """What och_world_fill_box and och_world_restore_box refuse before a world is looked at."""
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    assert status(ort, "och_world_fill_box", None, None, hi, 1, None) == INVALID and "lo or hi" in last_error(ort)
    assert status(ort, "och_world_fill_box", None, lo, hi, 1, None) == INVALID and "world is NULL" in last_error(ort)
    assert status(ort, "och_world_restore_box", None, 1, lo, None, None) == INVALID and "lo or hi" in last_error(ort)
    assert status(ort, "och_world_restore_box", None, 1, lo, hi, None) == INVALID and "world is NULL" in last_error(ort)
    assert C.sizeof(ort._lib.RegionStats) == 48
