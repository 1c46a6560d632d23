"""och_sphere_cubes (ort.sphere_cubes) and ort.sphere_records on the host: the maximal aligned cubes of a
ball, which a resident world's sphere strokes (World.fill_sphere / restore_sphere,
test_gpu_world_sphere.py) write as single child words, and the cells that straddle the ball.

The truth is independent of the code under test: the ball is the inequality of include/och_gpu.h over a
numpy grid; the cubes painted into a grid cover it exactly once, no cube's parent lies inside the ball,
the order is ascending height then ascending Morton key, and the per-height counts equal a Python
recount of the walk with the header's per-axis classifier in Python integers."""
import ctypes as C

import numpy as np
import pytest

from test_box_cubes_host import corner
from test_pool_diff_host import last_error, status

INVALID, CAPACITY = -1, -6
RANGE = 1 << 24
DIAMETERS = [0, 1, 2, 3, 5, 8, 11, 16, 23, 30]


def ball_grid(c2, d, depth):
    """The ball's voxels inside a tree of `depth` as a [z, y, x] mask, from the inequality itself."""
    g = 2 * np.arange(1 << depth, dtype=np.int64) + 1
    off = [(g - int(c)) ** 2 for c in c2]
    return off[2][:, None, None] + off[1][None, :, None] + off[0][None, None, :] <= int(d) * int(d)


def classify(c2, d, o, H):
    """The aligned cube [o, o + 2^H)^3 against the ball: 0 outside, 1 straddling, 2 inside."""
    far = near = 0
    for a in range(3):
        lo, hi = 2 * o[a] + 1 - c2[a], 2 * (o[a] + (1 << H)) - 1 - c2[a]
        far += max(abs(lo), abs(hi)) ** 2
        near += (min(abs(lo), abs(hi)) if (lo > 0) == (hi > 0) and lo and hi else 1 - c2[a] % 2) ** 2
    return 2 if far <= d * d else 0 if near > d * d else 1


def recount(c2, d, depth):
    """(cubes per height, cells per height) from a plain top-down recursion."""
    cubes, cells = [0] * (depth + 1), [0] * (depth + 1)

    def visit(o, H):
        c = classify(c2, d, o, H)
        if c == 2:
            cubes[H] += 1
        if c != 1:
            return
        assert H > 0, "a voxel never straddles"
        cells[H] += 1
        s = 1 << (H - 1)
        for k in range(8):
            visit((o[0] + (k & 1) * s, o[1] + ((k >> 1) & 1) * s, o[2] + ((k >> 2) & 1) * s), H - 1)

    visit((0, 0, 0), depth)
    return cubes, cells


def check_ball(ort, c2, d, depth, walk=True):
    keys, heights, cubes, cells = ort.sphere_cubes(c2, d, depth)
    assert keys.dtype == np.uint64 and heights.dtype == np.uint8 and len(keys) == len(heights) == int(cubes.sum())
    assert np.bincount(heights, minlength=depth + 1).tolist() == cubes.tolist()
    if walk:
        assert recount(c2, d, depth) == (cubes.tolist(), cells.tolist()), (c2, d, depth)
    order = heights.astype(np.uint64) << np.uint64(56) | keys
    assert (order[1:] > order[:-1]).all(), (c2, d, depth)
    paint = np.zeros((1 << depth,) * 3, np.uint8)
    for key, h in zip(keys.tolist(), heights.tolist()):
        assert key >> (3 * (depth - h)) == 0
        s = 1 << h
        x, y, z = (c * s for c in corner(key, depth - h))
        paint[z:z + s, y:y + s, x:x + s] += 1
        if h < depth:                                   # maximal: the parent cube is not inside the ball
            p = 2 * s
            assert classify(c2, d, (x // p * p, y // p * p, z // p * p), h + 1) != 2, (c2, d, key, h)
    assert np.array_equal(paint, ball_grid(c2, d, depth).astype(np.uint8)), (c2, d, depth)
    return keys, heights, cubes, cells


def test_balls_of_a_depth_3_tree(ort):
    """A seeded sample of centres over -3 .. 19 per axis, every parity on every axis, times the issue's diameters."""
    rng = np.random.default_rng(3)
    centres = {tuple(int(v) for v in rng.integers(-3, 20, 3)) for _ in range(160)}
    centres |= {(8 + i, 8 + j, 8 + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    assert {tuple(v % 2 for v in c) for c in centres} == {(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    kinds = {"nothing": 0, "whole": 0, "some": 0}
    for c2 in sorted(centres):
        for d in DIAMETERS:
            keys, heights, cubes, cells = check_ball(ort, c2, d, 3)
            kinds["nothing" if not len(keys) else "whole" if heights[0] == 3 else "some"] += 1
    assert min(kinds.values()) >= 10, kinds


def test_known_answers(ort):
    keys, heights, cubes, cells = check_ball(ort, (32, 32, 32), 56, 5, walk=False)
    assert keys.tolist() == [0] and heights.tolist() == [5] and not cells.any()
    keys, heights, cubes, cells = check_ball(ort, (31, 33, 30), 27, 5)
    assert (len(keys), int(cells.sum())) == (2050, 659)
    keys, heights, cubes, cells = ort.sphere_cubes((127, 129, 128), 125, 7)
    assert (len(keys), int(cells.sum())) == (47_680, 13_957)
    # diameter 0: the one voxel whose centre the ball's centre is, or nothing
    assert check_ball(ort, (7, 9, 3), 0, 3)[2].tolist() == [1, 0, 0, 0]
    assert len(check_ball(ort, (7, 8, 3), 0, 3)[0]) == 0
    # all even: the nearest centres are at (1, 1, 1), further than diameter 1
    assert len(check_ball(ort, (8, 8, 8), 1, 3)[0]) == 0
    assert check_ball(ort, (8, 8, 8), 2, 3)[2].tolist() == [8, 0, 0, 0]


def counts_only(ort, c2, d, depth):
    per_h, per_c, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
    assert status(ort, "och_sphere_cubes", (C.c_int32 * 3)(*c2), d, depth, None, None, 0, per_h, per_c, C.byref(n)) == 0
    assert n.value == sum(per_h) and not any(list(per_h)[depth + 1:]) and not any(list(per_c)[depth + 1:])
    return n.value, sum(per_c)


def test_depth_12_counts(ort):
    """The brush ball, the diameter-512 ball and the diameter-2047 clear of the world_sphere probe, counts
    only: the walk's cost follows the surface, 4.4e9 voxels are never visited."""
    assert len(ort.sphere_records((4000, 4200, 1800), 40, 1)) == 33_552
    assert counts_only(ort, (4000, 4200, 1800), 40, 12) == (4_628, 1_409)
    assert counts_only(ort, (4096, 4096, 1800), 512, 12) == (817_848, 236_089)
    cubes, cells = counts_only(ort, (4096, 4096, 1800), 2047, 12)
    assert (round(cubes / 1e5), round(cells / 1e5)) == (124, 36)          # 12.4 M and 3.6 M
    # the widest ball the arguments admit covers a whole tree of depth 21
    assert counts_only(ort, (1 << 21, 1 << 21, 1 << 21), RANGE, 21) == (1, 0)


def test_sphere_records_is_the_formula(ort):
    rng = np.random.default_rng(5)
    for _ in range(60):
        c2 = tuple(int(v) for v in rng.integers(-9, 40, 3))
        d = int(rng.integers(0, 14))
        rec = ort.sphere_records(c2, d, 0xFFFFFFFE)
        assert rec.dtype == np.uint32 and rec.shape[1:] == (4,) and (rec[:, 3] == 0xFFFFFFFE).all()
        lo = [-((d + 1 - c) // 2) for c in c2]                          # ceil((c2 - d - 1) / 2)
        hi = [(c + d - 1) // 2 + 1 for c in c2]
        want = [(x, y, z) for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])
                if (2 * x + 1 - c2[0]) ** 2 + (2 * y + 1 - c2[1]) ** 2 + (2 * z + 1 - c2[2]) ** 2 <= d * d]
        # box_records' order, and its wrapping of negative coordinates
        assert rec[:, :3].tolist() == [[v % (1 << 32) for v in p] for p in want], (c2, d)
        # nothing of the ball lies outside its axis box
        wide = [(x, y, z) for z in range(lo[2] - 1, hi[2] + 1) for y in range(lo[1] - 1, hi[1] + 1) for x in range(lo[0] - 1, hi[0] + 1)
                if (2 * x + 1 - c2[0]) ** 2 + (2 * y + 1 - c2[1]) ** 2 + (2 * z + 1 - c2[2]) ** 2 <= d * d]
        assert wide == want
    assert set(ort.sphere_records((-1, 3, 3), 3, 1)[:, 0].tolist()) == {0xFFFFFFFE, 0xFFFFFFFF, 0}
    assert ort.sphere_records((4, 4, 4), 0, 1).shape == (0, 4)
    with pytest.raises(ValueError):
        ort.sphere_records((4, 4, 4), 3, 1 << 32)
    with pytest.raises(ValueError):
        ort.sphere_records((4, 4, 4), 3, True)


def test_refusals(ort):
    c2 = (C.c_int32 * 3)(7, 9, 8)
    n = C.c_uint64(77)
    want = ort.sphere_cubes((7, 9, 8), 5, 3)
    total = len(want[0])
    assert total > 8
    keys, heights = np.zeros(total, np.uint64), np.zeros(total, np.uint8)
    args = (keys.ctypes.data, heights.ctypes.data)
    for depth in (0, 22, -1):
        assert status(ort, "och_sphere_cubes", c2, 5, depth, None, None, 0, None, None, C.byref(n)) == INVALID
        assert "depth" in last_error(ort)
    assert status(ort, "och_sphere_cubes", None, 5, 3, None, None, 0, None, None, C.byref(n)) == INVALID
    assert status(ort, "och_sphere_cubes", c2, 5, 3, None, None, 0, None, None, None) == INVALID
    assert status(ort, "och_sphere_cubes", c2, 5, 3, keys.ctypes.data, None, total, None, None, C.byref(n)) == INVALID
    assert status(ort, "och_sphere_cubes", c2, 5, 3, None, heights.ctypes.data, total, None, None, C.byref(n)) == INVALID
    assert n.value == 77 and not keys.any()
    # the argument range, from both sides
    for a in range(3):
        for v, ok in ((RANGE, True), (RANGE + 1, False), (-RANGE, True), (-RANGE - 1, False)):
            c = [7, 9, 8]
            c[a] = v
            got = status(ort, "och_sphere_cubes", (C.c_int32 * 3)(*c), 5, 3, None, None, 0, None, None, C.byref(n))
            assert got == (0 if ok else INVALID), (a, v)
            assert ok or "centre2" in last_error(ort)
    assert status(ort, "och_sphere_cubes", c2, RANGE, 3, None, None, 0, None, None, C.byref(n)) == 0 and n.value == 1
    assert status(ort, "och_sphere_cubes", c2, RANGE + 1, 3, None, None, 0, None, None, C.byref(n)) == INVALID
    assert "diameter" in last_error(ort)
    # capacity short by one: the counts complete, nothing written
    per_h = (C.c_uint64 * 22)()
    assert status(ort, "och_sphere_cubes", c2, 5, 3, *args, total - 1, per_h, None, C.byref(n)) == CAPACITY
    assert n.value == total and list(per_h)[:4] == want[2].tolist() and not keys.any() and not heights.any()
    assert str(total) in last_error(ort)
    assert status(ort, "och_sphere_cubes", c2, 5, 3, *args, total, None, None, C.byref(n)) == 0 and n.value == total
    assert np.array_equal(keys, want[0]) and np.array_equal(heights, want[1])
    for bad in [((7, 9), 5), ((7.5, 9, 8), 5), ((7, 9, 8), 5.0), ((7, 9, 8), -1), ((7, 9, 8), RANGE + 1),
                ((RANGE + 1, 9, 8), 5), ((7, True, 8), 5), (7, 5)]:
        with pytest.raises(ValueError):
            ort.sphere_cubes(*bad, 3)
        with pytest.raises(ValueError):
            ort.sphere_records(*bad, 1)


def test_sphere_entries_refuse_without_a_device(ort):
    """What och_world_fill_sphere and och_world_restore_sphere refuse before a world is looked at."""
    c2 = (C.c_int32 * 3)(1, 1, 1)
    assert status(ort, "och_world_fill_sphere", None, None, 3, 1, None) == INVALID and "centre2" in last_error(ort)
    assert status(ort, "och_world_fill_sphere", None, c2, 3, 1, None) == INVALID and "world is NULL" in last_error(ort)
    assert status(ort, "och_world_restore_sphere", None, 1, None, 3, None) == INVALID and "centre2" in last_error(ort)
    assert status(ort, "och_world_restore_sphere", None, 1, c2, 3, None) == INVALID and "world is NULL" in last_error(ort)
