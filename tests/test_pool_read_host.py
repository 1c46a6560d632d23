"""och_pool_read_box (NodePool.read_box) on the host, and what och_world_at / och_world_read_box /
och_world_tighten refuse before a device is touched.

Truth is stated without the product: the dictionary `surviving(depth, records)` leaves, scattered
into zeros.  A whole tree is read wherever it can be held (depth <= 7: 2^21 cells).  The depth-16
and depth-21 cases have 2^48 and 2^63 cells: there the whole-tree read must be refused for lack of
capacity, and 5^3 boxes around the eight corners of the tree and around up to 64 surviving voxels
(evenly spaced through the sorted dictionary) are compared cell by cell instead.
"""
import ctypes as C

import numpy as np
import pytest

from test_voxel_builder import CASES, same_build, surviving

U8, U32, LIST = 1, 2, 0
WHOLE_DEPTH = 7
NODES = np.array([[2, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]], np.uint32)   # voxel 3 at (0, 0, 0), depth 2


def status(ort, name, *args):
    return getattr(ort.load(), name)(*args)


def last_error(ort):
    return ort.load().och_last_error().decode()


def vec(*v):
    return (C.c_int32 * 3)(*v)


def scatter(cells, lo, hi, dtype):
    """The dictionary's voxels inside [lo, hi) as the (nz, ny, nx) grid a read must give."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    nx, ny, nz = (int(v) for v in hi - lo)
    grid = np.zeros((nz, ny, nx), dtype)
    for (x, y, z), v in cells.items():
        if lo[0] <= x < hi[0] and lo[1] <= y < hi[1] and lo[2] <= z < hi[2]:
            grid[z - lo[2], y - lo[1], x - lo[0]] = v
    return grid


def sample_boxes(depth, cells):
    """The deep cases' boxes: 5^3 around each corner of the tree (overhanging) and around sampled voxels."""
    d = (1 << depth) - 1
    centres = [(x, y, z) for z in (0, d) for y in (0, d) for x in (0, d)]
    keys = sorted(cells)
    centres += keys[::max(1, len(keys) // 64)][:64]
    return [(np.array(c, np.int64) - 2, np.array(c, np.int64) + 3) for c in centres]


def dtypes_for(cells):
    return (np.uint8, np.uint32) if all(v <= 255 for v in cells.values()) else (np.uint32,)


@pytest.fixture(scope="module")
def built(ort):
    """name -> (the host-built pool, the surviving dictionary), once for the module."""
    return {name: (ort.build_voxels(rec, depth=depth), surviving(depth, rec)) for name, (depth, rec) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_read_equals_the_dictionary(ort, built, name):
    depth = CASES[name][0]
    tree, cells = built[name]
    dim = 1 << depth
    for dtype in dtypes_for(cells):
        if depth <= WHOLE_DEPTH:
            grid = tree.read_box((0, 0, 0), (dim, dim, dim), dtype)
            assert grid.dtype == dtype and grid.shape == (dim, dim, dim)
            assert np.array_equal(grid, scatter(cells, (0, 0, 0), (dim, dim, dim), dtype))
            same_build(ort.build_voxels(grid), tree)                   # the round trip
        else:
            one = np.zeros(1, dtype)
            assert status(ort, "och_pool_read_box", tree.nodes.ctypes.data, tree.n_nodes, tree.root, depth, 1,
                          vec(0, 0, 0), vec(dim, dim, dim), U8 if dtype == np.uint8 else U32,
                          one.ctypes.data, one.nbytes) == -1
            assert "does not fit" in last_error(ort)
            for lo, hi in sample_boxes(depth, cells):
                assert np.array_equal(tree.read_box(lo, hi, dtype), scatter(cells, lo, hi, dtype)), (lo, hi)


def test_odd_ids_need_u32(ort, built):
    tree, cells = built["odd_ids"]
    assert max(cells.values()) == 0xFFFFFFFF
    grid = tree.read_box((0, 0, 0), (16, 16, 16), np.uint32)
    assert np.array_equal(grid, scatter(cells, (0, 0, 0), (16, 16, 16), np.uint32))
    with pytest.raises(ort.OchError, match="INVALID"):
        tree.read_box((0, 0, 0), (16, 16, 16), np.uint8)


def test_zero_based_pool(ort):
    tree = ort.build_terrain(3, dedup=False)
    assert tree.index_base == 0
    for dtype in (np.uint8, np.uint32):
        grid = tree.read_box((0, 0, 0), (8, 8, 8), dtype)
        assert grid.any()
        for z in range(8):
            for y in range(8):
                for x in range(8):
                    assert grid[z, y, x] == tree.at(x, y, z), (x, y, z)


BOX_CASE = "out_of_range"                                              # depth 5, some 300 voxels


@pytest.mark.parametrize("lo,hi", [(None, None), ((1, 2, 3), (6, 6, 12)), ((-3, -3, -3), (34, 34, 34))],
                         ids=["single", "unaligned", "overhang"])
def test_boxes(ort, built, lo, hi):
    tree, cells = built[BOX_CASE]
    assert tree.depth == 5 and len(cells) > 100
    if lo is None:                                                     # the single cell: one that holds a voxel
        lo = sorted(cells)[len(cells) // 2]
        hi = tuple(c + 1 for c in lo)
    for dtype in (np.uint8, np.uint32):
        grid = tree.read_box(lo, hi, dtype)
        assert grid.shape == tuple(int(h - l) for l, h in zip(lo[::-1], hi[::-1]))
        want = scatter(cells, lo, hi, dtype)
        assert want.any() and np.array_equal(grid, want)
    if lo[0] < 0:
        inner = grid[3:35, 3:35, 3:35]
        assert inner.any() and grid.sum() == inner.sum()               # the overhang reads 0


def test_empty_box_writes_nothing(ort, built):
    tree, _ = built[BOX_CASE]
    canary = np.full(64, 0xAB, np.uint8)
    for lo, hi in (((4, 4, 4), (4, 9, 9)), ((4, 4, 4), (9, 4, 9)), ((4, 4, 4), (9, 9, 4)), ((0, 0, 0), (0, 0, 0))):
        for kind in (U8, U32):
            assert status(ort, "och_pool_read_box", tree.nodes.ctypes.data, tree.n_nodes, tree.root, 5, 1, vec(*lo), vec(*hi),
                          kind, canary.ctypes.data, canary.nbytes) == 0
            assert (canary == 0xAB).all()
    assert tree.read_box((4, 4, 4), (9, 4, 9)).shape == (5, 0, 5)


def test_refusals(ort, built):
    tree, cells = built[BOX_CASE]
    nodes, n = tree.nodes.ctypes.data, tree.n_nodes
    lo, hi = vec(1, 2, 3), vec(6, 6, 12)
    canary = np.full(5 * 4 * 9 * 4, 0xAB, np.uint8)
    good = (nodes, n, tree.root, 5, 1, lo, hi, U8, canary.ctypes.data, canary.nbytes)
    assert status(ort, "och_pool_read_box", *good) == 0
    canary[:] = 0xAB
    for slot in (0, 5, 6, 8):                                          # nodes, lo, hi, grid
        args = list(good)
        args[slot] = None
        assert status(ort, "och_pool_read_box", *args) == -1, slot
        assert "NULL" in last_error(ort)
    for slot, bad, text in ((7, LIST, "kind"), (7, 3, "kind"), (4, 2, "index_base"), (4, -1, "index_base"),
                            (6, vec(6, 1, 12), "below"), (3, 0, "depth"), (2, n + 1, "root")):
        args = list(good)
        args[slot] = bad
        assert status(ort, "och_pool_read_box", *args) == -1, (slot, bad)
        assert text in last_error(ort), last_error(ort)
    # one byte short, in both kinds
    for kind, cell in ((U8, 1), (U32, 4)):
        args = list(good)
        args[7], args[9] = kind, 5 * 4 * 9 * cell - 1
        assert status(ort, "och_pool_read_box", *args) == -1
        assert "does not fit" in last_error(ort)
        args[9] += 1
        assert (canary == 0xAB).all()                                  # nothing was written by any refusal
        assert status(ort, "och_pool_read_box", *args) == 0
        canary[:] = 0xAB
    # extents of 2^32 - 1 per axis: the volume passes 64 bits and is still refused, not wrapped
    big = list(good)
    big[5], big[6] = vec(-(1 << 31), -(1 << 31), -(1 << 31)), vec((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)
    assert status(ort, "och_pool_read_box", *big) == -1 and (canary == 0xAB).all()


def test_u8_overflow_names_the_id(ort):
    tree = ort.build_voxels(np.array([[3, 4, 5, 255], [9, 9, 9, 256]], np.uint32), depth=4)
    assert tree.read_box((0, 0, 0), (9, 9, 9), np.uint8)[5, 4, 3] == 255   # the box leaves the 256 out
    with pytest.raises(ort.OchError, match="INVALID.*256") as e:
        tree.read_box((0, 0, 0), (16, 16, 16), np.uint8)
    assert e.value.status == -1
    assert tree.read_box((0, 0, 0), (16, 16, 16), np.uint32)[9, 9, 9] == 256


# ------------------------------------------------------------ the world's entries without a device

def test_null_world_and_long_lists(ort):
    coords, ids, grid = np.zeros((1, 3), np.int32), np.zeros(1, np.uint32), np.zeros(8, np.uint8)
    assert status(ort, "och_world_at", None, coords.ctypes.data, 1, ids.ctypes.data, 0) == -1
    assert "NULL" in last_error(ort)
    assert status(ort, "och_world_at", None, coords.ctypes.data, 1 << 31, ids.ctypes.data, 0) == -1
    assert "2^31" in last_error(ort)
    assert status(ort, "och_world_at", None, None, 1, ids.ctypes.data, 0) == -1
    assert status(ort, "och_world_at", None, coords.ctypes.data, 1, None, 0) == -1
    assert status(ort, "och_world_read_box", None, vec(0, 0, 0), vec(2, 2, 2), U8, grid.ctypes.data, 8, 0) == -1
    assert "world is NULL" in last_error(ort)
    assert status(ort, "och_world_read_box", None, vec(0, 0, 0), vec(2, 2, 2), LIST, grid.ctypes.data, 8, 0) == -1
    assert "kind" in last_error(ort)
    assert status(ort, "och_world_read_box", None, vec(0, 0, 0), vec(2, 2, 2), U8, grid.ctypes.data, 7, 0) == -1
    assert "does not fit" in last_error(ort)
    assert status(ort, "och_world_tighten", None) == -1
    assert "NULL" in last_error(ort)


def closed_world(ort):
    """What close() leaves behind, without the device a live world needs."""
    w = ort.World.__new__(ort.World)
    w._h, w.depth, w.device = C.c_void_p(), 3, 0
    assert w.closed
    return w


def test_python_side_checks(ort):
    w = closed_world(ort)
    for bad in (np.zeros((5, 4), np.int32), np.zeros(3, np.int32), np.zeros((2, 3, 3), np.int32)):
        with pytest.raises(ValueError, match="coordinate list"):
            w.at(bad)
    with pytest.raises(ValueError, match="integers"):
        w.at(np.zeros((5, 3), np.float32))
    for bad in (1 << 31, -(1 << 31) - 1):
        with pytest.raises(ValueError, match="int32"):
            w.at(np.array([[0, bad, 0]], np.int64))
    with pytest.raises(ValueError, match="int32"):
        w.at(np.array([[0, 1 << 40, 0]], np.uint64))
    with pytest.raises(ValueError, match="dtype"):
        w.read_box((0, 0, 0), (2, 2, 2), np.int16)
    with pytest.raises(ValueError, match="three integers"):
        w.read_box((0, 0), (2, 2, 2))
    with pytest.raises(ValueError, match="three integers"):
        w.read_box((0, 0, 0), (2.0, 2.0, 2.0))
    with pytest.raises(ValueError, match="below"):
        w.read_box((0, 3, 0), (2, 2, 2))
    with pytest.raises(ValueError, match="closed"):
        w.at(np.zeros((5, 3), np.int32))
    with pytest.raises(ValueError, match="closed"):
        w.at(np.zeros((0, 3), np.int64))
    for device in (False, True):
        with pytest.raises(ValueError, match="closed"):
            w.read_box((0, 0, 0), (2, 2, 2), device=device)
    with pytest.raises(ValueError, match="closed"):
        w.tighten()


def test_binding_lists_the_read_entries(ort):
    names = {"och_pool_read_box", "och_world_at", "och_world_read_box", "och_world_tighten"}
    assert names <= set(ort._lib.exported_symbols())
    assert all(hasattr(ort.load(), n) for n in names)
    assert C.sizeof(ort._lib.WorldStats) == 64


def test_c99_host_names_every_read_function(ort, tmp_path):
    """The new declarations compile as strict C99 and link: a C host that names all four entries,
    reads a tiny pool and runs the refusals that need no device."""
    import shutil
    import subprocess
    from pathlib import Path
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    root = Path(ort._lib.HEADER_PATH).resolve().parents[1]
    libdir = Path(ort.load()._name).resolve().parent
    src = tmp_path / "read.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "och_gpu.h"
int main(void)
{
    /* depth 2: voxel 3 at (0, 0, 0), voxel 300 at (3, 3, 3) */
    const uint32_t nodes[3][8] = {{2, 0, 0, 0, 0, 0, 0, 3}, {3, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 300}};
    const int32_t lo[3] = {-1, 0, 0}, hi[3] = {3, 2, 2}, all[3] = {4, 4, 4}, zero[3] = {0, 0, 0};
    const int32_t coords[3] = {0, 0, 0};
    uint8_t grid[16];
    uint32_t wide[64], id = 7;
    och_world *world = NULL;
    och_world_stats st;
    memset(grid, 0xAB, sizeof grid);
    if (sizeof st != 64) return 1;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, lo, hi, OCH_VOXELS_GRID_U8, grid, sizeof grid) != OCH_OK) return 2;
    if (grid[0] != 0 || grid[1] != 3 || grid[2] != 0 || grid[15] != 0) return 3;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, lo, hi, OCH_VOXELS_GRID_U8, grid, sizeof grid - 1) != OCH_E_INVALID) return 4;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, lo, hi, OCH_VOXELS_LIST, grid, sizeof grid) != OCH_E_INVALID) return 5;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, hi, lo, OCH_VOXELS_GRID_U8, grid, sizeof grid) != OCH_E_INVALID) return 6;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, zero, all, OCH_VOXELS_GRID_U32, wide, sizeof wide) != OCH_OK) return 7;
    if (wide[0] != 3 || wide[63] != 300 || wide[1] != 0) return 8;
    if (och_pool_read_box(&nodes[0][0], 3, 1, 2, 1, zero, all, OCH_VOXELS_GRID_U8, wide, sizeof wide) != OCH_E_INVALID) return 9;
    if (strstr(och_last_error(), "300") == NULL) return 10;
    if (och_world_at(world, coords, 1, &id, 0) != OCH_E_INVALID || id != 7) return 11;
    if (och_world_at(world, coords, (uint64_t)1 << 31, &id, 0) != OCH_E_INVALID) return 12;
    if (strstr(och_last_error(), "2^31") == NULL) return 13;
    if (och_world_read_box(world, lo, hi, OCH_VOXELS_GRID_U8, grid, sizeof grid, 0) != OCH_E_INVALID) return 14;
    if (och_world_tighten(world) != OCH_E_INVALID) return 15;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "read"
    cc = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{root / 'include'}",
                         str(src), f"-L{libdir}", "-loch_gpu", f"-Wl,-rpath,{libdir}", "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.returncode, run.stdout, run.stderr)
