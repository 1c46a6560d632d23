"""och_pool_diff (NodePool.diff) on the host, and what the world's history entries (och_world_snapshot,
_checkout, _release, _snapshots, _diff) refuse before a device is touched.

The truth is numpy throughout: both pools read whole as grids (NodePool.read_box), the coordinates where
the grids differ, sorted by their Morton key (x bit 0, y bit 1, z bit 2 per level); the records are
(x, y, z, grid_b[z, y, x]).  Records, n and box must be equal.  The GPU tests (test_gpu_world_history.py)
share these helpers."""
import ctypes as C

import numpy as np
import pytest

from test_voxel_builder import random_records

INVALID, CAPACITY = -1, -6


def status(ort, name, *args):
    return getattr(ort.load(), name)(*args)


def last_error(ort):
    return ort.load().och_last_error().decode()


def morton_keys(x, y, z, depth):
    x, y, z = (np.asarray(v, np.uint64) for v in (x, y, z))
    key = np.zeros(x.shape, np.uint64)
    for l in range(depth):
        s, one = np.uint64(l), np.uint64(1)
        key |= ((x >> s) & one) << np.uint64(3 * l) | ((y >> s) & one) << np.uint64(3 * l + 1) | \
               ((z >> s) & one) << np.uint64(3 * l + 2)
    return key


def truth_of_lists(depth, coords, ids):
    """(records, stats without pairs, keys) of the differing voxels given as coordinates and their new ids."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    keys = morton_keys(coords[:, 0], coords[:, 1], coords[:, 2], depth)
    order = np.argsort(keys, kind="stable")
    rec = np.zeros((len(order), 4), np.uint32)
    rec[:, :3] = coords[order]
    rec[:, 3] = np.asarray(ids, np.uint32)[order]
    n = len(order)
    lo = tuple(int(v) for v in coords.min(0)) if n else (0, 0, 0)
    hi = tuple(int(v) + 1 for v in coords.max(0)) if n else (0, 0, 0)
    return rec, {"n": n, "box_lo": lo, "box_hi": hi}, keys[order]


def whole_grid(pool):
    return pool.read_box((0, 0, 0), (1 << pool.depth,) * 3, np.uint32)


def truth_of_grids(depth, grid_a, grid_b):
    z, y, x = np.nonzero(grid_a != grid_b)
    return truth_of_lists(depth, np.stack([x, y, z], 1), grid_b[z, y, x])


def truth_of_pools(a, b):
    return truth_of_grids(a.depth, whole_grid(a), whole_grid(b))


def expected_pairs(keys, depth):
    """The tree positions at node heights 0 .. depth - 1 whose subtrees differ."""
    return sum(len(np.unique(keys >> np.uint64(3 * h))) for h in range(1, depth + 1))


def check_equal(got, want):
    (rec, st), (want_rec, want_st, _) = got, want
    assert rec.dtype == np.uint32 and rec.shape == want_rec.shape, (rec.shape, want_rec.shape)
    assert np.array_equal(rec, want_rec)
    assert {k: st[k] for k in ("n", "box_lo", "box_hi")} == want_st


# ------------------------------------------------------------ against the numpy truth

def all_pools(ort, depth, rng, count):
    """`count` pools of random occupancy at a depth small enough to enumerate cells."""
    dim, out = 1 << depth, []
    for _ in range(count):
        grid = rng.integers(0, 4, (dim,) * 3).astype(np.uint32) * (rng.random((dim,) * 3) < rng.random())
        out.append(ort.build_voxels(grid.astype(np.uint32), use_gpu=False))
    return out


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_small_depths(ort, depth):
    rng = np.random.default_rng(depth)
    empty = ort.build_voxels(np.zeros((0, 4), np.uint32), depth=depth, use_gpu=False)
    full = ort.build_voxels(np.full((1 << depth,) * 3, 7, np.uint32), use_gpu=False)
    pools = all_pools(ort, depth, rng, 6) + [empty, full]
    if depth == 1:   # exhaustively: every occupancy of the eight voxels against every eighth one
        pools = [ort.build_voxels(np.array([(m >> k) & 1 for k in range(8)], np.uint32).reshape(2, 2, 2), use_gpu=False)
                 for m in range(0, 256, 5)] + [full]
    for a in pools:
        for b in pools:
            check_equal(a.diff(b), truth_of_pools(a, b))


@pytest.mark.parametrize("depth,seed", [(5, 1), (6, 2)])
def test_random_base_and_stroke(ort, depth, seed):
    ids = np.array([1, 255, 256, 1 << 24, 0xFFFFFFFF], np.uint32)
    rng = np.random.default_rng(seed)
    base_rec = random_records(seed, 3000, depth)
    base_rec[:, 3] = np.where(base_rec[:, 3] != 0, ids[rng.integers(0, len(ids), len(base_rec))], 0)
    base = ort.build_voxels(base_rec, depth=depth, use_gpu=False)
    stroke = random_records(seed + 10, 1500, depth, remove=0.2)
    stroke[:, 3] = np.where(stroke[:, 3] != 0, ids[rng.integers(0, len(ids), len(stroke))], 0)
    grid = whole_grid(base)
    same = base_rec[:200].copy()                           # records that set a voxel to the id it already has
    same[:, 3] = grid[same[:, 2], same[:, 1], same[:, 0]]
    after = ort.edit_voxels(base, np.concatenate([stroke, same]), use_gpu=False)
    want = truth_of_pools(base, after)
    assert 0 < want[1]["n"] <= len(stroke)
    got = base.diff(after)
    check_equal(got, want)
    # the records that changed nothing do not appear
    changed = {tuple(r[:3]) for r in got[0].tolist()}
    final = whole_grid(after)
    assert all(tuple(r[:3]) not in changed for r in same.tolist() if final[r[2], r[1], r[0]] == grid[r[2], r[1], r[0]])
    # applied to a's content the records give b's
    assert np.array_equal(ort.edit_voxels(base, got[0], use_gpu=False).nodes, after.nodes)
    check_equal(after.diff(base), truth_of_pools(after, base))
    assert base.diff(after, records=False)[0] is None and base.diff(after, records=False)[1] == got[1]


def test_empty_against_non_empty_and_itself(ort):
    depth = 4
    empty = ort.build_voxels(np.zeros((0, 4), np.uint32), depth=depth, use_gpu=False)
    some = ort.build_voxels(random_records(3, 200, depth), depth=depth, use_gpu=False)
    assert empty.root == 0 and some.root == 1
    check_equal(empty.diff(some), truth_of_pools(empty, some))
    check_equal(some.diff(empty), truth_of_pools(some, empty))
    assert (some.diff(empty)[0][:, 3] == 0).all()
    for pool in (some, empty):
        rec, st = pool.diff(pool)
        assert rec.shape == (0, 4) and st == {"n": 0, "pairs": 0, "box_lo": (0, 0, 0), "box_hi": (0, 0, 0)}
    twin = ort.NodePool(some.nodes.copy(), some.root, depth, 1)      # another array: walked, still nothing
    rec, st = some.diff(twin)
    assert rec.shape == (0, 4) and st["n"] == 0 and st["pairs"] > 0


def test_zero_based_pools(ort):
    a = ort.build_terrain(3, dedup=False)
    b = ort.build_terrain(3, dedup=False, tunnels=False)
    assert a.index_base == 0 and b.index_base == 0
    want = truth_of_pools(a, b)
    if not want[1]["n"]:
        b = ort.build_terrain(3, dedup=False, rand_kind="msvc")
        want = truth_of_pools(a, b)
    assert want[1]["n"] > 0
    check_equal(a.diff(b), want)
    check_equal(b.diff(a), truth_of_pools(b, a))
    with pytest.raises(ValueError, match="index_base"):
        a.diff(ort.build_terrain(3))


def test_depth_21_far_corner(ort):
    d = (1 << 21) - 1
    changed, removed, added = (d, d, d), (d - 1, d, d - 2), (d, d - 3, 0)
    a = ort.build_voxels(np.array([changed + (5,), removed + (6,), (7, 7, 7, 9)], np.uint32), depth=21, use_gpu=False)
    b = ort.build_voxels(np.array([changed + (0xFFFFFFFF,), added + (8,), (7, 7, 7, 9)], np.uint32), depth=21, use_gpu=False)
    want = truth_of_lists(21, [changed, removed, added], [0xFFFFFFFF, 0, 8])
    assert int(want[2].max()) == (1 << 63) - 1                  # the key's full 63 bits
    check_equal(a.diff(b), want)
    assert a.diff(b)[1]["box_hi"] == (d + 1, d + 1, d + 1)


def test_non_canonical_slots(ort):
    depth = 4
    base = ort.build_voxels(random_records(5, 60, depth), depth=depth, use_gpu=False)
    with ort.Editor(base.nodes, base.root, depth, capacity=4096) as ed:
        for x, y, z, v in random_records(6, 80, depth, remove=0.3).tolist():
            ed.set(x, y, z, v)
        slots = ort.NodePool(ed.nodes(), ed.root, depth, 1)
    canonical = ort.edit_voxels(slots, np.zeros((0, 4), np.uint32), use_gpu=False)
    assert slots.n_nodes != canonical.n_nodes
    for a, b in ((slots, canonical), (canonical, slots)):
        rec, st = a.diff(b)
        assert rec.shape == (0, 4) and st["n"] == 0 and st["box_lo"] == st["box_hi"] == (0, 0, 0)
    check_equal(base.diff(slots), truth_of_pools(base, slots))


# ------------------------------------------------------------ refusals

def test_refusals(ort):
    from octree_ray_tracing_amd._lib import DiffStats
    depth = 3
    a = ort.build_voxels(random_records(1, 40, depth), depth=depth, use_gpu=False)
    b = ort.edit_voxels(a, random_records(2, 30, depth), use_gpu=False)
    n = a.diff(b)[1]["n"]
    assert n > 1
    st = DiffStats()
    buf = np.full((n, 4), 0xABABABAB, np.uint32)
    args = [a.nodes.ctypes.data, a.n_nodes, a.root, b.nodes.ctypes.data, b.n_nodes, b.root, depth, 1]
    assert status(ort, "och_pool_diff", *args, buf.ctypes.data, n - 1, C.byref(st)) == CAPACITY
    assert st.n == n and st.pairs > 0 and (buf == 0xABABABAB).all()
    assert tuple(st.box_lo) == a.diff(b)[1]["box_lo"] and tuple(st.box_hi) == a.diff(b)[1]["box_hi"]
    assert status(ort, "och_pool_diff", *args, buf.ctypes.data, n, C.byref(st)) == 0 and np.array_equal(buf, a.diff(b)[0])
    buf[:] = 0xABABABAB
    assert status(ort, "och_pool_diff", *args, buf.ctypes.data, n, None) == INVALID and "stats" in last_error(ort)
    for slot, bad in ((6, 0), (6, 22), (2, a.n_nodes + 1), (5, b.n_nodes + 1), (7, 2), (0, None), (3, None)):
        wrong = list(args)
        wrong[slot] = bad
        st.n = 77
        assert status(ort, "och_pool_diff", *wrong, buf.ctypes.data, n, C.byref(st)) == INVALID, (slot, bad)
        assert st.n == 77 and (buf == 0xABABABAB).all()
    bad_child = a.nodes.copy()
    bad_child[0, np.flatnonzero(bad_child[0])[0]] = a.n_nodes + 5
    wrong = list(args)
    wrong[0] = bad_child.ctypes.data
    assert status(ort, "och_pool_diff", *wrong, None, 0, C.byref(st)) == INVALID


def test_null_world(ort):
    from octree_ray_tracing_amd._lib import DiffStats
    st, s, n = DiffStats(), C.c_uint64(), C.c_uint32()
    assert status(ort, "och_world_snapshot", None, C.byref(s)) == INVALID and "world is NULL" in last_error(ort)
    assert status(ort, "och_world_snapshot", None, None) == INVALID and "snapshot is NULL" in last_error(ort)
    assert status(ort, "och_world_checkout", None, 1) == INVALID
    assert status(ort, "och_world_release", None, 1) == INVALID
    assert status(ort, "och_world_snapshots", None, None, 0, C.byref(n)) == INVALID
    assert status(ort, "och_world_snapshots", None, None, 0, None) == INVALID and "count" in last_error(ort)
    assert status(ort, "och_world_diff", None, 0, 0, None, 0, 0, C.byref(st)) == INVALID and "world is NULL" in last_error(ort)
    assert status(ort, "och_world_diff", None, 0, 0, None, 0, 0, None) == INVALID and "stats" in last_error(ort)


WORLD_ENTRIES = ["info", "edit", "pool_create", "flush", "download", "compact", "at", "read_box", "tighten", "snapshot",
                 "checkout", "release", "snapshots", "diff"]


@pytest.mark.parametrize("entry", WORLD_ENTRIES)
def test_null_world_every_entry(ort, entry):
    """Every och_world_* entry that takes a world, with a NULL world and otherwise valid arguments: INVALID,
    "<entry>: world is NULL", and every output as it was (och_world_pool_create hands out no pool: its handle is NULL)."""
    from octree_ray_tracing_amd._lib import DiffStats, HostPool, WorldStats
    fill = 0xAB
    out = np.full(128, fill, np.uint8)                     # any entry's output: a struct, a handle, ids, a grid, records
    p = out.ctypes.data
    recs = np.array([[1, 2, 3, 4]], np.uint32)
    coords = np.array([[1, 2, 3]], np.int32)
    lo, hi = np.zeros(3, np.int32), np.full(3, 2, np.int32)
    pool = C.c_void_p(p)                                   # never looked at: any non-NULL pool
    args = {"info": (C.cast(p, C.POINTER(WorldStats)),), "edit": (recs.ctypes.data, 1, 0),
            "pool_create": (C.cast(p, C.POINTER(C.c_void_p)),), "flush": (pool,), "download": (C.cast(p, C.POINTER(HostPool)),),
            "compact": (), "at": (coords.ctypes.data, 1, p, 0), "read_box": (lo.ctypes.data, hi.ctypes.data, 1, p, 64, 0),
            "tighten": (), "snapshot": (C.cast(p, C.POINTER(C.c_uint64)),), "checkout": (1,), "release": (1,),
            "snapshots": (p, 8, C.cast(p + 32, C.POINTER(C.c_uint32))), "diff": (0, 0, p + 40, 1, 0, C.cast(p, C.POINTER(DiffStats)))}
    assert max(C.sizeof(WorldStats), C.sizeof(HostPool), 40 + 16) <= out.size and C.sizeof(DiffStats) <= 40
    assert status(ort, f"och_world_{entry}", None, *args[entry]) == INVALID
    assert last_error(ort) == f"och_world_{entry}: world is NULL"
    if entry == "pool_create":
        assert not out[:8].any() and (out[8:] == fill).all()
    else:
        assert (out == fill).all()


# ------------------------------------------------------------ symbols, the Python side, a C99 host

NAMES = {"och_world_snapshot", "och_world_checkout", "och_world_release", "och_world_snapshots", "och_world_diff",
         "och_pool_diff"}


def test_binding_lists_the_history_entries(ort):
    assert NAMES <= set(ort._lib.exported_symbols())
    assert all(hasattr(ort.load(), n) for n in NAMES)
    assert C.sizeof(ort._lib.DiffStats) == 40
    assert C.sizeof(ort._lib.WorldStats) == 64


def test_python_side_checks(ort):
    w = ort.World.__new__(ort.World)                         # what close() leaves behind
    w._h, w.depth, w.device = C.c_void_p(), 3, 0
    assert w.closed
    for call in (w.snapshot, w.snapshots, lambda: w.checkout(1), lambda: w.release(1), lambda: w.diff(1),
                 lambda: w.diff(1, 2, device=True), lambda: w.diff(0, records=False), lambda: w.checkout("x")):
        with pytest.raises(ValueError, match="closed"):
            call()
    with pytest.raises(ValueError, match="closed"):
        ort.UndoStack(w)
    for bad in ("1", 1.0, None, True):
        with pytest.raises(ValueError, match="integer handle"):
            ort.World._handle(bad, "checkout")
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="uint64"):
            ort.World._handle(bad, "diff")
    assert ort.World._handle(np.uint64(3), "diff") == 3
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="limit"):
            ort.UndoStack(w, limit=bad)
    tree = ort.build_voxels(random_records(1, 10, 3), depth=3, use_gpu=False)
    with pytest.raises(ValueError, match="NodePool"):
        tree.diff((tree.nodes, 1, 3))
    with pytest.raises(ValueError, match="depth"):
        tree.diff(ort.build_voxels(random_records(1, 10, 4), depth=4, use_gpu=False))


def test_c99_host_names_every_history_function(ort, tmp_path):
    """The new declarations compile as strict C99 and link: a C host that names all six entries, runs
    och_pool_diff on a tiny pair and the refusals of the world's entries that need no device."""
    import shutil
    import subprocess
    from pathlib import Path
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    root = Path(ort._lib.HEADER_PATH).resolve().parents[1]
    libdir = Path(ort.load()._name).resolve().parent
    src = tmp_path / "history.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "och_gpu.h"
int main(void)
{
    /* depth 2: voxel 3 at (0, 0, 0); against voxel 4 there and voxel 9 at (3, 3, 3) */
    const uint32_t a[2][8] = {{2, 0, 0, 0, 0, 0, 0, 0}, {3, 0, 0, 0, 0, 0, 0, 0}};
    const uint32_t b[3][8] = {{2, 0, 0, 0, 0, 0, 0, 3}, {4, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 9}};
    uint32_t rec[2][4];
    uint64_t handle = 7, ids[2];
    uint32_t count = 7;
    och_world *world = NULL;
    och_diff_stats st;
    memset(&st, 0, sizeof st);
    memset(rec, 0xAB, sizeof rec);
    if (sizeof st != 40 || OCH_WORLD_CURRENT != 0 || OCH_WORLD_MAX_SNAPSHOTS != 65536) return 1;
    if (och_pool_diff(&a[0][0], 2, 1, &b[0][0], 3, 1, 2, 1, rec, 1, &st) != OCH_E_CAPACITY || st.n != 2) return 2;
    if (rec[0][0] != 0xABABABABu) return 3;
    if (och_pool_diff(&a[0][0], 2, 1, &b[0][0], 3, 1, 2, 1, rec, 2, &st) != OCH_OK || st.n != 2) return 4;
    if (rec[0][0] != 0 || rec[0][3] != 4 || rec[1][0] != 3 || rec[1][1] != 3 || rec[1][2] != 3 || rec[1][3] != 9) return 5;
    if (st.box_lo[0] != 0 || st.box_hi[2] != 4) return 6;
    if (och_pool_diff(&a[0][0], 2, 1, &b[0][0], 3, 1, 2, 1, NULL, 0, NULL) != OCH_E_INVALID) return 7;
    if (och_pool_diff(&a[0][0], 2, 1, &b[0][0], 3, 1, 22, 1, NULL, 0, &st) != OCH_E_INVALID) return 8;
    if (och_world_snapshot(world, &handle) != OCH_E_INVALID || handle != 7) return 9;
    if (strstr(och_last_error(), "NULL") == NULL) return 10;
    if (och_world_checkout(world, OCH_WORLD_CURRENT) != OCH_E_INVALID) return 11;
    if (och_world_release(world, 1) != OCH_E_INVALID) return 12;
    if (och_world_snapshots(world, ids, 2, &count) != OCH_E_INVALID || count != 7) return 13;
    if (och_world_diff(world, 1, OCH_WORLD_CURRENT, rec, 2, 0, &st) != OCH_E_INVALID) return 14;
    if (och_world_diff(world, 1, OCH_WORLD_CURRENT, NULL, 0, 0, NULL) != OCH_E_INVALID) return 15;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "history"
    cc = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{root / 'include'}",
                         str(src), f"-L{libdir}", "-loch_gpu", f"-Wl,-rpath,{libdir}", "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.returncode, run.stdout, run.stderr)
