"""A resident world's history on the GPU (World.snapshot / checkout / release / diff, ort.UndoStack):
a checkout gives back the state a snapshot remembered, node array for node array; the diff of two roots
is NodePool.diff of the two downloads byte for byte and the numpy truth of test_pool_diff_host.py, and
its `pairs` is the number of tree positions whose subtrees differ; compaction keeps live snapshots.

Store ids differ from run to run (claim order): only downloads, records, stats and frames are compared."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_world import BRUSH_POS, BRUSH_VIEW, check_frame, oracle_frame, roomy, thirds
from test_pool_diff_host import check_equal, expected_pairs, truth_of_lists, truth_of_pools
from test_voxel_builder import CASES, random_records, same_build

pytestmark = pytest.mark.gpu

SMALL = sorted(name for name, (depth, _) in CASES.items() if depth <= 7)
NOTHING = {"n": 0, "pairs": 0, "box_lo": (0, 0, 0), "box_hi": (0, 0, 0)}


def same_nodes(a, b):
    assert (a.root, a.depth) == (b.root, b.depth)
    assert a.nodes.shape == b.nodes.shape and np.array_equal(a.nodes, b.nodes)


def stroked(ort, name):
    """A world of the case's base with a snapshot and a download after the base and after each stroke."""
    depth, rec = CASES[name]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    world = ort.World(base, capacity=roomy(base, strokes, depth))
    snaps, downloads = [world.snapshot()], [world.download()]
    for s in strokes:
        world.edit(s)
        snaps.append(world.snapshot())
        downloads.append(world.download())
    return world, snaps, downloads


def check_diff(world, a, b, pool_a, pool_b, truth=None):
    """World.diff(a, b), host array and device tensor, against NodePool.diff of the downloads and the truth."""
    host_rec, host_st = pool_a.diff(pool_b)
    truth = truth or truth_of_pools(pool_a, pool_b)
    check_equal((host_rec, host_st), truth)
    rec, st = world.diff(a, b)
    assert rec.dtype == np.uint32 and rec.tobytes() == host_rec.tobytes()
    dev, dev_st = world.diff(a, b, device=True)
    assert dev.is_cuda and dev.device.index == world.device and tuple(dev.shape) == rec.shape
    assert dev.cpu().numpy().view(np.uint32).tobytes() == host_rec.tobytes()
    only, only_st = world.diff(a, b, records=False)
    assert only is None and st == dev_st == only_st
    assert {k: st[k] for k in ("n", "box_lo", "box_hi")} == {k: host_st[k] for k in ("n", "box_lo", "box_hi")}
    assert st["pairs"] == expected_pairs(truth[2], world.depth), (st, a, b)
    return rec, st


# ------------------------------------------------------------ 1. checkout restores a state

@pytest.mark.parametrize("name", SMALL)
def test_checkout_restores(ort, gpu_device, name):
    world, snaps, downloads = stroked(ort, name)
    with world:
        assert world.snapshots() == snaps == [1, 2, 3, 4]
        used = world.info()["used"]
        before = world.info()
        for i in np.random.default_rng(len(name)).permutation(len(snaps)).tolist() + [0, 3]:
            world.checkout(snaps[i])
            same_nodes(world.download(), downloads[i])
            info = world.info()
            assert info["used"] >= used
            used = info["used"]
            assert {k: info[k] for k in ("strokes", "generation", "capacity")} == {k: before[k] for k in ("strokes", "generation", "capacity")}
        world.checkout(0)                                    # OCH_WORLD_CURRENT: a no-op
        same_nodes(world.download(), downloads[3])
        assert world.info() == before                        # the last state again, box and all


def test_tighten_after_checkout(ort, gpu_device):
    world, snaps, downloads = stroked(ort, "all_removed")
    with world:
        for i in (1, 3, 0, 2):
            world.checkout(snaps[i])
            tree = downloads[i]
            assert world.tighten() == ort.occupied_box(tree.nodes, tree.root, tree.depth)


# ------------------------------------------------------------ 2. frames and pools

@pytest.fixture(scope="module")
def terrain(ort, gpu_device):
    base = ort.build_terrain(8, use_gpu=True)
    top = max(z for z in range(256) if base.at(128, 128, z))
    return base, np.array([108, 108, top - 20])


def test_frames_follow_checkout(ort, O, terrain):
    base, lo = terrain
    rec = ort.box_records(lo, lo + 40, 1)
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool, world.make_pool() as never_flushed:
        never_flushed.set_palette(ort.VoxelData().get_colours())
        s = world.snapshot()
        world.edit(rec)
        world.flush(pool)
        after = world.download()
        check_frame(ort, O, pool, after, BRUSH_POS, BRUSH_VIEW)
        world.checkout(s)
        world.flush(pool)
        same_nodes(world.download(), base)
        check_frame(ort, O, pool, base, BRUSH_POS, BRUSH_VIEW)
        old, new = (oracle_frame(ort, O, t, BRUSH_POS, BRUSH_VIEW) for t in (base, after))
        assert (old != new).sum() > 50
        assert np.array_equal(never_flushed.render(ort.camera(BRUSH_POS, *BRUSH_VIEW, 64, 36)), old)


def test_one_voxel_is_depth_pairs(ort, terrain):
    base, lo = terrain
    with ort.World(base, capacity=100_000) as world:
        s = world.snapshot()
        x, y, z = (int(v) for v in lo)
        world.edit(np.array([[x, y, z, base.at(x, y, z) + 1]], np.uint32))
        rec, st = world.diff(s)
        assert rec.tolist() == [[x, y, z, base.at(x, y, z) + 1]]
        assert st == {"n": 1, "pairs": 8, "box_lo": (x, y, z), "box_hi": (x + 1, y + 1, z + 1)}
        rec, st = world.diff(0, s)
        assert rec.tolist() == [[x, y, z, base.at(x, y, z)]] and st["pairs"] == 8


# ------------------------------------------------------------ 3. the diff against the host truth

@pytest.mark.parametrize("name", SMALL)
def test_diff_equals_host(ort, gpu_device, name):
    world, snaps, downloads = stroked(ort, name)
    with world:
        for a, b in ((0, 3), (3, 0), (1, 2), (2, 3), (0, 1)):
            check_diff(world, snaps[a], snaps[b], downloads[a], downloads[b])
        check_diff(world, snaps[1], 0, downloads[1], downloads[3])          # b = the current state
        world.checkout(snaps[1])
        check_diff(world, 0, snaps[2], downloads[1], downloads[2])
        twin = world.snapshot()                                           # a second handle of one state
        assert twin == 5
        for a, b in ((snaps[2], snaps[2]), (snaps[1], twin), (0, 0), (0, twin)):
            rec, st = world.diff(a, b)
            assert rec.shape == (0, 4) and st == NOTHING
            assert tuple(world.diff(a, b, device=True)[0].shape) == (0, 4)


def test_put_then_cut_is_nothing(ort, gpu_device):
    depth = 6
    base = ort.build_voxels(random_records(4, 2000, depth), depth=depth)
    lo, hi = np.array([10, 20, 30]), np.array([21, 27, 39])
    old = base.read_box(lo, hi, np.uint32)
    z, y, x = np.nonzero(np.ones_like(old))
    back = np.stack([x + lo[0], y + lo[1], z + lo[2], old[z, y, x]], 1).astype(np.uint32)
    with ort.World(base, capacity=50_000) as world:
        s = world.snapshot()
        world.edit(ort.box_records(lo, hi, 77))
        assert world.diff(s)[1]["n"] > 0
        world.edit(back)
        rec, st = world.diff(s)
        assert rec.shape == (0, 4) and st == NOTHING                     # equal content is equal root id
        same_nodes(world.download(), base)


# ------------------------------------------------------------ 4. wavefront and workgroup edges

@pytest.mark.parametrize("parents", [63, 64, 65, 255, 256, 257])
def test_sixty_four(ort, gpu_device, parents):
    """test_gpu_world.test_sixty_four's construction: the stroke touches exactly `parents` leaf-level nodes,
    empties every other one and gives the rest a second voxel.  Truth from the record lists (depth 10)."""
    depth, i = 10, np.arange(parents, dtype=np.uint32)
    base_rec = np.stack([2 * i, 3 + 0 * i, 5 + 0 * i, 1 + i % 5], 1).astype(np.uint32)
    edit = base_rec.copy()
    edit[::2, 3] = 0
    edit[1::2, 0] += 1
    edit[1::2, 3] += 100
    base = ort.build_voxels(base_rec, depth=depth)
    with ort.World(base, capacity=roomy(base, [edit], depth)) as world:
        s = world.snapshot()
        world.edit(edit)
        truth = truth_of_lists(depth, edit[:, :3], edit[:, 3])
        assert truth[1]["n"] == parents
        rec, st = check_diff(world, s, 0, base, world.download(), truth)
        assert len(np.unique(truth[2] >> np.uint64(3))) == parents       # that many leaf-level pairs
        back = truth_of_lists(depth, np.concatenate([base_rec[::2, :3], edit[1::2, :3]]),
                              np.concatenate([base_rec[::2, 3], 0 * edit[1::2, 3]]))
        check_diff(world, 0, s, world.download(), base, back)


@pytest.mark.parametrize("parents", [63, 64, 65, 257])
def test_one_box_reduction(ort, gpu_device, parents):
    """The stroke's box (World.info) and the diff's box come from one wavefront reduction: `parents` distinct
    random voxels into an empty world, a partial, a whole and more than one wavefront, more than one workgroup."""
    depth = 6
    rng = np.random.default_rng(parents)
    cells = rng.choice(1 << 3 * depth, parents, replace=False)
    rec = np.stack([cells & 63, cells >> 6 & 63, cells >> 12, rng.integers(1, 6, parents)], 1).astype(np.uint32)
    with ort.World((np.zeros((0, 8), np.uint32), 0, depth), capacity=10_000) as world:
        s = world.snapshot()
        world.edit(rec)
        lo = tuple(int(v) for v in rec[:, :3].min(0))
        hi = tuple(int(v) + 1 for v in rec[:, :3].max(0))
        info, (none, st) = world.info(), world.diff(s, 0, records=False)
        assert none is None and st["n"] == parents
        assert (tuple(info["box_lo"]), tuple(info["box_hi"])) == (tuple(st["box_lo"]), tuple(st["box_hi"])) == (lo, hi)


# ------------------------------------------------------------ 5. depths 1, 2 and 21; an empty world

@pytest.mark.parametrize("depth", [1, 2])
def test_shallow(ort, gpu_device, depth):
    dim = 1 << depth
    rng = np.random.default_rng(depth)
    grids = [(rng.integers(1, 5, (dim,) * 3) * (rng.random((dim,) * 3) < p)).astype(np.uint32) for p in (0.5, 0.9, 0.2)]
    z, y, x = np.nonzero(np.ones((dim,) * 3))
    with ort.World(ort.build_voxels(grids[0]), capacity=1000) as world:
        snaps, downloads = [world.snapshot()], [world.download()]
        for g in grids[1:]:
            world.edit(np.stack([x, y, z, g[z, y, x]], 1).astype(np.uint32))
            snaps.append(world.snapshot())
            downloads.append(world.download())
        for a in range(3):
            for b in range(3):
                if a != b:
                    check_diff(world, snaps[a], snaps[b], downloads[a], downloads[b])
        world.checkout(snaps[0])
        same_nodes(world.download(), downloads[0])


def test_depth_21(ort, gpu_device):
    d = (1 << 21) - 1
    changed, removed, added = (d, d, d), (d - 1, d, d - 2), (d, d - 3, 0)
    base = ort.build_voxels(np.array([changed + (5,), removed + (6,), (7, 7, 7, 9)], np.uint32), depth=21)
    stroke = np.array([changed + (0xFFFFFFFF,), removed + (0,), added + (8,), (7, 7, 7, 9)], np.uint32)
    with ort.World(base, capacity=2000) as world:
        s = world.snapshot()
        world.edit(stroke)
        truth = truth_of_lists(21, [changed, removed, added], [0xFFFFFFFF, 0, 8])
        rec, st = check_diff(world, s, 0, base, world.download(), truth)
        assert st["box_hi"] == (d + 1, d + 1, d + 1)
        world.checkout(s)
        same_nodes(world.download(), base)


def test_empty_world(ort, gpu_device):
    depth = 5
    paint = random_records(11, 500, depth, remove=0.0)
    with ort.World((np.zeros((0, 8), np.uint32), 0, depth), capacity=10_000) as world:
        empty = world.download()
        assert empty.root == 0
        s0 = world.snapshot()
        world.edit(paint)
        s1 = world.snapshot()
        painted = world.download()
        rec, st = check_diff(world, s0, s1, empty, painted)               # the `from` side is id 0 all the way
        assert st["n"] == painted.solid_voxels
        world.edit(paint * np.array([1, 1, 1, 0], np.uint32))
        assert world.info()["root"] == 0
        assert world.diff(s0)[1] == NOTHING
        rec, st = check_diff(world, s1, 0, painted, empty)                # the `to` side is
        assert (rec[:, 3] == 0).all()
        world.checkout(s1)
        same_nodes(world.download(), painted)


# ------------------------------------------------------------ 6. a replica follows by diffs

def test_replica(ort, gpu_device):
    import torch
    world, snaps, downloads = stroked(ort, "n20000_d7")
    with world:
        host, _ = world.diff(snaps[1], snaps[3])
        dev, _ = world.diff(snaps[1], snaps[3], device=True)
        assert dev.dtype == torch.int32
        for records in (host, dev):
            with ort.World(downloads[1], capacity=world.info()["capacity"]) as replica:
                replica.edit(records)
                same_nodes(replica.download(), downloads[3])


# ------------------------------------------------------------ 7. capacity and the summary form

def test_capacity_and_summary(ort, gpu_device):
    import torch
    from octree_ray_tracing_amd._lib import DiffStats
    world, snaps, downloads = stroked(ort, "n257_d7")
    with world:
        none, want = world.diff(snaps[0], snaps[3], records=False)
        assert none is None and want["n"] > 1
        n = want["n"]
        lib, st = ort.load(), DiffStats()
        buf = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert lib.och_world_diff(world._h, snaps[0], snaps[3], buf.data_ptr(), n - 1, 1, C.byref(st)) == -6
        assert "records" in lib.och_last_error().decode()
        assert (st.n, st.pairs, tuple(st.box_lo), tuple(st.box_hi)) == (n, want["pairs"], want["box_lo"], want["box_hi"])
        assert bool((buf == 0x5A5A5A5A).all())
        host = np.full((n, 4), 0x5A5A5A5A, np.uint32)
        assert lib.och_world_diff(world._h, snaps[0], snaps[3], host.ctypes.data, n - 1, 0, C.byref(st)) == -6
        assert (host == 0x5A5A5A5A).all()
        assert lib.och_world_diff(world._h, snaps[0], snaps[3], buf.data_ptr(), n, 1, C.byref(st)) == 0
        assert buf.cpu().numpy().view(np.uint32).tobytes() == downloads[0].diff(downloads[3])[0].tobytes()
        assert lib.och_world_diff(world._h, snaps[0], snaps[3], None, 0, 0, None) == -1
        same_nodes(world.download(), downloads[3])                        # a refused diff leaves the world usable


# ------------------------------------------------------------ 8. compaction keeps live snapshots

def distinct_subtrees(pools):
    """The distinct (height, content) subtrees reachable from the roots of canonical pools of one depth."""
    seen = set()
    for p in pools:
        if not p.root:
            continue
        memo = {}

        def visit(v, h):
            if (v, h) not in memo:
                row = p.nodes[v - 1].tolist()
                memo[(v, h)] = (h, tuple(row) if h == 0 else tuple(visit(c, h - 1) if c else None for c in row))
                seen.add(memo[(v, h)])
            return memo[(v, h)]
        visit(p.root, p.depth - 1)
    return len(seen)


def test_compaction_keeps_snapshots(ort, gpu_device):
    depth = 5
    base = ort.build_voxels(random_records(21, 1500, depth), depth=depth)
    with ort.World(base, capacity=60_000) as world:
        a, tree_a = world.snapshot(), world.download()
        world.edit(random_records(22, 800, depth, remove=0.3))
        world.edit(ort.box_records((3, 3, 3), (17, 12, 9), 4))
        b, tree_b = world.snapshot(), world.download()
        world.edit(ort.box_records((0, 0, 0), (32, 32, 28), 0))           # most of it cut away
        world.edit(random_records(23, 50, depth, remove=0.0))
        now = world.download()
        diff_ab = world.diff(a, b)
        before = world.info()
        world.compact()
        info = world.info()
        assert info["used"] - 1 == distinct_subtrees([tree_a, tree_b, now]) < before["used"] - 1
        assert info["generation"] == before["generation"] + 1 and world.snapshots() == [a, b]
        same_nodes(world.download(), now)
        after_ab = world.diff(a, b)
        assert after_ab[0].tobytes() == diff_ab[0].tobytes() and after_ab[1] == diff_ab[1]
        check_diff(world, b, 0, tree_b, now)
        assert world.tighten() == ort.occupied_box(now.nodes, now.root, depth)
        for s, tree in ((a, tree_a), (b, tree_b)):
            world.checkout(s)
            same_nodes(world.download(), tree)
            assert world.tighten() == ort.occupied_box(tree.nodes, tree.root, depth)
        world.checkout(a)
        world.edit(ort.box_records((1, 1, 1), (5, 5, 5), 9))              # the compacted store takes strokes
        same_build(world.download(), ort.edit_voxels(tree_a, ort.box_records((1, 1, 1), (5, 5, 5), 9)))
        # back to the cut-away state through a diff, then today's rule once nothing is remembered
        world.edit(world.diff(0, b)[0])
        world.edit(tree_b.diff(now)[0])
        same_nodes(world.download(), now)
        world.release(a)
        world.release(b)
        assert world.snapshots() == []
        world.compact()
        assert world.info()["used"] - 1 == distinct_subtrees([now]) and world.info()["generation"] == before["generation"] + 2
        same_nodes(world.download(), now)


# ------------------------------------------------------------ 9. UndoStack

def test_undo_stack(ort, gpu_device):
    depth = 5
    strokes = [random_records(30 + k, 300, depth) for k in range(6)]
    base = ort.build_voxels(random_records(29, 500, depth), depth=depth)
    with ort.World(base, capacity=60_000) as world:
        undo = ort.UndoStack(world, limit=4)
        states = [world.download()]
        assert world.snapshots() == undo.entries == [1] and not undo.undo() and not undo.redo()
        for s in strokes[:3]:
            world.edit(s)
            undo.push()
            states.append(world.download())
        assert world.snapshots() == undo.entries == [1, 2, 3, 4]
        assert undo.undo() and undo.undo()
        same_nodes(world.download(), states[1])
        assert undo.redo()
        same_nodes(world.download(), states[2])
        assert undo.current == 3 and world.snapshots() == [1, 2, 3, 4]
        world.edit(strokes[3])                                            # a new stroke: the undone branch goes
        assert undo.push() == 5
        branch = world.download()
        same_nodes(branch, ort.edit_voxels(states[2], strokes[3]))
        assert world.snapshots() == undo.entries == [1, 2, 3, 5] and not undo.redo()
        with pytest.raises(ort.OchError, match="INVALID.*snapshot 4"):
            world.checkout(4)
        world.edit(strokes[4])
        undo.push()                                                       # beyond the limit: the oldest goes
        assert world.snapshots() == undo.entries == [2, 3, 5, 6]
        assert undo.undo() and undo.undo() and undo.undo() and not undo.undo()
        same_nodes(world.download(), states[1])
        assert undo.redo() and undo.redo()
        same_nodes(world.download(), branch)


# ------------------------------------------------------------ 10. guards

def test_guards(ort, gpu_device):
    depth = 3
    base = ort.build_voxels(random_records(1, 100, depth), depth=depth)
    with ort.World(base, capacity=1000) as world, ort.World(base, capacity=1000) as other:
        s = world.snapshot()
        assert s == 1 and other.snapshots() == []
        for call in (lambda: other.checkout(s), lambda: other.release(s), lambda: other.diff(s), lambda: other.diff(0, s),
                     lambda: world.checkout(2), lambda: world.diff(s, 99, records=False)):
            with pytest.raises(ort.OchError, match="INVALID.*snapshot (1|2|99) ") as e:   # another world's handle, unknown ones
                call()
            assert e.value.status == -1
        with pytest.raises(ort.OchError, match="INVALID.*CURRENT"):
            world.release(0)
        world.release(s)
        for call in (lambda: world.checkout(s), lambda: world.release(s), lambda: world.diff(s)):
            with pytest.raises(ort.OchError, match="INVALID.*snapshot 1 "):
                call()
        assert world.snapshot() == 2                                      # never reused
        world.release(2)
        handles = [world.snapshot() for _ in range(65536)]
        assert handles[0] == 3 and handles[-1] == 65538 and len(world.snapshots()) == 65536
        before = world.info()
        with pytest.raises(ort.OchError, match="CAPACITY") as e:
            world.snapshot()
        assert e.value.status == -6 and world.info() == before
        world.release(handles[7])
        assert world.snapshot() == 65539
        world.compact()                                                   # one root, 65 536 handles
        assert len(world.snapshots()) == 65536
        world.checkout(handles[100])
        same_nodes(world.download(), base)
    for call in (world.snapshot, world.snapshots, lambda: world.checkout(3), lambda: world.release(3), lambda: world.diff(3)):
        with pytest.raises(ValueError, match="closed"):
            call()
