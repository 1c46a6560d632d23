"""och_edit_voxels on the GPU (use_gpu=True): the host path's pool slot for slot, with the same
statistics, for every case and cut of tests/test_voxel_edit.py and for inputs sized to cross
workgroups; then the edited pool traced and rendered."""
import numpy as np
import pytest

from test_voxel_builder import CASES, ORIGIN, random_records, same_build
from test_voxel_edit import SPLITS, check_capacity

pytestmark = pytest.mark.gpu

NONE = np.zeros((0, 4), np.uint32)


def both(ort, tree, rec):
    """The GPU edit, checked against the host edit."""
    gpu = ort.edit_voxels(tree, rec, use_gpu=True)
    same_build(gpu, ort.edit_voxels(tree, rec))
    return gpu


@pytest.mark.parametrize("name,k", SPLITS, ids=[f"{name}-{k}" for name, k in SPLITS])
def test_split_lists_equal_host(ort, gpu_device, name, k):
    depth, rec = CASES[name]
    both(ort, ort.build_voxels(rec[:k], depth=depth), rec[k:])


def test_across_workgroups(ort, gpu_device):
    depth, base_rec = 9, random_records(200, 300_000, 9)
    rng = np.random.default_rng(201)
    third = 100_000 // 3
    reset = base_rec[rng.integers(0, len(base_rec), third)].copy()
    reset[:, 3] = rng.integers(6, 200, third)
    remove = base_rec[rng.integers(0, len(base_rec), third)].copy()
    remove[:, 3] = 0
    fresh = random_records(202, 100_000 - 2 * third, depth, dup=0.0, remove=0.0)
    edit = np.concatenate([reset, remove, fresh])[rng.permutation(100_000)]
    base = ort.build_voxels(base_rec, depth=depth, use_gpu=True)
    gpu = both(ort, base, edit)
    same_build(gpu, ort.build_voxels(np.concatenate([base_rec, edit]), depth=depth, use_gpu=True))
    assert gpu.solid_voxels not in (0, base.solid_voxels)


def test_empty_rows_by_the_million(ort, gpu_device):
    solid = ort.build_voxels(np.full((128, 128, 128), 2, np.uint8), use_gpu=True)
    assert solid.n_nodes == 7
    gone = ort.edit_voxels(solid, ort.box_records((0, 0, 0), (128, 128, 128), 0), use_gpu=True)
    assert gone.root == 0 and gone.nodes.shape == (1, 8) and not gone.nodes.any()
    assert (gone.solid_voxels, gone.tree_nodes, sum(gone.voxel_hist)) == (0, 0, 0)
    hole = ort.edit_voxels(solid, ort.box_records((44, 44, 44), (84, 84, 84), 0), use_gpu=True)
    assert hole.solid_voxels == 128 ** 3 - 40 ** 3 and hole.at(44, 44, 44) == 0 and hole.at(43, 44, 44) == 2
    same_build(ort.edit_voxels(hole, ort.box_records((44, 44, 44), (84, 84, 84), 2), use_gpu=True), solid)


@pytest.mark.parametrize("parents", [63, 64, 65, 255, 256, 257])
def test_sixty_four(ort, gpu_device, parents):
    """Records touching exactly `parents` leaf-level nodes, every other one emptied: rows that fill a
    wavefront, a workgroup, and one more."""
    depth, i = 10, np.arange(parents, dtype=np.uint32)
    base_rec = np.stack([2 * i, 3 + 0 * i, 5 + 0 * i, 1 + i % 5], 1).astype(np.uint32)
    edit = base_rec.copy()
    edit[::2, 3] = 0                       # the lone voxel of every even parent goes
    edit[1::2, 0] += 1                     # every odd parent gets a second voxel
    tree = both(ort, ort.build_voxels(base_rec, depth=depth), edit)
    assert tree.solid_voxels == 2 * (parents // 2) and tree.at(1, 3, 5) == 0 and tree.at(3, 3, 5) == 2


@pytest.fixture(scope="module")
def brushed(ort, gpu_device):
    """The depth-8 terrain and the reference's 40^3 brush at its surface: (base, box lo, set, removed)."""
    base = ort.build_terrain(8, use_gpu=True)
    top = max(z for z in range(256) if base.at(128, 128, z))
    lo = np.array([108, 108, top - 20])
    put = ort.edit_voxels(base, ort.box_records(lo, lo + 40, 1), use_gpu=True)
    cut = ort.edit_voxels(put, ort.box_records(lo, lo + 40, 0), use_gpu=True)
    return base, lo, put, cut


def test_terrain_brush(ort, brushed):
    base, lo, put, cut = brushed
    same_build(put, ort.edit_voxels(base, ort.box_records(lo, lo + 40, 1)))
    same_build(cut, ort.edit_voxels(put, ort.box_records(lo, lo + 40, 0)))
    assert put.solid_voxels > base.solid_voxels > cut.solid_voxels
    # the same 64 000 set() calls per stroke through the editor, its slot array canonicalised
    with ort.Editor(base.nodes, base.root, 8) as ed:
        for id, want in ((1, put), (0, cut)):
            for x, y, z, v in ort.box_records(lo, lo + 40, id).tolist():
                ed.set(x, y, z, v)
            same_build(ort.edit_voxels((ed.nodes(), ed.root, 8), NONE, use_gpu=True), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_end_to_end(ort, O, brushed, layout):
    """The edited pool uploaded, traced and rendered: bit for bit the oracle on the same pool."""
    tree = brushed[2]
    lut = ort.host_rcp_lut()
    ref, rcp = O.OraclePool(tree.nodes, tree.root, 8, 1), O.Rcp(lut)
    rng = np.random.default_rng(72)
    dirs = rng.uniform(-1, 1, (4096, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    org = rng.uniform(1.01, 1.99, (4096, 3)).astype(np.float32)
    colours = ort.VoxelData().get_colours()
    with ort.HOctree(tree.nodes, tree.root, 8, device=0) as pool:
        pool.set_option("layout", layout)
        gd, gv, gt = pool.trace_batch(org, dirs)
        r = O.trace_batch(ref, rcp, org, dirs)
        assert np.array_equal(gd, r["dir"]) and np.array_equal(gv, r["voxel"])
        assert np.array_equal(gt.view(np.uint32), r["t"].view(np.uint32))
        assert (gd < 6).any() and (gd == 6).any()
        pool.set_palette(colours)
        frame = pool.render(ort.camera((1.5, 1.5, 1.5), 0.3, -0.6, 1.25, 64, 36))
        r = O.trace_batch(ref, rcp, ORIGIN, O.raygen(0.3, -0.6, 1.25, 64, 36))
        assert np.array_equal(frame, O.shade(r["dir"], r["voxel"], colours).reshape(36, 64))


def test_device_records(ort, gpu_device):
    import torch
    depth, rec = CASES["n20000_d7"]
    base = ort.build_voxels(rec[:12000], depth=depth)
    host = ort.edit_voxels(base, rec[12000:])
    for dtype in (torch.int32, torch.uint32):
        dev = torch.from_numpy(rec[12000:].view(np.int32)).cuda().view(dtype)
        same_build(ort.edit_voxels(base, dev, use_gpu=True), host)
    with pytest.raises(ValueError, match="use_gpu"):
        ort.edit_voxels(base, dev)
    with pytest.raises(ValueError):
        ort.edit_voxels(base, dev.view(torch.int32).float(), use_gpu=True)
    empty = torch.zeros((0, 4), dtype=torch.int32, device="cuda")
    same_build(ort.edit_voxels(base, empty, use_gpu=True), base)


def test_two_runs_identical_bytes(ort, gpu_device):
    depth, rec = CASES["n20000_d16"]
    base = ort.build_voxels(rec[:15000], depth=depth)
    a = ort.edit_voxels(base, rec[15000:], use_gpu=True)
    b = ort.edit_voxels(base, rec[15000:], use_gpu=True)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.root == b.root


def test_capacity(ort, gpu_device):
    check_capacity(ort, True)


def test_child_word_one_past_the_end(ort, gpu_device):
    """The smallest violation: an interior child word of n_nodes + 1, refused without being followed."""
    tree = ort.build_voxels(random_records(1, 100, 3), depth=3)
    past = tree.nodes.copy()
    past[0, int(np.argmax(past[0] != 0))] = tree.n_nodes + 1
    with pytest.raises(ort.OchError, match="INVALID.*child"):
        ort.edit_voxels((past, 1, 3), NONE, use_gpu=True)


def test_builders_unchanged(ort, gpu_device):
    g, h = ort.build_terrain(8, use_gpu=True), ort.build_terrain(8)
    same_build(g, h)
    depth, rec = CASES["n20000_d7"]
    same_build(ort.build_voxels(rec, depth=depth, use_gpu=True), ort.build_voxels(rec, depth=depth))
