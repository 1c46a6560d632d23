"""och_build_voxels on the GPU (use_gpu=True): the host path's pool slot for slot,
with the same statistics, for every case of tests/test_voxel_builder.py and for
inputs sized to cross workgroups; then the built pool traced and rendered."""
import numpy as np
import pytest

from test_voxel_builder import CASES, ORIGIN, grid_records, random_records, same_build, terrain_grid

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_list_equals_host(ort, gpu_device, name):
    depth, rec = CASES[name]
    same_build(ort.build_voxels(rec, depth=depth, use_gpu=True), ort.build_voxels(rec, depth=depth))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32])
def test_grid_equals_host_and_list(ort, gpu_device, dtype):
    rng = np.random.default_rng(40)
    grid = np.where(rng.random((32, 32, 32)) < 0.2, rng.integers(1, 200, (32, 32, 32)), 0).astype(dtype)
    if dtype == np.uint32:
        grid[3, 4, 5] = 0xFFFFFFFF
    host = ort.build_voxels(grid)
    same_build(ort.build_voxels(grid, use_gpu=True), host)
    same_build(ort.build_voxels(grid_records(grid), depth=5, use_gpu=True), host)
    same_build(ort.build_voxels(np.zeros((8, 8, 8), dtype), use_gpu=True), ort.build_voxels(np.zeros((8, 8, 8), dtype)))


def test_terrain_tie(ort, O, gpu_device):
    want = ort.build_terrain(6)
    grid = terrain_grid(O, 6)
    rec = grid_records(grid)
    rec = rec[np.random.default_rng(6).permutation(len(rec))]
    for tree in (ort.build_voxels(grid, use_gpu=True), ort.build_voxels(rec, depth=6, use_gpu=True)):
        assert tree.root == want.root and np.array_equal(tree.nodes, want.nodes)
        assert (tree.tree_nodes, tree.solid_voxels) == (want.tree_nodes, want.solid_voxels)
        assert list(tree.voxel_hist[1:5]) == list(want.voxel_hist[1:5])


def test_two_million_records(ort, gpu_device):
    rec = random_records(100, 2_000_000, 10, ids=(1, 6), dup=0.1, remove=0.05)
    gpu = ort.build_voxels(rec, depth=10, use_gpu=True)
    same_build(gpu, ort.build_voxels(rec, depth=10))
    assert gpu.solid_voxels > 1_500_000 and sum(gpu.voxel_hist[1:6]) == gpu.solid_voxels


def test_million_fold_duplicate(ort, gpu_device):
    """One coordinate's run spans thousands of workgroups; only its last record counts."""
    rec = np.empty((1_000_000, 4), np.uint32)
    rec[:, :3] = (300, 7, 511)
    rec[:, 3] = np.random.default_rng(101).integers(0, 1 << 32, len(rec), dtype=np.uint64)
    for last in (0x80000001, 0):
        rec[-1, 3] = last
        tree = ort.build_voxels(rec, depth=9, use_gpu=True)
        same_build(tree, ort.build_voxels(rec[-1:], depth=9))
        assert tree.at(300, 7, 511) == last and tree.solid_voxels == (last != 0)


def test_solid_box_contention(ort, gpu_device):
    """2^18 equal leaf rows, 2^15 equal rows above, ...: one table slot per level."""
    tree = ort.build_voxels(np.full((128, 128, 128), 2, np.uint8), use_gpu=True)
    assert tree.n_nodes == 7 and tree.solid_voxels == 128 ** 3 and tree.voxel_hist[2] == 128 ** 3
    assert tree.tree_nodes == sum(8 ** k for k in range(7))
    assert np.array_equal(tree.nodes[:6], np.repeat(np.arange(2, 8, dtype=np.uint32), 8).reshape(6, 8))
    assert (tree.nodes[6] == 2).all()


def test_device_tensor_input(ort, gpu_device):
    import torch
    depth, rec = CASES["n20000_d7"]
    host = ort.build_voxels(rec, depth=depth)
    for dtype in (torch.int32, torch.uint32):
        dev = torch.from_numpy(rec.view(np.int32)).cuda().view(dtype)
        same_build(ort.build_voxels(dev, depth=depth, use_gpu=True), host)
    with pytest.raises(ValueError, match="use_gpu"):
        ort.build_voxels(dev, depth=depth)
    with pytest.raises(ValueError):
        ort.build_voxels(dev.view(torch.int32).float(), depth=depth, use_gpu=True)
    empty = torch.zeros((0, 4), dtype=torch.int32, device="cuda")
    assert ort.build_voxels(empty, depth=depth, use_gpu=True).root == 0


def test_two_builds_identical_bytes(ort, gpu_device):
    depth, rec = CASES["n20000_d16"]
    a = ort.build_voxels(rec, depth=depth, use_gpu=True)
    b = ort.build_voxels(rec, depth=depth, use_gpu=True)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.root == b.root


def test_capacity(ort, gpu_device):
    rec = np.array([[5, 6, 7, 1]], np.uint32)
    assert ort.build_voxels(rec, depth=9, capacity=10, use_gpu=True).n_nodes == 9
    with pytest.raises(ort.OchError, match="CAPACITY"):
        ort.build_voxels(rec, depth=9, capacity=9, use_gpu=True)
    # shared subtrees need no ids of their own: 5 unique nodes + id 0
    assert ort.build_voxels(np.full((32, 32, 32), 1, np.uint8), capacity=6, use_gpu=True).n_nodes == 5
    with pytest.raises(ort.OchError, match="CAPACITY"):
        ort.build_voxels(np.full((32, 32, 32), 1, np.uint8), capacity=5, use_gpu=True)


def test_terrain_builder_unchanged(ort, gpu_device):
    g, h = ort.build_terrain(8, use_gpu=True), ort.build_terrain(8)
    assert g.root == h.root and np.array_equal(g.nodes, h.nodes)
    assert (g.tree_nodes, g.solid_voxels, list(g.voxel_hist)) == (h.tree_nodes, h.solid_voxels, list(h.voxel_hist))


@pytest.mark.parametrize("layout", [0, 1])
def test_end_to_end(ort, O, gpu_device, layout):
    """The GPU-built pool uploaded, traced and rendered: bit for bit the oracle on the same pool."""
    depth, rec = 7, random_records(70, 20000, 7)
    tree = ort.build_voxels(rec, depth=depth, use_gpu=True)
    lut = ort.host_rcp_lut()
    ref, rcp = O.OraclePool(tree.nodes, tree.root, depth, 1), O.Rcp(lut)
    rng = np.random.default_rng(72)
    dirs = rng.uniform(-1, 1, (4096, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    org = rng.uniform(1.01, 1.99, (4096, 3)).astype(np.float32)
    colours = ort.VoxelData().get_colours()
    with ort.HOctree(tree.nodes, tree.root, depth, device=0) as pool:
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
