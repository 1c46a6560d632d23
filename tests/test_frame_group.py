"""och_frame_group_*: multi-GPU frames from one host process (SURVEY §8(e):
one process, ncclCommInitAll over the devices, RCCL all-gather of the slices).

On the one-GPU test box the group has one device: the RCCL communicator, the
all-gather and the shade + unshard still run, and the frames must equal the
oracle's (and the single-pool render's) bit for bit."""
import ctypes as C

import numpy as np
import pytest

ORIGIN = np.array([1.5, 1.5, 1.5], np.float32)
PITCHES = (0.0, -0.6)


def test_group_needs_devices(ort):
    """Argument checks that need no GPU; without one the group reports OCH_E_NODEV."""
    import torch
    nodes = np.zeros((1, 8), np.uint32)
    nodes[0, 0] = 1
    with pytest.raises(ort.OchError):
        ort.FrameGroup(nodes, 1, 1, devices=[])
    if not torch.cuda.is_available():
        with pytest.raises(ort.OchError, match="NODEV"):
            ort.FrameGroup(nodes, 1, 1, devices=[0])


@pytest.mark.gpu
@pytest.mark.parametrize("bounce", [False, True])
def test_group_one_device_matches_oracle(ort, O, gpu_device, bounce):
    depth, W, H = 10, 1280, 720
    tree = ort.build_terrain(depth)
    pal = ort.VoxelData().get_colours()
    g = ort.FrameGroup(tree.nodes, tree.root, depth, devices=[0])
    g.set_palette(pal)
    g.set_option("cull", 1)                     # every replica's option; the cull is exact (and on by default)
    cams = [ort.camera(tuple(ORIGIN), 0.3, p, 1.25, W, H) for p in PITCHES]
    ref_pool = O.OraclePool(tree.nodes, tree.root, depth, 1)
    want = []
    for p in PITCHES:
        rays = O.raygen(0.3, p, 1.25, W, H)
        if bounce:
            r = O.trace_bounce_batch(ref_pool, O.Rcp(None), ORIGIN, rays, nthreads=16)
            want.append(O.shade_bounce(r["dir"], r["voxel"], r["dir2"], pal).reshape(H, W))
        else:
            r = O.trace_batch(ref_pool, O.Rcp(None), ORIGIN, rays, nthreads=16)
            want.append(O.shade_fast(r["dir"], r["voxel"], pal).reshape(H, W))
    for chunk in (8, 5):
        g.render(cams, row_chunk=chunk, bounce=bounce)
        got = g.download(0)
        for v in range(2):
            assert np.array_equal(got[v], want[v]), (chunk, v)
    g.plan(cams, row_chunk=8)                   # planned launch order (tile_order 2)
    g.render(cams, row_chunk=8, bounce=bounce)
    got = g.download(0)
    for v in range(2):
        assert np.array_equal(got[v], want[v]), ("planned", v)
    # a palette of more than OCH_CODE_MAX_VOXELS ids: RGBA8 slices travel instead of codes
    big = np.resize(np.asarray(pal, np.uint32).reshape(-1), 6 * 24)
    g.set_palette(big)
    g.render(cams, row_chunk=8, bounce=bounce)
    got = g.download(0)
    pool = ort.HOctree(tree.nodes, tree.root, depth, device=0)
    pool.set_palette(big)
    for v, cam in enumerate(cams):
        if not bounce:
            assert np.array_equal(got[v], pool.render(cam))
    pool.close()
    g.close()


@pytest.mark.gpu
def test_group_rejects_duplicates(ort, gpu_device):
    tree = ort.build_terrain(4)
    with pytest.raises(ort.OchError):
        ort.FrameGroup(tree.nodes, tree.root, 4, devices=[0, 0])
    import torch
    with pytest.raises(ort.OchError):
        ort.FrameGroup(tree.nodes, tree.root, 4, devices=[torch.cuda.device_count()])


@pytest.mark.gpu
def test_group_checks_before_queueing(ort, O, gpu_device):
    """A frame the group cannot complete is refused before any device queues
    its render or all-gather (a palette-less group cannot shade): the group
    stays usable -- no communicator aborted -- and renders once a palette is
    set; destroy releases the pools before the streams they point at."""
    tree = ort.build_terrain(6)
    g = ort.FrameGroup(tree.nodes, tree.root, 6, devices=[0])
    cams = [ort.camera(tuple(ORIGIN), 0.3, p, 1.25, 64, 40) for p in PITCHES]
    with pytest.raises(ort.OchError, match="palette"):
        g.render(cams)
    pal = ort.VoxelData().get_colours()
    g.set_palette(pal)
    g.render_steps(cams, 3, n_buffers=2)
    got = g.download(0)
    ref_pool = O.OraclePool(tree.nodes, tree.root, 6, 1)
    for v, p in enumerate(PITCHES):
        r = O.trace_batch(ref_pool, O.Rcp(None), ORIGIN, O.raygen(0.3, p, 1.25, 64, 40))
        assert np.array_equal(got[v], O.shade(r["dir"], r["voxel"], pal).reshape(40, 64))
    g.close()


@pytest.fixture(scope="module")
def small_scene(ort, O):
    """Depth 6, two 64x40 views: the tree, the cameras and the oracle's hit records (dir, voxel) per view."""
    tree = ort.build_terrain(6)
    cams = [ort.camera(tuple(ORIGIN), 0.3, p, 1.25, 64, 40) for p in PITCHES]
    ref_pool = O.OraclePool(tree.nodes, tree.root, 6, 1)
    hits = []
    for p in PITCHES:
        r = O.trace_batch(ref_pool, O.Rcp(None), ORIGIN, O.raygen(0.3, p, 1.25, 64, 40))
        hits.append((r["dir"].copy(), r["voxel"].copy()))
    return tree, cams, hits


@pytest.mark.gpu
def test_palette_regrow(ort, O, gpu_device, small_scene):
    """The palette and the code table are released, not shrunk, when a palette
    no longer fits the colour codes: a 24-id palette leaves no code table (the
    codes path refuses), the RGBA8 path shades with it, and the small palette
    brings the codes path back, each frame equal to the oracle's."""
    import torch
    from octree_ray_tracing_amd.frame import ShardedFrame
    tree, cams, hits = small_scene
    pal = ort.VoxelData().get_colours()
    big = np.resize(pal[::-1], 6 * 24)           # other colours than pal's for the ids the scene holds
    assert pal.size // 6 <= 20 < big.size // 6   # OCH_CODE_MAX_VOXELS
    want = {name: [O.shade(d, v, colours).reshape(40, 64) for d, v in hits] for name, colours in (("pal", pal), ("big", big))}
    assert not np.array_equal(want["pal"][1], want["big"][1])

    def codes_frames(pool):
        frames = ShardedFrame(pool, 64, 40, 8, n_views=2, indexed=True).render(cams)
        torch.cuda.synchronize()
        return frames.cpu().numpy().view(np.uint32)

    with ort.HOctree(tree.nodes, tree.root, 6, device=0) as pool:
        pool.set_palette(pal)
        got = codes_frames(pool)
        for v in range(2):
            assert np.array_equal(got[v], want["pal"][v]), ("codes", v)
        pool.set_palette(big)
        codes = torch.empty((2, 40, 64), dtype=torch.uint8, device="cuda")
        with pytest.raises(ort.OchError):
            pool.render_codes_views_dev(cams, codes, 8, 0, 1)
        for v in range(2):
            assert np.array_equal(pool.render(cams[v]), want["big"][v]), ("rgba", v)
        pool.set_palette(pal)
        got = codes_frames(pool)
        for v in range(2):
            assert np.array_equal(got[v], want["pal"][v]), ("codes again", v)


@pytest.mark.gpu
def test_group_restores_pool_stream(ort, O, gpu_device, small_scene):
    """After a window of group frames each replica enqueues on the stream it
    had before, not on one of the group's: a plain render on the replica and
    the group's last frame both equal the oracle's, and the group closes."""
    tree, cams, hits = small_scene
    pal = ort.VoxelData().get_colours()
    want = [O.shade(d, v, pal).reshape(40, 64) for d, v in hits]
    g = ort.FrameGroup(tree.nodes, tree.root, 6, devices=[0])
    g.set_palette(pal)
    g.render_steps(cams, 3, n_buffers=2)
    g.synchronize()
    replica = C.c_void_p()
    ort._lib.call("och_frame_group_pool", g._h, 0, C.byref(replica))
    out = np.empty((40, 64), np.uint32)
    ort._lib.call("och_gpu_render", replica, C.byref(cams[1]), out.ctypes.data)
    assert np.array_equal(out, want[1])
    got = g.download(0)
    for v in range(2):
        assert np.array_equal(got[v], want[v]), v
    g.close()
