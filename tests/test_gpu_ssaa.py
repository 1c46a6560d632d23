"""Supersampled frames (och_gpu_render_ssaa_views_dev, k_trace_ssaa) against
the oracle: the expected frame is the box mean, rounded half up per 8-bit
channel, of the oracle's frame at the sample resolution (trace_batch +
shade_fast on raygen's rays), downsampled here with this file's own numpy
code.  Every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORIGIN = (1.5, 1.5, 1.5)
YAW, FOV = 0.3, 1.25
PITCHES = (0.0, -0.6)                       # the horizon crosses both frames (chosen on the CPU, see test 1)
SKY, INSIDE = 0xFFFEBF00, 0xFF07193F
SENTINEL = 0x5A5A5A5A
# s, sample grid: widths and heights that are no multiple of the 8x8 tile
SHAPES = {2: (82, 50), 4: (84, 52), 8: (88, 56)}


def downsample(frame, s):
    """(Hs, Ws) RGBA8 words -> (Hs / s, Ws / s): per byte (sum + s*s/2) >> 2 log2 s."""
    hs, ws = frame.shape
    b = np.ascontiguousarray(frame).view(np.uint8).reshape(hs // s, s, ws // s, s, 4).astype(np.uint32)
    mean = (b.sum(axis=(1, 3)) + s * s // 2) >> (2 * (s.bit_length() - 1))
    assert mean.max() <= 255
    return np.ascontiguousarray(mean.astype(np.uint8)).view(np.uint32).reshape(hs // s, ws // s)


def oracle_frame(O, ref, pal, pos, yaw, pitch, ws, hs):
    r = O.trace_batch(ref, O.Rcp(None), np.array(pos, np.float32), O.raygen(yaw, pitch, FOV, ws, hs), nthreads=16)
    return O.shade_fast(r["dir"], r["voxel"], pal).reshape(hs, ws)


def render(pool, cams, s):
    """The device form into a sentinel-filled tensor: (views, H / s, W / s) words."""
    import torch
    w, h = cams[0].width // s, cams[0].height // s
    out = torch.full((len(cams), h, w), SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_ssaa_views_dev(cams, s, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {want.size} pixels differ, first {bad[:4].tolist()}: "
                           f"got {[hex(int(got[tuple(b)])) for b in bad[:4]]}, "
                           f"want {[hex(int(want[tuple(b)])) for b in bad[:4]]}")


@pytest.fixture(scope="module")
def pal(ort):
    return ort.VoxelData().get_colours()


@pytest.fixture(scope="module")
def d8(ort):
    return ort.build_terrain(8)


@pytest.fixture(scope="module")
def d8_ref(O, d8):
    return O.OraclePool(d8.nodes, d8.root, 8, 1)


@pytest.fixture(scope="module")
def samples(O, d8_ref, pal):
    """The oracle's frames at the sample resolution of every shape, both pitches; computed once."""
    return {s: [oracle_frame(O, d8_ref, pal, ORIGIN, YAW, p, ws, hs) for p in PITCHES]
            for s, (ws, hs) in SHAPES.items()}


@pytest.fixture
def pool(ort, gpu_device, d8, pal):
    p = ort.HOctree(d8.nodes, d8.root, 8, device=0)
    p.set_palette(pal)
    yield p
    p.close()


@pytest.mark.parametrize("s", [2, 4, 8])
def test_edge_shapes_two_views(ort, pool, samples, s):
    """1. Sample grids that are no multiple of the tile, every factor, two views in one call."""
    ws, hs = SHAPES[s]
    for f in samples[s]:
        # the reduction is exercised only by blocks whose samples differ: at
        # least 5 % of the output pixels, and some mixing sky with a hit (the
        # camera above was chosen on the CPU so that the oracle alone shows both)
        blocks = f.reshape(hs // s, s, ws // s, s).transpose(0, 2, 1, 3).reshape(hs // s, ws // s, s * s)
        mixed = (blocks != blocks[..., :1]).any(-1)
        assert mixed.mean() >= 0.05, mixed.mean()
        assert ((blocks == SKY).any(-1) & (blocks != SKY).any(-1)).any()
    cams = [ort.camera(ORIGIN, YAW, p, FOV, ws, hs) for p in PITCHES]
    got = render(pool, cams, s)
    assert_same(got, np.stack([downsample(f, s) for f in samples[s]]), f"s = {s}")
    assert (got >> 24 == 0xFF).all()


def test_special_cameras(ort, O, pool, d8, d8_ref, pal):
    """2. A camera inside a solid voxel (the INSIDE colour everywhere) and one
    outside the root (no camera shortcut: pos_ok = 0), s = 2 at 64 x 48 samples."""
    inside = (1 + 128.5 / 256, 1 + 128.5 / 256, 1 + 16.5 / 256)       # voxel (128, 128, 16): under the ground
    assert ort._lib.call("och_pool_at", d8.nodes.ctypes.data, int(d8.root), 8, 1, 128, 128, 16) != 0
    got = render(pool, [ort.camera(inside, YAW, -0.2, FOV, 64, 48)], 2)
    assert_same(got[0], downsample(oracle_frame(O, d8_ref, pal, inside, YAW, -0.2, 64, 48), 2), "inside")
    assert (got == INSIDE).all()
    outside = (-0.2, 1.5, 1.6)
    want = oracle_frame(O, d8_ref, pal, outside, 0.0, -0.3, 64, 48)
    assert (want == SKY).any() and (want != SKY).any()
    got = render(pool, [ort.camera(outside, 0.0, -0.3, FOV, 64, 48)], 2)
    assert_same(got[0], downsample(want, 2), "outside")


def test_option_invariance(ort, pool, samples):
    """3. Options change the dispatch only: the s = 4 frame of test 1 under each of them."""
    s = 4
    ws, hs = SHAPES[s]
    cams = [ort.camera(ORIGIN, YAW, p, FOV, ws, hs) for p in PITCHES]
    want = np.stack([downsample(f, s) for f in samples[s]])
    assert pool.get_option("layout") == 1
    first = render(pool, cams, s)
    assert_same(first, want, "defaults")
    for name, values in (("layout", (0, 1)), ("block", (256, 64)), ("cull", (0, 1)), ("tile_order", (1, 0))):
        for v in values:
            pool.set_option(name, v)
            assert_same(render(pool, cams, s), first, f"{name} = {v}")
    # a planned order of the same cameras: used (an unsplit permutation of this grid)
    pool.plan_views(cams)
    pool.set_option("tile_order", 2)
    assert_same(render(pool, cams, s), first, "tile_order 2, planned")
    pool.set_option("block", 256)                   # the plan is for block 64: natural order
    assert_same(render(pool, cams, s), first, "tile_order 2, stale plan")
    pool.set_option("block", 64)
    # a split plan: the 1-sample render runs its split form, this kernel must not
    for k, v in (("split", 1), ("split_segs", 4), ("split_level", 3)):
        pool.set_option(k, v)
    pool.plan_views(cams)
    assert pool.get_option("split_tiles") > 0
    assert_same(render(pool, cams, s), first, "tile_order 2, split plan")


def test_workload_scale(ort, O, gpu_device, pal):
    """4. Depth 12, 1920 x 1080 samples at s = 2, two views: against the oracle's
    frames and against render_views_dev's own frames, both downsampled here."""
    import torch
    ws, hs, s = 1920, 1080, 2
    tree = ort.build_terrain(12, use_gpu=True)
    ref = O.OraclePool(tree.nodes, tree.root, 12, 1)
    pool = ort.HOctree(tree.nodes, tree.root, 12, device=0)
    pool.set_palette(pal)
    cams = [ort.camera(ORIGIN, YAW, p, FOV, ws, hs) for p in PITCHES]
    got = render(pool, cams, s)
    full = torch.full((2, hs, ws), SENTINEL, dtype=torch.int32, device="cuda")
    pool.render_views_dev(cams, full)
    torch.cuda.synchronize()
    full = full.cpu().numpy().view(np.uint32)
    for v, p in enumerate(PITCHES):
        assert_same(got[v], downsample(full[v], s), f"view {v} vs render_views_dev")
        assert_same(got[v], downsample(oracle_frame(O, ref, pal, ORIGIN, YAW, p, ws, hs), s), f"view {v} vs oracle")
    pool.close()


def test_host_form_and_guards(ort, pool, samples):
    """5. render_ssaa (synchronous, host buffer) equals the device form; every
    refusal is an exception and leaves the output untouched."""
    import torch
    s = 4
    ws, hs = SHAPES[s]
    cams = [ort.camera(ORIGIN, YAW, p, FOV, ws, hs) for p in PITCHES]
    dev = render(pool, cams, s)
    for v, cam in enumerate(cams):
        host = pool.render_ssaa(cam, s)
        assert host.shape == (hs // s, ws // s) and host.dtype == np.uint32
        assert_same(host, dev[v], f"host form, view {v}")
    w, h = ws // s, hs // s
    out = torch.full((2 * h * w,), SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((out.cpu().numpy().view(np.uint32) == SENTINEL).all())

    with pytest.raises(ort.OchError) as e:                       # s = 3
        pool.render_ssaa_views_dev(cams, 3, out)
    assert e.value.status == -1 and untouched()
    narrow = [ort.camera(ORIGIN, YAW, p, FOV, 82, hs) for p in PITCHES]
    with pytest.raises(ort.OchError) as e:                       # 82 is no multiple of 4
        pool.render_ssaa_views_dev(narrow, s, out)
    assert e.value.status == -1 and untouched()
    with pytest.raises(ort.OchError) as e:                       # the host form checks the same
        pool.render_ssaa(narrow[0], s)
    assert e.value.status == -1
    unequal = [cams[0], ort.camera(ORIGIN, YAW, PITCHES[1], FOV, ws + 4, hs)]
    with pytest.raises(ort.OchError) as e:                       # views of unequal size
        pool.render_ssaa_views_dev(unequal, s, out)
    assert e.value.status == -1 and untouched()
    with pytest.raises(ValueError):                              # a tensor one pixel short: the wrapper's check
        pool.render_ssaa_views_dev(cams, s, out[:-1])
    assert untouched()
    with pytest.raises(ort.OchError) as e:                       # and the library's own, by the stated capacity
        pool.render_ssaa_views_dev(cams, s, out.data_ptr(), capacity_pixels=2 * h * w - 1)
    assert e.value.status == -1 and untouched()
    # the same buffer at its true capacity is accepted
    pool.render_ssaa_views_dev(cams, s, out.data_ptr(), capacity_pixels=2 * h * w)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().view(np.uint32).reshape(2, h, w), dev, "raw pointer")


def test_example_ssaa_argument(ort, O, gpu_device, d8_ref, pal, tmp_path):
    """examples/render_frame --ssaa 2: the PPM is the downsampled oracle frame of the sample grid."""
    import re
    import subprocess
    from conftest import ROOT
    exe = ROOT / "examples" / "render_frame"
    if not exe.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "examples")], check=True)
    w, h, s = 41, 25, 2
    out = tmp_path / "ssaa.ppm"
    r = subprocess.run([str(exe), "8", str(out), str(w), str(h), str(YAW), "-0.6", "--ssaa", str(s)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    assert (int(m.group(1)), int(m.group(2))) == (w, h)
    got = np.frombuffer(data[m.end():], np.uint8).reshape(h, w, 3)
    want = downsample(oracle_frame(O, d8_ref, pal, ORIGIN, YAW, -0.6, w * s, h * s), s)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(h, w, 4)[..., :3])


def test_kernel_time_is_reported(ort, pool):
    """6. och_gpu_last_kernel_ms after a supersampled launch."""
    ws, hs = SHAPES[2]
    render(pool, [ort.camera(ORIGIN, YAW, p, FOV, ws, hs) for p in PITCHES], 2)
    assert pool.last_kernel_ms() > 0.0
