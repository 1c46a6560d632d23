"""Supersampled lit frames (och_gpu_render_lit_ssaa_views_dev, k_trace_lit_ssaa)
against the oracle.

The expected frame comes from the oracle alone: raygen and trace_batch for the
primary rays of the sample grid, the secondary origins in numpy float32 (first
held against O.bounce_ray's origin), one trace_batch per secondary ray kind,
the definition's tests on those records, O.shade_fast, this file's own numpy
shade and then this file's own numpy box mean.  Every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORIGIN = (1.5, 1.5, 1.5)
YAW, FOV = 0.3, 1.25
PITCHES = (0.0, -0.6)
SHAPES = {2: (82, 50), 4: (84, 52), 8: (88, 56)}        # sample grids: multiples of s, none of the 8x8 tile
SKY, INSIDE = 0xFFFEBF00, 0xFF07193F
SENTINEL = 0x5A5A5A5A
SUN = (0.8, 0.35, 0.25)
SUN_SHADE, AO_SHADE = 96, 24
F32 = np.float32


def reach(depth):
    return 8 * 2.0 ** -depth                # eight voxels along each axis


def secondary_origins(o, d, hd, ht, depth):
    """Config 5's secondary origin of every hit, float32 step by step: q = o + d * t
    per axis (product rounded, then the sum), minus +-half a voxel on the hit axis."""
    o, d, t = np.asarray(o, F32), np.asarray(d, F32), np.asarray(ht, F32)
    q = (o[None, :] + (d * t[:, None]).astype(F32)).astype(F32)
    half = F32(2.0 ** -(depth + 1))
    off = np.where(hd < 3, half, -half).astype(F32)
    a = hd % 3
    rows = np.arange(len(hd))
    p = q.copy()
    p[rows, a] = (q[rows, a] - off).astype(F32)
    assert p.dtype == F32
    return p


def ao_dirs(hd, k):
    a = hd % 3
    rows = np.arange(len(hd))
    d = np.empty((len(hd), 3), F32)
    d[rows, a] = np.where(hd < 3, -1.0, 1.0)
    d[rows, (a + 1) % 3] = -1.0 if k & 1 else 1.0
    d[rows, (a + 2) % 3] = -1.0 if k & 2 else 1.0
    return d


class Expected:
    """The oracle's primary records of one sample-grid camera, and the records of its hits' secondary rays."""

    def __init__(self, O, ref, pal, depth, pos, yaw, pitch, w, h, sun=SUN, check_origins=True, fov=FOV):
        self.O, self.ref, self.depth, self.shape = O, ref, depth, (h, w)
        rcp = O.Rcp(None)
        o = np.array(pos, F32)
        rays = O.raygen(yaw, pitch, fov, w, h)
        r = O.trace_batch(ref, rcp, o, rays, nthreads=16)
        self.dir, self.plain = r["dir"], O.shade_fast(r["dir"], r["voxel"], pal)
        self.hit = np.nonzero(r["dir"] < 6)[0]
        self.hd = r["dir"][self.hit].astype(np.int64)
        self.p = secondary_origins(o, rays[self.hit], self.hd, r["t"][self.hit], depth)
        if check_origins:                   # numpy's float32 steps are the oracle's: up to 400 hits spread over the frame
            for i in self.hit[:: max(1, len(self.hit) // 400)]:
                o2, _ = O.bounce_ray(o, rays[i], int(r["dir"][i]), float(r["t"][i]), depth)
                k = np.searchsorted(self.hit, i)
                assert np.array_equal(o2.view(np.uint32), self.p[k].view(np.uint32)), (i, o2, self.p[k])
        self.ao = [O.trace_batch(ref, rcp, self.p, ao_dirs(self.hd, k), nthreads=16) for k in range(4)]
        self._sun = {}
        self.sun_records(sun)

    def sun_records(self, sun):
        key = tuple(float(x) for x in sun)
        if key not in self._sun:
            d = np.broadcast_to(np.array(sun, F32), (len(self.hit), 3)).copy()
            self._sun[key] = self.O.trace_batch(self.ref, self.O.Rcp(None), self.p, d, nthreads=16)
        return self._sun[key]

    def masks(self, flags=3, sun=SUN, ao_reach=None):
        ao_reach = F32(reach(self.depth) if ao_reach is None else ao_reach)
        m = np.full(self.dir.shape, 0x80, np.uint8)
        hm = np.zeros(len(self.hit), np.uint8)
        if flags & 1:
            s = np.array(sun, F32)[self.hd % 3]
            facing = np.where(self.hd < 3, s < 0, s > 0)
            blocked = self.sun_records(sun)["dir"] != 6
            hm |= np.where(~facing, 0x30, np.where(blocked, 0x10, 0)).astype(np.uint8)
        if flags & 2:
            for k, r in enumerate(self.ao):
                occluded = (r["dir"] != 6) & ((r["dir"] == 7) | (r["t"].astype(F32) < ao_reach))
                hm |= (occluded.astype(np.uint8) << k).astype(np.uint8)
        m[self.hit] = hm
        return m.reshape(self.shape)

    def plain_frame(self):
        return self.plain.reshape(self.shape)

    def frame(self, masks):
        """The lit frame at the sample resolution."""
        return shade(self.plain_frame(), masks)

    def resolved(self, s, flags=3, sun=SUN):
        return downsample(self.frame(self.masks(flags, sun)), s)


def shade(frame, masks, sun_shade=SUN_SHADE, ao_shade=AO_SHADE):
    """This file's own shade: per pixel and channel in Python integers' arithmetic (int64)."""
    f, m = frame.astype(np.int64), masks.astype(np.int64)
    count = sum((m >> k) & 1 for k in range(4))
    w = np.where(m == 0x80, 256, 256 - sun_shade * ((m >> 4) & 1) - ao_shade * count)
    out = f & 0xFF000000
    for sh in (0, 8, 16):
        out |= ((((f >> sh) & 0xFF) * w + 128) >> 8) << sh
    return out.astype(np.uint32)


def downsample(frame, s):
    """This file's own box mean: per channel, int64 sums over the s x s block, + s * s / 2, >> 2 log2 s."""
    h, w = frame.shape[0] // s, frame.shape[1] // s
    f = frame.astype(np.int64)
    out = np.zeros((h, w), np.int64)
    for sh in (0, 8, 16, 24):
        total = ((f >> sh) & 0xFF).reshape(h, s, w, s).sum(axis=(1, 3))
        out |= ((total + s * s // 2) // (s * s)) << sh
    return out.astype(np.uint32)


def blocks(a, s):
    """(h / s, w / s, s * s): every output pixel's samples."""
    h, w = a.shape[0] // s, a.shape[1] // s
    return a.reshape(h, s, w, s).transpose(0, 2, 1, 3).reshape(h, w, s * s)


def exercise(e, s, flags=3, sun=SUN):
    """(lighting-edge pixels, sky-mixed pixels, output pixels) of one view, from the oracle's data alone.
    A lighting edge: two face-hit samples of the block with the same plain colour word and different lit
    words -- only the lighting tells them apart.  Sky-mixed: the block holds a face hit and a non-hit."""
    m = e.masks(flags, sun)
    hit, plain, lit = blocks(m != 0x80, s), blocks(e.plain_frame(), s), blocks(e.frame(m), s)
    edge = np.zeros(hit.shape[:2], bool)
    for i in range(s * s):
        for j in range(i + 1, s * s):
            edge |= hit[..., i] & hit[..., j] & (plain[..., i] == plain[..., j]) & (lit[..., i] != lit[..., j])
    mixed = hit.any(axis=2) & ~hit.all(axis=2)
    return int(edge.sum()), int(mixed.sum()), edge.size


def tiles(m):
    """(empty, part-filled, full) 8x8 tiles -- one wave's 64 lanes each -- by their face-hit samples."""
    h, w = m.shape
    e = p = f = 0
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            n = int((m[y:y + 8, x:x + 8] != 0x80).sum())
            e, p, f = e + (n == 0), p + (0 < n < 64), f + (n == 64)
    return e, p, f


def make_light(ort, flags=3, sun=SUN, depth=8):
    return ort.Light(sun, reach(depth), SUN_SHADE, AO_SHADE, flags=flags)


def render(pool, cams, light, s):
    """The device form into a sentinel-filled tensor: (views, H / s, W / s) uint32."""
    import torch
    out = torch.full((len(cams), cams[0].height // s, cams[0].width // s), SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_lit_ssaa_views_dev(cams, light, s, out)
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
def grids(O, d8_ref, pal):
    """The oracle's records of test 1's sample grids, two views per factor; computed once, never changed."""
    return {s: [Expected(O, d8_ref, pal, 8, ORIGIN, YAW, p, w, h) for p in PITCHES] for s, (w, h) in SHAPES.items()}


@pytest.fixture
def pool(ort, gpu_device, d8, pal):
    p = ort.HOctree(d8.nodes, d8.root, 8, device=0)
    p.set_palette(pal)
    yield p
    p.close()


def cameras(ort, s):
    return [ort.camera(ORIGIN, YAW, p, FOV, *SHAPES[s]) for p in PITCHES]


@pytest.mark.parametrize("s", [2, 4, 8])
def test_every_factor_two_views(ort, pool, grids, s):
    """1. Two views in one call at edge shapes.  First, on the oracle's data alone: the frame
    exercises the reduction (sky-mixed blocks) and the lighting (edges only the lighting draws)."""
    views = grids[s]
    for v, e in enumerate(views):
        edge, mixed, n = exercise(e, s)
        print(f"s {s} view {v}: {edge} lighting-edge, {mixed} sky-mixed of {n}")
        assert edge >= 10 and mixed >= 10, (s, v, edge, mixed, n)
        if v == 1:
            assert edge >= 0.2 * n, (s, edge, n)
    if s == 2:
        assert tiles(views[0].masks())[1] >= 10, tiles(views[0].masks())     # pitch 0: tiles the queue has to compact
    got = render(pool, cameras(ort, s), make_light(ort), s)
    assert_same(got, np.stack([e.resolved(s) for e in views]), f"s = {s}")
    assert ((got >> 24) == 0xFF).all()
    assert pool.last_kernel_ms() > 0.0


@pytest.mark.parametrize("s", [2, 4, 8])
def test_flags(ort, pool, grids, s):
    """2. Each ray kind alone, none (render_ssaa_views_dev's frame), and a sun with zero components."""
    import torch
    views, cams = grids[s], cameras(ort, s)
    for flags in (1, 2):
        assert any(exercise(e, s, flags)[0] > 0 for e in views)
        got = render(pool, cams, make_light(ort, flags), s)
        assert_same(got, np.stack([e.resolved(s, flags) for e in views]), f"s = {s}, flags {flags}")
    ws, hs = SHAPES[s]
    plain = torch.full((2, hs // s, ws // s), SENTINEL, dtype=torch.int32, device="cuda")
    pool.render_ssaa_views_dev(cams, s, plain)
    torch.cuda.synchronize()
    got = render(pool, cams, make_light(ort, 0), s)
    assert_same(got, plain.cpu().numpy().view(np.uint32), f"s = {s}, flags 0 vs render_ssaa_views_dev")
    assert_same(got, np.stack([downsample(e.plain_frame(), s) for e in views]), f"s = {s}, flags 0 vs the oracle")
    up = (0.0, 0.0, 1.0)                    # two zero components, every side face self-shadowed
    assert any(exercise(e, s, 3, up)[0] > 0 for e in views)
    got = render(pool, cams, make_light(ort, 3, up), s)
    assert_same(got, np.stack([e.resolved(s, 3, up) for e in views]), f"s = {s}, sun (0, 0, 1)")


def test_special_cameras(ort, O, pool, d8, d8_ref, pal):
    """3. A camera outside the root (no camera shortcut, rays entering through the root's faces)
    and one inside a solid voxel (nothing is a face hit)."""
    s = 2
    outside = (-0.2, 1.5, 1.6)
    e = Expected(O, d8_ref, pal, 8, outside, 0.0, -0.3, 64, 48)
    edge, mixed, n = exercise(e, s)
    print(f"outside: {edge} lighting-edge, {mixed} sky-mixed of {n}")
    assert n == 768 and edge >= 50 and mixed >= 10, (edge, mixed, n)
    got = render(pool, [ort.camera(outside, 0.0, -0.3, FOV, 64, 48)], make_light(ort), s)
    assert_same(got[0], e.resolved(s), "outside")
    inside = (1 + 128.5 / 256, 1 + 128.5 / 256, 1 + 16.5 / 256)       # voxel (128, 128, 16): under the ground
    assert ort._lib.call("och_pool_at", d8.nodes.ctypes.data, int(d8.root), 8, 1, 128, 128, 16) != 0
    got = render(pool, [ort.camera(inside, YAW, -0.2, FOV, 64, 48)], make_light(ort), s)
    assert got.shape == (1, 24, 32) and (got == INSIDE).all()


def test_option_invariance(ort, pool, grids):
    """4. Options change the dispatch only: test 1's s = 4 frame under each of them."""
    s = 4
    cams, light = cameras(ort, s), make_light(ort)
    want = np.stack([e.resolved(s) for e in grids[s]])

    def check(what):
        assert_same(render(pool, cams, light, s), want, what)

    assert pool.get_option("layout") == 1
    check("defaults")
    for compact in (0, 1, 2):
        pool.set_option("bounce_compact", compact)
        for layout in (0, 1):
            pool.set_option("layout", layout)
            for block in (64, 256):
                pool.set_option("block", block)
                check(f"bounce_compact {compact}, layout {layout}, block {block}")
    pool.set_option("bounce_compact", 1)
    pool.set_option("block", 64)
    for name, values in (("cull", (0, 1)), ("tile_order", (1, 0))):
        for v in values:
            pool.set_option(name, v)
            check(f"{name} = {v}")
    # a planned order of the same cameras: used (an unsplit permutation of this grid)
    pool.plan_views(cams)
    pool.set_option("tile_order", 2)
    check("tile_order 2, planned")
    pool.set_option("block", 256)                   # the plan is for block 64: natural order
    check("tile_order 2, stale plan")
    pool.set_option("block", 64)
    # a split plan: the plain render runs its split form, this kernel must not
    for k, v in (("split", 1), ("split_segs", 4), ("split_level", 3)):
        pool.set_option(k, v)
    pool.plan_views(cams)
    assert pool.get_option("split_tiles") > 0
    for compact in (0, 1):
        pool.set_option("bounce_compact", compact)
        check(f"tile_order 2, split plan, bounce_compact {compact}")


def test_depth_12(ort, O, gpu_device, pal):
    """5. Depth 12, a 328 x 200 sample grid at s = 4, blocks 64 and 256: the queue's LDS offset
    follows the depth and the block.  Pitch -0.6 as issued: the oracle gives the lighting edges asked for."""
    s, w, h = 4, 328, 200
    tree = ort.build_terrain(12, use_gpu=True)
    ref = O.OraclePool(tree.nodes, tree.root, 12, 1)
    e = Expected(O, ref, pal, 12, ORIGIN, YAW, -0.6, w, h)
    edge, mixed, n = exercise(e, s)
    print(f"depth 12: {edge} lighting-edge, {mixed} sky-mixed of {n}")
    assert edge >= 50, (edge, mixed, n)
    want = e.resolved(s)
    pool = ort.HOctree(tree.nodes, tree.root, 12, device=0)
    pool.set_palette(pal)
    light = make_light(ort, depth=12)
    cam = [ort.camera(ORIGIN, YAW, -0.6, FOV, w, h)]
    for block in (64, 256):
        pool.set_option("block", block)
        for compact in (1, 0):
            pool.set_option("bounce_compact", compact)
            assert_same(render(pool, cam, light, s)[0], want, f"block {block}, bounce_compact {compact}")
    pool.close()


@pytest.mark.parametrize("s", [2, 4, 8])
def test_equals_the_composition(ort, pool, s):
    """6. The device's own lit frame of the sample cameras, box-averaged on the host, is the fused
    output: a consistency check of two device results, beside the oracle comparison."""
    import torch
    cams, light = cameras(ort, s), make_light(ort)
    ws, hs = SHAPES[s]
    full = torch.full((2, hs, ws), SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_lit_views_dev(cams, light, full)
    torch.cuda.synchronize()
    composed = ort.box_downsample(full.cpu().numpy().view(np.uint32), s)
    assert_same(render(pool, cams, light, s), composed, f"s = {s}")


def test_host_form_and_guards(ort, pool):
    """7. render_lit_ssaa (synchronous, host buffer) equals the device form; every
    refusal is an exception and leaves the output untouched."""
    import torch
    s = 4
    ws, hs = SHAPES[s]
    cams, light = cameras(ort, s), make_light(ort)
    dev = render(pool, cams, light, s)
    for v, cam in enumerate(cams):
        host = pool.render_lit_ssaa(cam, light, s)
        assert host.shape == (hs // s, ws // s) and host.dtype == np.uint32
        assert_same(host, dev[v], f"host form, view {v}")
    w, h = ws // s, hs // s
    out = torch.full((2 * h * w,), SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((out.cpu().numpy().view(np.uint32) == SENTINEL).all())

    with pytest.raises(ort.OchError) as e:                       # s = 3
        pool.render_lit_ssaa_views_dev(cams, light, 3, out)
    assert e.value.status == -1 and untouched()
    narrow = [ort.camera(ORIGIN, YAW, p, FOV, 82, hs) for p in PITCHES]
    with pytest.raises(ort.OchError) as e:                       # 82 is no multiple of 4
        pool.render_lit_ssaa_views_dev(narrow, light, s, out)
    assert e.value.status == -1 and untouched()
    with pytest.raises(ort.OchError) as e:                       # the host form checks the same
        pool.render_lit_ssaa(narrow[0], light, s)
    assert e.value.status == -1
    unequal = [cams[0], ort.camera(ORIGIN, YAW, PITCHES[1], FOV, ws + 4, hs)]
    with pytest.raises(ort.OchError) as e:                       # views of unequal size
        pool.render_lit_ssaa_views_dev(unequal, light, s, out)
    assert e.value.status == -1 and untouched()
    with pytest.raises(ValueError):                              # a tensor one pixel short: the wrapper's check
        pool.render_lit_ssaa_views_dev(cams, light, s, out[:-1])
    assert untouched()
    with pytest.raises(ort.OchError) as e:                       # and the library's own, by the stated capacity
        pool.render_lit_ssaa_views_dev(cams, light, s, out.data_ptr(), capacity_pixels=2 * h * w - 1)
    assert e.value.status == -1 and untouched()
    bad = ort.Light(SUN, reach(8), 300, 0)
    with pytest.raises(ort.OchError) as e:                       # a light och_light_check refuses
        pool.render_lit_ssaa_views_dev(cams, bad, s, out)
    assert e.value.status == -1 and untouched()
    with pytest.raises(ort.OchError) as e:
        pool.render_lit_ssaa(cams[0], bad, s)
    assert e.value.status == -1
    # the same buffer at its true capacity is accepted
    pool.render_lit_ssaa_views_dev(cams, light, s, out.data_ptr(), capacity_pixels=2 * h * w)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().view(np.uint32).reshape(2, h, w), dev, "raw pointer")


@pytest.mark.parametrize("flags", [("--ssaa", "2", "--lit"), ("--lit", "--ssaa", "2")])
def test_example_both_arguments(ort, O, gpu_device, d8_ref, pal, tmp_path, flags):
    """8. examples/render_frame --ssaa 2 --lit, in either order: the PPM is the oracle's lit
    82 x 50 frame of that camera, downsampled."""
    import re
    import subprocess
    from conftest import ROOT
    exe = ROOT / "examples" / "render_frame"
    if not exe.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "examples")], check=True)
    w, h, s = 41, 25, 2
    out = tmp_path / "lit_ssaa.ppm"
    r = subprocess.run([str(exe), "8", str(out), str(w), str(h), str(YAW), "-0.6", *flags],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    assert (int(m.group(1)), int(m.group(2))) == (w, h)
    got = np.frombuffer(data[m.end():], np.uint8).reshape(h, w, 3)
    e = Expected(O, d8_ref, pal, 8, ORIGIN, YAW, -0.6, w * s, h * s, check_origins=False)
    want = e.resolved(s)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(h, w, 4)[..., :3])
