"""Lit frames (och_gpu_render_lit_views_dev, k_trace_lit) against the oracle.

The expected masks come from the oracle alone: raygen and trace_batch for the
primary rays, the secondary origins in numpy float32 (first held against
O.bounce_ray's origin), one trace_batch per secondary ray kind, and the
definition's tests on those records.  The expected frame is O.shade_fast
followed by this file's own numpy shade.  Every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORIGIN = (1.5, 1.5, 1.5)
YAW, FOV = 0.3, 1.25
PITCHES = (0.0, -0.6)
W, H = 82, 50                               # no multiple of the 8x8 tile
SKY, INSIDE = 0xFFFEBF00, 0xFF07193F
SENTINEL, SENTINEL8 = 0x5A5A5A5A, 0x5A
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
    """The oracle's primary records of one camera, and the records of its hits' secondary rays."""

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

    def frame(self, masks):
        return shade(self.plain.reshape(self.shape), masks)


def shade(frame, masks, sun_shade=SUN_SHADE, ao_shade=AO_SHADE):
    """This file's own shade: per pixel and channel in Python integers' arithmetic (int64)."""
    f, m = frame.astype(np.int64), masks.astype(np.int64)
    count = sum((m >> k) & 1 for k in range(4))
    w = np.where(m == 0x80, 256, 256 - sun_shade * ((m >> 4) & 1) - ao_shade * count)
    out = f & 0xFF000000
    for sh in (0, 8, 16):
        out |= ((((f >> sh) & 0xFF) * w + 128) >> 8) << sh
    return out.astype(np.uint32)


def count_bins(m):
    hits = m[m != 0x80]
    return np.bincount(np.array([bin(int(x) & 15).count("1") for x in hits], np.int64), minlength=5)


def tiles(m):
    """(empty, part-filled, full) 8x8 tiles -- one wave's 64 lanes each -- by their face-hit pixels."""
    h, w = m.shape
    e = p = f = 0
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            n = int((m[y:y + 8, x:x + 8] != 0x80).sum())
            e, p, f = e + (n == 0), p + (0 < n < 64), f + (n == 64)
    return e, p, f


def make_light(ort, flags=3, sun=SUN, depth=8):
    return ort.Light(sun, reach(depth), SUN_SHADE, AO_SHADE, flags=flags)


def render(pool, cams, light, **kw):
    """Both device forms into sentinel-filled tensors: (frames, masks) as numpy, one slice per view."""
    import torch
    rows = pool.slice_rows(cams[0].height, kw.get("row_chunk") or cams[0].height, kw.get("n_shards", 1))
    rgba = torch.full((len(cams), rows, cams[0].width), SENTINEL, dtype=torch.int32, device="cuda")
    masks = torch.full((len(cams), rows, cams[0].width), SENTINEL8, dtype=torch.uint8, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_lit_views_dev(cams, light, rgba, **kw)
    pool.render_lit_masks_views_dev(cams, light, masks, **kw)
    torch.cuda.synchronize()
    return rgba.cpu().numpy().view(np.uint32), masks.cpu().numpy()


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
def views(O, d8_ref, pal):
    """The oracle's records of test 1's two cameras; computed once, never changed."""
    return [Expected(O, d8_ref, pal, 8, ORIGIN, YAW, p, W, H) for p in PITCHES]


@pytest.fixture
def pool(ort, gpu_device, d8, pal):
    p = ort.HOctree(d8.nodes, d8.root, 8, device=0)
    p.set_palette(pal)
    yield p
    p.close()


def cameras(ort):
    return [ort.camera(ORIGIN, YAW, p, FOV, W, H) for p in PITCHES]


def test_masks_and_frames_two_views(ort, pool, views):
    """1. Two views in one call, sentinel-filled outputs, masks and frames."""
    want_m = [v.masks() for v in views]
    m = want_m[1]                                          # pitch -0.6: every case of the definition is present
    assert (count_bins(m) > 0).all(), count_bins(m)
    hits = m[m != 0x80]
    assert ((hits & 0x10) == 0).any() and ((hits & 0x30) == 0x10).any() and ((hits & 0x30) == 0x30).any()
    assert tiles(want_m[0])[1] >= 10, tiles(want_m[0])     # pitch 0: tiles the queue has to compact
    assert all((x == 0x80).any() and (x != 0x80).any() for x in want_m)
    got_f, got_m = render(pool, cameras(ort), make_light(ort))
    assert_same(got_m, np.stack(want_m), "masks")
    assert_same(got_f, np.stack([v.frame(x) for v, x in zip(views, want_m)]), "frames")
    assert pool.last_kernel_ms() > 0.0


def test_flags(ort, pool, views):
    """2. Each ray kind alone, none, and a sun with zero components."""
    import torch
    cams = cameras(ort)
    for flags in (1, 2):
        want_m = [v.masks(flags) for v in views]
        assert any(((x != 0x80) & (x != 0)).any() for x in want_m)
        got_f, got_m = render(pool, cams, make_light(ort, flags))
        assert_same(got_m, np.stack(want_m), f"masks, flags {flags}")
        assert_same(got_f, np.stack([v.frame(x) for v, x in zip(views, want_m)]), f"frames, flags {flags}")
    # no flags: the plain render's frame word for word, masks 0 on hits
    plain = torch.full((2, H, W), SENTINEL, dtype=torch.int32, device="cuda")
    pool.render_views_dev(cams, plain)
    torch.cuda.synchronize()
    got_f, got_m = render(pool, cams, make_light(ort, 0))
    assert_same(got_f, plain.cpu().numpy().view(np.uint32), "flags 0 vs render_views_dev")
    assert_same(got_m, np.stack([v.masks(0) for v in views]), "masks, flags 0")
    # the sun straight up: two zero components, every side face self-shadowed
    up = (0.0, 0.0, 1.0)
    want_m = [v.masks(3, up) for v in views]
    pairs = {(int(x) >> 4 & 1, bin(int(x) & 15).count("1")) for x in want_m[1][want_m[1] != 0x80]}
    assert len(pairs) == 10, sorted(pairs)
    got_f, got_m = render(pool, cams, make_light(ort, 3, up))
    assert_same(got_m, np.stack(want_m), "masks, sun (0, 0, 1)")
    assert_same(got_f, np.stack([v.frame(x) for v, x in zip(views, want_m)]), "frames, sun (0, 0, 1)")


def test_special_cameras(ort, O, pool, d8, d8_ref, pal):
    """3. A camera outside the root (no camera shortcut, rays entering through the root's faces)
    and one inside a solid voxel (nothing is a face hit)."""
    outside = (-0.2, 1.5, 1.6)
    e = Expected(O, d8_ref, pal, 8, outside, 0.0, -0.3, 64, 48)
    want_m = e.masks()
    assert 0.3 < (want_m != 0x80).mean() < 0.7 and (count_bins(want_m) > 0).all(), count_bins(want_m)
    got_f, got_m = render(pool, [ort.camera(outside, 0.0, -0.3, FOV, 64, 48)], make_light(ort))
    assert_same(got_m[0], want_m, "outside, masks")
    assert_same(got_f[0], e.frame(want_m), "outside, frame")
    inside = (1 + 128.5 / 256, 1 + 128.5 / 256, 1 + 16.5 / 256)       # voxel (128, 128, 16): under the ground
    assert ort._lib.call("och_pool_at", d8.nodes.ctypes.data, int(d8.root), 8, 1, 128, 128, 16) != 0
    got_f, got_m = render(pool, [ort.camera(inside, YAW, -0.2, FOV, 64, 48)], make_light(ort))
    assert (got_m == 0x80).all() and (got_f == INSIDE).all()


def test_option_invariance(ort, pool, views):
    """4. Options change the dispatch only: test 1's frames and masks under each of them."""
    cams = cameras(ort)
    light = make_light(ort)
    want_m = np.stack([v.masks() for v in views])
    want_f = np.stack([v.frame(x) for v, x in zip(views, want_m)])

    def check(what):
        got_f, got_m = render(pool, cams, light)
        assert_same(got_m, want_m, f"masks, {what}")
        assert_same(got_f, want_f, f"frames, {what}")

    assert pool.get_option("layout") == 1
    check("defaults")
    for compact in (0, 1, 2):
        pool.set_option("bounce_compact", compact)
        for name, values in (("layout", (0, 1)), ("block", (256, 64))):
            for v in values:
                pool.set_option(name, v)
                check(f"bounce_compact {compact}, {name} = {v}")
    pool.set_option("bounce_compact", 1)
    for name, values in (("cull", (0, 1)), ("tile_order", (1, 0))):
        for v in values:
            pool.set_option(name, v)
            check(f"{name} = {v}")
    pool.set_option("layout", 0)
    pool.set_option("block", 256)
    check("layout 0, block 256")
    pool.set_option("layout", 1)
    pool.set_option("block", 64)
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


def test_sharding(ort, pool, views):
    """5. row_chunk 8 over 3 shards: the slices, reassembled by unshard_dev, are the whole frame."""
    import torch
    cams, light = cameras(ort), make_light(ort)
    want_m = np.stack([v.masks() for v in views])
    want_f = np.stack([v.frame(x) for v, x in zip(views, want_m)])
    n, chunk = 3, 8
    rows = pool.slice_rows(H, chunk, n)
    assert rows * n > H                             # the last chunks are short or missing: padding rows exist
    parts_f, parts_m = [], []
    for s in range(n):
        f, m = render(pool, cams, light, row_chunk=chunk, shard=s, n_shards=n)
        parts_f.append(f)
        parts_m.append(m)
    gathered = torch.from_numpy(np.stack(parts_f).view(np.int32)).cuda()        # [shard][view][rows][W]
    whole = torch.full((2, H, W), SENTINEL, dtype=torch.int32, device="cuda")
    pool.unshard_dev(gathered, whole, W, H, chunk, n, n_views=2)
    torch.cuda.synchronize()
    assert_same(whole.cpu().numpy().view(np.uint32), want_f, "unsharded frames")
    # the mask slices, row by row on the host (the deal is round-robin chunks)
    for s in range(n):
        rmap = ort.frame.slice_row_map(H, chunk, n, s)
        ok = rmap >= 0
        assert_same(parts_m[s][:, ok], want_m[:, rmap[ok]], f"mask slice {s}")
        assert (parts_m[s][:, ~ok] == SENTINEL8).all() and (parts_f[s][:, ~ok] == SENTINEL).all()


def test_depth_12_block_256(ort, O, gpu_device, pal):
    """6. Depth 12, 160 x 96, block 256: the queue and the stacks at their largest together."""
    w, h = 160, 96
    tree = ort.build_terrain(12, use_gpu=True)
    ref = O.OraclePool(tree.nodes, tree.root, 12, 1)
    e = Expected(O, ref, pal, 12, ORIGIN, YAW, -0.6, w, h)
    want_m = e.masks()
    assert (count_bins(want_m) > 0).all() and (want_m == 0x80).any(), count_bins(want_m)
    pool = ort.HOctree(tree.nodes, tree.root, 12, device=0)
    pool.set_palette(pal)
    pool.set_option("block", 256)
    light = make_light(ort, depth=12)
    cam = [ort.camera(ORIGIN, YAW, -0.6, FOV, w, h)]
    for compact in (1, 0):
        pool.set_option("bounce_compact", compact)
        got_f, got_m = render(pool, cam, light)
        assert_same(got_m[0], want_m, f"masks, bounce_compact {compact}")
        assert_same(got_f[0], e.frame(want_m), f"frame, bounce_compact {compact}")
    pool.close()


def test_host_form_and_guards(ort, pool, views):
    """7. render_lit (synchronous, host buffer) equals the device form; every
    refusal is an exception and leaves the output untouched."""
    import torch
    cams, light = cameras(ort), make_light(ort)
    dev_f, _ = render(pool, cams, light)
    for v, cam in enumerate(cams):
        host = pool.render_lit(cam, light)
        assert host.shape == (H, W) and host.dtype == np.uint32
        assert_same(host, dev_f[v], f"host form, view {v}")
    out = torch.full((2 * H * W,), SENTINEL, dtype=torch.int32, device="cuda")
    out8 = torch.full((2 * H * W,), SENTINEL8, dtype=torch.uint8, device="cuda")
    pool.set_stream(torch.cuda.current_stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((out.cpu().numpy().view(np.uint32) == SENTINEL).all() and (out8.cpu().numpy() == SENTINEL8).all())

    forms = ((pool.render_lit_views_dev, out), (pool.render_lit_masks_views_dev, out8))
    for fn, buf in forms:
        with pytest.raises(ort.OchError) as e:                       # the library's check, by the stated capacity
            fn(cams, light, buf.data_ptr(), capacity_pixels=2 * H * W - 1)
        assert e.value.status == -1 and untouched()
        with pytest.raises(ValueError):                              # a tensor one pixel short: the wrapper's check
            fn(cams, light, buf[:-1])
        assert untouched()
        unequal = [cams[0], ort.camera(ORIGIN, YAW, PITCHES[1], FOV, W - 2, H)]
        with pytest.raises(ort.OchError) as e:                       # views of unequal size
            fn(unequal, light, buf)
        assert e.value.status == -1 and untouched()
        for bad in (ort.Light(SUN, reach(8), 96, 41), ort.Light((0, 0, 0), reach(8)), ort.Light(SUN, 0.0),
                    ort.Light(SUN, reach(8), flags=7)):
            with pytest.raises(ort.OchError) as e:                   # a bad light
                fn(cams, bad, buf)
            assert e.value.status == -1 and untouched()
    with pytest.raises(ort.OchError) as e:                           # the host form checks the same
        pool.render_lit(cams[0], ort.Light(SUN, reach(8), 96, 41))
    assert e.value.status == -1
    # the same buffer at its true capacity is accepted
    pool.render_lit_views_dev(cams, light, out.data_ptr(), capacity_pixels=2 * H * W)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().view(np.uint32).reshape(2, H, W), dev_f, "raw pointer")


def test_example_lit_argument(ort, O, gpu_device, d8_ref, pal, tmp_path):
    """examples/render_frame --lit: the PPM is the oracle's lit frame of that camera."""
    import re
    import subprocess
    from conftest import ROOT
    exe = ROOT / "examples" / "render_frame"
    if not exe.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "examples")], check=True)
    w, h = 41, 25
    out = tmp_path / "lit.ppm"
    r = subprocess.run([str(exe), "8", str(out), str(w), str(h), str(YAW), "-0.6", "--lit"],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    assert (int(m.group(1)), int(m.group(2))) == (w, h)
    got = np.frombuffer(data[m.end():], np.uint8).reshape(h, w, 3)
    e = Expected(O, d8_ref, pal, 8, ORIGIN, YAW, -0.6, w, h, check_origins=False)
    want = e.frame(e.masks())
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(h, w, 4)[..., :3])
