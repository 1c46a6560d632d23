"""Camera launches through their tile table (csrc/och_tiles.cpp, CameraSource in
csrc/och_kernels.hip): every kernel that renders a camera frame reads, per wave,
one descriptor of the tile it walks.  A wrong descriptor moves or drops pixels,
so every check here is bit for bit against the oracle's frames (raygen +
trace_batch + shade_fast, and the oracle's bounce, lit and box-mean forms) on
the depth-8 terrain, over frames smaller than a tile, ragged ones, heights that
are no multiple of the row chunk, every launch order and two block sizes.

The oracle's frames are computed once per module and never changed.
"""
import numpy as np
import pytest

from test_gpu_lit_ssaa import Expected, downsample, make_light

pytestmark = pytest.mark.gpu

ORIGIN = (1.5, 1.5, 1.5)
YAW, FOV = 0.3, 1.25
PITCHES = (-0.25, -0.6)                   # two views of different pitch
PAN = ((0.9, -0.4), (-1.1, -0.7))         # the panning camera's (yaw, pitch)
# 1x1 .. 72x40, and heights that are no multiple of the 8-row chunk (19, 43)
SHAPES = ((1, 1), (8, 8), (9, 9), (65, 3), (72, 40), (40, 19), (24, 43))
CHUNK = 8
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pal(ort):
    return ort.VoxelData().get_colours()


@pytest.fixture(scope="module")
def d8(ort):
    return ort.build_terrain(8)


@pytest.fixture(scope="module")
def d8_ref(O, d8):
    return O.OraclePool(d8.nodes, d8.root, 8, 1)


def oracle_views(O, ref, pal, W, H, views):
    """The oracle's plain and config-5 frames of the (yaw, pitch) views: (n, H, W) uint32 each."""
    plain, bounce = [], []
    for yaw, pitch in views:
        rays = O.raygen(yaw, pitch, FOV, W, H)
        r = O.trace_batch(ref, O.Rcp(None), np.array(ORIGIN, np.float32), rays, nthreads=16)
        plain.append(O.shade_fast(r["dir"], r["voxel"], pal).reshape(H, W))
        b = O.trace_bounce_batch(ref, O.Rcp(None), ORIGIN, rays, nthreads=16)
        bounce.append(O.shade_bounce(b["dir"], b["voxel"], b["dir2"], pal).reshape(H, W))
    return np.stack(plain), np.stack(bounce)


@pytest.fixture(scope="module")
def want(O, d8_ref, pal):
    """Per frame shape: the oracle's plain, bounce and lit frames of the two views and, where
    the shape allows 2x2 samples, the plain frames' box mean."""
    out = {}
    for W, H in SHAPES:
        plain, bounce = oracle_views(O, d8_ref, pal, W, H, [(YAW, p) for p in PITCHES])
        lit = []
        for v, p in enumerate(PITCHES):
            e = Expected(O, d8_ref, pal, 8, ORIGIN, YAW, p, W, H, check_origins=False)
            assert np.array_equal(e.plain_frame(), plain[v])
            lit.append(e.frame(e.masks()))
        out[(W, H)] = {"plain": plain, "bounce": bounce, "lit": np.stack(lit),
                       "ssaa": np.stack([downsample(f, 2) for f in plain]) if W % 2 == 0 and H % 2 == 0 else None}
    return out


@pytest.fixture
def pool(ort, gpu_device, d8, pal):
    import torch
    p = ort.HOctree(d8.nodes, d8.root, 8, device=0)
    p.set_palette(pal)
    p.set_stream(torch.cuda.current_stream())
    yield p
    p.close()


def cameras(ort, W, H, views=None):
    return [ort.camera(ORIGIN, y, p, FOV, W, H) for y, p in (views or [(YAW, p) for p in PITCHES])]


def words(t):
    return t.cpu().numpy().view(np.uint32)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, f"{what}: {len(bad)} pixels differ, first {bad[:4].tolist()}"


def render_all(ort, pool, cams, w, what):
    """Every camera kernel's frame of these views against the oracle's."""
    import torch
    W, H, n = cams[0].width, cams[0].height, len(cams)
    # RGBA8, one shard: slices of whole row chunks
    rows = pool.slice_rows(H, CHUNK, 1)
    out = torch.full((n, rows, W), GUARD, dtype=torch.int32, device="cuda")
    pool.render_views_dev(cams, out, CHUNK)
    same(words(out)[:, :H], w["plain"], f"{what} rgba")
    assert np.all(words(out)[:, H:] == GUARD), f"{what} rgba: rows past the frame written"
    # indexed colour as 3 shards, shaded and unsharded on the device
    rows3 = pool.slice_rows(H, CHUNK, 3)
    gathered = torch.zeros((3, n, rows3, W), dtype=torch.uint8, device="cuda")
    for shard in (0, 2, 1):
        pool.render_codes_views_dev(cams, gathered[shard], CHUNK, shard, 3)
    frames = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    pool.shade_unshard_dev(gathered, frames, W, H, CHUNK, 3, n)
    same(words(frames), w["plain"], f"{what} codes, 3 shards")
    # config 5
    out.fill_(GUARD)
    pool.render_bounce_views_dev(cams, out, CHUNK)
    same(words(out)[:, :H], w["bounce"], f"{what} bounce")
    # lit
    lit = torch.full((n, H, W), GUARD, dtype=torch.int32, device="cuda")
    pool.render_lit_views_dev(cams, make_light(ort), lit)
    same(words(lit), w["lit"], f"{what} lit")
    # 2x2 supersampled: these cameras as the sample grid
    if w["ssaa"] is not None:
        ss = torch.full((n, H // 2, W // 2), GUARD, dtype=torch.int32, device="cuda")
        pool.render_ssaa_views_dev(cams, 2, ss)
        same(words(ss), w["ssaa"], f"{what} ssaa 2x2")
    torch.cuda.synchronize()


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("order", ["natural", "planned", "xcd"])
def test_every_kernel_every_shape(ort, pool, want, order, block):
    pool.set_option("block", block)
    pool.set_option("tile_order", {"natural": 0, "planned": 2, "xcd": 3}[order])
    for W, H in SHAPES:
        cams = cameras(ort, W, H)
        if order != "natural":
            pool.plan_views(cams, CHUNK)                    # the one-shard frames' plan; the shards run unplanned
        render_all(ort, pool, cams, want[(W, H)], f"{W}x{H} {order} block {block}")


def test_supertile_order(ort, pool, want):
    """tile_order 1: tiles enumerated in supertiles, grouped per XCD."""
    pool.set_option("tile_order", 1)
    for W, H in ((72, 40), (65, 3), (24, 43)):
        render_all(ort, pool, cameras(ort, W, H), want[(W, H)], f"{W}x{H} tile_order 1")


def test_split_frame(ort, pool, want):
    """A split plan (threshold 1 %, 4 lanes a ray, level 3): the split waves find their tile
    through the table."""
    import torch
    W, H = 72, 40
    cams = cameras(ort, W, H)
    for k, v in (("split", 1), ("split_segs", 4), ("split_level", 3), ("tile_order", 2)):
        pool.set_option(k, v)
    pool.plan_views(cams, CHUNK)
    assert pool.get_option("split_tiles") > 0
    out = torch.full((2, H, W), GUARD, dtype=torch.int32, device="cuda")
    pool.render_views_dev(cams, out, CHUNK)
    same(words(out), want[(W, H)]["plain"], "split frame")
    # the planner is deterministic: the same plan twice (the counting render's buffer is cleared)
    tiles = pool.get_option("split_tiles")
    pool.plan_views(cams, CHUNK)
    assert pool.get_option("split_tiles") == tiles


def test_panning_camera_and_a_change_of_frame_size(ort, O, d8_ref, pal, pool, want):
    """The table depends on the geometry alone: frames of other cameras after plan_views on the
    first ones, then another frame size on the same pool and back (the table's key changes)."""
    import torch
    pool.set_option("tile_order", 2)
    pool.plan_views(cameras(ort, 72, 40), CHUNK)
    pan = cameras(ort, 72, 40, PAN)
    want_pan, _ = oracle_views(O, d8_ref, pal, 72, 40, PAN)
    out = torch.full((2, 40, 72), GUARD, dtype=torch.int32, device="cuda")
    pool.render_views_dev(pan, out, CHUNK)
    same(words(out), want_pan, "panned cameras")
    for W, H in ((40, 19), (72, 40), (9, 9), (72, 40)):
        rows = pool.slice_rows(H, CHUNK, 1)
        out = torch.full((2, rows, W), GUARD, dtype=torch.int32, device="cuda")
        pool.render_views_dev(cameras(ort, W, H), out, CHUNK)
        same(words(out)[:, :H], want[(W, H)]["plain"], f"{W}x{H} after another size")


@pytest.mark.parametrize("deal", [False, True])
def test_slices_of_exactly_shard_rows(ort, pool, want, deal):
    """Slices sized exactly to the shard's rows with guard words behind them: a wrong slice row
    is a failure here, not a silent write into the allocator's slack."""
    import torch
    W, H, n = 40, 19, 3                                     # 3 chunks, the last of 3 rows
    cams = cameras(ort, W, H)
    if deal:
        pool.set_row_deal(H, CHUNK, n, [1, 1, 0])           # shard 2 holds padding chunks only
    rows = pool.slice_rows(H, CHUNK, n)
    assert rows == (2 * CHUNK if deal else ort.shard_rows(H, CHUNK, n))
    size = 2 * rows * W
    gathered = torch.zeros((n, 2, rows, W), dtype=torch.int32, device="cuda")
    for shard in range(n):
        buf = torch.full((size + 64,), GUARD, dtype=torch.int32, device="cuda")
        pool.render_views_dev(cams, buf[:size], CHUNK, shard, n)
        assert np.all(words(buf)[size:] == GUARD), f"shard {shard}: words behind the slices written"
        gathered[shard] = buf[:size].view(2, rows, W)
        codes = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        pool.render_codes_views_dev(cams, codes[:size], CHUNK, shard, n)
        assert np.all(codes.cpu().numpy()[size:] == 0x5A), f"shard {shard}: bytes behind the code slices written"
    frames = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
    pool.unshard_dev(gathered, frames, W, H, CHUNK, n, 2)
    same(words(frames), want[(W, H)]["plain"], "unsharded slices")
