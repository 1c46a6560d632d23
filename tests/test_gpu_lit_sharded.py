"""Lit frames through the sharded paths: 2-byte lit codes (code | mask << 8),
their shade + unshard kernel, the native lit windows, the frame group and the
two multi-GPU examples, all against tests/test_gpu_lit.py's oracle records
(its `Expected`: cameras, light and the 82 x 50 size are that file's).  Every
comparison is bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_lit as L
from test_gpu_lit import d8, d8_ref, pal, pool, views  # noqa: F401  (that file's fixtures, one copy per module)

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
CHUNK = 8
SENTINEL16 = 0x5A5A
MAGENTA, INSIDE, SKY = 125, 126, 127


def lit_codes(pool, cams, light, **kw):
    """Lit codes into a sentinel-filled int16 tensor: numpy uint16, one slice per view."""
    import torch
    rows = pool.slice_rows(cams[0].height, kw.get("row_chunk") or cams[0].height, kw.get("n_shards", 1))
    out = torch.full((len(cams), rows, cams[0].width), SENTINEL16, dtype=torch.int16, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_lit_codes_views_dev(cams, light, out, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


def plain_codes(pool, cams, **kw):
    import torch
    rows = pool.slice_rows(cams[0].height, kw.get("row_chunk") or cams[0].height, kw.get("n_shards", 1))
    out = torch.full((len(cams), rows, cams[0].width), L.SENTINEL8, dtype=torch.uint8, device="cuda")
    pool.set_stream(torch.cuda.current_stream())
    pool.render_codes_views_dev(cams, out, kw.get("row_chunk"), kw.get("shard", 0), kw.get("n_shards", 1), False)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def want_frames(views, flags=3):
    masks = [v.masks(flags) for v in views]
    return np.stack([v.frame(m) for v, m in zip(views, masks)])


def test_lit_codes_one_shard(ort, pool, views):
    """1. Two views: the low byte is the plain code byte, the high byte the lit mask byte."""
    cams, light = L.cameras(ort), L.make_light(ort)
    want_m = np.stack([v.masks() for v in views])

    def check(what):
        got = lit_codes(pool, cams, light)
        assert got.shape == (2, H, W)
        L.assert_same(got & 0xFF, plain_codes(pool, cams).astype(np.uint16), f"code byte, {what}")
        _, dev_m = L.render(pool, cams, light)
        L.assert_same(got >> 8, dev_m.astype(np.uint16), f"mask byte vs the mask output, {what}")
        L.assert_same(got >> 8, want_m.astype(np.uint16), f"mask byte vs the oracle, {what}")
        return got

    got = check("defaults")
    low = got & 0xFF
    assert (low == SKY).any() and (low < 120).any() and not (low >= 128).any()
    assert ((got >> 8)[low == SKY] == 0x80).all()
    for layout in (0, 1):                              # raw and packed
        pool.set_option("layout", layout)
        for compact in (0, 1):
            pool.set_option("bounce_compact", compact)
            for block in (64, 256):
                pool.set_option("block", block)
                check(f"layout {layout}, bounce_compact {compact}, block {block}")
    pool.set_option("block", 64)
    pool.plan_views(cams)
    pool.set_option("tile_order", 2)
    check("tile_order 2, planned")
    assert pool.last_kernel_ms() > 0.0


@pytest.mark.parametrize("dealt", [False, True])
def test_shards(ort, pool, views, dealt):
    """2. row_chunk 8 over 3 shards (7 chunks, the last partial), round-robin and under a weighted
    deal: all shards' lit codes, laid out as an all-gather lays them, shaded into the oracle's frame."""
    import torch
    cams, light = L.cameras(ort), L.make_light(ort)
    n = 3
    deal = None
    if dealt:
        deal = ort.deal_chunks(np.ones(-(-H // CHUNK), np.float32), n, [0.4, 1.0, 1.0])
        assert len(deal) == 7 and len(set(np.bincount(deal, minlength=n).tolist())) > 1, deal
        pool.set_row_deal(H, CHUNK, n, deal)
    rows = pool.slice_rows(H, CHUNK, n)
    assert rows * n > H and H % CHUNK
    parts = [lit_codes(pool, cams, light, row_chunk=CHUNK, shard=s, n_shards=n) for s in range(n)]
    padding = 0
    for s in range(n):                                   # padding rows keep their sentinel
        rmap = ort.frame.slice_row_map(H, CHUNK, n, s, deal)
        padding += int((rmap < 0).sum())
        assert (parts[s][:, rmap < 0] == SENTINEL16).all(), s
        assert (parts[s][:, rmap >= 0] != SENTINEL16).all(), s
    assert padding == rows * n - H                       # the short last chunk and the slices' unused chunks
    gathered = torch.from_numpy(np.stack(parts).view(np.int16)).cuda()             # [shard][view][rows][W]
    frames = torch.full((2, H, W), L.SENTINEL, dtype=torch.int32, device="cuda")
    pool.shade_lit_unshard_dev(gathered, frames, W, H, CHUNK, n, light, n_views=2)
    torch.cuda.synchronize()
    L.assert_same(frames.cpu().numpy().view(np.uint32), want_frames(views), f"dealt {dealt}")


def random_lit_codes(rng, shape, n_face_codes):
    codes = np.concatenate([np.arange(n_face_codes), [MAGENTA, INSIDE, SKY]]).astype(np.uint16)
    masks = np.array([0x80] + [m | s for m in range(16) for s in (0, 0x10, 0x30)], np.uint16)
    return (rng.choice(codes, shape) | (rng.choice(masks, shape) << 8)).astype(np.uint16)


@pytest.mark.parametrize("shards,n_views", [(1, 1), (3, 2)])
@pytest.mark.parametrize("height", [50, 1])
@pytest.mark.parametrize("width,offset", [(82, 0), (84, 0), (1028, 0), (84, 1)])
def test_shade_kernel_on_data(ort, pool, pal, width, offset, height, shards, n_views):
    """3. k_shade_lit_unshard / k_shade_lit_unshard4 on random valid (code, mask) pairs: width 82 takes
    the scalar form, 84 and 1028 the vector form (1028: a last, partial block of 256 threads),
    offset 1: the source starts 2 bytes off, so the scalar form serves a width that is a multiple of 4."""
    import torch
    rng = np.random.default_rng(width * 1000 + height * 10 + shards + offset)
    rows = pool.slice_rows(height, CHUNK, shards)
    codes = random_lit_codes(rng, (shards, n_views, rows, width), np.asarray(pal).size)
    buf = torch.zeros(codes.size + offset, dtype=torch.int16, device="cuda")
    src = buf[offset:]
    assert src.data_ptr() % 8 == 2 * offset
    src.copy_(torch.from_numpy(codes.reshape(-1).view(np.int16)))
    pool.set_stream(torch.cuda.current_stream())
    lights = (L.make_light(ort), ort.Light(L.SUN, L.reach(8), 256, 0))     # the default; weight 0 in shadow
    for light in lights:
        frames = torch.full((n_views, height, width), L.SENTINEL, dtype=torch.int32, device="cuda")
        pool.shade_lit_unshard_dev(src, frames, width, height, CHUNK, shards, light, n_views=n_views)
        torch.cuda.synchronize()
        want = np.stack([ort.shade_lit_codes(ort.frame.unshard_host(codes[:, v], height, CHUNK), pal, light)
                         for v in range(n_views)])
        L.assert_same(frames.cpu().numpy().view(np.uint32), want, f"sun_shade {light.sun_shade}")
    # the last light has weight 0 in shadow: those pixels are black, alpha kept
    whole = np.stack([ort.frame.unshard_host(codes[:, v], height, CHUNK) for v in range(n_views)])
    black = want[((whole >> 8) & 0x10) != 0]
    assert black.size and ((black & 0x00FFFFFF) == 0).all()


def make_window(ort, pool, comm, exchange, light, n_streams=3):
    import torch
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]
    shade = "all" if exchange == "all_gather" else "display"
    mode = "gather" if exchange == "gather" else "all_gather"
    sfs = []
    for s in streams:
        with torch.cuda.stream(s):
            sfs.append(ort.ShardedFrame(pool, W, H, CHUNK, n_views=2, indexed=True, shade=shade, comm=comm,
                                        sharded=True, exchange=mode, light=light))
    return streams, sfs


@pytest.mark.parametrize("exchange", ["all_gather", "display", "gather"])
def test_lit_window_world1(ort, pool, views, exchange):
    """4. och_gpu_render_lit_sharded_steps_dev at world size 1: 7 frames over 3 streams and buffer sets."""
    import torch
    cams, light = L.cameras(ort), L.make_light(ort)
    want = want_frames(views)
    comm = ort.RcclComm.local(0)
    streams, sfs = make_window(ort, pool, comm, exchange, light)
    assert all(f.slice.dtype == torch.int16 and f.gathered.dtype == torch.int16 for f in sfs)
    steps = ort.ShardedSteps(sfs, streams, comm, cams)
    assert steps.light is light and steps.exchange == ort._lib.EXCHANGE[exchange]
    for f in sfs:
        f.frames.fill_(L.SENTINEL)
    steps.run(7)
    torch.cuda.synchronize()
    for b, f in enumerate(sfs):
        L.assert_same(f.frames.cpu().numpy().view(np.uint32), want, f"{exchange}, buffer set {b}")
    # the same frame issued from Python through ShardedFrame.render on this communicator
    for f in sfs:
        f.frames.fill_(L.SENTINEL)
    with torch.cuda.stream(streams[1]):
        pool.set_stream(streams[1])
        sfs[1].render(cams)
    torch.cuda.synchronize()
    L.assert_same(sfs[1].frames.cpu().numpy().view(np.uint32), want, f"{exchange}, ShardedFrame.render")
    # flags = 0: the plain window's frames, word for word
    dark = L.make_light(ort, 0)
    streams0, lit0 = make_window(ort, pool, comm, exchange, dark)
    _, plain = make_window(ort, pool, comm, exchange, None)
    ort.ShardedSteps(lit0, streams0, comm, cams).run(3)
    ort.ShardedSteps(plain, streams0, comm, cams).run(3)
    torch.cuda.synchronize()
    for a, b in zip(lit0, plain):
        L.assert_same(a.frames.cpu().numpy().view(np.uint32), b.frames.cpu().numpy().view(np.uint32), "flags 0")
    L.assert_same(plain[0].frames.cpu().numpy().view(np.uint32), np.stack([v.plain.reshape(H, W) for v in views]),
                  "the plain window")
    pool.set_stream(torch.cuda.current_stream())
    comm.close()


def test_render_lit_steps(ort, pool, views):
    """5. och_gpu_render_lit_steps_dev: 5 frames over 2 buffers equal render_lit_views_dev's."""
    import torch
    cams, light = L.cameras(ort), L.make_light(ort)
    one, _ = L.render(pool, cams, light)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    frames = [torch.full((2, H, W), L.SENTINEL, dtype=torch.int32, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    pool.render_lit_steps_dev(cams, light, frames, streams, 5)
    torch.cuda.synchronize()
    for b, f in enumerate(frames):
        L.assert_same(f.cpu().numpy().view(np.uint32), one, f"buffer {b}")
    L.assert_same(one, want_frames(views), "render_lit_views_dev")
    with pytest.raises(ort.OchError) as e:                           # refused before the first frame
        pool.render_lit_steps_dev(cams, ort.Light(L.SUN, L.reach(8), 96, 41), frames, streams, 5)
    assert e.value.status == -1


def test_frame_group_one_device(ort, gpu_device, d8, pal, views):
    """6. FrameGroup.render(light=) and render_steps(light=); a palette of 21 ids takes the RGBA8 fallback."""
    import torch
    cams, light = L.cameras(ort), L.make_light(ort)
    want = want_frames(views)
    g = ort.FrameGroup(d8.nodes, d8.root, 8, devices=[0])
    g.set_palette(pal)
    g.render(cams, row_chunk=CHUNK, light=light)
    L.assert_same(g.download(0), want, "render(light=)")
    g.render_steps(cams, 5, n_buffers=3, row_chunk=CHUNK, light=light)
    L.assert_same(g.download(0), want, "render_steps(light=)")
    g.render(cams, row_chunk=CHUNK)                                   # and back: the plain frame, 1-byte codes
    L.assert_same(g.download(0), np.stack([v.plain.reshape(H, W) for v in views]), "plain after lit")
    flat = np.ascontiguousarray(pal, np.uint32).reshape(-1)
    pal21 = np.tile(flat, -(-21 * 6 // flat.size))[:21 * 6]           # the same first entries, 21 ids
    assert pal21.size // 6 > ort.GpuPool.CODE_MAX_VOXELS and np.array_equal(pal21[:flat.size], flat)
    g.set_palette(pal21)
    g.render_steps(cams, 4, n_buffers=2, row_chunk=CHUNK, light=light)
    got = g.download(0)
    g.close()
    pool = ort.HOctree(d8.nodes, d8.root, 8, device=0)
    pool.set_palette(pal21)
    sl, _ = L.render(pool, cams, light, row_chunk=CHUNK, shard=0, n_shards=1)
    whole = torch.full((2, H, W), L.SENTINEL, dtype=torch.int32, device="cuda")
    pool.unshard_dev(torch.from_numpy(sl.view(np.int32)).cuda(), whole, W, H, CHUNK, 1, n_views=2)
    torch.cuda.synchronize()
    L.assert_same(got, whole.cpu().numpy().view(np.uint32), "21 ids: render_lit_views_dev + unshard")
    L.assert_same(got, want, "21 ids vs the oracle")                  # the tree's ids name the same colours
    pool.close()


def test_guards(ort, pool, pal):
    """7. Every refusal is OCH_E_INVALID and comes before anything is written."""
    import torch
    lib = ort.load()
    cams, light = L.cameras(ort), L.make_light(ort)
    arr = (ort._lib.Camera * 2)(*cams)
    codes = torch.full((2 * H * W,), SENTINEL16, dtype=torch.int16, device="cuda")
    frames = torch.full((2 * H * W,), L.SENTINEL, dtype=torch.int32, device="cuda")
    pool.set_stream(torch.cuda.current_stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((codes.cpu().numpy().view(np.uint16) == SENTINEL16).all() and
                    (frames.cpu().numpy().view(np.uint32) == L.SENTINEL).all())

    def render(light_ref, capacity=2 * H * W):
        return lib.och_gpu_render_lit_codes_views_dev(pool._h, C.cast(arr, C.c_void_p), 2, light_ref,
                                                      codes.data_ptr(), capacity, H, 0, 1)

    assert render(None) == -1 and untouched()                                    # a NULL light
    for bad in (ort.Light(L.SUN, L.reach(8), 96, 41), ort.Light((0, 0, 0), L.reach(8)), ort.Light(L.SUN, 0.0),
                ort.Light(L.SUN, L.reach(8), flags=7)):
        assert render(C.byref(bad)) == -1 and untouched()                        # a light och_light_check refuses
        assert lib.och_gpu_shade_lit_unshard_views_dev(pool._h, codes.data_ptr(), frames.data_ptr(), W, H, H, 1, 2,
                                                       C.byref(bad)) == -1 and untouched()
    assert lib.och_gpu_shade_lit_unshard_views_dev(pool._h, codes.data_ptr(), frames.data_ptr(), W, H, H, 1, 2,
                                                   None) == -1 and untouched()
    assert render(C.byref(light), 2 * H * W - W) == -1 and untouched()           # too small by one row
    assert b"pixels" in lib.och_last_error()
    with pytest.raises(ValueError):                                              # the wrapper's own size check
        pool.render_lit_codes_views_dev(cams, light, codes[:-W])
    with pytest.raises(ValueError):                                              # 1-byte elements for lit codes
        pool.render_lit_codes_views_dev(cams, light, torch.empty(4 * H * W, dtype=torch.int8, device="cuda"))
    assert untouched()
    # the window: a missing frames entry on the shading rank, a NULL light, a bad light
    comm = ort.RcclComm.local(0)
    st = (C.c_void_p * 1)(torch.cuda.current_stream().cuda_stream)
    sp = (C.c_void_p * 1)(codes.data_ptr())
    fp = (C.c_void_p * 1)(frames.data_ptr())
    none = (C.c_void_p * 1)(None)

    def window(frames_p, light_ref):
        return lib.och_gpu_render_lit_sharded_steps_dev(pool._h, comm.handle, C.cast(arr, C.c_void_p), 2, 3, st, sp, sp,
                                                        frames_p, 1, None, None, CHUNK, light_ref, 0)

    assert window(none, C.byref(light)) == -1 and b"frames" in lib.och_last_error() and untouched()
    assert window(None, C.byref(light)) == -1 and untouched()
    assert window(fp, None) == -1 and untouched()
    assert window(fp, C.byref(ort.Light(L.SUN, L.reach(8), 96, 41))) == -1 and untouched()
    # a light together with bounce: refused by the wrappers, nothing issued
    streams, sfs = make_window(ort, pool, comm, "all_gather", light, n_streams=1)
    sfs[0].slice.fill_(SENTINEL16)
    with pytest.raises(ValueError):
        ort.ShardedSteps(sfs, streams, comm, cams, bounce=True)
    with pytest.raises(ValueError):
        sfs[0].render(cams, bounce=True)
    torch.cuda.synchronize()
    assert (sfs[0].slice.cpu().numpy().view(np.uint16) == SENTINEL16).all()
    # a palette of 21 ids: no lit codes, no lit window (refused before the first frame)
    flat = np.ascontiguousarray(pal, np.uint32).reshape(-1)
    pool.set_palette(np.tile(flat, -(-21 * 6 // flat.size))[:21 * 6])
    assert render(C.byref(light)) == -1 and b"palette" in lib.och_last_error() and untouched()
    assert window(fp, C.byref(light)) == -1 and untouched()
    assert lib.och_gpu_shade_lit_unshard_views_dev(pool._h, codes.data_ptr(), frames.data_ptr(), W, H, H, 1, 2,
                                                   C.byref(light)) == -1 and untouched()
    pool.set_palette(pal)
    assert render(C.byref(light)) == 0                                           # and accepted again
    torch.cuda.synchronize()
    assert not (codes.cpu().numpy().view(np.uint16) == SENTINEL16).any()
    comm.close()


def read_ppm(path):
    data = path.read_bytes()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    return np.frombuffer(data[m.end():], np.uint8).reshape(int(m.group(2)), int(m.group(1)), 3)


@pytest.mark.parametrize("example", ["multi_gpu_frame", "sharded_frame"])
def test_examples_lit(ort, O, gpu_device, d8_ref, pal, tmp_path, example):
    """8. The two multi-GPU examples with --lit on one device: view 1 is the oracle's lit frame."""
    from conftest import ROOT
    exe = ROOT / "examples" / example
    if not exe.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "examples")], check=True)
    w, h = 82, 50
    out = tmp_path / "lit.ppm"
    if example == "multi_gpu_frame":
        cmd = [str(exe), "8", str(w), str(h), str(out), "1", "2", "1", "--lit"]
    else:
        cmd = [str(exe), "8", str(w), str(h), str(out), "0", "1", str(tmp_path / "id"), "4", "1", "--lit"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr
    e = L.Expected(O, d8_ref, pal, 8, L.ORIGIN, L.YAW, -0.6, w, h, check_origins=False)
    want = e.frame(e.masks())
    assert np.array_equal(read_ppm(out), np.ascontiguousarray(want).view(np.uint8).reshape(h, w, 4)[..., :3])


def _rank(rank, world, port, root_dir, q):
    """One of two ranks on device 0, gloo collectives through the host (tests/test_gpu_multirank.py's
    arrangement): lit codes through ShardedFrame, round-robin and dealt."""
    import sys
    sys.path.insert(0, root_dir)
    sys.path.insert(0, os.path.join(root_dir, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import octree_ray_tracing_amd as ort
    import test_gpu_lit as L
    tree = ort.build_terrain(8)
    pool = ort.HOctree(tree.nodes, tree.root, 8, device=0)
    pool.set_palette(ort.VoxelData().get_colours())
    cams, light = L.cameras(ort), L.make_light(ort)
    out = {}
    for name, deal, shade in (("rr", None, "all"),
                              ("deal", ort.deal_chunks(np.ones(-(-L.H // CHUNK), np.float32), world, [0.6, 1.0]), "display")):
        sf = ort.ShardedFrame(pool, L.W, L.H, CHUNK, n_views=2, indexed=True, deal=deal, shade=shade, light=light)
        frames = sf.render(cams)
        torch.cuda.synchronize()
        out[name] = (None if frames is None else frames.cpu().numpy().view(np.uint32).copy(), str(sf.slice.dtype))
    pool.close()
    dist.destroy_process_group()
    q.put((rank, out))


def test_lit_codes_two_ranks(ort, gpu_device, views):
    """Two ranks wide: each renders its rows as lit codes, the all-gather carries int16, both (or the
    display rank alone) shade the oracle's lit frames."""
    import torch.multiprocessing as mp
    from conftest import ROOT
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() + 7) % 1000
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(ROOT), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=110) for _ in range(2))
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    want = want_frames(views)
    for rank in (0, 1):
        for name in ("rr", "deal"):
            frames, dtype = got[rank][name]
            assert dtype == "torch.int16"
            if name == "deal" and rank != 0:
                assert frames is None
                continue
            L.assert_same(frames, want, f"rank {rank}, {name}")
