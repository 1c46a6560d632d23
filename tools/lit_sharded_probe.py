"""Lit frames through the sharded paths, measured on one GPU.

Depth-12 terrain, the bench's two views, sun (0.8, 0.35, 0.25), AO reach eight
voxels, shades 96 / 24.  Three measurements, each with its arms alternating in
one process after a warm-up of every arm; medians, quartiles and extremes:

  render   the lit launch at 1920x1080, one shard, and again as rank 0 of 8
           (row_chunk 8): k_trace_lit<LitCodeSink> (2-byte lit codes) against
           k_trace_lit<LitFrameSink> (RGBA8 words) -- the same walk, a half of
           the bytes stored.  Kernel times from och_gpu_last_kernel_ms.
  window   world size 1 on the library's communicator, 20 steps, three frames
           in flight, at 3840x2160 and 1920x1080: the native lit window
           (och_gpu_render_lit_sharded_steps_dev, lit codes) against what a
           caller had before it, issued per frame from Python:
           render_lit_views_dev (RGBA8 slices), comm.all_gather, unshard_dev.
           Per step: GPU time (an event before the first frame on idle streams,
           one behind the last frame of every stream, the longest span) and the
           host's issue time.  The frames of both arms are compared first.
           One GPU cannot price the exchange over xGMI: at world size 1 the
           collective is a copy on the device, 2 against 4 bytes per pixel.
  shade    k_shade_lit_unshard4 alone at 3840x2160 x 2 views against
           k_shade_unshard4 on the same geometry (6 against 5 bytes per pixel),
           each timed over a batch of launches; achieved bytes per second.

One process; set-up and every measurement run under a time limit (a watchdog
ends the process, without starting anything more, when one overruns it).

python tools/lit_sharded_probe.py [--out profiles/lit_sharded/probe.json] [--reps 30] [--window-reps 10]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

PITCHES = (0.0, -0.6)
ORIGIN = (1.5, 1.5, 1.5)
SUN = (0.8, 0.35, 0.25)
CHUNK = 8


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
            "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--shade-batch", type=int, default=20)
    ap.add_argument("--window-sizes", default="3840x2160,1920x1080")
    ap.add_argument("--limit", type=int, default=240, help="seconds for the set-up and for each measurement")
    ap.add_argument("--out", default="profiles/lit_sharded/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("lit_sharded_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    tree = ort.build_terrain(a.depth, use_gpu=True)
    pool = ort.HOctree(tree.nodes, tree.root, a.depth, device=0)
    pal = ort.VoxelData().get_colours()
    pool.set_palette(pal)
    main_stream = torch.cuda.current_stream()
    pool.set_stream(main_stream)
    light = ort.Light(SUN, 8 * 2.0 ** -a.depth, 96, 24)
    ort.light_check(light)
    nv = len(PITCHES)
    res = {"depth": a.depth, "views": nv, "device": torch.cuda.get_device_name(0), "row_chunk": CHUNK,
           "light": {"sun_dir": list(SUN), "ao_reach": light.ao_reach, "sun_shade": 96, "ao_shade": 24},
           "reps": a.reps, "window_reps": a.window_reps, "warmup": a.warmup}
    ok = True

    # ---- the render launch
    W, H = 1920, 1080
    cams = [ort.camera(ORIGIN, 0.3, p, 1.25, W, H) for p in PITCHES]
    res["render"] = {}
    for name, rc, shard, n_shards in (("one_shard", H, 0, 1), ("rank0_of_8", CHUNK, 0, 8)):
        watchdog()
        rows = pool.slice_rows(H, rc, n_shards)
        codes = torch.empty((nv, rows, W), dtype=torch.int16, device=dev)
        rgba = torch.empty((nv, rows, W), dtype=torch.int32, device=dev)
        masks = torch.empty((nv, rows, W), dtype=torch.uint8, device=dev)
        plain = torch.empty((nv, rows, W), dtype=torch.uint8, device=dev)
        arms = (("lit_codes", lambda: pool.render_lit_codes_views_dev(cams, light, codes, None, rc, shard, n_shards)),
                ("lit_rgba8", lambda: pool.render_lit_views_dev(cams, light, rgba, None, rc, shard, n_shards)))
        for _ in range(a.warmup):
            for _, fn in arms:
                fn()
        pool.render_lit_masks_views_dev(cams, light, masks, None, rc, shard, n_shards)
        pool.render_codes_views_dev(cams, plain, rc, shard, n_shards, False)
        torch.cuda.synchronize()
        got = codes.cpu().numpy().view(np.uint16)
        same = bool(np.array_equal(got >> 8, masks.cpu().numpy()) and np.array_equal(got & 0xFF, plain.cpu().numpy()))
        lit_words = ort.shade_lit_codes(got, pal, light)
        same_words = bool(np.array_equal(lit_words, rgba.cpu().numpy().view(np.uint32)))
        ok = ok and same and same_words
        t = {k: [] for k, _ in arms}
        for _ in range(a.reps):                           # alternating, so drift hits both alike
            for key, fn in arms:
                fn()
                torch.cuda.synchronize()
                t[key].append(pool.last_kernel_ms())
        pixels = nv * rows * W
        res["render"][name] = {"size": [W, H], "slice_rows": rows, "pixels": pixels,
                               "bytes_stored": {"lit_codes": 2 * pixels, "lit_rgba8": 4 * pixels},
                               "codes_equal_code_and_mask_outputs": same, "shaded_codes_equal_rgba8": same_words,
                               **{k + "_kernel": spread(v) for k, v in t.items()}}
        print(json.dumps({name: res["render"][name]}), flush=True)

    # ---- the window
    comm = ort.RcclComm.local(0)
    B = a.inflight
    streams = [main_stream] + [torch.cuda.Stream(device=dev) for _ in range(B - 1)]
    res["window"] = {}
    for size in a.window_sizes.split(","):
        watchdog()
        W, H = (int(x) for x in size.split("x"))
        cams = [ort.camera(ORIGIN, 0.3, p, 1.25, W, H) for p in PITCHES]
        rows = pool.slice_rows(H, CHUNK, 1)
        sfs = []
        for s in streams:
            with torch.cuda.stream(s):
                sfs.append(ort.ShardedFrame(pool, W, H, CHUNK, n_views=nv, indexed=True, shade="all", comm=comm,
                                            sharded=True, light=light))
        steps = ort.ShardedSteps(sfs, streams, comm, cams)
        issue_native = steps.prepare(a.steps)
        # the composition a caller had before the lit window: per frame, from the interpreter
        sl = [torch.empty((nv, rows, W), dtype=torch.int32, device=dev) for _ in streams]
        ga = [torch.empty((1, nv, rows, W), dtype=torch.int32, device=dev) for _ in streams]
        fr = [torch.empty((nv, H, W), dtype=torch.int32, device=dev) for _ in streams]

        def issue_composed():
            for k in range(a.steps):
                b = k % B
                pool.set_stream(streams[b])
                pool.render_lit_views_dev(cams, light, sl[b], None, CHUNK, 0, 1)
                comm.all_gather(sl[b], ga[b], streams[b])
                pool.unshard_dev(ga[b], fr[b], W, H, CHUNK, 1, nv)
            pool.set_stream(main_stream)

        def window(issue):
            """(GPU ms per step, host issue ms per step) of one window on idle streams."""
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True)
            ends = [torch.cuda.Event(enable_timing=True) for _ in streams]
            e0.record(streams[0])
            for s in streams[1:]:
                s.wait_event(e0)
            t0 = time.perf_counter()
            issue()
            t1 = time.perf_counter()
            for s, e in zip(streams, ends):
                e.record(s)
            torch.cuda.synchronize()
            return max(e0.elapsed_time(e) for e in ends) / a.steps, (t1 - t0) * 1e3 / a.steps

        arms = (("native_lit_codes", issue_native), ("composed_rgba8", issue_composed))
        for _ in range(2):
            for _, fn in arms:
                window(fn)
        same = all(bool(torch.equal(f.frames, g)) for f, g in zip(sfs, fr))
        ok = ok and same
        t = {f"{k}_{what}": [] for k, _ in arms for what in ("gpu", "issue")}
        for _ in range(a.window_reps):
            for key, fn in arms:
                g_ms, i_ms = window(fn)
                t[key + "_gpu"].append(g_ms)
                t[key + "_issue"].append(i_ms)
        pixels = nv * rows * W
        res["window"][size] = {"steps": a.steps, "inflight": B, "world_size": 1, "frames_equal": same,
                               "exchange_bytes_per_step": {"native_lit_codes": 2 * pixels, "composed_rgba8": 4 * pixels},
                               **{k + "_ms_per_step": spread(v) for k, v in t.items()}}
        print(json.dumps({size: res["window"][size]}), flush=True)
        del sfs, steps, sl, ga, fr
    comm.close()

    # ---- the shade kernel
    watchdog()
    W, H = 3840, 2160
    rng = np.random.default_rng(5)
    n_codes = np.asarray(pal).size
    valid_codes = np.concatenate([np.arange(n_codes), [125, 126, 127]]).astype(np.uint16)
    valid_masks = np.array([0x80] + [m | s for m in range(16) for s in (0, 0x10, 0x30)], np.uint16)
    c = rng.choice(valid_codes, (1, nv, H, W))
    lit_src = torch.from_numpy((c | (rng.choice(valid_masks, c.shape) << 8)).astype(np.uint16).view(np.int16)).to(dev)
    plain_src = torch.from_numpy(c.astype(np.uint8)).to(dev)
    out = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
    pool.set_stream(main_stream)
    arms = (("shade_lit_unshard4", lambda: pool.shade_lit_unshard_dev(lit_src, out, W, H, CHUNK, 1, light, nv), 6),
            ("shade_unshard4", lambda: pool.shade_unshard_dev(plain_src, out, W, H, CHUNK, 1, nv), 5))
    for _ in range(a.warmup):
        for _, fn, _ in arms:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in arms}
    for _ in range(a.reps):
        for key, fn, _ in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main_stream)
            for _ in range(a.shade_batch):
                fn()
            e1.record(main_stream)
            torch.cuda.synchronize()
            t[key].append(e0.elapsed_time(e1) / a.shade_batch)
    res["shade"] = {"size": [W, H], "views": nv, "launches_per_sample": a.shade_batch}
    for key, _, bpp in arms:
        sp = spread(t[key])
        sp["bytes_per_pixel"] = bpp
        sp["achieved_tb_per_s"] = round(bpp * nv * W * H / (sp["median_ms"] * 1e-3) / 1e12, 3)
        res["shade"][key] = sp
    res["shade"]["ratio_of_medians"] = round(res["shade"]["shade_lit_unshard4"]["median_ms"] /
                                             res["shade"]["shade_unshard4"]["median_ms"], 3)
    print(json.dumps({"shade": res["shade"]}), flush=True)
    faulthandler.cancel_dump_traceback_later()
    res["all_outputs_equal"] = ok
    pool.close()
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
