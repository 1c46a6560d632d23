"""The supersampled lit launch against what a caller had before it: the lit
frame of the sample cameras into a device buffer and a torch box mean.

Depth-12 terrain, the bench's two views, 1920x1080 output at s = 2 (a 3840x2160
sample grid); sun (0.8, 0.35, 0.25), AO reach eight voxels, shades 96 / 24.  In
one process, alternating, after a warm-up of every arm:
  (a0) och_gpu_render_lit_ssaa_views_dev, OCH_OPT_BOUNCE_COMPACT 0 (in place);
  (a1) the same launch with the block's hit samples queued (1);
  (b)  och_gpu_render_lit_views_dev of the sample cameras (queued) into a
       device buffer of s * s times the output, then a torch box mean;
  (c0) och_gpu_render_lit_views_dev of the sample cameras alone, in place;
  (c1) the same, queued: the yardstick -- existing code that traces the same
       rays and stores s * s times the words.
Before timing the arms' frames are checked against each other word for word:
(a1) against (a0), (b) against (a0), and the host box mean of (c0)'s and
(c1)'s frames against (a0).  Kernel times are the library's own
(och_gpu_last_kernel_ms: the dispatch's events); stream times are HIP events
around the whole of each arm.  Median, quartiles and extremes over the repeats.

One process; set-up and measurement each run under a time limit (a watchdog
ends the process, without starting anything more, when one overruns it).

python tools/lit_ssaa_probe.py [--out profiles/lit_ssaa/probe.json] [--reps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

PITCHES = (0.0, -0.6)
ORIGIN = (1.5, 1.5, 1.5)
SUN = (0.8, 0.35, 0.25)


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
            "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--width", type=int, default=1920, help="of the output frame")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s", type=int, default=2, choices=(2, 4, 8))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for the set-up, and for the measurement")
    ap.add_argument("--out", default="profiles/lit_ssaa/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("lit_ssaa_probe: no GPU visible (there is nothing to measure without one)")
    faulthandler.dump_traceback_later(a.limit, exit=True)
    torch.cuda.set_device(0)
    tree = ort.build_terrain(a.depth, use_gpu=True)
    pool = ort.HOctree(tree.nodes, tree.root, a.depth, device=0)
    pool.set_palette(ort.VoxelData().get_colours())
    stream = torch.cuda.current_stream()
    pool.set_stream(stream)
    s, W, H, nv = a.s, a.width, a.height, len(PITCHES)
    Ws, Hs, log2_s = W * s, H * s, a.s.bit_length() - 1
    light = ort.Light(SUN, 8 * 2.0 ** -a.depth, 96, 24)
    ort.light_check(light)
    cams = [ort.camera(ORIGIN, 0.3, p, 1.25, Ws, Hs) for p in PITCHES]        # the sample grid's cameras
    dev = torch.device("cuda", 0)
    out_a0 = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
    out_a1 = torch.empty_like(out_a0)
    full = torch.empty((nv, Hs, Ws), dtype=torch.int32, device=dev)            # arm (b)'s and (c)'s sample frame

    def run_a0():
        pool.set_option("bounce_compact", 0)
        pool.render_lit_ssaa_views_dev(cams, light, s, out_a0)

    def run_a1():
        pool.set_option("bounce_compact", 1)
        pool.render_lit_ssaa_views_dev(cams, light, s, out_a1)

    def run_c0():
        pool.set_option("bounce_compact", 0)
        pool.render_lit_views_dev(cams, light, full)

    def run_c1():
        pool.set_option("bounce_compact", 1)
        pool.render_lit_views_dev(cams, light, full)

    def box_mean(x):
        out = torch.zeros((nv, H, W), dtype=torch.int32, device=dev)
        for sh in (0, 8, 16, 24):
            total = ((x >> sh) & 0xFF).view(nv, H, s, W, s).sum(dim=(2, 4), dtype=torch.int32)
            out |= ((total + s * s // 2) >> (2 * log2_s)) << sh
        return out

    composed = []

    def run_b():
        run_c1()
        composed[:] = [box_mean(full)]

    def timed(fn):
        """(stream ms by events around fn, the library's kernel ms of fn's render launch)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), pool.last_kernel_ms()

    arms = (("a0", run_a0), ("a1", run_a1), ("b", run_b), ("c0", run_c0), ("c1", run_c1))
    for _ in range(a.warmup):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    # the arms' frames against each other, word for word
    want = out_a0.cpu().numpy().view(np.uint32)
    equal = {"queued_equals_in_place": bool(torch.equal(out_a0, out_a1)),
             "composition_equals_fused": bool(torch.equal(composed[0], out_a0))}
    for key, fn in (("lit_in_place_downsampled_equals_fused", run_c0), ("lit_queued_downsampled_equals_fused", run_c1)):
        fn()
        torch.cuda.synchronize()
        equal[key] = bool(np.array_equal(ort.box_downsample(full.cpu().numpy().view(np.uint32), s), want))
    pool.set_option("bounce_compact", 1)
    plain = torch.empty_like(out_a0)
    pool.render_ssaa_views_dev(cams, s, plain)
    torch.cuda.synchronize()
    changed = int((plain != out_a0).sum().item())
    faulthandler.cancel_dump_traceback_later()
    faulthandler.dump_traceback_later(a.limit, exit=True)
    t = {f"{k}_{what}": [] for k, _ in arms for what in ("stream", "kernel")}
    for _ in range(a.reps):                             # alternating, so drift hits all alike
        for key, fn in arms:
            s_ms, k_ms = timed(fn)
            t[key + "_stream"].append(s_ms)
            t[key + "_kernel"].append(k_ms)
    faulthandler.cancel_dump_traceback_later()
    res = {"depth": a.depth, "views": nv, "s": s, "output_size": [W, H], "sample_grid": [Ws, Hs],
           "device": torch.cuda.get_device_name(0),
           "light": {"sun_dir": list(SUN), "ao_reach": light.ao_reach, "sun_shade": 96, "ao_shade": 24},
           **equal, "output_pixels_changed_by_light": changed}
    res.update({k: spread(v) for k, v in t.items()})
    print(json.dumps(res), flush=True)
    pool.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
