"""Fused supersampled render against the two-pass way to the same pixels.

Per case (depth-12 terrain, the bench's two views; sample grid and s):
  (a) och_gpu_render_ssaa_views_dev: one launch, the samples resolved in registers;
  (b) och_gpu_render_views_dev at the sample size into a full RGBA8 buffer, then
      a torch box-downsample of that buffer on the same stream.
Kernel times are the library's own (och_gpu_last_kernel_ms: the dispatch's
events) for (a) and for (b)'s render; stream times are HIP events around the
whole of (a) and of (b).  The two alternate within one process after a warm-up
of both; median, quartiles and extremes over the repeats are reported, and the
two results are compared word for word once per case.

One process; every case runs under its own time limit (a watchdog thread ends
the process, without starting anything more, when a case overruns it).

python tools/ssaa_probe.py [--out profiles/ssaa/ssaa_probe.json] [--reps 40] [--warmup 10]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CASES = [(3840, 2160, 2), (1920, 1080, 2), (1920, 1080, 4)]      # sample grid, samples per axis
PITCHES = (0.0, -0.6)


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
            "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per case (and for the set-up)")
    ap.add_argument("--out", default="profiles/ssaa/ssaa_probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("ssaa_probe: no GPU visible (there is nothing to measure without one)")
    faulthandler.dump_traceback_later(a.limit, exit=True)
    torch.cuda.set_device(0)
    tree = ort.build_terrain(a.depth, use_gpu=True)
    pool = ort.HOctree(tree.nodes, tree.root, a.depth, device=0)
    pool.set_palette(ort.VoxelData().get_colours())
    stream = torch.cuda.current_stream()
    pool.set_stream(stream)
    faulthandler.cancel_dump_traceback_later()
    res = {"depth": a.depth, "views": len(PITCHES), "device": torch.cuda.get_device_name(0), "cases": []}

    for ws, hs, s in CASES:
        faulthandler.dump_traceback_later(a.limit, exit=True)
        w, h, shift = ws // s, hs // s, 2 * (s.bit_length() - 1)
        cams = [ort.camera((1.5, 1.5, 1.5), 0.3, p, 1.25, ws, hs) for p in PITCHES]
        fused = torch.empty((len(cams), h, w), dtype=torch.int32, device="cuda")
        full = torch.empty((len(cams), hs, ws), dtype=torch.int32, device="cuda")

        def run_a():
            pool.render_ssaa_views_dev(cams, s, fused)

        def run_b():
            pool.render_views_dev(cams, full)
            ch = full.view(torch.uint8).view(len(cams), h, s, w, s, 4)
            mean = (ch.sum(dim=(2, 4), dtype=torch.int32) + (s * s // 2)) >> shift
            return mean.to(torch.uint8).view(torch.int32).view(len(cams), h, w)

        def timed(fn):
            """(stream ms by events around fn, the library's kernel ms of fn's traversal launch)"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), pool.last_kernel_ms()

        for _ in range(a.warmup):
            run_a()
            two_pass = run_b()
        torch.cuda.synchronize()
        equal = bool(torch.equal(fused, two_pass))
        t = {"a_stream": [], "a_kernel": [], "b_stream": [], "b_render_kernel": []}
        for _ in range(a.reps):                     # alternating, so drift hits both alike
            sa, ka = timed(run_a)
            sb, kb = timed(run_b)
            t["a_stream"].append(sa)
            t["a_kernel"].append(ka)
            t["b_stream"].append(sb)
            t["b_render_kernel"].append(kb)
        row = {"samples": [ws, hs], "s": s, "out": [w, h], "equal": equal,
               "sample_buffer_bytes": 4 * len(cams) * ws * hs, "frame_bytes": 4 * len(cams) * w * h}
        row.update({k: spread(v) for k, v in t.items()})
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
        del fused, full, two_pass
        faulthandler.cancel_dump_traceback_later()

    pool.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")
    return 0 if all(c["equal"] for c in res["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
