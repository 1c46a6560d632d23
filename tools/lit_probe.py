"""The lit launch against its in-place arm, against today's composition of the
same pixels, and against the plain render.

Depth-12 terrain, 1920x1080, the bench's two views; sun (0.8, 0.35, 0.25), AO
reach eight voxels, shades 96 / 24.  In one process, alternating, after a
warm-up of all four:
  (a) och_gpu_render_lit_views_dev, OCH_OPT_BOUNCE_COMPACT 0: every hit lane
      walks its own pixel's secondary rays;
  (b) the same launch with the block's hit pixels queued and their rays dealt
      over its lanes (OCH_OPT_BOUNCE_COMPACT 1);
  (c) the composition a caller had before: per view raygen, a tiled trace, the
      hit pixels compacted and their secondary rays built in torch, one
      trace_batch_dev per ray kind, a torch shade;
  (d) och_gpu_render_views_dev, the plain frame.
(c) is first checked against (a) word for word, and (b) against (a).  Kernel
times are the library's own (och_gpu_last_kernel_ms: the dispatch's events;
for (c) the sum over its traversal launches, taken in passes of their own
because reading them waits for each launch); stream times are HIP events
around the whole of each.  Median, quartiles and extremes over the repeats.

One process; set-up and measurement each run under a time limit (a watchdog
ends the process, without starting anything more, when one overruns it).

python tools/lit_probe.py [--out profiles/lit/lit_probe.json] [--reps 30] [--warmup 5]
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
SKY, INSIDE, MAGENTA = 0xFFFEBF00, 0xFF07193F, 0xFFFF00FF


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
            "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for the set-up, and for the measurement")
    ap.add_argument("--out", default="profiles/lit/lit_probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("lit_probe: no GPU visible (there is nothing to measure without one)")
    faulthandler.dump_traceback_later(a.limit, exit=True)
    torch.cuda.set_device(0)
    tree = ort.build_terrain(a.depth, use_gpu=True)
    pool = ort.HOctree(tree.nodes, tree.root, a.depth, device=0)
    pal_np = ort.VoxelData().get_colours()
    pool.set_palette(pal_np)
    stream = torch.cuda.current_stream()
    pool.set_stream(stream)
    W, H, nv = a.width, a.height, len(PITCHES)
    light = ort.Light(SUN, 8 * 2.0 ** -a.depth, 96, 24)
    ort.light_check(light)
    cams = [ort.camera(ORIGIN, 0.3, p, 1.25, W, H) for p in PITCHES]
    dev = torch.device("cuda", 0)
    lit_a = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
    lit_b = torch.empty_like(lit_a)
    plain = torch.empty_like(lit_a)
    pal = torch.from_numpy(pal_np.astype(np.int64)).to(dev)
    n_vox = pal.numel() // 6
    origin = torch.tensor(ORIGIN, dtype=torch.float32, device=dev)
    sun = torch.tensor(SUN, dtype=torch.float32, device=dev)
    dirs = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    hd, hv = (torch.empty(H * W, dtype=torch.int32, device=dev) for _ in range(2))
    ht = torch.empty(H * W, dtype=torch.float32, device=dev)
    half = 2.0 ** -(a.depth + 1)
    kernel_ms = []                           # (c)'s traversal launches, when a pass asks for them

    def run_a():
        pool.set_option("bounce_compact", 0)
        pool.render_lit_views_dev(cams, light, lit_a)

    def run_b():
        pool.set_option("bounce_compact", 1)
        pool.render_lit_views_dev(cams, light, lit_b)

    def run_d():
        pool.render_views_dev(cams, plain)

    def run_c(want_kernel=False):
        frames = []
        for cam in cams:
            pool.raygen_dev(cam, dirs)
            pool.trace_batch_tiled_dev(origin, dirs, W, hd, hv, ht)
            if want_kernel:
                kernel_ms.append(pool.last_kernel_ms())
            hit = torch.nonzero(hd < 6).squeeze(1)                      # waits for the trace: the hit count
            d1, fd, t = dirs[hit], hd[hit].long(), ht[hit]
            axis = fd % 3
            q = origin + d1 * t[:, None]                                # two torch ops: product rounded, then the sum
            off = torch.where(fd < 3, half, -half).to(torch.float32)
            p = q.clone()
            rows = torch.arange(hit.numel(), device=dev)
            p[rows, axis] = q[rows, axis] - off
            n = hit.numel()
            sd, sv = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
            st = torch.empty(n, dtype=torch.float32, device=dev)
            mask = torch.zeros(n, dtype=torch.int32, device=dev)
            s_a = sun[axis]
            facing = torch.where(fd < 3, s_a < 0, s_a > 0)
            pool.trace_batch_dev(p, sun.expand(n, 3).contiguous(), sd, sv, st)
            if want_kernel:
                kernel_ms.append(pool.last_kernel_ms())
            mask |= torch.where(~facing, 0x30, torch.where(sd != 6, 0x10, 0)).int()
            normal = torch.where(fd < 3, -1.0, 1.0).to(torch.float32)
            for k in range(4):
                ad = torch.empty((n, 3), dtype=torch.float32, device=dev)
                ad[rows, axis] = normal
                ad[rows, (axis + 1) % 3] = -1.0 if k & 1 else 1.0
                ad[rows, (axis + 2) % 3] = -1.0 if k & 2 else 1.0
                pool.trace_batch_dev(p, ad, sd, sv, st)
                if want_kernel:
                    kernel_ms.append(pool.last_kernel_ms())
                mask |= ((sd != 6) & ((sd == 7) | (st < light.ao_reach))).int() << k
            # the plain colours, then the shade
            vox = hv.long()
            ok = (hd < 6) & (vox >= 1) & (vox <= n_vox)
            col = torch.where(ok, pal[torch.where(ok, 6 * (vox - 1) + hd.long(), 0)], MAGENTA)
            col = torch.where(hd == 6, SKY, torch.where(hd == 7, INSIDE, col))
            w = torch.full((H * W,), 256, dtype=torch.int64, device=dev)
            cnt = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1)
            w[hit] = (256 - light.sun_shade * ((mask >> 4) & 1) - light.ao_shade * cnt).long()
            out = col & 0xFF000000
            for sh in (0, 8, 16):
                out = out | (((((col >> sh) & 0xFF) * w + 128) >> 8) << sh)
            frames.append(out)
        return torch.stack(frames).view(nv, H, W)

    def timed(fn):
        """(stream ms by events around fn, the library's kernel ms of fn's last traversal launch)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), pool.last_kernel_ms()

    for _ in range(a.warmup):
        run_a()
        run_b()
        composed = run_c()
        run_d()
    torch.cuda.synchronize()
    word = lambda x: (x & 0xFFFFFFFF).to(torch.int64)                    # noqa: E731
    equal_c = bool(torch.equal(word(composed), word(lit_a.long())))
    equal_b = bool(torch.equal(lit_a, lit_b))
    hits = int((lit_a != plain).sum().item())
    faulthandler.cancel_dump_traceback_later()
    faulthandler.dump_traceback_later(a.limit, exit=True)
    t = {k: [] for k in ("a_stream", "a_kernel", "b_stream", "b_kernel", "c_stream", "c_kernel_sum", "d_stream",
                         "d_kernel")}
    for _ in range(a.reps):                             # alternating, so drift hits all alike
        for key, fn in (("a", run_a), ("b", run_b), ("d", run_d)):
            s_ms, k_ms = timed(fn)
            t[key + "_stream"].append(s_ms)
            t[key + "_kernel"].append(k_ms)
        t["c_stream"].append(timed(run_c)[0])
        kernel_ms.clear()
        run_c(want_kernel=True)
        t["c_kernel_sum"].append(sum(kernel_ms))
    faulthandler.cancel_dump_traceback_later()
    res = {"depth": a.depth, "views": nv, "size": [W, H], "device": torch.cuda.get_device_name(0),
           "light": {"sun_dir": list(SUN), "ao_reach": light.ao_reach, "sun_shade": 96, "ao_shade": 24},
           "composition_equals_lit": equal_c, "queued_equals_in_place": equal_b, "pixels_changed_by_light": hits,
           "c_traversal_launches": len(kernel_ms)}
    res.update({k: spread(v) for k, v in t.items()})
    print(json.dumps(res), flush=True)
    pool.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")
    return 0 if equal_c and equal_b else 1


if __name__ == "__main__":
    sys.exit(main())
