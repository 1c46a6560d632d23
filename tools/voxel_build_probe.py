"""och_build_voxels measured on one GPU.

Three inputs, the arms of each alternating in one process after three warm-up
runs of every arm; every timing is a host clock around the whole call (which
returns the pool on the host, so it ends in a synchronise); medians, quartiles
and extremes of at least seven runs:

  list_1m    a seeded random list of 2^20 records at depth 12 (ids 1-5, a
             tenth repeated coordinates, a twentieth removals):
             gpu          build_voxels(use_gpu=True), records in host memory
             gpu_tensor   the same records as a CUDA tensor
             host_16      build_voxels(threads=16)
             editor_set   what a caller had before: Editor.set() per record from
                          an empty tree, then one flush to a device pool
  list_16m   2^24 such records: gpu, gpu_tensor, host_16
  terrain_d9 the depth-9 terrain as a 512^3 uint8 grid: gpu, host_16, beside
             build_terrain(9, use_gpu=True)

Each arm's OCH_BUILD_TRACE phase lines are recorded from one further run, and
the pools of an input's arms are compared before anything is timed.

One process; the set-up and every input run under a time limit (a watchdog ends
the process, without starting anything more, when one overruns it).

python tools/voxel_build_probe.py [--out profiles/voxel_build/probe.json] [--reps 7]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def spread(seconds):
    a = np.asarray(seconds, np.float64) * 1e3
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3),
            "min_ms": round(float(a.min()), 3), "max_ms": round(float(a.max()), 3), "n": int(a.size)}


def random_records(seed, n, depth):
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 4), np.uint32)
    rec[:, :3] = rng.integers(0, 1 << depth, (n, 3))
    rec[:, 3] = rng.integers(1, 6, n)
    n_dup = n // 10
    rec[n - n_dup:, :3] = rec[rng.integers(0, n - n_dup, n_dup), :3]
    rec[rng.random(n) < 0.05, 3] = 0
    return rec


def pool_to_grid(tree, dtype):
    """The pool's voxels as a dense [z, y, x] grid: one level of children at a time."""
    ids = np.array([[[tree.root]]], np.uint32)
    for _ in range(tree.depth):
        n = ids.shape[0]
        ch = np.where((ids > 0)[..., None], tree.nodes[np.maximum(ids, 1) - 1], 0).astype(np.uint32)
        ids = ch.reshape(n, n, n, 2, 2, 2).transpose(0, 3, 1, 4, 2, 5).reshape(2 * n, 2 * n, 2 * n)
    return np.ascontiguousarray(ids.astype(dtype))


def traced(fn):
    """fn() with OCH_BUILD_TRACE=1: the builder's phase lines (written to stderr by the library)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.environ["OCH_BUILD_TRACE"] = "1"
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["OCH_BUILD_TRACE"]
        f.seek(0)
        return [ln.strip() for ln in f.read().decode(errors="replace").splitlines() if ln.startswith("[och_build]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--terrain-depth", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=400, help="seconds for the set-up and for each input")
    ap.add_argument("--out", default="profiles/voxel_build/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("voxel_build_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "host_threads": a.threads,
           "clock": "time.perf_counter around the call; the call returns the pool on the host"}
    ok = True

    def same(p, q):
        return bool(p.root == q.root and np.array_equal(p.nodes, q.nodes) and p.solid_voxels == q.solid_voxels and
                    p.tree_nodes == q.tree_nodes and list(p.voxel_hist) == list(q.voxel_hist))

    def measure(name, arms, facts):
        """arms: (key, fn) pairs; fn() runs one build."""
        nonlocal ok
        watchdog()
        for _ in range(a.warmup):
            for _, fn in arms:
                fn()
        t = {k: [] for k, _ in arms}
        inside = {k: [] for k, _ in arms}
        for _ in range(a.reps):                                # alternating, so drift hits all alike
            for key, fn in arms:
                t0 = time.perf_counter()
                pool = fn()
                t[key].append(time.perf_counter() - t0)
                if pool is not None:
                    inside[key].append(pool.build_seconds)     # the library's own clock: without the binding's copy
        out = dict(facts)
        for key, fn in arms:
            out[key] = spread(t[key])
            if inside[key]:
                out[key]["build_seconds_median_ms"] = round(float(np.median(inside[key])) * 1e3, 3)
            out[key]["trace"] = traced(fn)
        res[name] = out
        print(json.dumps({name: out}), flush=True)

    def editor_arm(rec, depth, capacity):
        rows = rec.tolist()

        def run():
            with ort.Editor(np.zeros((0, 8), np.uint32), 0, depth, capacity=capacity) as ed:
                pool = ed.make_pool(device=0)
                try:
                    for x, y, z, v in rows:
                        ed.set(x, y, z, v)
                    ed.flush(pool)
                    pool.synchronize()
                finally:
                    pool.close()
        return run

    for name, n in (("list_1m", 1 << 20), ("list_16m", 1 << 24)):
        watchdog()
        rec = random_records(n, n, a.depth)
        dev = torch.from_numpy(rec.view(np.int32)).cuda()
        g = ort.build_voxels(rec, depth=a.depth, use_gpu=True)
        h = ort.build_voxels(rec, depth=a.depth, threads=a.threads)
        t = ort.build_voxels(dev, depth=a.depth, use_gpu=True)
        equal = same(g, h) and same(g, t)
        ok = ok and equal
        arms = [("gpu", lambda: ort.build_voxels(rec, depth=a.depth, use_gpu=True)),
                ("gpu_tensor", lambda: ort.build_voxels(dev, depth=a.depth, use_gpu=True)),
                ("host_16", lambda: ort.build_voxels(rec, depth=a.depth, threads=a.threads))]
        if n == 1 << 20:
            arms.append(("editor_set", editor_arm(rec, a.depth, 2 * g.tree_nodes)))
        measure(name, arms, {"records": n, "depth": a.depth, "solid_voxels": g.solid_voxels, "tree_nodes": g.tree_nodes,
                             "unique_nodes": g.n_nodes, "pools_equal": equal})
        del rec, dev

    watchdog()
    d = a.terrain_depth
    terrain = ort.build_terrain(d, use_gpu=True)
    grid = pool_to_grid(terrain, np.uint8)
    g = ort.build_voxels(grid, use_gpu=True)
    h = ort.build_voxels(grid, threads=a.threads)
    equal = same(g, h) and bool(np.array_equal(g.nodes, terrain.nodes)) and g.solid_voxels == terrain.solid_voxels
    ok = ok and equal
    measure(f"terrain_d{d}", [("gpu", lambda: ort.build_voxels(grid, use_gpu=True)),
                              ("host_16", lambda: ort.build_voxels(grid, threads=a.threads)),
                              ("build_terrain_gpu", lambda: ort.build_terrain(d, use_gpu=True))],
            {"grid": list(grid.shape), "dtype": "uint8", "depth": d, "solid_voxels": g.solid_voxels,
             "tree_nodes": g.tree_nodes, "unique_nodes": g.n_nodes, "pools_equal_and_equal_build_terrain": equal})

    faulthandler.cancel_dump_traceback_later()
    res["all_pools_equal"] = ok
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
