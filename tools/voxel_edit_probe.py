"""och_edit_voxels measured on one GPU, by §7c's method.

Every timing is a host clock around the whole call (which returns the pool on
the host, so it ends in a synchronise); three warm-up runs of every arm, then
the arms of an input alternating in one process; medians, quartiles and
extremes of seven runs, the library's own build_seconds beside them.

  brush_put    the depth-12 terrain with the reference's 40^3 brush already cut
               out at its surface (64 000 records), the same box set to id 1:
               gpu          edit_voxels(use_gpu=True)
               host_16      edit_voxels(threads=16)
               editor_set   what a caller had before: Editor.set() per record on
                            an editor that has already adopted the pool, then one
                            flush to its device pool
  brush_cut    the result of brush_put, the same box set to id 0: the same arms
  terrain_1m   the depth-12 terrain + 2^20 random records (§7c's mix): the same
               arms, the editor adopted afresh (not timed) before every run
  list_1m_1m   the 2^20-record world of §7c + 2^20 more records: gpu, host_16,
               and build_voxels of the concatenation from scratch on the GPU

The editor's adoption of the depth-12 pool (och_editor_create and its device
pool) is timed on its own.  Each library arm's OCH_BUILD_TRACE phase lines are
recorded from one further run, and the pools of an input's arms are compared
before anything is timed.

One process; the set-up and every input run under a time limit (a watchdog ends
the process, without starting anything more, when one overruns it).

python tools/voxel_edit_probe.py [--out profiles/voxel_edit/probe.json] [--reps 7]
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
sys.path.insert(0, str(Path(__file__).resolve().parent))

from voxel_build_probe import random_records, spread, traced  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=400, help="seconds for the set-up and for each input")
    ap.add_argument("--out", default="profiles/voxel_edit/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("voxel_edit_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    depth = a.depth
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "host_threads": a.threads,
           "clock": "time.perf_counter around the call; the call returns the pool on the host"}
    ok = True

    def same(p, q):
        return bool(p.root == q.root and np.array_equal(p.nodes, q.nodes) and p.solid_voxels == q.solid_voxels and
                    p.tree_nodes == q.tree_nodes and list(p.voxel_hist) == list(q.voxel_hist))

    def library_arm(fn):
        """fn() is one library call that returns a pool: (seconds, build_seconds)."""
        def run():
            t0 = time.perf_counter()
            pool = fn()
            return time.perf_counter() - t0, pool.build_seconds
        run.traced = fn
        return run

    def measure(name, arms, facts):
        """arms: (key, run) pairs; run() does one edit and returns (seconds, build_seconds or None)."""
        watchdog()
        for _ in range(a.warmup):
            for _, run in arms:
                run()
        t = {k: [] for k, _ in arms}
        inside = {k: [] for k, _ in arms}
        for _ in range(a.reps):                                # alternating, so drift hits all alike
            for key, run in arms:
                s, b = run()
                t[key].append(s)
                if b is not None:
                    inside[key].append(b)                      # the library's own clock: without the binding's copy
        out = dict(facts)
        for key, run in arms:
            out[key] = spread(t[key])
            if inside[key]:
                out[key]["build_seconds_median_ms"] = round(float(np.median(inside[key])) * 1e3, 3)
            if hasattr(run, "traced"):
                out[key]["trace"] = traced(run.traced)
        res[name] = out
        print(json.dumps({name: out}), flush=True)

    def stroke(ed, pool, rows):
        t0 = time.perf_counter()
        for x, y, z, v in rows:
            ed.set(x, y, z, v)
        ed.flush(pool)
        pool.synchronize()
        return time.perf_counter() - t0

    # ---- the depth-12 terrain and the brush at its surface
    terrain = ort.build_terrain(depth, use_gpu=True)
    c = 1 << (depth - 1)
    top = max(z for z in range(1 << depth) if terrain.at(c, c, z))
    lo = np.array([c - 20, c - 20, top - 20])
    put_rec, cut_rec = ort.box_records(lo, lo + 40, 1), ort.box_records(lo, lo + 40, 0)
    cut0 = ort.edit_voxels(terrain, cut_rec, use_gpu=True)
    put = ort.edit_voxels(cut0, put_rec, use_gpu=True)
    cut = ort.edit_voxels(put, cut_rec, use_gpu=True)
    equal = same(cut, cut0) and same(put, ort.edit_voxels(cut, put_rec, threads=a.threads)) and \
        same(cut, ort.edit_voxels(put, cut_rec, threads=a.threads))
    capacity = terrain.n_nodes + (1 << 24)                 # room for every path copy of 2^20 set() calls
    adopt = []
    for _ in range(3):
        t0 = time.perf_counter()
        ed = ort.Editor(cut.nodes, cut.root, depth, capacity=capacity)
        t1 = time.perf_counter()
        dev = ed.make_pool(device=0)
        dev.synchronize()
        adopt.append((t1 - t0, time.perf_counter() - t1))
        dev.close()
        ed.close()
    res["editor_adoption"] = {"pool_nodes": cut.n_nodes, "capacity": capacity,
                              "och_editor_create_ms": [round(s * 1e3, 1) for s, _ in adopt],
                              "device_pool_ms": [round(s * 1e3, 1) for _, s in adopt]}
    print(json.dumps({"editor_adoption": res["editor_adoption"]}), flush=True)

    with ort.Editor(cut.nodes, cut.root, depth, capacity=capacity) as ed:
        dev = ed.make_pool(device=0)
        try:
            put_rows, cut_rows = put_rec.tolist(), cut_rec.tolist()
            stroke(ed, dev, put_rows)
            equal = equal and same(put, ort.edit_voxels((ed.nodes(), ed.root, depth), np.zeros((0, 4), np.uint32), use_gpu=True))
            stroke(ed, dev, cut_rows)
            ok = ok and equal

            def editor_put():                                  # from the cut tree and back to it
                s = stroke(ed, dev, put_rows)
                stroke(ed, dev, cut_rows)
                return s, None

            def editor_cut():
                stroke(ed, dev, put_rows)
                return stroke(ed, dev, cut_rows), None

            facts = {"depth": depth, "records": len(put_rec), "box_lo": lo.tolist(), "pool_nodes": cut.n_nodes,
                     "pools_equal": equal}
            measure("brush_put", [("gpu", library_arm(lambda: ort.edit_voxels(cut, put_rec, use_gpu=True))),
                                  ("host_16", library_arm(lambda: ort.edit_voxels(cut, put_rec, threads=a.threads))),
                                  ("editor_set", editor_put)], dict(facts, result_nodes=put.n_nodes))
            measure("brush_cut", [("gpu", library_arm(lambda: ort.edit_voxels(put, cut_rec, use_gpu=True))),
                                  ("host_16", library_arm(lambda: ort.edit_voxels(put, cut_rec, threads=a.threads))),
                                  ("editor_set", editor_cut)], dict(facts, result_nodes=cut.n_nodes))
        finally:
            dev.close()
    del cut0, put, cut

    # ---- the terrain + 2^20 random records
    watchdog()
    n = 1 << 20
    rec = random_records(n, n, depth)
    g = ort.edit_voxels(terrain, rec, use_gpu=True)
    equal = same(g, ort.edit_voxels(terrain, rec, threads=a.threads))
    rows = rec.tolist()
    with ort.Editor(terrain.nodes, terrain.root, depth, capacity=capacity) as ed:
        for x, y, z, v in rows:
            ed.set(x, y, z, v)
        equal = equal and same(g, ort.edit_voxels((ed.nodes(), ed.root, depth), np.zeros((0, 4), np.uint32), use_gpu=True))
    ok = ok and equal

    def editor_1m():
        with ort.Editor(terrain.nodes, terrain.root, depth, capacity=capacity) as ed:
            dev = ed.make_pool(device=0)
            try:
                return stroke(ed, dev, rows), None
            finally:
                dev.close()

    measure("terrain_1m", [("gpu", library_arm(lambda: ort.edit_voxels(terrain, rec, use_gpu=True))),
                           ("host_16", library_arm(lambda: ort.edit_voxels(terrain, rec, threads=a.threads))),
                           ("editor_set", editor_1m)],
            {"depth": depth, "records": n, "pool_nodes": terrain.n_nodes, "result_nodes": g.n_nodes, "pools_equal": equal})
    del rows, g

    # ---- the 2^20-record world + 2^20 more records
    watchdog()
    more = random_records(n + 1, n, depth)
    world = ort.build_voxels(rec, depth=depth, use_gpu=True)
    both = np.concatenate([rec, more])
    g = ort.edit_voxels(world, more, use_gpu=True)
    equal = same(g, ort.edit_voxels(world, more, threads=a.threads)) and same(g, ort.build_voxels(both, depth=depth, use_gpu=True))
    ok = ok and equal
    measure("list_1m_1m", [("gpu", library_arm(lambda: ort.edit_voxels(world, more, use_gpu=True))),
                           ("host_16", library_arm(lambda: ort.edit_voxels(world, more, threads=a.threads))),
                           ("build_voxels_gpu", library_arm(lambda: ort.build_voxels(both, depth=depth, use_gpu=True)))],
            {"depth": depth, "records": n, "pool_nodes": world.n_nodes, "result_nodes": g.n_nodes, "pools_equal": equal})

    faulthandler.cancel_dump_traceback_later()
    res["all_pools_equal"] = ok
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
