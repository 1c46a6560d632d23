"""och_world measured on one GPU, by §7d's method.

Every timing is a host clock around the whole step, synchronisation included: a step ends when the
new content can be drawn (the pool that shows it exists, or the flush has returned).  Three warm-up
runs of every arm, then the arms alternating in one process; medians, quartiles and extremes of
seven runs.

  brush        the depth-12 terrain and the reference's 40^3 brush at its surface (64 000 records),
               set and removed in turn, one stroke per run:
               edit_voxels+pool  the parent's way: edit_voxels(use_gpu=True) on the host pool, then
                                 the HOctree that shows the result
               editor_set        the parent's other way: Editor.set() per record on an editor that
                                 has adopted the pool, then one flush to its device pool
               world             World.edit + World.flush on one world and one pool
               world+frame       the same, then one two-view 1920x1080 frame, synchronised
  brush_moving the same brush dragged (7, 5, 0) voxels per stroke, ids changing: world alone
  random_1m    the depth-12 terrain + 2^20 random records (a fresh list every run):
               edit_voxels+pool and world (a fresh world per run, made outside the clock)

Also recorded: the ids a stroke consumes (info()["used"] deltas, what sizes a capacity), compact()
and download() on the brushed world, och_world_create, and each world step's OCH_BUILD_TRACE phase
lines from one further run.  Downloads are compared with the edit_voxels chain before anything is timed.

One process; the set-up and every input run under a time limit (a watchdog ends the process,
without starting anything more, when one overruns it).

python tools/world_probe.py [--out profiles/world/probe.json] [--reps 7]
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
    ap.add_argument("--limit", type=int, default=300, help="seconds for the set-up and for each input")
    ap.add_argument("--out", default="profiles/world/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    depth = a.depth
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "clock": "time.perf_counter around the whole step, synchronisation included"}

    def same(p, q):
        return bool(p.root == q.root and np.array_equal(p.nodes, q.nodes) and p.solid_voxels == q.solid_voxels and
                    p.tree_nodes == q.tree_nodes and list(p.voxel_hist) == list(q.voxel_hist))

    def clocked(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def measure(name, arms, facts):
        """arms: (key, run) pairs; run(i) does step i and returns its seconds."""
        watchdog()
        step = 0
        for _ in range(a.warmup):
            for _, run in arms:
                run(step)
            step += 1
        t = {k: [] for k, _ in arms}
        for _ in range(a.reps):                                # alternating, so drift hits all alike
            for key, run in arms:
                t[key].append(run(step))
            step += 1
        out = dict(facts)
        for key, _ in arms:
            out[key] = spread(t[key])
        res[name] = out
        print(json.dumps({name: out}), flush=True)
        return step

    # ---- the depth-12 terrain and the brush at its surface
    terrain = ort.build_terrain(depth, use_gpu=True)
    c = 1 << (depth - 1)
    top = max(z for z in range(1 << depth) if terrain.at(c, c, z))
    lo = np.array([c - 20, c - 20, top - 20])
    strokes = [ort.box_records(lo, lo + 40, 1), ort.box_records(lo, lo + 40, 0)]          # put, cut, put, ...
    put = ort.edit_voxels(terrain, strokes[0], use_gpu=True)
    cut = ort.edit_voxels(put, strokes[1], use_gpu=True)
    capacity = 1 << 24                                         # the most a packed layout can number
    t0 = time.perf_counter()
    world = ort.World(terrain, capacity=capacity, device=0)
    res["world_create_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    pool = world.make_pool()
    res["world_make_pool_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    used0 = world.info()["used"]
    world.edit(strokes[0])
    equal = same(world.download(), put)
    world.edit(strokes[1])
    equal = equal and same(world.download(), cut)
    world.flush(pool)
    res["brush_ids_per_stroke_first"] = world.info()["used"] - used0
    framed = ort.World(cut, capacity=capacity, device=0)       # the world+frame arm's own world: every arm alternates
    framed_pool = framed.make_pool()
    ed_capacity = terrain.n_nodes + (1 << 22)
    ed = ort.Editor(cut.nodes, cut.root, depth, capacity=ed_capacity)
    ed_pool = ed.make_pool(device=0)
    rows = [s.tolist() for s in strokes]
    host = {"tree": cut}                                       # the parent's way keeps its world on the host
    used = []
    framed_pool.set_palette(ort.VoxelData().get_colours())
    cams = [ort.camera((1.5, 1.5, 1.5), 0.3, p, 1.25, 1920, 1080) for p in (0.0, -0.6)]
    frames = torch.zeros((2, 1080, 1920), dtype=torch.int32, device="cuda")

    def parent_way(i):
        def step():
            host["tree"] = ort.edit_voxels(host["tree"], strokes[i % 2], use_gpu=True)
            with ort.HOctree(host["tree"].nodes, host["tree"].root, depth, device=0) as shown:
                shown.synchronize()
        return clocked(step)

    def editor_way(i):
        def step():
            for x, y, z, v in rows[i % 2]:
                ed.set(x, y, z, v)
            ed.flush(ed_pool)
            ed_pool.synchronize()
        return clocked(step)

    def world_step(i):
        world.edit(strokes[i % 2])
        world.flush(pool)

    def world_way(i):
        before = world.info()["used"]
        s = clocked(lambda: world_step(i))
        used.append(world.info()["used"] - before)
        return s

    def world_frame(i):
        def step():
            framed.edit(strokes[i % 2])
            framed.flush(framed_pool)
            framed_pool.render_views_dev(cams, frames)
            framed_pool.synchronize()
        return clocked(step)

    try:
        n = measure("brush", [("edit_voxels+pool", parent_way), ("editor_set", editor_way), ("world", world_way),
                              ("world+frame", world_frame)],
                    {"depth": depth, "records": len(strokes[0]), "box_lo": lo.tolist(), "pool_nodes": terrain.n_nodes,
                     "world_capacity": capacity, "downloads_equal": equal})
        res["brush"]["world_ids_per_stroke"] = used[a.warmup:]
        res["brush"]["world_trace"] = traced(lambda: world_step(n))
        # the same brush dragged along the surface: every stroke makes nodes the store has not seen
        # (put and cut in turn re-intern what two strokes ago left there: 0 new ids)
        moved = []

        def moving(i):
            rec = ort.box_records(lo + (7 * (i + 1), 5 * (i + 1), 0), lo + 40 + (7 * (i + 1), 5 * (i + 1), 0), 1 + i % 5)
            before = world.info()["used"]
            sec = clocked(lambda: (world.edit(rec), world.flush(pool)))
            moved.append(world.info()["used"] - before)
            return sec

        measure("brush_moving", [("world", moving)], {"depth": depth, "records": len(strokes[0]), "step": [7, 5, 0]})
        res["brush_moving"]["world_ids_per_stroke"] = moved[a.warmup:]
        info = world.info()
        res["brushed_world"] = {"used": info["used"], "strokes": info["strokes"],
                                "download_ms": spread([clocked(world.download) for _ in range(3)]),
                                "download_trace": traced(world.download)}
        t = clocked(world.compact)
        res["brushed_world"]["compact_ms"] = round(t * 1e3, 1)
        res["brushed_world"]["used_after_compact"] = world.info()["used"]
        res["brushed_world"]["flush_after_compact_ms"] = round(clocked(lambda: world.flush(pool)) * 1e3, 1)
    finally:
        ed_pool.close()
        ed.close()
        framed_pool.close()
        framed.close()
        pool.close()
        world.close()
    print(json.dumps({"brushed_world": res["brushed_world"]}), flush=True)

    # ---- the terrain + 2^20 random records, a fresh list and a fresh world every run
    watchdog()
    n_rec, runs = 1 << 20, a.warmup + a.reps
    lists = [random_records(100 + i, n_rec, depth) for i in range(runs + 1)]
    with ort.World(terrain, capacity=capacity, device=0) as w:
        w.edit(lists[runs])
        equal = same(w.download(), ort.edit_voxels(terrain, lists[runs], use_gpu=True))
        ids_1m = w.info()["used"] - used0
    ids = []

    def parent_1m(i):
        def step():
            tree = ort.edit_voxels(terrain, lists[i], use_gpu=True)
            with ort.HOctree(tree.nodes, tree.root, depth, device=0) as shown:
                shown.synchronize()
        return clocked(step)

    def world_1m(i):
        with ort.World(terrain, capacity=capacity, device=0) as w, w.make_pool() as p:
            def step():
                w.edit(lists[i])
                w.flush(p)
            s = clocked(step)
            ids.append(w.info()["used"] - used0)
            if i == runs - 1:
                res["random_1m_world_trace"] = traced(lambda: (w.edit(lists[i]), w.flush(p)))
        return s

    measure("random_1m", [("edit_voxels+pool", parent_1m), ("world", world_1m)],
            {"depth": depth, "records": n_rec, "pool_nodes": terrain.n_nodes, "world_capacity": capacity,
             "downloads_equal": equal, "ids_first": ids_1m})
    res["random_1m"]["world_ids_per_stroke"] = ids[a.warmup:]

    faulthandler.cancel_dump_traceback_later()
    ok = bool(res["brush"]["downloads_equal"] and res["random_1m"]["downloads_equal"])
    res["all_downloads_equal"] = ok
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
