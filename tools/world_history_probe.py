"""A resident world's history, measured on one GPU, by §7e's method.

Every timing is a host clock around the whole synchronised step.  Three warm-up runs of every arm,
then the arms alternating in one process; medians, quartiles and extremes of seven runs.  Every arm
is compared with its baseline before anything is timed, and the probe stops there, with nothing of
those arms timed or written, if one differs.  What brings the world into the state an arm starts
from (a stroke, a checkout, a flush) is outside the clock.

Everything runs on the depth-12 terrain world at capacity 2^24.  Two strokes: the 40^3 brush (64 000
records) at the surface, and 2^20 random records.

  undo        back from the brushed world to the terrain, shown on a pool:
              checkout+flush        World.checkout(snapshot) + flush
              read_box+edit+flush   what the parent commit can do on the device: read_box (device) of the
                                    brush box before the stroke, then at undo time the old voxels as records,
                                    edit and flush; both parts are in the time, reported apart as well
              download+new_world    the parent's other way: download() before the stroke, then a new World
                                    and pool from it (the old ones closed outside the clock)
  diff        for each stroke, before against after:
              summary               World.diff(records=False)
              host                  World.diff into host memory (its summary call included)
              device                World.diff(device=True) (its summary call included)
              two_downloads         the parent's only way is download() before and after plus a host
                                    comparison; the two downloads alone are timed, a lower bound.  (och_pool_diff
                                    of two depth-12 downloads is not that comparison: two arrays share no ids,
                                    so it walks every position of the expanded trees, some 10^9 of them.)
              The truth every arm is compared with: World.at under both roots at the stroke's coordinates.
  compact     one compaction of the world after both strokes with no snapshot live and one with both
              strokes' snapshots live (single runs on fresh worlds: a compaction changes the store)

Also recorded: the diff's OCH_BUILD_TRACE phase line and n, pairs and the frontier per level.

python tools/world_history_probe.py [--out profiles/world_history/probe.json] [--reps 7]
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

from voxel_build_probe import spread, traced  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the set-up and for each group of arms")
    ap.add_argument("--out", default="profiles/world_history/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_history_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    depth, dim = a.depth, 1 << a.depth
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "clock": "time.perf_counter around the whole step, synchronisation included"}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)

    def save():
        outp.write_text(json.dumps(res, indent=1) + "\n")

    def clocked(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def measure(name, arms, facts):
        if not facts["equal"]:
            raise SystemExit(f"world_history_probe: {name}: an arm differs from its baseline; nothing timed")
        watchdog()
        for i in range(a.warmup):
            for _, run in arms:
                run(i)
        t = {k: [] for k, _ in arms}
        for i in range(a.reps):                                # alternating, so drift hits all alike
            for key, run in arms:
                t[key].append(run(a.warmup + i))
        out = dict(facts)
        for key, _ in arms:
            out[key] = spread(t[key])
        res[name] = out
        print(json.dumps({name: out}), flush=True)
        save()

    terrain = ort.build_terrain(depth, use_gpu=True)
    c = dim // 2
    top = max(z for z in range(dim) if terrain.at(c, c, z))
    lo = np.array([c - 20, c - 20, top - 20])
    brush = ort.box_records(lo, lo + 40, 1)
    rng = np.random.default_rng(20)
    scatter = np.empty((1 << 20, 4), np.uint32)
    scatter[:, :3] = rng.integers(0, dim, (1 << 20, 3))
    scatter[:, 3] = rng.integers(1, 6, 1 << 20)
    capacity = 1 << 24
    world = ort.World(terrain, capacity=capacity, device=0)
    pool = world.make_pool()
    try:
        s_terrain = world.snapshot()
        world.edit(brush)
        s_brush = world.snapshot()
        world.edit(scatter)
        s_scatter = world.snapshot()
        res["world"] = {"depth": depth, "capacity": capacity, "used": world.info()["used"], "pool_nodes": terrain.n_nodes,
                        "brush_lo": lo.tolist(), "brush_records": len(brush), "scatter_records": len(scatter)}

        # ---- undo: from s_brush back to s_terrain, on `pool`
        parts = {"read_box": [], "edit+flush": [], "download": [], "new_world": []}

        def to_brushed():
            world.checkout(s_brush)
            world.flush(pool)

        def undo_checkout(i):
            to_brushed()
            return clocked(lambda: (world.checkout(s_terrain), world.flush(pool)))

        def undo_read_box(i):
            world.checkout(s_terrain)
            kept = {}
            t1 = clocked(lambda: kept.__setitem__("grid", world.read_box(lo, lo + 40, np.uint32, device=True)))
            world.edit(brush)                                  # the stroke itself, as the application makes it
            world.flush(pool)

            def undo():
                back = torch.from_numpy(brush.view(np.int32)).cuda()
                back[:, 3] = kept["grid"].reshape(-1)           # box_records and the grid are both x fastest, then y, then z
                world.edit(back)
                world.flush(pool)
            t2 = clocked(undo)
            parts["read_box"].append(t1)
            parts["edit+flush"].append(t2)
            return t1 + t2

        spare = {}

        def undo_download(i):
            world.checkout(s_terrain)
            kept = {}
            t1 = clocked(lambda: kept.__setitem__("tree", world.download()))
            to_brushed()

            def undo():
                spare["world"] = ort.World(kept["tree"], capacity=capacity, device=0)
                spare["pool"] = spare["world"].make_pool()
            t2 = clocked(undo)
            spare["nodes"] = spare["world"].download().nodes
            spare["pool"].close()
            spare["world"].close()
            parts["download"].append(t1)
            parts["new_world"].append(t2)
            return t1 + t2

        equal = True
        undo_checkout(0)
        equal = equal and np.array_equal(world.download().nodes, terrain.nodes)
        undo_read_box(0)
        equal = equal and np.array_equal(world.download().nodes, terrain.nodes)
        undo_download(0)
        equal = equal and np.array_equal(spare["nodes"], terrain.nodes)
        for v in parts.values():
            v.clear()
        used_before = world.info()["used"]
        measure("undo", [("checkout+flush", undo_checkout), ("read_box+edit+flush", undo_read_box),
                         ("download+new_world", undo_download)], {"equal": bool(equal)})
        res["undo"]["parts"] = {k: spread(v[a.warmup:]) for k, v in parts.items()}
        res["undo"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
        save()

        # ---- diff
        def morton(rec):
            x, y, z = (rec[:, k].astype(np.uint64) for k in range(3))
            keys = np.zeros(len(rec), np.uint64)
            for l in range(depth):
                keys |= ((x >> np.uint64(l)) & np.uint64(1)) << np.uint64(3 * l) | \
                        ((y >> np.uint64(l)) & np.uint64(1)) << np.uint64(3 * l + 1) | \
                        ((z >> np.uint64(l)) & np.uint64(1)) << np.uint64(3 * l + 2)
            return keys

        def truth(stroke, s_a, s_b):
            """Only the stroke's coordinates can differ: World.at under both roots, the differing ones in Morton order."""
            coords = np.unique(stroke[:, :3], axis=0).astype(np.int32)
            world.checkout(s_a)
            ids_a = world.at(coords)
            world.checkout(s_b)
            ids_b = world.at(coords)
            rec = np.concatenate([coords.astype(np.uint32), ids_b[:, None]], 1)[ids_a != ids_b]
            keys = morton(rec)
            order = np.argsort(keys)
            return np.ascontiguousarray(rec[order]), keys[order]

        for name, stroke, s_a, s_b in (("brush", brush, s_terrain, s_brush), ("scatter", scatter, s_brush, s_scatter)):
            got = {}

            def summary(i):
                return clocked(lambda: got.__setitem__("summary", world.diff(s_a, s_b, records=False)))

            def host(i):
                return clocked(lambda: got.__setitem__("host", world.diff(s_a, s_b)))

            def device(i):
                return clocked(lambda: got.__setitem__("device", world.diff(s_a, s_b, device=True)))

            def downloads(i):
                def step():
                    world.checkout(s_a)
                    got["before"] = world.download()
                    world.checkout(s_b)
                    got["after"] = world.download()
                return clocked(step)

            summary(0), host(0), device(0), downloads(0)
            want, keys = truth(stroke, s_a, s_b)
            st = got["host"][1]
            frontier = [int(len(np.unique(keys >> np.uint64(3 * h)))) for h in range(depth, 0, -1)]
            equal = bool(got["host"][0].tobytes() == want.tobytes() and
                         got["device"][0].cpu().numpy().view(np.uint32).tobytes() == want.tobytes() and
                         got["summary"][1] == st == got["device"][1] and st["n"] == len(want) and
                         st["pairs"] == sum(frontier) and
                         st["box_lo"] == tuple(int(v) for v in want[:, :3].min(0)) and
                         st["box_hi"] == tuple(int(v) + 1 for v in want[:, :3].max(0)))
            measure(f"diff_{name}", [("summary", summary), ("host", host), ("device", device), ("two_downloads", downloads)],
                    {"equal": equal, "n": st["n"], "pairs": st["pairs"], "box_lo": list(st["box_lo"]), "box_hi": list(st["box_hi"]),
                     "frontier_per_level_root_first": frontier, "download_nodes": [got["before"].n_nodes, got["after"].n_nodes],
                     "two_downloads_is": "a lower bound of the parent's way: the host comparison of the two pools comes on top"})
            res[f"diff_{name}"]["device_trace"] = traced(lambda: world.diff(s_a, s_b, device=True))
            save()
    finally:
        pool.close()
        world.close()

    # ---- compact: one run each, on fresh worlds
    watchdog()
    out = {}
    for key, keep in (("no_snapshot", False), ("two_snapshots", True)):
        with ort.World(terrain, capacity=capacity, device=0) as w:
            w.edit(brush)
            s1 = w.snapshot()
            w.edit(scatter)
            s2 = w.snapshot()
            w.edit(brush * np.array([1, 1, 1, 0], np.uint32))
            want = w.download().nodes
            if not keep:
                w.release(s1), w.release(s2)
            used = w.info()["used"]
            ms = clocked(w.compact) * 1e3
            ok = bool(np.array_equal(w.download().nodes, want))
            out[key] = {"ms": round(ms, 3), "used_before": used, "used_after": w.info()["used"], "equal": ok,
                        "trace": traced(w.compact)}
    out["equal"] = bool(out["no_snapshot"]["equal"] and out["two_snapshots"]["equal"])
    res["compact"] = out
    print(json.dumps({"compact": out}), flush=True)

    faulthandler.cancel_dump_traceback_later()
    keys = [k for k in res if isinstance(res[k], dict) and "equal" in res[k]]
    ok = all(res[k]["equal"] for k in keys)
    res["all_equal"] = bool(ok)
    save()
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
