"""A resident world's box strokes, measured on one GPU, by §7e's method.

Every timing is a host clock around the whole synchronised step.  Three warm-up runs of every arm,
then the arms alternating in one process; medians, quartiles and extremes of seven runs.  Every arm
is compared with its truth before anything is timed, and the probe stops there, with nothing of
those arms timed or written, if one differs.  What brings the world into the state an arm starts
from (a checkout, a flush) is outside the clock.

Everything runs on the depth-12 terrain world at capacity 2^24.

  brush       the reference's 40^3 brush at the surface, put and cut in turn, the box dragged three voxels
              a run; each time is one put + flush and one cut + flush:
              fill_box+flush        World.fill_box(lo, lo + 40, 1 / 0) + flush
              edit+flush            the parent's way: World.edit(box_records(...)) from host memory + flush
  box256      an unaligned 256^3 box across the surface set to id 1:
              fill_box              World.fill_box
              edit_device           the parent's way: World.edit of its 2^24 records from a device tensor
  clear1024   an unaligned 1024^3 box cleared: fill_box alone.  The parent's way would need a list of 2^30
              records (16 GiB), which is recorded in place of a time.
  restore     the brush box put back as it was before the stroke:
              restore_box+flush     World.restore_box(snapshot, box) + flush
              read_box+edit+flush   §7g's second arm: read_box (device) before the stroke, the old voxels as
                                    records, edit and flush; both parts are in the time
  The truth: the two arms of a pair must leave the same root id (one store: equal ids are equal content),
  World.at over the box's voxels (a sample of them for the large boxes) and around it must give the id
  inside and the terrain's voxels outside, and the stats must equal ort.box_cubes' totals.

Also recorded: each region stroke's OCH_BUILD_TRACE phase lines, its stats and the ids it consumed.

python tools/world_region_probe.py [--out profiles/world_region/probe.json] [--reps 7]
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
    ap.add_argument("--out", default="profiles/world_region/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_region_probe: no GPU visible (there is nothing to measure without one)")

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
            raise SystemExit(f"world_region_probe: {name}: an arm differs from its truth; nothing timed")
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
    capacity = 1 << 24
    world = ort.World(terrain, capacity=capacity, device=0)
    pool = world.make_pool()
    rng = np.random.default_rng(21)

    def sample(lo, hi, n=1 << 16):
        """Coordinates in and around the box: its corners, n inside it and n in the shell of width 8 around it."""
        lo, hi = np.asarray(lo), np.asarray(hi)
        inside = rng.integers(lo, hi, (n, 3))
        shell = rng.integers(lo - 8, hi + 8, (n, 3))
        corners = np.array([[(lo, hi - 1)[(k >> ax) & 1][ax] for ax in range(3)] for k in range(8)])
        return np.concatenate([corners, inside, shell]).astype(np.int32)

    def at_truth(coords, lo, hi, id, before):
        """World.at after a fill of [lo, hi) with id, given the ids before it."""
        inside = ((coords >= np.asarray(lo)) & (coords < np.asarray(hi))).all(1)
        return np.where(inside, np.uint32(id), before)

    def stats_equal(st, lo, hi):
        keys, heights, cubes, cells = ort.box_cubes(lo, hi, depth)
        return (st["cubes"], st["cells"]) == (len(keys), int(cells.sum()))

    try:
        s_terrain = world.snapshot()
        root_terrain = world.info()["root"]
        res["world"] = {"depth": depth, "capacity": capacity, "used": world.info()["used"], "pool_nodes": terrain.n_nodes}

        # ---- brush: put and cut in turn, dragged
        lo0 = np.array([c - 20, c - 20, top - 20])

        def brush_box(i):
            lo = lo0 + np.array([3 * i, 0, 0])
            return lo, lo + 40

        roots = {}

        def brush_fill(i):
            lo, hi = brush_box(i)
            world.checkout(s_terrain)
            world.flush(pool)

            def step():
                world.fill_box(lo, hi, 1)
                world.flush(pool)
                roots["fill put"] = world.info()["root"]
                world.fill_box(lo, hi, 0)
                world.flush(pool)
            t = clocked(step)
            roots["fill cut"] = world.info()["root"]
            return t

        def brush_edit(i):
            lo, hi = brush_box(i)
            world.checkout(s_terrain)
            world.flush(pool)

            def step():
                world.edit(ort.box_records(lo, hi, 1))
                world.flush(pool)
                roots["edit put"] = world.info()["root"]
                world.edit(ort.box_records(lo, hi, 0))
                world.flush(pool)
            t = clocked(step)
            roots["edit cut"] = world.info()["root"]
            return t

        lo, hi = brush_box(0)
        coords = sample(lo, hi, 1 << 14)
        world.checkout(s_terrain)
        before = world.at(coords)
        st_put = world.fill_box(lo, hi, 1)
        equal = np.array_equal(world.at(coords), at_truth(coords, lo, hi, 1, before)) and stats_equal(st_put, lo, hi)
        st_cut = world.fill_box(lo, hi, 0)
        equal = equal and np.array_equal(world.at(coords), at_truth(coords, lo, hi, 0, before)) and stats_equal(st_cut, lo, hi)
        brush_fill(0), brush_edit(0)
        equal = equal and roots["fill put"] == roots["edit put"] and roots["fill cut"] == roots["edit cut"]
        used_before = world.info()["used"]
        measure("brush", [("fill_box+flush", brush_fill), ("edit+flush", brush_edit)],
                {"equal": bool(equal), "lo": lo.tolist(), "records": 64000, "put": st_put, "cut": st_cut,
                 "each_time_is": "one put + flush and one cut + flush"})
        res["brush"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
        world.checkout(s_terrain)
        res["brush"]["trace_put"] = traced(lambda: world.fill_box(lo, hi, 1))
        res["brush"]["trace_cut"] = traced(lambda: world.fill_box(lo, hi, 0))
        save()

        # ---- an unaligned 256^3 box across the surface
        lo = np.array([c - 131, c - 125, top - 129])
        hi = lo + 256
        ax = [torch.arange(int(l), int(h), dtype=torch.int32, device="cuda") for l, h in zip(lo, hi)]
        z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        records = torch.stack([x, y, z, torch.ones_like(x)], -1).reshape(-1, 4).contiguous()
        del x, y, z
        coords = sample(lo, hi)
        world.checkout(s_terrain)
        before = world.at(coords)
        used = world.info()["used"]
        st = world.fill_box(lo, hi, 1)
        ids_fill = world.info()["used"] - used
        root_fill = world.info()["root"]
        equal = np.array_equal(world.at(coords), at_truth(coords, lo, hi, 1, before)) and stats_equal(st, lo, hi)
        world.checkout(s_terrain)
        used = world.info()["used"]
        world.edit(records)
        equal = equal and world.info()["root"] == root_fill

        def box_fill(i):
            world.checkout(s_terrain)
            return clocked(lambda: world.fill_box(lo, hi, 1))

        def box_edit(i):
            world.checkout(s_terrain)
            return clocked(lambda: world.edit(records))

        measure("box256", [("fill_box", box_fill), ("edit_device", box_edit)],
                {"equal": bool(equal), "lo": lo.tolist(), "records": int(records.shape[0]), "record_bytes": int(records.shape[0]) * 16,
                 "stats": st, "ids_first_fill": ids_fill, "ids_edit_after_fill": world.info()["used"] - used})
        world.checkout(s_terrain)
        res["box256"]["trace"] = traced(lambda: world.fill_box(lo, hi, 1))
        del records
        save()

        # ---- an unaligned 1024^3 box cleared
        lo = np.array([c - 517, c - 509, top - 700])
        hi = lo + 1024
        coords = sample(lo, hi)
        world.checkout(s_terrain)
        before = world.at(coords)
        used = world.info()["used"]
        st = world.fill_box(lo, hi, 0)
        ids_clear = world.info()["used"] - used
        equal = np.array_equal(world.at(coords), at_truth(coords, lo, hi, 0, before)) and stats_equal(st, lo, hi)
        equal = equal and int((before != 0).sum()) > 1000          # the box does hold terrain

        def clear(i):
            world.checkout(s_terrain)
            return clocked(lambda: world.fill_box(lo, hi, 0))

        measure("clear1024", [("fill_box", clear)],
                {"equal": bool(equal), "lo": lo.tolist(), "stats": st, "ids_first_clear": ids_clear,
                 "the_parents_record_list": {"records": 1 << 30, "bytes": 16 << 30}})
        world.checkout(s_terrain)
        res["clear1024"]["trace"] = traced(lambda: world.fill_box(lo, hi, 0))
        save()

        # ---- restore: the brush box back as it was before the stroke
        lo, hi = brush_box(0)
        brush = ort.box_records(lo, hi, 1)
        world.checkout(s_terrain)
        world.edit(brush)
        s_brush = world.snapshot()
        kept = {}

        def restore(i):
            world.checkout(s_brush)
            world.flush(pool)
            t = clocked(lambda: (kept.__setitem__("stats", world.restore_box(s_terrain, lo, hi)), world.flush(pool)))
            kept["root restore"] = world.info()["root"]
            return t

        def paint_back(i):
            world.checkout(s_terrain)
            t1 = clocked(lambda: kept.__setitem__("grid", world.read_box(lo, hi, np.uint32, device=True)))
            world.checkout(s_brush)
            world.flush(pool)

            def undo():
                back = torch.from_numpy(brush.view(np.int32)).cuda()
                back[:, 3] = kept["grid"].reshape(-1)           # box_records and the grid are both x fastest, then y, then z
                world.edit(back)
                world.flush(pool)
            t2 = clocked(undo)
            kept["root paint"] = world.info()["root"]
            return t1 + t2

        restore(0), paint_back(0)
        equal = kept["root restore"] == kept["root paint"] == root_terrain
        used_before = world.info()["used"]
        measure("restore", [("restore_box+flush", restore), ("read_box+edit+flush", paint_back)],
                {"equal": bool(equal), "stats": kept["stats"]})
        res["restore"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
        world.checkout(s_brush)
        res["restore"]["trace"] = traced(lambda: world.restore_box(s_terrain, lo, hi))
        res["world"]["used_at_the_end"] = world.info()["used"]
        save()
    finally:
        pool.close()
        world.close()

    faulthandler.cancel_dump_traceback_later()
    keys = [k for k in res if isinstance(res[k], dict) and "equal" in res[k]]
    ok = all(res[k]["equal"] for k in keys)
    res["all_equal"] = bool(ok)
    save()
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
