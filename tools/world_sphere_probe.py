"""A resident world's sphere strokes, measured on one GPU, by §7h's method.

Every timing is a host clock around the whole synchronised step.  Three warm-up runs of every arm,
then the arms alternating in one process; medians, quartiles and extremes of seven runs.  Every arm
is compared with its truth before anything is timed, and the probe stops there, with nothing of
those arms timed or written, if one differs.  What brings the world into the state an arm starts
from (a checkout, a flush) is outside the clock.

Everything runs on the depth-12 terrain world at capacity 2^24.  A ball is (centre2, diameter): twice its
centre in voxels and its diameter in voxels (include/och_gpu.h).

  brush       the diameter-40 ball at the surface, put and cut in turn, dragged three voxels a run; each time
              is one put + flush and one cut + flush:
              fill_sphere+flush     World.fill_sphere(c2, 40, 1 / 0) + flush
              edit+flush            the parent's way: World.edit(sphere_records(...)) from host memory + flush
              fill_box+flush        the ball's axis box (40^3) by World.fill_box: the fixed-cost yardstick
  ball512     the diameter-512 ball across the surface set to id 1:
              fill_sphere           World.fill_sphere
              edit_device           the parent's way: World.edit of its 70 277 000 records from a device tensor
  clear2047   the diameter-2047 ball cleared: fill_sphere alone.  The parent's way would need a list of
              4.4e9 records (71 GB), which is recorded in place of a time.
  restore     the brush ball put back as it was before the stroke:
              restore_sphere+flush  World.restore_sphere(snapshot, ball) + flush
              read_box+edit+flush   read_box (device) of the ball's axis box before the stroke, the ball's
                                    old voxels as records, edit and flush; both parts are in the time
  The truth: the two arms of a pair must leave the same root id (one store: equal ids are equal content),
  World.at over a sample of voxels in and around the ball must give the id inside (the inequality itself,
  in numpy int64) and the terrain's voxels outside, and the stats must equal ort.sphere_cubes' totals.

Also recorded: each sphere stroke's OCH_BUILD_TRACE phase lines, its stats and the ids it consumed.

python tools/world_sphere_probe.py [--out profiles/world_sphere/probe.json] [--reps 7] [--arms brush,ball512]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--out", default="profiles/world_sphere/probe.json")
    ap.add_argument("--arms", default="brush,ball512,clear2047,restore", help="the groups of arms to run, comma-separated")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_sphere_probe: no GPU visible (there is nothing to measure without one)")

    def watchdog():
        faulthandler.cancel_dump_traceback_later()
        faulthandler.dump_traceback_later(a.limit, exit=True)

    watchdog()
    torch.cuda.set_device(0)
    depth, dim = a.depth, 1 << a.depth
    groups = set(a.arms.split(","))
    if not groups <= {"brush", "ball512", "clear2047", "restore"}:
        raise SystemExit(f"world_sphere_probe: --arms names brush, ball512, clear2047 and restore, not {a.arms!r}")
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
            raise SystemExit(f"world_sphere_probe: {name}: an arm differs from its truth; nothing timed")
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
    rng = np.random.default_rng(22)

    def in_ball(coords, c2, d):
        off = 2 * coords.astype(np.int64) + 1 - np.asarray(c2, np.int64)
        return (off * off).sum(1) <= d * d

    def sample(c2, d, n=1 << 16):
        """Coordinates in and around the ball: n in its axis box grown by 8 voxels, n near its surface."""
        lo, hi = (np.asarray(c2) - d) // 2 - 8, (np.asarray(c2) + d) // 2 + 9
        box = rng.integers(lo, hi, (n, 3))
        v = rng.normal(size=(n, 3))
        shell = np.asarray(c2) / 2 + v / np.linalg.norm(v, axis=1)[:, None] * (d / 2 + rng.uniform(-2, 2, (n, 1)))
        return np.concatenate([box, np.floor(shell).astype(np.int64)]).astype(np.int32)

    def at_truth(coords, c2, d, id, before):
        return np.where(in_ball(coords, c2, d), np.uint32(id), before)

    def counts(c2, d):
        cubes, cells, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
        ort._lib.call("och_sphere_cubes", (C.c_int32 * 3)(*c2), d, depth, None, None, 0, cubes, cells, C.byref(n))
        return int(n.value), int(sum(cells))

    def stats_equal(st, c2, d):
        return (st["cubes"], st["cells"]) == counts(c2, d)

    try:
        s_terrain = world.snapshot()
        root_terrain = world.info()["root"]
        res["world"] = {"depth": depth, "capacity": capacity, "used": world.info()["used"], "pool_nodes": terrain.n_nodes}

        # ---- brush: put and cut in turn, dragged
        def brush_ball(i):
            return (2 * (c + 3 * i), 2 * c, 2 * top), 40

        def axis_box(c2, d):
            return tuple((v - d) // 2 for v in c2), tuple((v + d - 1) // 2 + 1 for v in c2)

        roots = {}

        def put_and_cut(name, put, cut):
            def run(i):
                world.checkout(s_terrain)
                world.flush(pool)

                def step():
                    put(i)
                    world.flush(pool)
                    roots[name + " put"] = world.info()["root"]
                    cut(i)
                    world.flush(pool)
                t = clocked(step)
                roots[name + " cut"] = world.info()["root"]
                return t
            return run

        brush_fill = put_and_cut("fill", lambda i: world.fill_sphere(*brush_ball(i), 1), lambda i: world.fill_sphere(*brush_ball(i), 0))
        brush_edit = put_and_cut("edit", lambda i: world.edit(ort.sphere_records(*brush_ball(i), 1)),
                                 lambda i: world.edit(ort.sphere_records(*brush_ball(i), 0)))
        brush_box = put_and_cut("box", lambda i: world.fill_box(*axis_box(*brush_ball(i)), 1),
                                lambda i: world.fill_box(*axis_box(*brush_ball(i)), 0))

        if "brush" in groups:
            c2, d = brush_ball(0)
            coords = sample(c2, d, 1 << 14)
            world.checkout(s_terrain)
            before = world.at(coords)
            st_put = world.fill_sphere(c2, d, 1)
            equal = np.array_equal(world.at(coords), at_truth(coords, c2, d, 1, before)) and stats_equal(st_put, c2, d)
            st_cut = world.fill_sphere(c2, d, 0)
            equal = equal and np.array_equal(world.at(coords), at_truth(coords, c2, d, 0, before)) and stats_equal(st_cut, c2, d)
            brush_fill(0), brush_edit(0)
            equal = equal and roots["fill put"] == roots["edit put"] and roots["fill cut"] == roots["edit cut"]
            used_before = world.info()["used"]
            measure("brush", [("fill_sphere+flush", brush_fill), ("edit+flush", brush_edit), ("fill_box+flush", brush_box)],
                    {"equal": bool(equal), "centre2": list(c2), "diameter": d, "records": len(ort.sphere_records(c2, d, 1)),
                     "put": st_put, "cut": st_cut, "each_time_is": "one put + flush and one cut + flush"})
            res["brush"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
            world.checkout(s_terrain)
            res["brush"]["trace_put"] = traced(lambda: world.fill_sphere(c2, d, 1))
            res["brush"]["trace_cut"] = traced(lambda: world.fill_sphere(c2, d, 0))
            world.checkout(s_terrain)
            res["brush"]["trace_edit_put"] = traced(lambda: world.edit(ort.sphere_records(c2, d, 1)))
            save()

        # ---- the diameter-512 ball across the surface
        if "ball512" in groups:
            c2, d = (2 * c, 2 * c, 2 * top), 512
            lo, hi = axis_box(c2, d)
            ax = [torch.arange(int(l), int(h), dtype=torch.int64, device="cuda") for l, h in zip(lo, hi)]
            off = [(2 * v + 1 - m) ** 2 for v, m in zip(ax, c2)]
            inside = (off[2][:, None, None] + off[1][None, :, None] + off[0][None, None, :]) <= d * d
            z, y, x = torch.nonzero(inside, as_tuple=True)
            del inside
            records = torch.stack([x + lo[0], y + lo[1], z + lo[2], torch.ones_like(x)], -1).to(torch.int32).contiguous()
            del x, y, z
            coords = sample(c2, d)
            world.checkout(s_terrain)
            before = world.at(coords)
            used = world.info()["used"]
            st = world.fill_sphere(c2, d, 1)
            ids_fill = world.info()["used"] - used
            root_fill = world.info()["root"]
            equal = np.array_equal(world.at(coords), at_truth(coords, c2, d, 1, before)) and stats_equal(st, c2, d)
            world.checkout(s_terrain)
            used = world.info()["used"]
            world.edit(records)
            equal = equal and world.info()["root"] == root_fill

            def ball_fill(i):
                world.checkout(s_terrain)
                return clocked(lambda: world.fill_sphere(c2, d, 1))

            def ball_edit(i):
                world.checkout(s_terrain)
                return clocked(lambda: world.edit(records))

            measure("ball512", [("fill_sphere", ball_fill), ("edit_device", ball_edit)],
                    {"equal": bool(equal), "centre2": list(c2), "diameter": d, "records": int(records.shape[0]),
                     "record_bytes": int(records.shape[0]) * 16, "stats": st, "ids_first_fill": ids_fill,
                     "ids_edit_after_fill": world.info()["used"] - used})
            world.checkout(s_terrain)
            res["ball512"]["trace"] = traced(lambda: world.fill_sphere(c2, d, 1))
            del records
            save()

        # ---- the diameter-2047 ball cleared
        if "clear2047" in groups:
            c2, d = (2 * c, 2 * c, 2 * top), 2047
            coords = sample(c2, d)
            world.checkout(s_terrain)
            before = world.at(coords)
            used = world.info()["used"]
            st = world.fill_sphere(c2, d, 0)
            ids_clear = world.info()["used"] - used
            equal = np.array_equal(world.at(coords), at_truth(coords, c2, d, 0, before)) and stats_equal(st, c2, d)
            equal = equal and int((before != 0).sum()) > 1000          # the ball does hold terrain

            def clear(i):
                world.checkout(s_terrain)
                return clocked(lambda: world.fill_sphere(c2, d, 0))

            measure("clear2047", [("fill_sphere", clear)],
                    {"equal": bool(equal), "centre2": list(c2), "diameter": d, "stats": st, "ids_first_clear": ids_clear,
                     "the_parents_record_list": {"records": 4_400_000_000, "bytes": 71_000_000_000}})
            world.checkout(s_terrain)
            res["clear2047"]["trace"] = traced(lambda: world.fill_sphere(c2, d, 0))
            save()

        # ---- restore: the brush ball back as it was before the stroke
        if "restore" in groups:
            c2, d = brush_ball(0)
            lo, hi = axis_box(c2, d)
            brush = ort.sphere_records(c2, d, 1)
            world.checkout(s_terrain)
            world.edit(brush)
            s_brush = world.snapshot()
            kept = {}
            at = torch.from_numpy(brush[:, :3].astype(np.int64) - np.asarray(lo, np.int64)).cuda()

            def restore(i):
                world.checkout(s_brush)
                world.flush(pool)
                t = clocked(lambda: (kept.__setitem__("stats", world.restore_sphere(s_terrain, c2, d)), world.flush(pool)))
                kept["root restore"] = world.info()["root"]
                return t

            def paint_back(i):
                world.checkout(s_terrain)
                t1 = clocked(lambda: kept.__setitem__("grid", world.read_box(lo, hi, np.uint32, device=True)))
                world.checkout(s_brush)
                world.flush(pool)

                def undo():
                    back = torch.from_numpy(brush.view(np.int32)).cuda()
                    back[:, 3] = kept["grid"][at[:, 2], at[:, 1], at[:, 0]]     # the grid is indexed [z, y, x]
                    world.edit(back)
                    world.flush(pool)
                t2 = clocked(undo)
                kept["root paint"] = world.info()["root"]
                return t1 + t2

            restore(0), paint_back(0)
            equal = kept["root restore"] == kept["root paint"] == root_terrain
            used_before = world.info()["used"]
            measure("restore", [("restore_sphere+flush", restore), ("read_box+edit+flush", paint_back)],
                    {"equal": bool(equal), "stats": kept["stats"]})
            res["restore"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
            world.checkout(s_brush)
            res["restore"]["trace"] = traced(lambda: world.restore_sphere(s_terrain, c2, d))
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
