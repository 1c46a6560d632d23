"""A resident world's conditional strokes, measured on one GPU, by §7h's method.

Every timing is a host clock around the whole synchronised step.  Three warm-up runs of every arm,
then the arms alternating in one process; medians, quartiles and extremes of seven runs.  Every arm
is compared with its truth before anything is timed, and the probe stops there, with nothing of
those arms timed or written, if one differs.  What brings the world into the state an arm starts
from (a checkout, a flush) is outside the clock.

Everything runs on the depth-12 terrain world at capacity 2^24.  `new` is an id the terrain does not hold.

  brush       the diameter-40 ball at the surface, its solid voxels painted `new`, dragged three voxels a run:
              paint_sphere+flush    World.paint_sphere(c2, 40, new) + flush
              read+edit+flush       the parent's way: read_box(device=True) of the ball's axis box, the mask
                                    (the ball's inequality and grid != 0) and the records in torch, World.edit
                                    of them + flush; all of it inside the clock
  box256      an unaligned 256^3 box across the surface, (WHEN_IS_NOT, 0, new):
              paint_box             World.paint_box
              read+edit             the parent's way from device tensors, as above, without the flush
  under1024   (WHEN_IS, 0, new) over an unaligned 1024^3 box: paint_box alone.  The parent's way would need
              one record per empty voxel of the box; their number is recorded in place of a time.
  replace     (WHEN_IS, m, new) for the terrain's most common id m over the whole tree, on a world of its own:
              the stroke's worst case, every node of the DAG is mapped; nodes and new_ids beside the time.
  The truth: the two arms of a pair must leave the same root id (one store: equal ids are equal content), and
  World.at over a sample of voxels in and around the shape must give pred(before) ? new : before.

Also recorded: each stroke's OCH_BUILD_TRACE phase lines, its stats and the ids it consumed.

python tools/world_paint_probe.py [--out profiles/world_paint/probe.json] [--reps 7]
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
    ap.add_argument("--out", default="profiles/world_paint/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_paint_probe: no GPU visible (there is nothing to measure without one)")

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
            raise SystemExit(f"world_paint_probe: {name}: an arm differs from its truth; nothing timed")
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
    common = int(np.argmax(np.asarray(terrain.voxel_hist[1:8])) + 1)
    new = 200
    IS, IS_NOT = ort.WHEN_IS, ort.WHEN_IS_NOT
    rng = np.random.default_rng(23)

    def pred(when, match, v):
        return (v == np.uint32(match)) != bool(when)

    def in_ball(coords, c2, d):
        off = 2 * coords.astype(np.int64) + 1 - np.asarray(c2, np.int64)
        return (off * off).sum(1) <= d * d

    def in_box(coords, lo, hi):
        return ((coords >= np.asarray(lo)) & (coords < np.asarray(hi))).all(1)

    def sample(lo, hi, n=1 << 16):
        """Coordinates in and around a box: n in it grown by 8 voxels, n within 3 voxels of its faces."""
        lo, hi = np.asarray(lo), np.asarray(hi)
        box = rng.integers(lo - 8, hi + 8, (n, 3))
        face = rng.integers(lo - 3, hi + 3, (n, 3))
        axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
        face[np.arange(n), axis] = np.where(side, hi[axis], lo[axis]) + rng.integers(-3, 3, n)
        return np.concatenate([box, face]).astype(np.int32)

    def ball_box(c2, d):
        return tuple((v - d) // 2 for v in c2), tuple((v + d - 1) // 2 + 1 for v in c2)

    def parents_way(world, lo, hi, when, match, id, ball=None):
        """What a caller without the stroke does: the box as a device grid, a mask, the records, an edit."""
        grid = world.read_box(lo, hi, np.uint32, device=True)
        hit = (grid == match) if when == IS else (grid != match)
        if ball is not None:
            ax = [torch.arange(int(l), int(h), dtype=torch.int64, device="cuda") for l, h in zip(lo, hi)]
            off = [(2 * v + 1 - m) ** 2 for v, m in zip(ax, ball[0])]
            hit &= (off[2][:, None, None] + off[1][None, :, None] + off[0][None, None, :]) <= ball[1] * ball[1]
        z, y, x = torch.nonzero(hit, as_tuple=True)
        records = torch.stack([x + lo[0], y + lo[1], z + lo[2], torch.full_like(x, id)], -1).to(torch.int32).contiguous()
        world.edit(records)
        return int(records.shape[0])

    world = ort.World(terrain, capacity=capacity, device=0)
    pool = world.make_pool()
    try:
        s_terrain = world.snapshot()
        res["world"] = {"depth": depth, "capacity": capacity, "used": world.info()["used"], "pool_nodes": terrain.n_nodes,
                        "most_common_id": common, "painted_id": new}
        kept = {}

        # ---- brush: the solid voxels of the diameter-40 ball, dragged
        def brush_ball(i):
            return (2 * (c + 3 * i), 2 * c, 2 * top), 40

        def brush_paint(i):
            world.checkout(s_terrain)
            world.flush(pool)
            t = clocked(lambda: (kept.__setitem__("st", world.paint_sphere(*brush_ball(i), new)), world.flush(pool)))
            kept["root paint"] = world.info()["root"]
            return t

        def brush_parent(i):
            world.checkout(s_terrain)
            world.flush(pool)
            ball = brush_ball(i)
            t = clocked(lambda: (kept.__setitem__("n", parents_way(world, *ball_box(*ball), IS_NOT, 0, new, ball)), world.flush(pool)))
            kept["root parent"] = world.info()["root"]
            return t

        c2, d = brush_ball(0)
        lo, hi = ball_box(c2, d)
        coords = sample(lo, hi, 1 << 14)
        world.checkout(s_terrain)
        before = world.at(coords)
        brush_paint(0)
        want = np.where(in_ball(coords, c2, d) & pred(IS_NOT, 0, before), np.uint32(new), before)
        equal = np.array_equal(world.at(coords), want) and int((want != before).sum()) > 100
        brush_parent(0)
        equal = equal and kept["root paint"] == kept["root parent"]
        used_before = world.info()["used"]
        measure("brush", [("paint_sphere+flush", brush_paint), ("read+edit+flush", brush_parent)],
                {"equal": bool(equal), "centre2": list(c2), "diameter": d, "when": "IS_NOT", "match": 0, "stats": kept["st"],
                 "records_of_the_parents_way": kept["n"]})
        res["brush"]["ids_added_by_the_arms"] = world.info()["used"] - used_before
        world.checkout(s_terrain)
        res["brush"]["trace"] = traced(lambda: world.paint_sphere(c2, d, new))
        save()

        # ---- box256: an unaligned 256^3 box across the surface
        lo = (c - 128 + 3, c - 128 + 5, top - 128 + 7)
        hi = tuple(v + 256 for v in lo)

        def box_paint(i):
            world.checkout(s_terrain)
            t = clocked(lambda: kept.__setitem__("st", world.paint_box(lo, hi, new)))
            kept["root paint"] = world.info()["root"]
            return t

        def box_parent(i):
            world.checkout(s_terrain)
            t = clocked(lambda: kept.__setitem__("n", parents_way(world, lo, hi, IS_NOT, 0, new)))
            kept["root parent"] = world.info()["root"]
            return t

        coords = sample(lo, hi)
        world.checkout(s_terrain)
        before = world.at(coords)
        used = world.info()["used"]
        box_paint(0)
        ids_first = world.info()["used"] - used
        want = np.where(in_box(coords, lo, hi) & pred(IS_NOT, 0, before), np.uint32(new), before)
        equal = np.array_equal(world.at(coords), want) and int((want != before).sum()) > 1000
        box_parent(0)
        equal = equal and kept["root paint"] == kept["root parent"]
        measure("box256", [("paint_box", box_paint), ("read+edit", box_parent)],
                {"equal": bool(equal), "lo": list(lo), "hi": list(hi), "when": "IS_NOT", "match": 0, "stats": kept["st"],
                 "ids_first_paint": ids_first, "records_of_the_parents_way": kept["n"], "record_bytes": kept["n"] * 16})
        world.checkout(s_terrain)
        res["box256"]["trace"] = traced(lambda: world.paint_box(lo, hi, new))
        save()

        # ---- under1024: fill under an unaligned 1024^3 box
        lo = (c - 512 + 3, c - 512 + 5, top - 512 + 7)
        hi = tuple(v + 1024 for v in lo)
        world.checkout(s_terrain)
        empty = 0
        for z in range(lo[2], hi[2], 128):                     # the parent's record list: one record per empty voxel
            slab = world.read_box((lo[0], lo[1], z), (hi[0], hi[1], min(z + 128, hi[2])), np.uint8, device=True)
            empty += int((slab == 0).sum())
            del slab
        coords = sample(lo, hi)
        before = world.at(coords)
        used = world.info()["used"]
        st = world.paint_box(lo, hi, new, IS, 0)
        ids_first = world.info()["used"] - used
        want = np.where(in_box(coords, lo, hi) & pred(IS, 0, before), np.uint32(new), before)
        equal = np.array_equal(world.at(coords), want) and int((want != before).sum()) > 1000

        def under(i):
            world.checkout(s_terrain)
            return clocked(lambda: world.paint_box(lo, hi, new, IS, 0))

        measure("under1024", [("paint_box", under)],
                {"equal": bool(equal), "lo": list(lo), "hi": list(hi), "when": "IS", "match": 0, "stats": st, "ids_first_paint": ids_first,
                 "the_parents_record_list": {"records": empty, "bytes": empty * 16}})
        world.checkout(s_terrain)
        res["under1024"]["trace"] = traced(lambda: world.paint_box(lo, hi, new, IS, 0))
        res["world"]["used_at_the_end"] = world.info()["used"]
        save()
    finally:
        pool.close()
        world.close()

    # ---- replace: the most common material over the whole tree, on a world of its own
    world = ort.World(terrain, capacity=capacity, device=0)
    try:
        s_terrain = world.snapshot()
        coords = rng.integers(0, dim, (1 << 17, 3)).astype(np.int32)
        coords[:, 2] = rng.integers(max(top - 300, 0), min(top + 40, dim), len(coords))
        before = world.at(coords)
        used = world.info()["used"]
        st = world.paint_box((0, 0, 0), (dim, dim, dim), new, IS, common)
        ids_first = world.info()["used"] - used
        want = np.where(pred(IS, common, before), np.uint32(new), before)
        equal = np.array_equal(world.at(coords), want) and int((want != before).sum()) > 1000 and (st["cubes"], st["cells"]) == (1, 0)

        def replace(i):
            world.checkout(s_terrain)
            return clocked(lambda: world.paint_box((0, 0, 0), (dim, dim, dim), new, IS, common))

        measure("replace", [("paint_box", replace)],
                {"equal": bool(equal), "when": "IS", "match": common, "stats": st, "nodes": st["nodes"], "new_ids_first_paint": ids_first,
                 "used_before": used})
        world.checkout(s_terrain)
        res["replace"]["trace"] = traced(lambda: world.paint_box((0, 0, 0), (dim, dim, dim), new, IS, common))
        res["replace"]["used_at_the_end"] = world.info()["used"]
        save()
    finally:
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
