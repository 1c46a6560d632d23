"""Reading a resident world back, measured on one GPU, by §7e's method.

Every timing is a host clock around the whole synchronised step.  Three warm-up runs of every arm,
then the arms alternating in one process; medians, quartiles and extremes of seven runs.  Every arm
is compared with its baseline arm before anything is timed, and the probe stops there, with nothing
of those arms timed or written, if one differs.

Everything runs on the depth-12 terrain world at capacity 2^24, after one 40^3 brush stroke.

  at          n = 1, 64 and 2^20 coordinates (random ones inside the tree, the same for both arms):
              download+pool_at  the parent's only way: World.download(), then och_pool_at per
                                coordinate (called from Python: the per-call cost of ctypes is in it)
              world_at          World.at on host coordinates
              world_at_dev      World.at on a device tensor
  read_box    the 40^3 brush box and a 256^3 box at the surface:
              download+read_box World.download(), then NodePool.read_box (uint8)
              world_read_dev    World.read_box(device=True)
              world_read_host   World.read_box into host memory
              with the share of the box's aligned 4x4x4 bricks that hold no voxel: those wavefronts
              end during the shared descent
  tighten     first           the first call on a fresh world (made outside the clock)
              after_stroke    a call after one brush stroke (put and cut in turn, outside the clock;
                              these strokes make no new ids after the first pair)
              after_moving_stroke  a call after a stroke of the brush dragged (7, 5, 0) voxels, its id
                              changing: new ids every time
              after_compact   a call after compact() (outside the clock)
              render          och_gpu_last_kernel_ms of the two-view 1920x1080 frame of a world whose
                              top 64 layers were cut, before and after the tighten, alternating
                              between two pools of one world

Also recorded: each step's OCH_BUILD_TRACE phase lines from one further run.

python tools/world_read_probe.py [--out profiles/world_read/probe.json] [--reps 7]
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
    ap.add_argument("--out", default="profiles/world_read/probe.json")
    a = ap.parse_args()

    import torch
    import octree_ray_tracing_amd as ort

    if not torch.cuda.is_available():
        raise SystemExit("world_read_probe: no GPU visible (there is nothing to measure without one)")

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
        """arms: (key, run) pairs; run(i) does step i and returns its seconds.  Nothing is timed, and
        nothing of these arms is written, unless the arms equalled their baseline (facts["equal"])."""
        if not facts.get("equal", facts.get("frames_equal")):
            raise SystemExit(f"world_read_probe: {name}: an arm differs from its baseline; nothing timed")
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
        save()

    # ---- the depth-12 terrain, the brush at its surface, the world after one stroke
    terrain = ort.build_terrain(depth, use_gpu=True)
    c = dim // 2
    top = max(z for z in range(dim) if terrain.at(c, c, z))
    lo = np.array([c - 20, c - 20, top - 20])
    strokes = [ort.box_records(lo, lo + 40, 1), ort.box_records(lo, lo + 40, 0)]
    capacity = 1 << 24
    world = ort.World(terrain, capacity=capacity, device=0)
    world.edit(strokes[0])
    res["world"] = {"depth": depth, "capacity": capacity, "used": world.info()["used"], "pool_nodes": terrain.n_nodes,
                    "brush_lo": lo.tolist()}
    lib_at = ort.load().och_pool_at

    try:
        # ---- at
        rng = np.random.default_rng(12)
        for n in (1, 64, 1 << 20):
            coords = rng.integers(0, dim, (n, 3)).astype(np.int32)
            coords[:, 2] = rng.integers(max(0, top - 200), min(dim, top + 56), n)       # around the surface: hits and misses
            dev_coords = torch.from_numpy(coords).cuda()
            rows = coords.tolist()
            got = {}

            def baseline(i):
                def step():
                    tree = world.download()
                    p, r, d, b = tree.nodes.ctypes.data, tree.root, tree.depth, tree.index_base
                    got["base"] = [lib_at(p, r, d, b, x, y, z) for x, y, z in rows]
                return clocked(step)

            def world_at(i):
                return clocked(lambda: got.__setitem__("host", world.at(coords)))

            def world_at_dev(i):
                def step():
                    got["dev"] = world.at(dev_coords)          # complete on return
                return clocked(step)

            baseline(0), world_at(0), world_at_dev(0)
            want = np.array(got["base"], np.uint32)
            equal = bool(np.array_equal(got["host"], want) and
                         np.array_equal(got["dev"].cpu().numpy().view(np.uint32), want))
            measure(f"at_{n}", [("download+pool_at", baseline), ("world_at", world_at), ("world_at_dev", world_at_dev)],
                    {"n": n, "hits": int((want != 0).sum()), "equal": equal})
            if n == 1 << 20:
                res[f"at_{n}"]["world_at_trace"] = traced(lambda: world.at(coords))
                res[f"at_{n}"]["download_trace"] = traced(world.download)

        # ---- read_box
        boxes = {"brush_40": (lo, lo + 40), "surface_256": (np.array([c - 128, c - 128, top - 128]),
                                                            np.array([c + 128, c + 128, top + 128]))}
        for name, (blo, bhi) in boxes.items():
            got = {}

            def baseline(i):
                return clocked(lambda: got.__setitem__("base", world.download().read_box(blo, bhi, np.uint8)))

            def read_dev(i):
                return clocked(lambda: got.__setitem__("dev", world.read_box(blo, bhi, np.uint8, device=True)))

            def read_host(i):
                return clocked(lambda: got.__setitem__("host", world.read_box(blo, bhi, np.uint8)))

            baseline(0), read_dev(0), read_host(0)
            equal = bool(np.array_equal(got["dev"].cpu().numpy(), got["base"]) and np.array_equal(got["host"], got["base"]))
            # the box's aligned bricks (both boxes lie inside the tree): a brick without a voxel ends its wavefront early
            b0, b1 = blo // 4 * 4, -(-bhi // 4) * 4
            whole = world.read_box(b0, b1, np.uint8)
            nb = [(int(b1[k]) - int(b0[k])) // 4 for k in (2, 1, 0)]
            solid = whole.reshape(nb[0], 4, nb[1], 4, nb[2], 4).any(axis=(1, 3, 5))
            measure(f"read_box_{name}", [("download+read_box", baseline), ("world_read_dev", read_dev),
                                         ("world_read_host", read_host)],
                    {"lo": blo.tolist(), "hi": bhi.tolist(), "dtype": "uint8", "equal": equal,
                     "voxels": int((got["base"] != 0).sum()), "bricks": int(solid.size),
                     "bricks_ending_early": int(solid.size - solid.sum()),
                     "share_ending_early": round(float(1 - solid.mean()), 4)})
            res[f"read_box_{name}"]["world_read_dev_trace"] = traced(lambda: world.read_box(blo, bhi, np.uint8, device=True))

        # ---- tighten
        def exact(w):
            t = w.download()
            return ort.occupied_box(t.nodes, t.root, t.depth)

        fresh = {}

        def first(i):
            with ort.World(terrain, capacity=capacity, device=0) as w:
                s = clocked(lambda: fresh.__setitem__("box", w.tighten()))
            if "trace" not in fresh:
                with ort.World(terrain, capacity=capacity, device=0) as w:
                    fresh["trace"] = traced(w.tighten)
            return s

        def after_stroke(i):
            world.edit(strokes[(i + 1) % 2])
            used = world.info()["used"]
            s = clocked(world.tighten)
            fresh.setdefault("ids", []).append(used - fresh.get("boxed", 1))   # the ids the call visited
            fresh["boxed"] = used
            return s

        # put and cut in turn find every row they make in the store (§7e): no new ids, the call is the root's
        # box alone.  The brush dragged (7, 5, 0) voxels a stroke, its id changing, interns new nodes every time.
        moved = []

        def after_moving_stroke(i):
            off = np.array([7 * (i + 1), 5 * (i + 1), 0])
            world.edit(ort.box_records(lo + off, lo + 40 + off, 1 + i % 5))
            used = world.info()["used"]
            s = clocked(world.tighten)
            moved.append(used - fresh["boxed"])
            fresh["boxed"] = used
            return s

        first(0)
        world.tighten()                                        # the strokes' calls are all incremental
        fresh["boxed"] = world.info()["used"]
        equal = fresh["box"] == ort.occupied_box(terrain.nodes, terrain.root, depth)
        for arm in (after_stroke, after_moving_stroke):        # each arm once, untimed, against the download's box
            arm(-1)
            info = world.info()
            equal = equal and (info["box_lo"], info["box_hi"]) == exact(world)
        fresh["ids"].clear()
        moved.clear()
        measure("tighten", [("first", first), ("after_stroke", after_stroke), ("after_moving_stroke", after_moving_stroke)],
                {"equal": bool(equal), "box": [list(v) for v in fresh["box"]], "first_trace": fresh["trace"],
                 "ids_used": world.info()["used"]})
        res["tighten"]["after_stroke_new_ids"] = fresh["ids"][a.warmup:]
        res["tighten"]["after_moving_stroke_new_ids"] = moved[a.warmup:]
        res["tighten"]["after_stroke_equal"] = bool(world.tighten() == exact(world))
        res["tighten"]["after_stroke_trace"] = traced(lambda: (world.edit(strokes[0]), world.tighten()))

        def after_compact(i):
            world.compact()
            return clocked(world.tighten)

        ids_before = world.info()["used"]
        world.compact()
        equal = bool(world.tighten() == exact(world))
        measure("tighten_after_compact", [("after_compact", after_compact)],
                {"equal": equal, "ids_used": ids_before, "ids_used_after": world.info()["used"]})
    finally:
        world.close()
    save()

    # ---- the render before and after tightening a world whose top 64 layers were cut
    watchdog()
    try:
        top_all = ort.occupied_box(terrain.nodes, terrain.root, depth)[1][2]
        # a layer is 2^24 records: four strokes of a quarter layer each (2^22 records), 256 strokes in all
        strip = torch.from_numpy(ort.box_records((0, 0, 0), (dim, dim // 4, 1), 0).view(np.int32)).cuda()
        y0 = strip[:, 1].clone()
        with ort.World(terrain, capacity=capacity, device=0) as w:
            t0 = time.perf_counter()
            for z in range(top_all - 64, top_all):
                for q in range(4):
                    strip[:, 1] = y0 + q * (dim // 4)
                    strip[:, 2] = z
                    try:
                        w.edit(strip)
                    except ort.OchError as e:
                        if e.status != -6:
                            raise
                        w.compact()
                        w.edit(strip)
            cut_s = time.perf_counter() - t0
            with w.make_pool() as loose, w.make_pool() as tight:
                before = w.info()
                box = w.tighten()
                w.flush(tight)                                 # `loose` keeps the superset it was made with
                cams = [ort.camera((1.5, 1.5, 1.5), 0.3, p, 1.25, 1920, 1080) for p in (0.0, -0.6)]
                frames = {k: torch.zeros((2, 1080, 1920), dtype=torch.int32, device="cuda") for k in ("loose", "tight")}
                for p in (loose, tight):
                    p.set_palette(ort.VoxelData().get_colours())

                def render(key, p):
                    def run(i):
                        p.render_views_dev(cams, frames[key])
                        p.synchronize()
                        return p.last_kernel_ms() / 1e3
                    return run

                render("loose", loose)(0), render("tight", tight)(0)
                equal = bool(torch.equal(frames["loose"], frames["tight"]))
                measure("render_after_cut", [("loose_box", render("loose", loose)), ("tight_box", render("tight", tight))],
                        {"layers_cut": 64, "cut_seconds": round(cut_s, 2), "box_before": [list(before["box_lo"]), list(before["box_hi"])],
                         "box_after": [list(v) for v in box], "frames_equal": equal,
                         "times": "och_gpu_last_kernel_ms of the two-view 1920x1080 launch"})
    except Exception as e:                                     # the cut is 64 strokes of 2^24 records: say so if it does not fit
        res["render_after_cut"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps({"render_after_cut": res["render_after_cut"]}), flush=True)

    faulthandler.cancel_dump_traceback_later()
    keys = [k for k in res if isinstance(res[k], dict) and "equal" in res[k]]
    ok = all(res[k]["equal"] for k in keys) and res.get("render_after_cut", {}).get("frames_equal", True)
    res["all_equal"] = bool(ok)
    save()
    print(f"wrote {outp}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
