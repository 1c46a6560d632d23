"""One fixed, seeded list of world calls with the library OCH_GPU_LIB names (or the tree's own); everything that is
content and not a store id goes, per case, into the JSON file argv[1].  `--compare a.json b.json out.json` compares two.

Cases: every entry of tests/test_voxel_builder.CASES as the three GPU world test files stroke it (a base of the first third,
three strokes), a depth-12 terrain world with the 40^3 brush and 2^20 random records, and the refusals the GPU tests
provoke through arguments.  Root ids are claim-ordered and left out; `used`, handles, boxes, statuses, texts and SHA-256 of
every byte array are in."""
import ctypes as C
import hashlib
import json
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]


def sha(a):
    if a is None:
        return "none"
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compare(a, b, out):
    A, B = json.load(open(a)), json.load(open(b))
    differ = [k for k in sorted(set(A) | set(B)) if A.get(k) != B.get(k)]
    refused = sum(1 for k, v in A.items() for s in v if isinstance(s, dict) and "refused" in s)
    res = {"cases": len(A), "steps": sum(len(v) for v in A.values()), "refusals": refused, "differ": differ}
    json.dump({"summary": res, "parent": A, "new": B}, open(out, "w"), indent=1)
    print(json.dumps(res))
    return 1 if differ else 0


def main():
    if sys.argv[1] == "--compare":
        return compare(*sys.argv[2:5])
    import torch
    import octree_ray_tracing_amd as ort
    from test_gpu_world import CAPACITY_BASE, CAPACITY_EDIT, SECOND, roomy, thirds
    from test_voxel_builder import CASES
    from voxel_build_probe import traced

    torch.cuda.set_device(0)
    lib = ort.load()
    out = {}

    def state(world, what):
        i = world.info()
        return {"step": what, **{k: i[k] for k in ("capacity", "used", "depth", "strokes", "generation", "box_lo", "box_hi")},
                "has_root": bool(i["root"]), "snapshots": world.snapshots()}

    def content(world, coords, lo, hi):
        t = world.download()
        ids = world.at(coords)
        dev = world.at(torch.from_numpy(coords).cuda())
        g32 = world.read_box(lo, hi, np.uint32)
        gdev = world.read_box(lo, hi, np.uint32, device=True)
        return {"download": sha(t.nodes), "n_nodes": int(t.n_nodes), "root": int(t.root), "at": sha(ids), "at_device": sha(dev.cpu().numpy()),
                "read_box": sha(g32), "read_box_device": sha(gdev.cpu().numpy()), "solid": int(np.count_nonzero(g32))}

    def diffs(world, a, b):
        rec, st = world.diff(a, b)
        dev, dst = world.diff(a, b, device=True)
        _, sst = world.diff(a, b, records=False)
        return {"step": f"diff {a} {b}", "records": sha(rec), "device": sha(dev.cpu().numpy()), "stats": [st, dst, sst]}

    def refused(what, fn):
        try:
            r = fn()
            return {"refused": what, "status": r if isinstance(r, int) else 0, "text": lib.och_last_error().decode() if isinstance(r, int) and r else ""}
        except (ort.OchError, ValueError) as e:
            return {"refused": what, "status": getattr(e, "status", "ValueError"), "text": str(e)}

    # ---- the test files' cases
    for name, (depth, rec) in sorted(CASES.items()):
        first, strokes = thirds(rec)
        base = ort.build_voxels(first, depth=depth)
        dim = 1 << depth
        rng = np.random.default_rng(len(name))
        coords = np.concatenate([rec[:, :3].astype(np.int32), rng.integers(-2, dim + 2, (2048, 3)).astype(np.int32)])
        c = np.minimum(rec[0, :3].astype(np.int64), dim - 8) if len(rec) else np.zeros(3, np.int64)
        lo, hi = ((0, 0, 0), (dim,) * 3) if depth <= 7 else (tuple(int(v) - 24 for v in c), tuple(int(v) + 40 for v in c))
        steps = []
        with ort.World(base, capacity=roomy(base, strokes + [strokes[2], first], depth)) as world, world.make_pool() as pool:
            snaps = [world.snapshot()]
            steps += [state(world, "create"), content(world, coords, lo, hi)]
            for k, s in enumerate(strokes):
                world.edit(torch.from_numpy(s.view(np.int32)).cuda() if k == 1 and s.dtype == np.uint32 else s)
                world.flush(pool)
                snaps.append(world.snapshot())
                steps += [state(world, f"stroke {k}"), content(world, coords, lo, hi), {"pool_root": bool(pool.info()["root"])}]
            steps += [diffs(world, snaps[0], snaps[3]), diffs(world, snaps[3], snaps[1]), diffs(world, snaps[2], 0), diffs(world, 0, 0)]
            box = world.tighten()
            steps += [{"tighten": box}, state(world, "tighten")]
            world.checkout(snaps[1])
            world.flush(pool)
            steps += [state(world, "checkout 1"), content(world, coords, lo, hi)]
            world.edit(strokes[2])                                   # a branch off snapshot 1
            steps += [state(world, "branch"), content(world, coords, lo, hi), diffs(world, snaps[3], 0)]
            world.compact()                                          # snapshots live
            world.flush(pool)
            steps += [state(world, "compact, snapshots live"), content(world, coords, lo, hi), diffs(world, snaps[0], snaps[3])]
            world.tighten()
            steps += [state(world, "tighten after compact")]
            world.checkout(snaps[3])
            for s in snaps:
                world.release(s)
            world.compact()                                          # none live
            world.flush(pool)
            steps += [state(world, "compact, none live"), content(world, coords, lo, hi)]
            world.edit(first * np.array([1, 1, 1, 0], np.uint32))
            steps += [state(world, "base removed"), content(world, coords, lo, hi)]
        out[name] = steps

    # ---- the depth-12 terrain, the 40^3 brush, 2^20 random records
    depth, dim = 12, 1 << 12
    terrain = ort.build_terrain(depth, use_gpu=True)
    cc = dim // 2
    top = max(z for z in range(dim) if terrain.at(cc, cc, z))
    lo = np.array([cc - 20, cc - 20, top - 20])
    brush = ort.box_records(lo, lo + 40, 1)
    rng = np.random.default_rng(20)
    scatter = np.empty((1 << 20, 4), np.uint32)
    scatter[:, :3] = rng.integers(0, dim, (1 << 20, 3))
    scatter[:, 3] = rng.integers(1, 6, 1 << 20)
    coords = np.concatenate([brush[::7, :3], scatter[::64, :3]]).astype(np.int32)
    blo, bhi = tuple(int(v) - 4 for v in lo), tuple(int(v) + 44 for v in lo)
    steps, traces = [], {}
    with ort.World(terrain, capacity=1 << 24, device=0) as world, world.make_pool() as pool:
        s0 = world.snapshot()
        steps += [state(world, "create"), content(world, coords, blo, bhi)]
        traces["stroke"] = traced(lambda: world.edit(brush))
        world.flush(pool)
        s1 = world.snapshot()
        steps += [state(world, "brush"), content(world, coords, blo, bhi)]
        world.edit(scatter)
        world.flush(pool)
        s2 = world.snapshot()
        steps += [state(world, "scatter"), content(world, coords, blo, bhi), diffs(world, s0, s1), diffs(world, s1, s2), diffs(world, s2, s0)]
        traces["diff"] = traced(lambda: world.diff(s0, s1, device=True))
        traces["tighten"] = traced(world.tighten)
        steps += [state(world, "tighten")]
        world.edit(brush * np.array([1, 1, 1, 0], np.uint32))
        world.tighten()
        steps += [state(world, "brush cut, tighten"), content(world, coords, blo, bhi)]
        traces["compact_history"] = traced(world.compact)
        world.flush(pool)
        steps += [state(world, "compact, snapshots live"), content(world, coords, blo, bhi), diffs(world, s0, 0)]
        world.checkout(s1)
        for s in (s0, s1, s2):
            world.release(s)
        traces["compact"] = traced(world.compact)
        world.flush(pool)
        steps += [state(world, "compact, none live"), content(world, coords, blo, bhi)]
    mask = lambda lines: [re.sub(r"\d+\.\d+ s$", "#.# s", ln) for ln in lines]
    out["terrain_12"] = steps + [{"trace": k, "lines": mask(v)} for k, v in sorted(traces.items())]

    # ---- refusals through arguments
    steps = []
    base = ort.build_voxels(CAPACITY_BASE)
    steps.append(refused("capacity 3", lambda: ort.World(base, capacity=3)))
    with ort.World(base, capacity=9) as world, ort.World(base) as other, world.make_pool() as pool:
        world.edit(CAPACITY_EDIT)
        steps += [refused("edit past capacity", lambda: world.edit(SECOND)), state(world, "after the refused stroke")]
        with ort.HOctree(base.nodes, base.root, base.depth, device=0) as foreign, other.make_pool() as theirs:
            steps += [refused("flush foreign", lambda: world.flush(foreign)), refused("flush theirs", lambda: world.flush(theirs))]
        steps.append(refused("flush NULL pool", lambda: lib.och_world_flush(world._h, None)))
        s = world.snapshot()
        for what, fn in (("checkout 99", lambda: world.checkout(99)), ("release 0", lambda: world.release(0)),
                         ("release 99", lambda: world.release(99)), ("diff 99 0", lambda: world.diff(99, 0)),
                         ("diff 0 99", lambda: world.diff(0, 99))):
            steps.append(refused(what, fn))
        world.compact()
        world.edit(SECOND)
        n = world.diff(s, 0)[1]["n"]
        st = ort._lib.DiffStats()
        host = np.full((n, 4), 0x5A5A5A5A, np.uint32)
        steps.append(refused("diff short buffer", lambda: lib.och_world_diff(world._h, s, 0, host.ctypes.data, n - 1, 0, C.byref(st))))
        steps.append({"stats": [int(st.n), int(st.pairs), list(st.box_lo), list(st.box_hi)], "untouched": bool((host == 0x5A5A5A5A).all())})
        steps.append(refused("diff NULL stats", lambda: lib.och_world_diff(world._h, s, 0, None, 0, 0, None)))
        other.edit(np.array([[1, 1, 1, 300]], np.uint32))
        steps.append(refused("u8 grid, id 300", lambda: other.read_box((0, 0, 0), (8, 8, 8), np.uint8)))
        steps.append(refused("u8 grid, id 300, device", lambda: other.read_box((0, 0, 0), (8, 8, 8), np.uint8, device=True)))
        one = np.zeros(1, np.uint8)
        vec = lambda *v: np.array(v, np.int32).ctypes.data_as(C.c_void_p)
        steps.append(refused("read_box short grid", lambda: lib.och_world_read_box(world._h, vec(0, 0, 0), vec(8, 8, 8), 1, one.ctypes.data, 1, 0)))
        steps.append(refused("read_box NULL grid", lambda: lib.och_world_read_box(world._h, vec(0, 0, 0), vec(8, 8, 8), 1, None, 1 << 16, 0)))
        steps.append(refused("read_box hi < lo", lambda: lib.och_world_read_box(world._h, vec(4, 4, 4), vec(3, 9, 9), 1, one.ctypes.data, 1, 0)))
        steps.append({"empty box": list(world.read_box((4, 4, 4), (9, 4, 9)).shape), "at none": int(len(world.at(np.zeros((0, 3), np.int32))))})
        steps.append(refused("at int64", lambda: world.at(torch.zeros((5, 3), dtype=torch.int64, device="cuda"))))
        steps.append(refused("edit 2^31", lambda: lib.och_world_edit(world._h, host.ctypes.data, 1 << 31, 0)))
        steps.append(refused("at NULL ids", lambda: lib.och_world_at(world._h, host.ctypes.data, 1, None, 0)))
        for _ in range(ort._lib.WORLD_MAX_SNAPSHOTS - len(world.snapshots())):
            world.snapshot()
        steps += [refused("snapshot 65537", world.snapshot), state(world, "end")["used"]]
    out["refusals"] = steps

    json.dump(out, open(sys.argv[1], "w"), indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    print("world_cmp:", len(out), "cases,", sum(len(v) for v in out.values()), "steps ->", sys.argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
