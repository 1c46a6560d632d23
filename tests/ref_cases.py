"""Trees and rays that pin the oracle and the kernels to the reference's own
tracers (oracle/_ref/ref_trace: ORT/och_h_octree.h:292-447 and
ORT/och_octree.cpp:167-320 compiled where they lie).

One generator, shared by tests/test_oracle_pins.py (oracle vs the binary, live
and from fixtures), tests/test_gpu_reference.py (kernels vs both) and
tests/make_golden.py (which records the binary's answers into
tests/golden/ref_trace_*.npz).  Everything is a pure function of the case's
name; inputs are finite (the reference need not terminate on NaN or inf).

Every ray of every case is compared: direction, voxel and the bit pattern of
t, misses included (+inf for h_octree, 0.0 for octree).
"""
from __future__ import annotations

import zlib

import numpy as np

from make_golden import edge_rays

LOG2_TABLE_CAPACITY = 19            # h_octree<19, D>, as oracle/ref_trace.cpp instantiates it

# (kind, depth): "h" = och::h_octree (DAG, 1-based, miss t = +inf),
#                "o" = och::octree (pointer tree, 0-based, miss t = 0.0)
CASES = [("h", 2), ("h", 3), ("h", 6), ("h", 8), ("h", 12), ("h", 16),
         ("o", 2), ("o", 3), ("o", 6), ("o", 8)]
O_CAPACITY = {2: 16, 3: 96, 6: 8192, 8: 32768}
DENORMAL = np.float32(1e-40)


def case_name(kind, depth):
    return f"{kind}{depth}"


def fixture_name(kind, depth):
    return f"ref_trace_{kind}{depth}.npz"


def _rng(kind, depth, what):
    return np.random.default_rng(zlib.crc32(f"{kind}{depth}:{what}".encode()))


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _voxel_id(xyz):
    return (1 + xyz.sum(axis=1) % 4).astype(np.uint32)


def _random_voxels(rng, depth):
    """Uniformly random voxels, and at the deeper levels blobs of them so
    that rays meet something (a uniform 2500 of 2^24 cells would not)."""
    dim = 1 << depth
    if depth <= 3:
        n = (dim ** 3) * 3 // 10
        return rng.integers(0, dim, (n, 3))
    n_uniform, n_blobs, per_blob = (1000, 25, 40) if depth == 6 else (600, 45, 40)
    parts = [rng.integers(0, dim, (n_uniform, 3))]
    for c in rng.integers(4, dim - 4, (n_blobs, 3)):
        parts.append(np.clip(c + rng.integers(-3, 4, (per_blob, 3)), 0, dim - 1))
    return np.concatenate(parts)


def _centre_clusters(rng, depth):
    """tests/test_gpu_parity.py::test_deep_sparse_trees' tree: clusters of
    voxels 2^k away from the cube's centre, k = 2 .. depth - 2."""
    c = 1 << (depth - 1)
    vox = []
    for k in range(2, depth - 1):
        base = c + rng.integers(-(1 << k), 1 << k, 3)
        vox.append(np.clip(base + rng.integers(-2, 3, (40, 3)), 0, (1 << depth) - 1))
    return np.concatenate(vox)


def tree_ops(kind, depth):
    """uint32 (n, 4) records x, y, z, v in the order the reference applies
    them.  "h": set(x, y, z, v), v == 0 removing a voxel (path copies leave
    gravestones in the hash table).  "o": v != 0 is set, v == 0 is unset."""
    rng = _rng(kind, depth, "tree")
    xyz = _centre_clusters(rng, depth) if depth >= 12 else _random_voxels(rng, depth)
    first = np.column_stack([xyz, _voxel_id(xyz)])
    dim = 1 << depth
    # set / unset / set again: every voxel of one octant of the cube goes (an
    # emptied subtree: its nodes return to octree's free list, h_octree's
    # become gravestones), then every other remaining voxel, then some come
    # back (with another id) into the freed slots.
    in_octant = np.all(xyz < dim // 2, axis=1)
    gone = xyz[in_octant]
    rest = xyz[~in_octant]
    gone = np.concatenate([gone, rest[::2]])
    back = gone[rng.random(len(gone)) < 0.35]
    ops = np.concatenate([
        first,
        np.column_stack([gone, np.zeros(len(gone), np.int64)]),
        np.column_stack([back, 1 + (_voxel_id(back) % 4)]),
    ])
    return np.ascontiguousarray(ops, np.uint32)


def final_voxels(ops):
    """{(x, y, z): v} after the ops, removed voxels dropped."""
    cells = {}
    for x, y, z, v in ops.tolist():
        if v:
            cells[(x, y, z)] = v
        else:
            cells.pop((x, y, z), None)
    return cells


def rays(kind, depth, ops):
    """(origins, dirs, aimed): float32 (n, 3) each and a boolean mask of the
    rays aimed at voxel centres and corners.  Categories:
      a  random origins in the cube, random unit directions
      b  a stride of make_golden.edge_rays() (every direction, every origin row)
      c  one and two direction components +0.0, -0.0, denormal
      d  axis-aligned directions
      e  unnormalised directions scaled by 1e-20 .. 1e20
      f  origins snapped to cell faces of every level of the tree
      g  origins on and just past the cube's faces (0.9 .. 2.1, 2.0000768, 1.0, 2.0)
      h  rays aimed at voxel centres and corners (grid origins: exact ties)
    """
    rng = _rng(kind, depth, "rays")
    dim = 1 << depth
    O, D = [], []

    def add(o, d):
        O.append(np.asarray(o, np.float64).reshape(-1, 3))
        D.append(np.asarray(d, np.float64).reshape(-1, 3))

    def rnd_o(n):
        return rng.uniform(1.0, 2.0, (n, 3))

    def rnd_d(n):
        return _unit(rng.uniform(-1, 1, (n, 3)))

    # a
    add(rnd_o(700), rnd_d(700))
    # b: stride 5 is coprime to the 18 directions and to the 4 z origins
    eo, ed = edge_rays()
    sel = np.arange((CASES.index((kind, depth))) % 5, len(eo), 5)
    add(eo[sel], ed[sel])
    # c
    special = np.array([0.0, -0.0, DENORMAL, -DENORMAL], np.float64)
    n = 640
    d = rnd_d(n)
    o = rnd_o(n)
    o[::3] = rng.choice([1.25, 1.5, 1.75, 1.125], (len(o[::3]), 3))
    for i in range(n):
        axes = rng.permutation(3)[: 1 + i % 2]
        d[i, axes] = rng.choice(special, len(axes))
    add(o, d)
    # d
    axis_d = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
    n = 360
    o = rnd_o(n)
    o[::2] = 1.0 + rng.integers(0, dim + 1, (len(o[::2]), 3)) / dim
    d = axis_d[np.arange(n) % 6].copy()
    d[n // 2:] = np.where(d[n // 2:] == 0, rng.choice([0.0, -0.0], (n - n // 2, 3)), d[n // 2:])
    add(o, d)
    # e
    n = 440
    scale = rng.choice(np.array([1e-20, 1e-12, 1e-5, 3.0, 1e7, 1e20]), (n, 1))
    add(rnd_o(n), rnd_d(n) * scale)
    # f
    n = 640
    o = rnd_o(n)
    lvl = 1 + np.arange(n) % depth
    for i in range(n):
        axes = rng.permutation(3)[: 1 + i % 3]
        o[i, axes] = 1.0 + rng.integers(0, (1 << lvl[i]) + 1, len(axes)) / (1 << lvl[i])
    d = rnd_d(n)
    d[::5] = axis_d[rng.integers(0, 6, len(d[::5]))]
    d[1::5] = _unit(rng.choice([-1.0, 1.0], (len(d[1::5]), 3)))          # diagonals: tx == ty == tz
    add(o, d)
    # g
    n = 640
    o = rng.uniform(0.9, 2.1, (n, 3))
    o[:120, rng.integers(0, 3)] = np.float32(2.0000768)
    face = rng.choice([1.0, 2.0], 120)
    o[120:240] = rnd_o(120)
    o[np.arange(120, 240), rng.integers(0, 3, 120)] = face
    add(o, rnd_d(n))
    # h
    cells = np.array(list(final_voxels(ops)), np.float64)
    n = 840
    tgt = cells[rng.integers(0, len(cells), n)]
    tgt = tgt + np.where(rng.random((n, 1)) < 0.5, 0.5, rng.integers(0, 2, (n, 3)))
    o = np.tile(1.5, (n, 3))
    o[n // 2:] = rng.uniform(1.25, 1.75, (n - n // 2, 3))
    o[n // 2::4] = 1.0 + rng.integers(0, dim + 1, (len(o[n // 2::4]), 3)) / dim
    d = (1.0 + tgt / dim) - o
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1), [[0.6, 0.0, -0.8]])
    d[::7] = (1.0 + tgt[::7] / dim) - o[::7]                               # some left unnormalised
    n_before = sum(len(x) for x in O)
    add(o, d)

    o = np.ascontiguousarray(np.concatenate(O), np.float32)
    d = np.ascontiguousarray(np.concatenate(D), np.float32)
    zero = ~np.any(d != 0, axis=1)
    d[zero] = np.float32([0.6, 0.0, -0.8])
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(d))
    aimed = np.zeros(len(o), bool)
    aimed[n_before:] = True
    return o, d, aimed


def case(kind, depth):
    ops = tree_ops(kind, depth)
    o, d, aimed = rays(kind, depth, ops)
    return {"kind": kind, "depth": depth, "ops": ops, "o": o, "d": d, "aimed": aimed,
            "capacity": O_CAPACITY[depth] if kind == "o" else None}


def oracle_tree(O, kind, depth, ops, capacity=None):
    """The oracle's restatement of the reference's tree after the same ops:
    (HRef | ORef, tail) with tail = root (h) or node_cnt (o)."""
    if kind == "h":
        T = O.HRef(depth, LOG2_TABLE_CAPACITY)
        for x, y, z, v in ops.tolist():
            T.set(x, y, z, v)
        return T, T.root
    T = O.ORef(depth, capacity)
    for x, y, z, v in ops.tolist():
        if v:
            T.set(x, y, z, v)
        else:
            T.unset(x, y, z)
    return T, T.node_cnt


def records_differ(a, b):
    """Indices of rays whose (direction, voxel, t bits) differ."""
    return np.nonzero((np.asarray(a["dir"]) != np.asarray(b["dir"]))
                      | (np.asarray(a["voxel"]).view(np.uint32) != np.asarray(b["voxel"]).view(np.uint32))
                      | (np.asarray(a["t"]).view(np.uint32) != np.asarray(b["t"]).view(np.uint32)))[0]


def describe(c, i, **records):
    """One mismatching ray with its tree and each named record, for a report."""
    rec = {k: (int(r["dir"][i]), int(np.asarray(r["voxel"]).view(np.uint32)[i]),
               hex(int(np.asarray(r["t"]).view(np.uint32)[i]))) for k, r in records.items()}
    return (f"tree {case_name(c['kind'], c['depth'])} ray {int(i)}: o={c['o'][i].view(np.uint32)} "
            f"({c['o'][i]}) d={c['d'][i].view(np.uint32)} ({c['d'][i]}) {rec}")
