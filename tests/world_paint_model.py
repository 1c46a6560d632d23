"""What a conditional stroke (och_world_paint_box, och_world_paint_sphere) counts, from a dense grid
and include/och_gpu.h's definitions alone: paint_counts gives (cubes, cells, nodes, T).

A cube of height h is open when the stroke can touch it: always for h >= 1 and content, otherwise (an
empty cube, a voxel) iff pred(word).  cells counts the straddling open cells from the root cell down,
cubes the open cubes inside the shape whose parent straddles (or the tree itself), nodes the distinct
non-empty subtrees of height >= 1 at or below a counted cube -- hash-consed by (height, content bytes),
as the DAG shares them -- and T the greatest height of a counted cube when pred(0) and id != 0.
Nothing here knows of the store or of the code under test."""
import numpy as np

WHEN_IS, WHEN_IS_NOT = 0, 1


def pred(when, match, v):
    return (int(v) == int(match)) != bool(when)


def box_classifier(lo, hi):
    """classify(o, H) of the box lo <= (x, y, z) < hi: 0 outside, 1 straddling, 2 inside."""
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    nothing = any(h <= l for l, h in zip(lo, hi))

    def classify(o, H):
        if nothing:
            return 0
        inside, outside = True, False
        for a in range(3):
            c, e = o[a], o[a] + (1 << H)
            inside = inside and lo[a] <= c and e <= hi[a]
            outside = outside or c >= hi[a] or e <= lo[a]
        return 0 if outside else 2 if inside else 1
    return classify


def ball_classifier(c2, d):
    from test_sphere_cubes_host import classify
    c2, d = tuple(int(v) for v in c2), int(d)
    return lambda o, H: classify(c2, d, o, H)


def paint_counts(grid, classify, when, match, id):
    """(cubes, cells, nodes, T) of the stroke on a dense [z, y, x] grid of side 2^depth."""
    d = paint_detail(grid, classify, when, match, id)
    return d["cubes"], d["cells"], sum(d["nodes_per_height"]), d["T"]


def paint_detail(grid, classify, when, match, id):
    """paint_counts' numbers by name, with the cubes and the distinct nodes N_h per height (index h)."""
    grid = np.ascontiguousarray(grid, np.uint32)
    depth = int(grid.shape[0]).bit_length() - 1
    assert grid.shape == (1 << depth,) * 3
    out = {"cubes": 0, "cells": 0, "top": 0, "cubes_per_height": [0] * (depth + 1)}
    seen = set()

    def block(o, H):
        s = 1 << H
        return grid[o[2]:o[2] + s, o[1]:o[1] + s, o[0]:o[0] + s]

    def children(o, H):
        s = 1 << (H - 1)
        return [(o[0] + (k & 1) * s, o[1] + ((k >> 1) & 1) * s, o[2] + ((k >> 2) & 1) * s) for k in range(8)]

    def add_node(o, H):
        b = block(o, H)
        if not b.any():
            return
        key = (H, b.tobytes())
        if key in seen:
            return
        seen.add(key)
        if H > 1:
            for c in children(o, H):
                add_node(c, H - 1)

    def visit(o, H):
        c = classify(o, H)
        if not c:
            return
        b = block(o, H)
        if not ((H >= 1 and b.any()) or pred(when, match, b.flat[0] if H == 0 else 0)):
            return
        if c == 2:
            out["cubes"] += 1
            out["top"] = max(out["top"], H)
            out["cubes_per_height"][H] += 1
            if H >= 1:
                add_node(o, H)
            return
        assert H > 0, "a voxel never straddles"
        out["cells"] += 1
        for k in children(o, H):
            visit(k, H - 1)

    visit((0, 0, 0), depth)
    out["T"] = out["top"] if pred(when, match, 0) and id and out["cubes"] else 0
    out["nodes_per_height"] = [sum(1 for h, _ in seen if h == H) for H in range(depth + 1)]
    return out


def painted(grid, mask, when, match, id):
    """The grid after the stroke: inside the mask pred(v) ? id : v."""
    grid = np.asarray(grid, np.uint32)
    hit = ((grid == np.uint32(match)) != bool(when)) & mask
    return np.where(hit, np.uint32(id), grid).astype(np.uint32)
