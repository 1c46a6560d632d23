"""The random walks of tests/world_sphere_model.py -- every operation of tests/world_model.py with sphere
strokes mixed in -- against a stand-in made of the host paths alone, and the quotas that keep the
walks from being vacuous.

SphereHostWorld is test_world_walk_host.HostWorld plus fill_sphere(), the editor over ort.sphere_records
(a clear of any size: the tree's diff against an empty pool filtered to the ball and applied), and
restore_sphere(), its diff against the snapshot's tree likewise; their stats come from och_sphere_cubes'
counts and, for a restore at depth <= 5, from differing() over the two dense grids.  The quotas are
counted from the model alone, over all seeds of SPHERE_WALKS together; the seeds are chosen so that the
model meets them."""
import collections
import ctypes as C
import time

import numpy as np
import pytest

from test_world_walk_host import HostWorld, base_records
from world_sphere_model import SphereModel, SphereWalk

# (seed, depth, capacity, steps) as test_world_walk_host.WALKS: depths 2 to 6, and one walk at 21
SPHERE_WALKS = [(201, 2, 20, 150), (202, 3, 30, 160), (203, 4, 30, 160), (204, 5, 40, 170), (205, 6, 100, 160),
                (206, 21, 2000, 130)]


def make_model(seed, depth, capacity):
    base = base_records(seed, depth)
    model = SphereModel(depth, base, None)
    if capacity is not None:
        model.capacity = model.used + capacity * depth
    return model, base


class SphereHostWorld(HostWorld):
    def _axis_box(self, c2, d):
        n = 1 << self.depth
        lo = tuple(min(max(-((d + 1 - c) // 2), 0), n) for c in c2)
        hi = tuple(min(max((c + d - 1) // 2 + 1, 0), n) for c in c2)
        return (lo, hi) if all(l < h for l, h in zip(lo, hi)) else ((0, 0, 0), (0, 0, 0))

    def _become_in_ball(self, other, c2, d):
        """Inside the ball the voxels of `other`: its diff against the current tree, filtered to the ball, applied."""
        rec, _ = self.tree.diff(other)
        off = 2 * rec[:, :3].astype(np.int64) + 1 - np.array(c2, np.int64)
        rec = rec[(off * off).sum(1) <= d * d]
        if len(rec):
            self.tree = self.ort.edit_voxels(self.tree, rec, use_gpu=False, threads=int(self.rng.integers(1, 6)))

    def _sphere_counts(self, c2, d):
        cubes, cells, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
        assert self.ort.load().och_sphere_cubes((C.c_int32 * 3)(*c2), d, self.depth, None, None, 0, cubes, cells, C.byref(n)) == 0
        assert sum(cubes) == n.value
        return int(n.value), int(sum(cells))

    def fill_sphere(self, c2, d, id):
        self.strokes += 1
        lo, hi = self._axis_box(c2, d)
        cubes, cells = self._sphere_counts(c2, d)
        if cubes and id:
            self.tree = self.ort.edit_voxels(self.tree, self.ort.sphere_records(c2, d, id), use_gpu=False,
                                             threads=int(self.rng.integers(1, 6)))
        elif cubes:
            self._become_in_ball(self.ort.build_voxels(np.zeros((0, 4), np.uint32), depth=self.depth, use_gpu=False), c2, d)
        return {"cubes": cubes, "cells": cells, "lo": lo, "hi": hi}

    def restore_sphere(self, s, c2, d):
        from test_gpu_world_region import whole_grid
        from test_gpu_world_sphere import differing
        self.strokes += 1
        lo, hi = self._axis_box(c2, d)
        out = {"lo": lo, "hi": hi}
        snap = self._state(s)
        if self.depth <= 5:            # the counts from the two dense grids
            a, b = whole_grid(self.tree), whole_grid(snap)
            cubes, cells = differing(self.depth, c2, d, a, b)
            out.update(cubes=cubes, cells=cells)
        self._become_in_ball(snap, c2, d)
        return out


@pytest.fixture(scope="module")
def tallies():
    return {}


def walk(ort, seed, depth, capacity, steps, tally):
    model, base = make_model(seed, depth, capacity)
    SphereWalk(ort, SphereHostWorld(ort, depth, base, seed), model, seed, tally=tally).run(steps)


@pytest.mark.parametrize("seed,depth,capacity,steps", SPHERE_WALKS)
def test_walk_host(ort, tallies, seed, depth, capacity, steps):
    t0, tallies[seed] = time.perf_counter(), collections.Counter()
    walk(ort, seed, depth, capacity, steps, tallies[seed])
    print(f"walk {seed} depth {depth}: {steps} operations in {time.perf_counter() - t0:.1f} s")


QUOTAS = {"sphere fills with cubes > 0": ("sphere_fill", 20), "sphere clears": ("sphere_clear", 20),
          "sphere restores that change something": ("sphere_restore_change", 20), "no-effect sphere strokes": ("sphere_no_effect", 20),
          "a ball without a voxel in a non-empty axis box": ("sphere_nothing_in_a_box", 1),
          "a restore whose differences all lie outside the ball": ("sphere_restore_untouched", 1),
          "whole-tree sphere fills": ("sphere_whole_fill", 1), "whole-tree sphere clears": ("sphere_whole_clear", 1),
          "whole-tree sphere restores": ("sphere_whole_restore", 1), "refused sphere strokes": ("sphere_refused", 3),
          "sphere strokes directly after a root-changing checkout": ("sphere_after_checkout", 1),
          "a sphere stroke refused, and admitted after the compaction": ("sphere_retry_admitted", 1),
          "a sphere clear refused at used + need == capacity + 1": ("sphere_bound_refused_clear", 1),
          "a sphere clear admitted at used + need == capacity": ("sphere_bound_admitted_clear", 1),
          "a sphere restore refused at used + need == capacity + 1": ("sphere_bound_refused_restore", 1),
          "a sphere restore admitted at used + need == capacity": ("sphere_bound_admitted_restore", 1),
          "box fills among them": ("fill_box", 10), "box restores among them": ("restore_box", 10), "record strokes among them": ("admitted", 60)}


def test_quotas(ort, tallies):
    """The walks meet what they are for.  A seed whose walk has not run in this session is walked here."""
    tally = collections.Counter()
    for seed, depth, capacity, steps in SPHERE_WALKS:
        if seed not in tallies:
            tallies[seed] = collections.Counter()
            walk(ort, seed, depth, capacity, steps, tallies[seed])
        tally.update(tallies[seed])
    print(dict(tally))
    short = {name: (tally[key], least) for name, (key, least) in QUOTAS.items() if tally[key] < least}
    assert not short, short
