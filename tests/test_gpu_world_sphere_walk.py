"""ort.World walked through the random operation lists of tests/world_sphere_model.py -- every operation
of tests/world_model.py with sphere strokes (World.fill_sphere, World.restore_sphere) mixed in -- every
answer compared with the model bit for bit: the whole stats dict, `used`, the loose box and every
refusal.  The seeds, depths and capacities are those of tests/test_world_sphere_walk_host.py, which
proves the same lists against the host paths and asserts their quotas."""
import time

import pytest

from test_world_sphere_walk_host import SPHERE_WALKS, make_model
from world_sphere_model import SphereWalk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,depth,capacity,steps", SPHERE_WALKS)
def test_walk(ort, O, gpu_device, seed, depth, capacity, steps):
    model, base = make_model(seed, depth, capacity)
    tree = ort.build_voxels(base, depth=depth)
    t0 = time.perf_counter()
    with ort.World(tree, capacity=None if capacity is None else model.capacity) as world:
        SphereWalk(ort, world, model, seed, O=O, on_gpu=True).run(steps)
    print(f"walk {seed} depth {depth}: {steps} operations in {time.perf_counter() - t0:.1f} s")
