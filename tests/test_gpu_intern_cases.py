"""The adversarial interning cases of tests/intern_cases.py on the GPU: probe_node, k_intern_rows and
k_settle (csrc/och_dag.h) with one chain of 300 rows that starts at the table's last slot and wraps
to slot 0, contended by one wavefront and by several in one dispatch, and with an interior row that
spells a leaf-level row's words and lands on its slot.  Expected is the Python pool
(test_voxel_builder.check_pool) and, for a world, `used` of the model (tests/world_model.py).

Every probe loop of the store is bounded by the table size: nothing here can spin."""
import numpy as np
import pytest

import intern_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain():
    return ic.chain_values()[0]


@pytest.fixture(scope="module")
def two_heights():
    found = ic.two_heights_search()
    assert len([c for c in found if c[0] <= 4]) >= 8
    return found


@pytest.mark.parametrize("place", ["adjacent", "threefold"])
def test_chain_builders(ort, gpu_device, chain, place):
    rec = ic.chain_adjacent(chain) if place == "adjacent" else ic.chain_threefold(chain)
    for use_gpu in (True, False):
        ic.run_builders(ort, ic.CHAIN_DEPTH, rec, use_gpu)
    import torch
    tree = ort.build_voxels(torch.from_numpy(rec.view(np.int32)).cuda(), depth=ic.CHAIN_DEPTH, use_gpu=True)
    assert np.array_equal(tree.nodes, ort.build_voxels(rec, depth=ic.CHAIN_DEPTH).nodes)


def test_chain_world(ort, gpu_device, chain):
    ic.run_chain_world(ort, chain)


def test_two_heights_world(ort, gpu_device, two_heights):
    """Each configuration in a world of its capacity: the table the search simulated."""
    for depth, capacity, h, k in two_heights:
        ic.run_two_heights_world(ort, depth, capacity, h, k)


def test_two_heights_builders(ort, gpu_device, two_heights):
    """The builders' store holds min(capacity, depth + 1) ids: the configurations that meet in that table."""
    met = [c for c in two_heights if ic.two_heights_meet(c[0], c[2], c[3], ic.builder_slots(c[0], c[1]))]
    assert len({(d, h, k) for d, _, h, k in met}) >= 8
    for depth, capacity, h, k in two_heights:
        ic.run_two_heights_builders(ort, depth, capacity, h, k, True)
