"""The adversarial interning cases of tests/intern_cases.py on the CPU: the numpy twin of
csrc/och_hash.h's node_hash against a program compiled from that header (so the cases can never
silently stop colliding), the searches, and both cases through the host builders.

The host NodeStore shares the hash and the table rule with the device store, and CHAIN meets them
here: without the wrap of its probe the host build reads past its table.  TWO HEIGHTS does not
reach the host store's height term: NodeStore::intern sends a leaf-level row whose words are all
below 8 through its direct leaf map, and here v = h <= 5, so the leaf row never enters the hash
table and the height-h row cannot meet it.  On the host that case checks the result only; the height
term that is covered is the device store's (probe_node), by tests/test_gpu_intern_cases.py."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import intern_cases as ic

CSRC = Path(__file__).resolve().parents[1] / "octree_ray_tracing_amd" / "csrc"

# n, then n lines of "h c0 .. c7" -> n lines of the hash
DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <iostream>
#include "och_hash.h"
int main()
{
    size_t n;
    std::cin >> n;
    for (size_t i = 0; i < n; ++i) {
        int h;
        uint32_t c[8];
        std::cin >> h;
        for (auto &w : c) std::cin >> w;
        printf("%llu\n", (unsigned long long)och_hash::node_hash(c, h));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def chain():
    return ic.chain_values()


@pytest.fixture(scope="module")
def two_heights():
    return ic.two_heights_search()


@pytest.fixture(scope="module")
def compiled_hash(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("intern_cases_host")
    src, exe = tmp / "hash.cpp", tmp / "hash"
    src.write_text(DRIVER)
    run = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]

    def hashes(rows, heights):
        lines = [f"{len(rows)}"] + [f"{h} " + " ".join(str(int(w)) for w in row) for row, h in zip(rows, heights)]
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-3000:]
        return np.array([int(v) for v in out.stdout.split()], np.uint64)
    return hashes


def test_twin_equals_the_compiled_header(compiled_hash, chain, two_heights):
    rng = np.random.default_rng(2026)
    rows = rng.integers(0, 1 << 32, (1000, 8), dtype=np.uint64).astype(np.uint32)
    rows[::7, 1:] = 0                                        # leaf rows of one voxel, as the cases'
    heights = rng.integers(0, 21, 1000)
    heights[:21] = np.arange(21)
    chain_rows = np.zeros((len(chain[0]), 8), np.uint32)
    chain_rows[:, 0] = chain[0]
    pairs = [(row, j) for d, _, h, k in two_heights for j, row in enumerate(ic.two_heights_rows(d, h, k))]
    rows = np.concatenate([rows, chain_rows, np.array([p[0] for p in pairs], np.uint32)])
    heights = np.concatenate([heights, np.zeros(len(chain_rows), np.int64), np.array([p[1] for p in pairs])])
    got = compiled_hash(rows, heights)
    assert got.shape == (len(rows),) and np.array_equal(got, ic.node_hash(rows, heights))
    assert (got[1000:1000 + len(chain_rows)] & np.uint64(ic.CHAIN_BITS) == np.uint64(ic.CHAIN_BITS)).all()


def test_chain_is_one_chain(chain):
    values, seconds = chain
    print(f"CHAIN: {len(values)} rows below v = {int(values[-1])} in {seconds:.2f} s")
    assert len(values) == ic.CHAIN_ROWS == len(set(values.tolist())) and values.min() >= 8
    for slots in (1024, 16384):
        table = ic.Table(slots)
        for n, v in enumerate(values.tolist()):
            id, visited = table.intern([v, 0, 0, 0, 0, 0, 0, 0], 0)
            # every row starts at the last slot and wraps to slot 0: row n walks n + 1 slots
            assert id == n + 1 and visited == [slots - 1] + list(range(n))


def test_two_heights_search(two_heights):
    small = [c for c in two_heights if c[0] <= 4]
    print(f"TWO HEIGHTS: {len(two_heights)} configurations, {len(small)} with depth <= 4: {small}")
    assert len(small) >= 8 and (2, 3, 1, 1) in small
    assert ic.two_heights_record(2, 1, 1).tolist() == [[3, 0, 0, 1]]
    for depth, capacity, h, k in two_heights:
        rows = ic.two_heights_rows(depth, h, k)
        assert rows[h] == rows[0]
        # what the term decides: a table that compared the words alone hands back id 1 at height h
        blind = ic.Table(ic.table_size(capacity), respect_height=False)
        assert [blind.intern(row, j)[0] for j, row in enumerate(rows)][h] == 1


@pytest.mark.parametrize("threads", [1, 5])
@pytest.mark.parametrize("place", ["adjacent", "threefold"])
def test_chain_host_builders(ort, chain, place, threads):
    rec = ic.chain_adjacent(chain[0]) if place == "adjacent" else ic.chain_threefold(chain[0])
    assert len(np.unique(rec[:, :3] >> 1, axis=0)) == len(rec) == (300 if place == "adjacent" else 900)
    ic.run_builders(ort, ic.CHAIN_DEPTH, rec, False, threads)


@pytest.mark.parametrize("threads", [1, 5])
def test_two_heights_host_builders(ort, two_heights, threads):
    for depth, capacity, h, k in two_heights:
        ic.run_two_heights_builders(ort, depth, capacity, h, k, False, threads)
