"""GPU parity with the reference itself: the gfx950 kernels against the records
of the reference's own tracers (oracle/_ref/ref_trace: ORT/och_h_octree.h and
ORT/och_octree.cpp compiled where they lie), bit for bit, no ray excluded.

Two sources of the expectation, neither of them the oracle:
  * tests/golden/ref_trace_*.npz, what the binary answered on the recording
    host, with that host's RCPPS table uploaded to the pool;
  * the binary run on this host (where oracle/_ref/ was built), against the
    pool's default table, which is this host's.  Only the binary is read, never
    the reference tree.
The trees are uploaded in the reference's own table layout (HRef.nodes() with
its gravestones, ORef.nodes() with its free list), which tests/test_oracle_pins.py
ties to the reference by get_root() / get_node_cnt() and by the same records.
The oracle appears only in a failure's report, beside the other two records."""
import numpy as np
import pytest

import ref_cases as RC
from conftest import GOLD
from test_gpu_parity import gpu_trace_dev

pytestmark = pytest.mark.gpu

REF_CASES = [pytest.param(k, d, id=RC.case_name(k, d)) for k, d in RC.CASES]
N_SINGLE = 36                       # rays also sent through the single-ray sse_trace entry


def _fixture(kind, depth):
    g = np.load(GOLD / RC.fixture_name(kind, depth))
    return {"kind": kind, "depth": depth, "ops": g["ops"], "o": g["o"], "d": g["d"],
            "capacity": int(g["capacity"]) or None, "lut": g["lut"], "tail": int(g["tail"]),
            "ref": {"dir": g["dir"].astype(np.int32), "voxel": g["vox"], "t": g["t"].view(np.float32)}}


def _upload(ort, O, c):
    """The reference-layout table of the case's tree, as a pool on device 0."""
    T, tail = RC.oracle_tree(O, c["kind"], c["depth"], c["ops"], c["capacity"])
    if c["kind"] == "h":
        return T, ort.HOctree(T.nodes(), T.root, c["depth"], device=0)
    return T, ort.Octree(T.nodes(), c["depth"], device=0)


def _assert_kernel(O, c, T, rcp, ref, got, what):
    bad = RC.records_differ(ref, got)
    if bad.size:
        ora = O.trace_batch(T.pool(), rcp, c["o"], c["d"])
        pytest.fail(f"{what}: {bad.size} of {len(c['o'])} records differ; " +
                    "; ".join(RC.describe(c, i, reference=ref, oracle=ora, kernel=got) for i in bad[:3]))


@pytest.mark.parametrize("kind,depth", REF_CASES)
def test_kernels_match_reference_fixture(ort, O, gpu_device, kind, depth):
    c = _fixture(kind, depth)
    T, pool = _upload(ort, O, c)
    pool.set_rcp_lut(c["lut"])
    ref = c["ref"]
    for layout in (0, 1):
        pool.set_option("layout", layout)
        got = gpu_trace_dev(pool, c["o"], c["d"], want_push=False)
        _assert_kernel(O, c, T, O.Rcp(c["lut"]), ref, got, f"layout {layout}")
    for i in np.linspace(0, len(c["o"]) - 1, N_SINGLE).astype(int):
        d, v, t = pool.sse_trace(*c["o"][i].tolist(), *c["d"][i].tolist())
        got = (int(d), int(v), int(np.float32(t).view(np.uint32)))
        want = (int(ref["dir"][i]), int(ref["voxel"][i]), int(ref["t"][i].view(np.uint32)))
        assert got == want, RC.describe(c, i, reference=ref) + f" single-ray kernel {got}"
    pool.close()


@pytest.mark.parametrize("kind,depth", REF_CASES)
def test_kernels_match_live_reference(ort, O, gpu_device, kind, depth):
    if not O.ref_trace_available():
        pytest.skip("oracle/_ref/ref_trace not built (no reference tree where this tree was built)")
    c = _fixture(kind, depth)
    ref = O.ref_trace(kind, depth, c["ops"], c["o"], c["d"], c["capacity"])
    T, pool = _upload(ort, O, c)
    assert (T.root if kind == "h" else T.node_cnt) == ref["tail"]
    for layout in (0, 1):
        pool.set_option("layout", layout)
        got = gpu_trace_dev(pool, c["o"], c["d"], want_push=False)
        _assert_kernel(O, c, T, O.Rcp(None), ref, got, f"layout {layout}, this host's RCPPS")
    pool.close()
