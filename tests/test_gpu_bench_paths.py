"""bench.py's multi-GPU launch paths on the one-GPU box, end to end.

* `--launch group --gpus 1`: the one-process device group (och_frame_group_*:
  ncclCommInitAll, one issuing thread per device, RCCL all-gather, shade),
  its last frames checked against the oracle inside the bench line;
* the N > 1 per-process path as two gloo ranks sharing the GPU (the
  driver's 8-GPU form rehearsed at world size 2): the one-frame exchange
  check before the timed window, parity of rank 0's frames against the
  oracle, and scaling_base -- rank 0 alone rendering the same frame the
  N = 1 way, whose frames must equal the sharded run's.
Depth 10 keeps both runs short; the code paths are the depth-12 ones."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SMALL = ["--full", "--depth", "10", "--steps", "5", "--warmup", "2", "--sustain", "0", "--no-bounce", "--no-cull-off",
         "--no-cpu-baseline", "--no-other-configs", "--moving-steps", "0"]


def _line(stdout: str) -> dict:
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "OCH_DIST_BACKEND")}


@pytest.mark.gpu
def test_bench_group_launch_one_device_matches_oracle():
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--launch", "group", *SMALL],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _line(p.stdout)
    assert line["n_gpus"] == 1 and "och_frame_group" in line["config"]["launch"]
    assert line["parity"]["mismatches"] == 0 and line["parity"]["pixels"] == 2 * 1920 * 1080
    assert line["parity"]["devices_equal_rank0"] is True
    assert line["value"] > 0


@pytest.mark.gpu
def test_bench_two_gloo_ranks_exchange_check_and_scaling_base():
    env = dict(_env(), OCH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(29600 + os.getpid() % 300), str(ROOT / "bench.py"), "--gpus", "2",
           "--width", "960", "--height", "544", *SMALL]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _line(p.stdout)
    assert line["n_gpus"] == 2
    assert line["exchange_check"]["mismatches"] == 0 and line["exchange_check"]["slices"] == 2
    assert "gloo" in line["config"]["exchange"] and "rehearsal" in line["config"]["workload"]
    assert line["parity"]["mismatches"] == 0 and line["parity"]["pixels"] == 2 * 960 * 544
    base = line["scaling_base"]
    assert base["frames_equal_sharded"] is True and base["value"] > 0 and base["frames_in_flight"] == 3


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_last_frames(tmp_path, ort, O):
    """A plain run (no --full): the headline fields, every side measurement
    null, and --dump-outputs writes the last timed step's frames -- here small
    enough to be written whole, and equal to the oracle's."""
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import bench
    W, H, depth = 256, 144, 8
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--depth", str(depth), "--width", str(W),
                        "--height", str(H), "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _line(p.stdout)
    assert line["full"] is False and line["steps"] == 4 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "Mrays/s"
    # value = the steps' rays / their wall time; ms_per_step is that time, rounded to 1e-4 ms
    assert abs(line["value"] - 2 * W * H / line["ms_per_step"] / 1e3) <= line["value"] * (1e-4 / line["ms_per_step"] + 1e-3)
    for k in ("roofline", "cpu_baseline", "parity", "sustained", "cull_off", "trace_batch", "bounce", "other_configs"):
        assert line[k] is None, k
    assert [f.name for f in tmp_path.iterdir()] == ["frames.npy"]
    got = np.load(tmp_path / "frames.npy")
    assert got.dtype == np.float32 and got.shape == (2, H, W, 4)
    tree = ort.build_terrain(depth)
    ref_pool, rcp = O.OraclePool(tree.nodes, tree.root, depth, 1), O.Rcp(None)
    pal = ort.VoxelData().get_colours()
    for v, pitch in enumerate(bench.PITCHES):
        r = O.trace_batch(ref_pool, rcp, np.array(bench.ORIGIN, np.float32), O.raygen(bench.YAW, pitch, bench.FOV, W, H))
        want = O.shade_fast(r["dir"], r["voxel"], pal).reshape(H, W)
        assert np.array_equal(got[v].astype(np.uint8).reshape(H, W * 4).view(np.uint32), want), f"view {v}"
