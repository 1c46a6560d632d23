"""och_world_* (ort.World) without a GPU: what is refused before the device is touched, the Python
side's own checks, and the header's new section as a strict-C99 host sees it."""
import ctypes as C

import numpy as np
import pytest

from test_voxel_builder import random_records

NODES = np.array([[2, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]], np.uint32)   # voxel 3 at (0, 0, 0), depth 2
RECORDS = np.array([[0, 0, 0, 1]], np.uint32)


def status(ort, name, *args):
    return getattr(ort.load(), name)(*args)


def test_create_refusals(ort):
    h = C.c_void_p()
    for depth in (0, 22, -1):
        assert status(ort, "och_world_create", NODES.ctypes.data, 2, 1, depth, 0, -1, C.byref(h)) == -1 and not h.value
        assert b"depth" in ort.load().och_last_error()
    assert status(ort, "och_world_create", None, 2, 1, 2, 0, -1, C.byref(h)) == -1 and not h.value
    assert b"nodes" in ort.load().och_last_error()
    assert status(ort, "och_world_create", NODES.ctypes.data, 2, 3, 2, 0, -1, C.byref(h)) == -1 and not h.value
    assert b"root" in ort.load().och_last_error()
    assert status(ort, "och_world_create", NODES.ctypes.data, 2, 1, 2, 0, -1, None) == -1
    for depth in (0, 22):
        with pytest.raises(ort.OchError, match="INVALID.*depth"):
            ort.World((NODES, 1, depth))
    with pytest.raises(ort.OchError, match="INVALID.*root"):
        ort.World((NODES, 3, 2))
    zero_based = ort.build_terrain(3, dedup=False)
    with pytest.raises(ort.OchError, match="INVALID"):
        ort.World(zero_based)
    with pytest.raises(ValueError, match="capacity"):
        ort.World((NODES, 1, 2), capacity=1 << 32)


def test_null_world_and_long_lists(ort):
    from octree_ray_tracing_amd._lib import HostPool, WorldStats
    st, hp, pool = WorldStats(), HostPool(), C.c_void_p()
    # a list of 2^31 records is refused whatever the world
    assert status(ort, "och_world_edit", None, RECORDS.ctypes.data, 1 << 31, 0) == -1
    assert b"2^31" in ort.load().och_last_error()
    assert status(ort, "och_world_edit", None, RECORDS.ctypes.data, 1, 0) == -1
    assert b"NULL" in ort.load().och_last_error()
    assert status(ort, "och_world_info", None, C.byref(st)) == -1
    assert status(ort, "och_world_pool_create", None, C.byref(pool)) == -1 and not pool.value
    assert status(ort, "och_world_flush", None, None) == -1
    assert status(ort, "och_world_download", None, C.byref(hp)) == -1 and not hp.nodes
    assert status(ort, "och_world_compact", None) == -1
    assert status(ort, "och_world_destroy", None) == 0


def test_needs_a_gpu(ort):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ort.OchError, match="NODEV") as e:
        ort.World((NODES, 1, 2))
    assert e.value.status == -3
    with pytest.raises(ort.OchError, match="NODEV"):
        ort.World(ort.build_voxels(random_records(1, 100, 3), depth=3), capacity=1000)


def closed_world(ort):
    """What close() leaves behind, without the device a live world needs."""
    w = ort.World.__new__(ort.World)
    w._h, w.depth, w.device = C.c_void_p(), 3, 0
    assert w.closed
    return w


def test_python_side_checks(ort):
    w = closed_world(ort)
    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((5, 3), np.uint32), np.zeros(4, np.uint32)):
        with pytest.raises(ValueError, match="record list"):
            w.edit(bad)
    with pytest.raises(ValueError, match="integers"):
        w.edit(np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match="id"):
        w.edit(np.array([[0, 0, 0, 1 << 32]], np.int64))

    class FakeDeviceTensor:
        is_cuda = True

    with pytest.raises(ValueError, match="closed"):
        w.edit(FakeDeviceTensor())
    with pytest.raises(ValueError, match="closed"):
        w.edit(RECORDS)
    for call in (w.info, w.make_pool, w.download, w.compact):
        with pytest.raises(ValueError, match="closed"):
            call()
    w.close()                                            # closing twice is fine


def test_binding_lists_the_world(ort):
    names = {"och_world_create", "och_world_destroy", "och_world_info", "och_world_edit", "och_world_pool_create",
             "och_world_flush", "och_world_download", "och_world_compact"}
    assert names <= set(ort._lib.exported_symbols())
    assert C.sizeof(ort._lib.WorldStats) == 64


def test_c99_host_names_every_world_function(ort, tmp_path):
    """The world section compiles as strict C99 and links: a C host that names every och_world_*
    entry and runs the refusals that need no device."""
    import shutil
    import subprocess
    from pathlib import Path
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    root = Path(ort._lib.HEADER_PATH).resolve().parents[1]
    libdir = Path(ort.load()._name).resolve().parent
    src = tmp_path / "world.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "och_gpu.h"
int main(void)
{
    const uint32_t nodes[2][8] = {{2, 0, 0, 0, 0, 0, 0, 0}, {3, 0, 0, 0, 0, 0, 0, 0}};
    const uint32_t rec[4] = {0, 0, 0, 1};
    och_world *world = NULL;
    och_gpu_pool *pool = NULL;
    och_world_stats st;
    och_host_pool hp;
    memset(&st, 0, sizeof st);
    memset(&hp, 0, sizeof hp);
    if (sizeof st != 64) return 1;
    if (och_world_create(&nodes[0][0], 2, 1, 0, 0, -1, &world) != OCH_E_INVALID || world != NULL) return 2;
    if (strstr(och_last_error(), "depth") == NULL) return 3;
    if (och_world_create(&nodes[0][0], 2, 3, 2, 0, -1, &world) != OCH_E_INVALID || world != NULL) return 4;
    if (och_world_info(world, &st) != OCH_E_INVALID) return 5;
    if (och_world_edit(world, rec, 1, 0) != OCH_E_INVALID) return 6;
    if (och_world_pool_create(world, &pool) != OCH_E_INVALID || pool != NULL) return 7;
    if (och_world_flush(world, pool) != OCH_E_INVALID) return 8;
    if (och_world_download(world, &hp) != OCH_E_INVALID || hp.nodes != NULL) return 9;
    if (och_world_compact(world) != OCH_E_INVALID) return 10;
    if (och_world_destroy(world) != OCH_OK) return 11;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "world"
    cc = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{root / 'include'}",
                         str(src), f"-L{libdir}", "-loch_gpu", f"-Wl,-rpath,{libdir}", "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.returncode, run.stdout, run.stderr)
