"""ort.World walked through the random operation lists of tests/world_model.py, every answer compared
with the model bit for bit (the seeds, depths and capacities of tests/test_world_walk_host.py, which
proves the same lists against the host paths and asserts their quotas); and a used world's pool --
claim-ordered ids, rows of an abandoned branch, a packed layout by k_world_pack, a plan made for older
content -- through the frame kernels that the other world tests never reach."""
import time

import numpy as np
import pytest

from test_gpu_lit import make_light, render
from test_gpu_tiled_batch import tiled_dev
from test_gpu_world import BRUSH_POS, BRUSH_VIEW, random_rays
from test_world_walk_host import REGION_STEPS, WALKS, make_model
from world_model import Walk

pytestmark = pytest.mark.gpu

W, H = 82, 50                                # no multiple of the 8x8 tile, as tests/test_gpu_lit.py


@pytest.mark.parametrize("seed,depth,capacity,steps", WALKS)
def test_walk(ort, O, gpu_device, seed, depth, capacity, steps):
    model, base = make_model(seed, depth, capacity)
    tree = ort.build_voxels(base, depth=depth)
    t0 = time.perf_counter()
    with ort.World(tree, capacity=None if capacity is None else model.capacity) as world:
        Walk(ort, world, model, seed, big=capacity == "roomy", O=O, on_gpu=True).run(steps + REGION_STEPS)
    print(f"walk {seed} depth {depth}: {steps + REGION_STEPS} operations in {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------ a used world's pool through the other frame kernels

def entries(ort, pool, cams, light, rays):
    """name -> what each entry gives, in both layouts."""
    import torch
    out = {}
    pos, (yaw, pitch, fov) = BRUSH_POS, BRUSH_VIEW
    for layout in (0, 1):
        pool.set_option("layout", layout)
        pool.set_option("tile_order", 0)
        pool.set_option("bounce_compact", 1)
        out[layout, "lit"], out[layout, "masks"] = render(pool, cams, light)
        for s in (2, 4):
            out[layout, "ssaa", s] = pool.render_ssaa(ort.camera(pos, yaw, pitch, fov, W * s, H * s), s)
        out[layout, "lit_ssaa"] = pool.render_lit_ssaa(ort.camera(pos, yaw, pitch, fov, W * 2, H * 2), light, 2)
        for compact in (0, 1, 2):
            pool.set_option("bounce_compact", compact)
            frames = torch.full((len(cams), H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            pool.render_bounce_views_dev(cams, frames)
            torch.cuda.synchronize()
            out[layout, "bounce", compact] = frames.cpu().numpy().view(np.uint32)
        for k, v in tiled_dev(pool, rays[0], rays[1], 64).items():
            out[layout, "tiled", k] = v
        pool.set_option("tile_order", 2)                 # the plan is the caller's, made before
        for split in (60, 0):
            pool.set_option("split", split)
            frames = torch.full((len(cams), H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            pool.render_views_dev(cams, frames)
            torch.cuda.synchronize()
            out[layout, "planned", split] = frames.cpu().numpy().view(np.uint32)
        pool.set_option("split", 60)
    return out


def test_used_pool_through_the_frame_kernels(ort, gpu_device):
    base = ort.build_terrain(8, use_gpu=True)
    top = max(z for z in range(256) if base.at(128, 128, z))
    lo = np.array([108, 108, top - 20])
    colours = ort.VoxelData().get_colours()
    cams = [ort.camera(BRUSH_POS, *BRUSH_VIEW, W, H), ort.camera((1.5, 1.5, 1.5), 0.3, -0.6, 1.25, W, H)]
    light = make_light(ort, 3, depth=8)
    rays = random_rays(8, 4096)

    def planned(pool):
        pool.set_palette(colours)
        pool.set_option("layout", 1)
        for k, v in (("split", 60), ("split_segs", 4), ("split_level", 4)):
            pool.set_option(k, v)
        pool.set_option("tile_order", 2)
        pool.plan_views(cams)

    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool:
        planned(pool)                                    # a plan and a split for the content before the strokes
        before = pool.render(cams[0])
        first = world.snapshot()
        world.edit(ort.box_records(lo, lo + 40, 1))
        second = world.snapshot()
        world.edit(ort.box_records(lo, lo + 40, 0))
        world.checkout(first)                            # the put and the cut: an abandoned branch
        world.edit(ort.box_records(lo + (4, 6, 8), lo + (34, 30, 36), 2))
        world.compact()
        assert world.snapshots() == [first, second]
        world.edit(np.concatenate([ort.box_records(lo + (10, 10, 26), lo + (20, 22, 36), 0),
                                   ort.box_records(lo + (-12, 2, 20), lo + (2, 12, 30), 3)]))
        world.flush(pool)
        tree = world.download()
        got = entries(ort, pool, cams, light, rays)
        pool.set_option("tile_order", 0)
        after = pool.render(cams[0])
    with ort.HOctree(tree.nodes, tree.root, 8, device=0) as ref:
        planned(ref)
        want = entries(ort, ref, cams, light, rays)
        ref.set_option("tile_order", 0)
        assert np.array_equal(ref.render(cams[0]), after)
    assert sorted(got, key=str) == sorted(want, key=str)
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name
    # the entries are live: the lit frame is not the plain one, the strokes show
    assert (got[1, "lit"][0] != after).sum() > 50
    assert (after != before).sum() > 50
