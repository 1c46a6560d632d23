"""och_world (ort.World) on the GPU: strokes against a resident store give the pool one build gives,
the pools a world publishes trace and render bit for bit as the oracle does on the downloaded pool,
earlier roots stay valid, and the capacity rule refuses a stroke before it changes anything.

Store ids differ from run to run (claim order): only downloads, records and frames are compared."""
import numpy as np
import pytest

from test_voxel_builder import CASES, ORIGIN, same_build
from test_voxel_edit import CAPACITY_BASE, CAPACITY_EDIT, check_case

pytestmark = pytest.mark.gpu

W, H = 64, 36
VIEW = (0.3, -0.6, 1.25)
# above the depth-8 terrain's brush box, looking down at it: the three strokes change well over a hundred
# of this frame's pixels each (the default view does not see the box at all)
BRUSH_POS, BRUSH_VIEW = (1.5, 1.5, 1.35), (0.3, -1.2, 1.25)


def thirds(rec):
    """(the base's records, the three strokes): cut at thirds of the list."""
    n = len(rec)
    return rec[:n // 3], np.array_split(rec[n // 3:], 3)


def roomy(base, strokes, depth):
    """A capacity no stroke of `strokes` can exhaust: a stroke's level counts are at most depth rows per
    record, and `used` grows by no more than they allow."""
    return base.n_nodes + 1 + depth * sum(len(s) for s in strokes)


def oracle_of(ort, O, tree):
    return O.OraclePool(tree.nodes, tree.root, tree.depth, 1), O.Rcp(ort.host_rcp_lut())


def random_rays(seed, n=4096):
    rng = np.random.default_rng(seed)
    dirs = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return rng.uniform(1.01, 1.99, (n, 3)).astype(np.float32), dirs


def check_traces(ort, O, pool, tree, org, dirs):
    """pool's records of these rays, in both layouts where it has both, bit for bit the oracle's on tree."""
    ref, rcp = oracle_of(ort, O, tree)
    r = O.trace_batch(ref, rcp, org, dirs)
    for layout in ([0, 1] if pool.info()["n_nodes"] <= 1 << 24 else [0]):
        pool.set_option("layout", layout)
        assert pool.get_option("layout") == layout
        gd, gv, gt = pool.trace_batch(org, dirs)
        assert np.array_equal(gd, r["dir"]) and np.array_equal(gv, r["voxel"]), layout
        assert np.array_equal(gt.view(np.uint32), r["t"].view(np.uint32)), layout
    return r


def oracle_frame(ort, O, tree, pos=ORIGIN, view=VIEW):
    ref, rcp = oracle_of(ort, O, tree)
    r = O.trace_batch(ref, rcp, np.asarray(pos, np.float32), O.raygen(*view, W, H))
    return O.shade(r["dir"], r["voxel"], ort.VoxelData().get_colours()).reshape(H, W)


def check_frame(ort, O, pool, tree, pos=ORIGIN, view=VIEW):
    want = oracle_frame(ort, O, tree, pos, view)
    pool.set_palette(ort.VoxelData().get_colours())
    for layout in (0, 1):
        pool.set_option("layout", layout)
        assert np.array_equal(pool.render(ort.camera(tuple(pos), *view, W, H)), want), layout


# ------------------------------------------------------------ 1. strokes equal one build

@pytest.mark.parametrize("name", sorted(CASES))
def test_strokes_equal_one_build(ort, gpu_device, name):
    depth, rec = CASES[name]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    with ort.World(base, capacity=roomy(base, strokes, depth)) as world:
        for s in strokes:
            world.edit(s)
        assert world.info()["strokes"] == sum(len(s) > 0 for s in strokes)
        check_case(world.download(), name)


def test_device_records_and_one_stroke(ort, gpu_device):
    import torch
    name = "n20000_d7"
    depth, rec = CASES[name]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    for dtype in (torch.int32, torch.uint32):
        with ort.World(base, capacity=roomy(base, strokes, depth)) as world:
            for s in strokes:
                world.edit(torch.from_numpy(s.view(np.int32)).cuda().view(dtype))
            check_case(world.download(), name)
    with ort.World(base, capacity=roomy(base, strokes, depth)) as world:
        world.edit(np.concatenate(strokes))
        check_case(world.download(), name)
        world.edit(torch.zeros((0, 4), dtype=torch.int32, device="cuda"))          # no records: no stroke
        assert world.info()["strokes"] == 1
        with pytest.raises(ValueError):
            world.edit(torch.zeros((5, 4), dtype=torch.float32, device="cuda"))


# ------------------------------------------------------------ 2. wavefront and workgroup edges

@pytest.mark.parametrize("parents", [63, 64, 65, 255, 256, 257])
def test_sixty_four(ort, O, gpu_device, parents):
    """tests/test_gpu_voxel_edit.py's construction: the stroke touches exactly `parents` leaf-level nodes,
    empties every other one and gives the rest a second voxel, here with ids no base voxel has."""
    depth, i = 10, np.arange(parents, dtype=np.uint32)
    base_rec = np.stack([2 * i, 3 + 0 * i, 5 + 0 * i, 1 + i % 5], 1).astype(np.uint32)
    edit = base_rec.copy()
    edit[::2, 3] = 0
    edit[1::2, 0] += 1
    edit[1::2, 3] += 100
    base = ort.build_voxels(base_rec, depth=depth)
    with ort.World(base, capacity=roomy(base, [edit], depth)) as world, world.make_pool() as pool:
        world.edit(edit)
        world.flush(pool)
        tree = world.download()
        same_build(tree, ort.edit_voxels(base, edit))
        info = world.info()
        # the base's box and the stroke's new voxels; removals never shrink it
        assert info["box_lo"] == (0, 3, 5) and info["box_hi"] == (max(2 * parents - 1, int(edit[1::2, 0].max()) + 1), 4, 6)
        centres = (1.0 + (edit[:, :3].astype(np.float64) + 0.5) / (1 << depth)).astype(np.float32)
        aimed = centres - ORIGIN
        aimed /= np.linalg.norm(aimed, axis=1, keepdims=True)
        r = check_traces(ort, O, pool, tree, ORIGIN, aimed.astype(np.float32))
        assert (r["voxel"] > 100).sum() >= parents // 4, "the stroke's voxels are not hit: the new nodes are not walked"
        check_traces(ort, O, pool, tree, *random_rays(parents))


# ------------------------------------------------------------ 3. the reference's brush

@pytest.fixture(scope="module")
def terrain(ort, gpu_device):
    """The depth-8 terrain and the 40^3 box at its surface (test_gpu_voxel_edit.py's `brushed` geometry)."""
    base = ort.build_terrain(8, use_gpu=True)
    top = max(z for z in range(256) if base.at(128, 128, z))
    return base, np.array([108, 108, top - 20])


def test_brush_put_cut_put(ort, O, terrain):
    base, lo = terrain
    chain = base
    # three strokes of 40^3 records each allow themselves some 9 300 rows: 100 000 ids hold the terrain's 19 318 and them
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool:
        check_frame(ort, O, pool, base, BRUSH_POS, BRUSH_VIEW)
        frames = [oracle_frame(ort, O, base, BRUSH_POS, BRUSH_VIEW)]
        for n, id in enumerate((1, 0, 1)):
            rec = ort.box_records(lo, lo + 40, id)
            chain = ort.edit_voxels(chain, rec)                       # the host path's pool of the same strokes
            world.edit(rec)
            world.flush(pool)
            check_traces(ort, O, pool, chain, *random_rays(72 + n))
            check_frame(ort, O, pool, chain, BRUSH_POS, BRUSH_VIEW)
            frames.append(oracle_frame(ort, O, chain, BRUSH_POS, BRUSH_VIEW))
            assert (frames[-1] != frames[-2]).sum() > 50             # the frame does show the stroke
            same_build(world.download(), chain)
        assert world.info()["strokes"] == 3 and world.info()["generation"] == 0


# ------------------------------------------------------------ 4. snapshot

def test_frames_in_flight_keep_their_world(ort, O, terrain):
    import torch
    base, lo = terrain
    rec = ort.box_records(lo, lo + 40, 1)
    after = ort.edit_voxels(base, rec)
    cams = [ort.camera(BRUSH_POS, *BRUSH_VIEW, W, H)]
    colours = ort.VoxelData().get_colours()
    with ort.World(base, capacity=100_000) as world, world.make_pool() as pool, world.make_pool() as never_flushed:
        pool.set_palette(colours)
        never_flushed.set_palette(colours)
        a = torch.zeros((1, H, W), dtype=torch.int32, device="cuda")
        b = torch.zeros((1, H, W), dtype=torch.int32, device="cuda")
        pool.render_views_dev(cams, a)                                # queued, not waited for
        world.edit(rec)
        world.flush(pool)
        pool.render_views_dev(cams, b)
        torch.cuda.synchronize()
        old, new = (oracle_frame(ort, O, t, BRUSH_POS, BRUSH_VIEW) for t in (base, after))
        assert (old != new).sum() > 50
        assert np.array_equal(a.cpu().numpy().view(np.uint32)[0], old)
        assert np.array_equal(b.cpu().numpy().view(np.uint32)[0], new)
        assert np.array_equal(never_flushed.render(cams[0]), old)     # its root still reaches only what it had
        check_traces(ort, O, never_flushed, base, *random_rays(5))


# ------------------------------------------------------------ 5. capacity
#
# The solid 8^3 box of id 3 is 3 nodes: adopted, the store uses 4 ids (id 0 included).  The rule is
# used + the stroke's level counts > capacity, one id per row of the records' own tree.
#   CAPACITY_EDIT, (0, 0, 0) and (2, 0, 0) := 5: two leaf-level rows, one above them, the root: 2 + 1 + 1 = 4.
#       4 + 4 = 8 <= 9: it fits.  The two leaf rows are equal: 3 new nodes, used = 7.
#   SECOND, (4, 4, 4) := 0 and (5, 4, 4) := 6, two voxels of one leaf-level node: 1 + 1 + 1 = 3 rows.
#       7 + 3 = 10 > 9: refused.  compact() drops the old root, the one node of the 6 that the new
#       root no longer reaches: used = 6, and 6 + 3 = 9 <= 9 fits, 3 new nodes, used = 9: the store is full.
SECOND = np.array([[4, 4, 4, 0], [5, 4, 4, 6]], np.uint32)
CAVITY = (1.0 + 4.5 / 8,) * 3                                         # the centre of the voxel SECOND removes


def test_capacity(ort, O, gpu_device):
    base = ort.build_voxels(CAPACITY_BASE)
    assert base.n_nodes == 3
    with pytest.raises(ort.OchError, match="CAPACITY") as e:
        ort.World(base, capacity=3)                                   # the reachable nodes + 1 is the least
    assert e.value.status == -6
    with ort.World(base) as world:
        assert world.info()["capacity"] == 2 * 3 + 64 * 3             # the default: twice the reachable nodes + 64 * depth
    with ort.World(base, capacity=9) as world, world.make_pool() as pool:
        assert (world.info()["capacity"], world.info()["used"]) == (9, 4)
        world.edit(CAPACITY_EDIT)
        assert world.info()["used"] == 7
        before, tree = world.info(), world.download()
        same_build(tree, ort.edit_voxels(base, CAPACITY_EDIT))
        with pytest.raises(ort.OchError, match="CAPACITY") as e:
            world.edit(SECOND)
        assert e.value.status == -6
        assert world.info() == before
        same_build(world.download(), tree)
        world.compact()
        assert world.info()["used"] == 6 and world.info()["generation"] == before["generation"] + 1
        assert (world.info()["box_lo"], world.info()["box_hi"], world.info()["capacity"]) == ((0, 0, 0), (8, 8, 8), 9)
        same_build(world.download(), tree)
        world.edit(SECOND)
        assert world.info()["used"] == 9
        want = ort.edit_voxels(tree, SECOND)
        same_build(world.download(), want)
        world.flush(pool)                                             # made before the compaction: rewritten whole
        check_frame(ort, O, pool, want, pos=CAVITY, view=(0.4, -0.3, 1.25))
        rng = np.random.default_rng(9)
        dirs = rng.uniform(-1, 1, (512, 3)).astype(np.float32)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = check_traces(ort, O, pool, want, np.array(CAVITY, np.float32), dirs)
        assert (r["voxel"] == 6).any() and (r["voxel"] == 3).any()


# ------------------------------------------------------------ 6. raw-only pool

def test_raw_only_pool(ort, O, gpu_device):
    depth, rec = CASES["n257_d3"]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    with ort.World(base, capacity=2 ** 24 + 1) as world, world.make_pool() as pool:
        assert pool.info()["n_nodes"] == 2 ** 24 + 1
        with pytest.raises(ort.OchError, match="INVALID"):
            pool.set_option("layout", 1)
        assert pool.get_option("layout") == 0
        check_traces(ort, O, pool, base, *random_rays(1))
        world.edit(np.concatenate(strokes))
        world.flush(pool)
        tree = world.download()
        check_case(tree, "n257_d3")
        check_traces(ort, O, pool, tree, *random_rays(2))


# ------------------------------------------------------------ 7. guards

def test_guards(ort, O, gpu_device):
    depth, rec = CASES["n20000_d7"]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    downloads = []
    for run in range(2):
        with ort.World(base, capacity=roomy(base, strokes, depth)) as world:
            for s in strokes:
                world.edit(s)
            downloads.append(world.download())
    assert downloads[0].nodes.tobytes() == downloads[1].nodes.tobytes() and downloads[0].root == downloads[1].root
    with ort.World(base, capacity=200_000) as world, ort.World(base) as other, world.make_pool() as pool:
        with pytest.raises(ort.OchError, match="INVALID") as e:
            pool.update(1, base.nodes[:1], 1)
        assert e.value.status == -1
        # an editor of exactly the pool's size: only the mark tells the pool from one of its own
        with ort.Editor(base.nodes, base.root, depth, capacity=pool.info()["n_nodes"] - 1) as ed:
            with pytest.raises(ort.OchError, match="INVALID") as e:
                ed.flush(pool)
            assert e.value.status == -1
        with ort.HOctree(base.nodes, base.root, depth, device=0) as foreign, other.make_pool() as theirs:
            for p in (foreign, theirs):
                with pytest.raises(ort.OchError, match="INVALID") as e:
                    world.flush(p)
                assert e.value.status == -1
        check_traces(ort, O, pool, base, *random_rays(3))             # the refusals changed nothing

        # a stroke that removes everything, then one that paints into the empty world
        world.edit(first * np.array([1, 1, 1, 0], np.uint32))
        world.flush(pool)
        assert world.info()["root"] == 0
        gone = world.download()
        assert gone.root == 0 and gone.nodes.shape == (1, 8) and not gone.nodes.any()
        pool.set_palette(ort.VoxelData().get_colours())
        for layout in (0, 1):
            pool.set_option("layout", layout)
            assert np.all(pool.render(ort.camera(width=W, height=H)) == 0xFFFEBF00)
        world.edit(strokes[0])
        world.flush(pool)
        painted = world.download()
        same_build(painted, ort.build_voxels(strokes[0], depth=depth))
        check_traces(ort, O, pool, painted, *random_rays(4))
        check_frame(ort, O, pool, painted)
