"""Reading a resident world back on the GPU: World.at, World.read_box and World.tighten
(och_world_at, och_world_read_box, och_world_tighten).

Truth is always the host path on world.download() (NodePool.read_box, ort.occupied_box) or the
dictionary `surviving(depth, records)`.  A whole tree is read wherever it can be held (depth <= 7);
the depth-16 and depth-21 cases are read in tests/test_pool_read_host.py's sampled 5^3 boxes, for
the reason given there.  corner_records(1) names a coordinate below 0, which its uint32 array
cannot hold, so at depth 1 the full 2^3 tree of CASES["full_d1"] stands in for it."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_world import H, W, check_frame, oracle_frame, roomy, thirds
from test_pool_read_host import WHOLE_DEPTH, dtypes_for, sample_boxes, scatter, vec
from test_voxel_builder import CASES, corner_records, random_records, same_build, surviving

pytestmark = pytest.mark.gpu

U8, U32 = 1, 2
SKY = 0xFFFEBF00


def status(ort, name, *args):
    return getattr(ort.load(), name)(*args)


def painted(ort, name):
    """A world of the case's first third with its three strokes applied and never flushed."""
    depth, rec = CASES[name]
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    world = ort.World(base, capacity=roomy(base, strokes, depth))
    for s in strokes:
        world.edit(s)
    return world


def probe_coordinates(depth, cells, seed):
    dim = 1 << depth
    rng = np.random.default_rng(seed)
    d = dim - 1
    coords = [list(k) for k in cells]
    coords += rng.integers(0, dim, (2000, 3)).tolist()
    coords += [[x, y, z] for z in (0, d) for y in (0, d) for x in (0, d)]
    inside = [d // 3, d // 2, d]
    for outside in (-1, dim, 2 ** 31 - 1):
        for axis in range(3):
            c = list(inside)
            c[axis] = outside
            coords.append(c)
        coords.append([outside] * 3)
    return np.array(coords, np.int64).reshape(-1, 3)


def expected_ids(cells, coords):
    return np.array([cells.get(tuple(c), 0) for c in coords.tolist()], np.uint32)


# ------------------------------------------------------------ 1. at

@pytest.mark.parametrize("name", sorted(CASES))
def test_at_cases(ort, gpu_device, name):
    depth, rec = CASES[name]
    cells = surviving(depth, rec)
    coords = probe_coordinates(depth, cells, len(name))
    want = expected_ids(cells, coords)
    with painted(ort, name) as world:
        got = world.at(coords)
        assert got.dtype == np.uint32 and got.shape == (len(coords),)
        assert np.array_equal(got, want)
        world.compact()
        assert np.array_equal(world.at(coords.astype(np.int32)), want)


@pytest.fixture(scope="module")
def d7(ort, gpu_device):
    """The depth-7 world of 20 000 records, its dictionary and its download, shared and left unchanged."""
    name = "n20000_d7"
    with painted(ort, name) as world:
        yield world, surviving(*CASES[name]), world.download()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_at_sizes(ort, d7, n):
    world, cells, _ = d7
    hits = np.array(sorted(cells)[:n:2], np.int32).reshape(-1, 3)
    rng = np.random.default_rng(n)
    coords = np.concatenate([hits, rng.integers(-2, 130, (n - len(hits), 3)).astype(np.int32)])
    got = world.at(coords)
    assert got.shape == (n,) and np.array_equal(got, expected_ids(cells, coords))
    assert n < 2 or got.any()


def test_at_device(ort, d7):
    import torch
    world, cells, _ = d7
    coords = probe_coordinates(7, cells, 3).astype(np.int32)
    host = world.at(coords)
    dev = world.at(torch.from_numpy(coords).cuda())
    assert dev.is_cuda and dev.dtype == torch.int32 and dev.shape == (len(coords),)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host)
    assert world.at(torch.zeros((0, 3), dtype=torch.int32, device="cuda")).shape == (0,)
    with pytest.raises(ValueError, match="int32"):
        world.at(torch.zeros((5, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int32"):
        world.at(torch.zeros((5, 4), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------ 2. read_box

@pytest.mark.parametrize("depth", [1, 2, 3])
def test_read_box_shallow_trees(ort, gpu_device, depth):
    dim = 1 << depth
    one = np.array([[dim - 1, 0, dim // 2, 9]], np.uint32)
    corners = corner_records(depth) if depth > 1 else CASES["full_d1"][1]
    for rec in (one, corners, np.zeros((0, 4), np.uint32)):
        cells = surviving(depth, rec)
        with ort.World(ort.build_voxels(rec, depth=depth)) as world:
            for dtype in (np.uint8, np.uint32):
                grid = world.read_box((0, 0, 0), (dim, dim, dim), dtype)
                assert np.array_equal(grid, scatter(cells, (0, 0, 0), (dim, dim, dim), dtype))
                lo, hi = (-1, -2, -3), (dim + 3, dim + 2, dim + 1)
                assert np.array_equal(world.read_box(lo, hi, dtype), scatter(cells, lo, hi, dtype))
            coords = np.array(sorted(cells) + [(0, 0, 0), (dim, 0, 0)], np.int32).reshape(-1, 3)
            assert np.array_equal(world.at(coords), expected_ids(cells, coords))


@pytest.mark.parametrize("name", sorted(CASES))
def test_read_box_cases(ort, gpu_device, name):
    depth = CASES[name][0]
    dim = 1 << depth
    with painted(ort, name) as world:
        tree = world.download()
        cells = surviving(*CASES[name])
        for dtype in dtypes_for(cells):
            if depth <= WHOLE_DEPTH:
                grid = world.read_box((0, 0, 0), (dim, dim, dim), dtype)
                assert grid.dtype == dtype
                assert np.array_equal(grid, tree.read_box((0, 0, 0), (dim, dim, dim), dtype))
                same_build(ort.build_voxels(grid, use_gpu=True), tree)
            else:
                for lo, hi in sample_boxes(depth, cells):
                    assert np.array_equal(world.read_box(lo, hi, dtype), tree.read_box(lo, hi, dtype)), (lo, hi)
        if depth > WHOLE_DEPTH:
            one = np.zeros(1, np.uint8)
            assert status(ort, "och_world_read_box", world._h, vec(0, 0, 0), vec(dim, dim, dim), U8, one.ctypes.data, 1, 0) == -1
        elif np.uint8 not in dtypes_for(cells):
            with pytest.raises(ort.OchError, match="INVALID"):
                world.read_box((0, 0, 0), (dim, dim, dim), np.uint8)


BOXES = {"unaligned": ((1, 2, 3), (6, 6, 12)), "overhang": ((-3, -3, -3), (130, 130, 130)),
         "one_brick": ((8, 12, 16), (12, 16, 20)), "brick_and_a_cell": ((7, 11, 15), (13, 17, 21)),
         "off_by_one_brick": ((9, 13, 17), (13, 17, 21)), "outside": ((-9, 3, 3), (-1, 9, 9)),
         "slab": ((0, 0, 63), (128, 128, 66))}


@pytest.fixture(scope="module")
def dense7(ort, gpu_device):
    """A depth-7 world dense enough (one cell in twelve) that every box below but "outside" holds voxels."""
    depth, rec = 7, random_records(31, 200_000, 7)
    first, strokes = thirds(rec)
    base = ort.build_voxels(first, depth=depth)
    with ort.World(base, capacity=roomy(base, strokes, depth)) as world:
        for s in strokes:
            world.edit(s)
        tree = world.download()
        same_build(tree, ort.build_voxels(rec, depth=depth))
        yield world, surviving(depth, rec), tree


@pytest.mark.parametrize("box", sorted(BOXES))
def test_read_box_boxes(ort, dense7, box):
    world, cells, tree = dense7
    lo, hi = BOXES[box]
    for dtype in (np.uint8, np.uint32):
        grid = world.read_box(lo, hi, dtype)
        want = tree.read_box(lo, hi, dtype)
        assert grid.shape == want.shape and np.array_equal(grid, want)
        assert np.array_equal(want, scatter(cells, lo, hi, dtype))
        assert box == "outside" or want.any()


def test_read_box_single_and_empty(ort, d7):
    world, cells, tree = d7
    cell = sorted(cells)[len(cells) // 2]
    for dtype in (np.uint8, np.uint32):
        grid = world.read_box(cell, tuple(c + 1 for c in cell), dtype)
        assert grid.shape == (1, 1, 1) and grid[0, 0, 0] == cells[cell]
    canary = np.full(64, 0xAB, np.uint8)
    for lo, hi in (((4, 4, 4), (4, 9, 9)), ((4, 4, 4), (9, 4, 9)), ((4, 4, 4), (9, 9, 4))):
        for kind in (U8, U32):
            assert status(ort, "och_world_read_box", world._h, vec(*lo), vec(*hi), kind, canary.ctypes.data, 64, 0) == 0
            assert (canary == 0xAB).all()
    assert world.read_box((4, 4, 4), (9, 4, 9)).shape == (5, 0, 5)
    assert world.read_box((4, 4, 4), (9, 4, 9), device=True).shape == (5, 0, 5)


def test_read_box_device_and_refusals(ort, d7):
    import torch
    world, cells, tree = d7
    lo, hi = (1, 2, 3), (70, 66, 12)
    for dtype, tdtype in ((np.uint8, torch.uint8), (np.uint32, torch.int32)):
        dev = world.read_box(lo, hi, dtype, device=True)
        assert dev.is_cuda and dev.dtype == tdtype and tuple(dev.shape) == (9, 64, 69)
        assert np.array_equal(dev.cpu().numpy().view(dtype), tree.read_box(lo, hi, dtype))
    # a capacity one byte short: refused with the device buffer as it was
    for kind, cell in ((U8, 1), (U32, 4)):
        need = 9 * 64 * 69 * cell
        canary = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert status(ort, "och_world_read_box", world._h, vec(*lo), vec(*hi), kind, canary.data_ptr(), need - 1, 1) == -1
        assert b"does not fit" in ort.load().och_last_error()
        assert bool((canary == 0xAB).all())
        assert status(ort, "och_world_read_box", world._h, vec(*lo), vec(*hi), kind, canary.data_ptr(), need, 1) == 0
        assert np.array_equal(canary.cpu().numpy().view(np.uint8 if kind == U8 else np.uint32).reshape(9, 64, 69),
                              tree.read_box(lo, hi, np.uint8 if kind == U8 else np.uint32))
    for bad in ((None, vec(*hi), U8), (vec(*lo), None, U8), (vec(*lo), vec(*hi), 0), (vec(*hi), vec(*lo), U8)):
        one = np.zeros(1 << 16, np.uint8)
        assert status(ort, "och_world_read_box", world._h, bad[0], bad[1], bad[2], one.ctypes.data, one.nbytes, 0) == -1
    assert status(ort, "och_world_read_box", world._h, vec(*lo), vec(*hi), U8, None, 1 << 16, 0) == -1


def test_read_box_more_bricks_than_one_pass(ort, gpu_device):
    """A launch holds at most 2^16 workgroups of four wavefronts (kReadMaxBlocks): a box of more than
    2^18 bricks makes every wavefront take several.  128 x 128 x 76 = 1 245 184 bricks here, the box
    overhanging the depth-9 tree on every side but the top: 4.75 passes, the last one partial."""
    depth, rec = 9, random_records(77, 60_000, 9, ids=(1, 250))
    lo, hi = (-2, -2, -2), (514, 514, 302)
    with ort.World(ort.build_voxels(rec, depth=depth)) as world:
        tree = world.download()
        want = tree.read_box(lo, hi, np.uint8)
        assert (want != 0).sum() > 25_000 and want[2:, 2:514, 2:514][-8:].any() and want[2:10, 2:514, 2:514].any()
        assert np.array_equal(world.read_box(lo, hi, np.uint8), want)
        assert np.array_equal(world.read_box(lo, hi, np.uint8, device=True).cpu().numpy(), want)


def test_read_box_u8_overflow(ort, gpu_device):
    base = ort.build_voxels(np.array([[3, 4, 5, 255]], np.uint32), depth=4)
    with ort.World(base) as world:
        world.edit(np.array([[9, 9, 9, 300]], np.uint32))
        assert world.read_box((0, 0, 0), (9, 9, 9), np.uint8)[5, 4, 3] == 255      # the box leaves the 300 out
        for device in (False, True):
            with pytest.raises(ort.OchError, match="INVALID.*300") as e:
                world.read_box((0, 0, 0), (16, 16, 16), np.uint8, device=device)
            assert e.value.status == -1
        assert world.read_box((0, 0, 0), (16, 16, 16), np.uint32)[9, 9, 9] == 300
        assert world.at(np.array([[9, 9, 9]])).tolist() == [300]                  # the refusal broke nothing


# ------------------------------------------------------------ 3. tighten

def exact_box(ort, world):
    tree = world.download()
    return ort.occupied_box(tree.nodes, tree.root, tree.depth)


def test_tighten_box(ort, O, gpu_device):
    depth = 6
    base = ort.build_terrain(depth, use_gpu=True)
    lo0, hi0 = ort.occupied_box(base.nodes, base.root, depth)
    top = hi0[2]
    cut = ort.box_records((0, 0, top - 2), (64, 64, top), 0)           # the slab that holds the topmost voxels
    with ort.World(base, capacity=roomy(base, [cut], depth)) as world, world.make_pool() as pool, \
            world.make_pool() as never_flushed:
        assert (world.info()["box_lo"], world.info()["box_hi"]) == (lo0, hi0)
        world.edit(cut)
        assert world.info()["box_hi"][2] == top                        # removals never shrink it
        after = world.download()
        want = ort.occupied_box(after.nodes, after.root, depth)
        assert want[1][2] <= top - 2
        assert world.tighten() == want
        assert (world.info()["box_lo"], world.info()["box_hi"]) == want
        same_build(world.download(), after)                            # the content is untouched
        world.flush(pool)
        check_frame(ort, O, pool, after)
        never_flushed.set_palette(ort.VoxelData().get_colours())
        for layout in (0, 1):
            never_flushed.set_option("layout", layout)
            assert np.array_equal(never_flushed.render(ort.camera((1.5, 1.5, 1.5), 0.3, -0.6, 1.25, W, H)),
                                  oracle_frame(ort, O, base)), layout


def test_tighten_incremental(ort, O, gpu_device):
    depth = 7
    blob = ort.box_records((10, 12, 14), (20, 21, 22), 3)
    far = np.array([[100, 110, 120, 5]], np.uint32)
    base = ort.build_voxels(blob, depth=depth)
    with ort.World(base, capacity=4096) as world, world.make_pool() as pool:
        first = world.tighten()
        assert first == ((10, 12, 14), (20, 21, 22)) == exact_box(ort, world)
        world.edit(far)
        assert (world.info()["box_lo"], world.info()["box_hi"]) == ((10, 12, 14), (101, 111, 121))
        assert world.tighten() == exact_box(ort, world) == ((10, 12, 14), (101, 111, 121))
        world.edit(far * np.array([1, 1, 1, 0], np.uint32))
        assert world.info()["box_hi"] == (101, 111, 121)               # a superset until the next tighten
        assert world.tighten() == first
        world.edit(np.array([[10, 12, 14, 0], [19, 20, 21, 0]], np.uint32))        # two corners of the blob go
        assert world.tighten() == exact_box(ort, world) == first       # the faces they lay in still hold voxels
        world.edit(ort.box_records((10, 12, 14), (11, 21, 22), 0))     # the whole x = 10 face goes
        assert world.tighten() == exact_box(ort, world) == ((11, 12, 14), (20, 21, 22))
        world.compact()
        assert world.tighten() == ((11, 12, 14), (20, 21, 22))
        world.edit(far)
        assert world.tighten() == ((11, 12, 14), (101, 111, 121))      # incremental again after the compaction
        world.edit(np.concatenate([blob, far]) * np.array([1, 1, 1, 0], np.uint32))
        assert world.info()["root"] == 0
        assert world.tighten() == ((0, 0, 0), (0, 0, 0))
        world.flush(pool)
        pool.set_palette(ort.VoxelData().get_colours())
        for layout in (0, 1):
            pool.set_option("layout", layout)
            assert np.all(pool.render(ort.camera(width=W, height=H)) == SKY)
        world.edit(far)                                                # and the box grows from nothing again
        assert (world.info()["box_lo"], world.info()["box_hi"]) == ((100, 110, 120), (101, 111, 121))
        assert world.tighten() == ((100, 110, 120), (101, 111, 121))


@pytest.mark.parametrize("parents", [63, 64, 65, 255, 256, 257])
def test_tighten_edges(ort, gpu_device, parents):
    """tests/test_gpu_world.py::test_sixty_four's construction between two tightens: the stroke touches
    exactly `parents` leaf-level nodes, so the incremental range [boxed, used) crosses that size."""
    depth, i = 10, np.arange(parents, dtype=np.uint32)
    base_rec = np.stack([2 * i, 3 + 0 * i, 5 + 0 * i, 1 + i % 5], 1).astype(np.uint32)
    edit = base_rec.copy()
    edit[::2, 3] = 0
    edit[1::2, 0] += 1
    edit[1::2, 3] += 100
    again = base_rec.copy()
    again[:, 1] += 40
    again[:, 3] = 1000 + i
    base = ort.build_voxels(base_rec, depth=depth)
    with ort.World(base, capacity=roomy(base, [edit, again], depth)) as world:
        assert world.tighten() == ((0, 3, 5), (2 * parents - 1, 4, 6)) == exact_box(ort, world)
        used = world.info()["used"]
        world.edit(edit)
        assert world.info()["used"] > used
        want = exact_box(ort, world)
        assert want[0] == (2, 3, 5)                                    # the voxel at x = 0 went: the box shrinks
        assert world.tighten() == want
        assert world.tighten() == want                                 # nothing new: the root's box alone
        # the stroke's leaf-level rows repeat five patterns and are shared; ids of its own make every one distinct
        used = world.info()["used"]
        world.edit(again)
        assert world.info()["used"] - used >= parents
        want = exact_box(ort, world)
        assert (want[0][1], want[1][1]) == (3, 44)
        assert world.tighten() == want
