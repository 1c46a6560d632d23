"""Adversarial keys for the interning of DAG rows (NodeStore::intern, probe_node / k_intern_rows /
k_settle in csrc/och_dag.h): a numpy twin of csrc/och_hash.h's node_hash, the search for rows that
meet in one table slot, and a Python simulation of the table's linear probing.

A helper module, not a test file.  tests/test_intern_cases_host.py pins the twin to the compiled
header, so the cases can never silently stop colliding; tests/test_gpu_intern_cases.py runs them on
the device.

CHAIN       300 distinct leaf-level rows [v, 0, 0, 0, 0, 0, 0, 0] whose hash ends in fourteen one
            bits: in every table of at most 16 384 slots they all start at the last slot and wrap
            to slot 0, one chain of 300.
TWO HEIGHTS a single voxel painted into an empty store allocates one row per level in order, so
            its ids are known: the leaf row is e_k0 * v with id 1, the height-j row e_kj * j.  With
            v = h and the same child digit at level 0 and level h, the height-h row spells the
            leaf row's eight words; the configurations kept are those whose probe also reaches
            the leaf row's slot, where only the level term of the comparison tells them apart.
"""
import time

import numpy as np

U64 = np.uint64
CHAIN_BITS = 0x3FFF
CHAIN_ROWS = 300
CHAIN_DEPTH = 6


def mix64(h):
    h = np.asarray(h, U64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> U64(33)
        h *= U64(0xFF51AFD7ED558CCD)
        h ^= h >> U64(33)
        h *= U64(0xC4CEB9FE1A85EC53)
        h ^= h >> U64(33)
    return h


def node_hash(rows, h):
    """csrc/och_hash.h's node_hash of (n, 8) rows at height h (a scalar or one per row): (n,) uint64."""
    c = np.asarray(rows, np.uint32).reshape(-1, 8).astype(U64)
    h = np.broadcast_to(np.asarray(h, U64), (c.shape[0],))
    with np.errstate(over="ignore"):
        hs = mix64(h * U64(0x9E3779B97F4A7C15) ^ (c[:, 1] << U64(32) | c[:, 0]))
    for k in (2, 4, 6):
        hs = mix64(hs ^ (c[:, k + 1] << U64(32) | c[:, k]))
    return hs


def table_size(cap):
    """The slots of a store of cap ids: the next power of two at or above 2 cap (NodeStore::init, gpu_store_create)."""
    ts = 1
    while ts < 2 * cap:
        ts <<= 1
    return ts


class Table:
    """Linear probing as the stores do it, one row after another: ids 1, 2, ... in insertion order."""

    def __init__(self, size, respect_height=True):
        self.size, self.slots, self.rows, self.respect_height = size, [0] * size, [None], respect_height

    def intern(self, row, h):
        """(id, the slots visited).  respect_height=False is a store that compares the words alone."""
        row = tuple(int(w) for w in row)
        i = int(node_hash([row], h)[0]) & (self.size - 1)
        visited = []
        for _ in range(self.size):
            visited.append(i)
            v = self.slots[i]
            if v == 0:
                self.rows.append((h, row))
                self.slots[i] = len(self.rows) - 1
                return self.slots[i], visited
            if self.rows[v][1] == row and (self.rows[v][0] == h or not self.respect_height):
                return v, visited
            i = (i + 1) & (self.size - 1)
        raise AssertionError("table full")


# ------------------------------------------------------------ CHAIN

def chain_values(count=CHAIN_ROWS):
    """(the first `count` v >= 8 with node_hash([v, 0, ...], 0) & 0x3FFF == 0x3FFF, the seconds the scan took).
    v < 8 would take the host store's direct leaf map, past the table."""
    t0, found, lo, step = time.perf_counter(), [], 8, 1 << 20
    rows = np.zeros((step, 8), np.uint32)
    while len(found) < count:
        assert lo < 1 << 31, "the scan ran away"
        rows[:, 0] = np.arange(lo, lo + step, dtype=np.uint32)
        hit = np.flatnonzero((node_hash(rows, 0) & U64(CHAIN_BITS)) == U64(CHAIN_BITS))
        found += (hit + lo).tolist()
        lo += step
    return np.array(found[:count], np.uint32), time.perf_counter() - t0


def demorton(p, levels):
    x = y = z = 0
    for l in range(levels):
        x |= (p >> 3 * l & 1) << l
        y |= (p >> 3 * l + 1 & 1) << l
        z |= (p >> 3 * l + 2 & 1) << l
    return x, y, z


def parent_records(parents, values, depth=CHAIN_DEPTH):
    """The voxel values[i] at local slot 0 of the leaf-level parent with Morton index parents[i]."""
    rec = np.zeros((len(parents), 4), np.uint32)
    for i, (p, v) in enumerate(zip(parents, values)):
        x, y, z = demorton(int(p), depth - 1)
        rec[i] = (2 * x, 2 * y, 2 * z, v)
    return rec


def chain_adjacent(values, first=0):
    """Row i at parent first + i: adjacent in Morton order, so the rows of one level-0 dispatch, in order."""
    return parent_records(np.arange(len(values)) + first, values)


def chain_threefold(values):
    """Each row at three parents, 900 in all: at 2 i and 2 i + 1 (lane 0 of every wavefront and its
    neighbour hold equal rows: the `follows` shortcut) and at 600 + i (an equal row workgroups away:
    the comparison with a claimed slot's claimant)."""
    n = len(values)
    i = np.arange(n)
    return parent_records(np.concatenate([2 * i, 2 * i + 1, 2 * n + i]), np.concatenate([values] * 3))


# ------------------------------------------------------------ TWO HEIGHTS

def two_heights_record(depth, h, k):
    """The record whose child digit is k at levels 0 and h and 0 elsewhere, with id h."""
    c = [((k >> a & 1) << 0) | ((k >> a & 1) << h) for a in range(3)]
    return np.array([[c[0], c[1], c[2], h]], np.uint32)


def two_heights_rows(depth, h, k):
    """The rows an empty store interns for that record, height 0 first: e_k0 * v, then e_kj * j."""
    rows = []
    for j in range(depth):
        row = [0] * 8
        row[k if j in (0, h) else 0] = h if j == 0 else j
        rows.append(row)
    return rows


def two_heights_meet(depth, h, k, slots):
    """Whether, in a table of `slots`, the height-h row's probe visits the leaf row's slot: a store
    that ignored the height would hand back id 1 there."""
    table, leaf_slot = Table(slots), None
    for j, row in enumerate(two_heights_rows(depth, h, k)):
        id, visited = table.intern(row, j)
        assert id == j + 1
        if j == 0:
            leaf_slot = visited[-1]
        if j == h:
            return leaf_slot in visited
    return False


def two_heights_search(max_depth=6, max_capacity=40):
    """Every (depth, capacity, h, k) with capacity >= depth + 1 whose height-h row meets the leaf row
    in a world's table (2 * capacity slots rounded up), smallest first."""
    out = []
    for depth in range(2, max_depth + 1):
        for capacity in range(depth + 1, max_capacity):
            for h in range(1, depth):
                for k in range(8):
                    if two_heights_meet(depth, h, k, table_size(capacity)):
                        out.append((depth, capacity, h, k))
    return out


def builder_slots(depth, capacity):
    """A builder's table for one voxel: its store holds min(capacity, depth + 1) ids."""
    return table_size(min(capacity, depth + 1) if capacity else depth + 1)


# ------------------------------------------------------------ the entries the cases run through
# (shared by tests/test_intern_cases_host.py and tests/test_gpu_intern_cases.py)

def empty_tree(depth):
    return np.zeros((0, 8), np.uint32), 0, depth


def run_builders(ort, depth, rec, use_gpu, threads=0, capacity=0):
    """build_voxels of the records; edit_voxels with half of them as the base, half as the stroke and
    a quarter of the base removed again; both against the Python pool."""
    from test_voxel_builder import check_pool
    tree = ort.build_voxels(rec, depth=depth, use_gpu=use_gpu, threads=threads, capacity=capacity)
    check_pool(tree, depth, rec)
    half = len(rec) // 2
    if not half:
        check_pool(ort.edit_voxels(empty_tree(depth), rec, use_gpu=use_gpu, threads=threads, capacity=capacity), depth, rec)
        return tree
    base_rec = rec[:half]
    stroke = np.concatenate([rec[half:], base_rec[::4] * np.array([1, 1, 1, 0], np.uint32)])
    base = ort.build_voxels(base_rec, depth=depth, use_gpu=use_gpu, threads=threads)
    check_pool(ort.edit_voxels(base, stroke, use_gpu=use_gpu, threads=threads), depth, np.concatenate([base_rec, stroke]))
    return tree


def chain_world_strokes(values):
    """An empty world's strokes: 64, 65 and 171 rows of the chain, the same rows at new parents (the
    finished-id path along the whole chain), removals, a compaction (None: re-interning into a fresh
    table) and a last stroke."""
    first = [chain_adjacent(values[:64], 0), chain_adjacent(values[64:129], 64), chain_adjacent(values[129:], 129)]
    again = chain_adjacent(values, 4096)
    gone = np.concatenate([first[0][::3], again[1::2]]) * np.array([1, 1, 1, 0], np.uint32)
    last = np.concatenate([chain_adjacent(values[::2], 8192), chain_adjacent(values[:10], 0)])
    return first + [again, gone, None, last]


def run_chain_world(ort, values, capacity=8192):
    from test_voxel_builder import check_pool
    from world_model import Model
    model = Model(CHAIN_DEPTH, np.zeros((0, 4), np.int64), capacity)
    done = [np.zeros((0, 4), np.uint32)]
    with ort.World(empty_tree(CHAIN_DEPTH), capacity=capacity) as world:
        assert world.info()["used"] == model.used == 1
        for stroke in chain_world_strokes(values):
            if stroke is None:
                model.compact()
                world.compact()
            else:
                assert model.edit(stroke) == "stroke"
                world.edit(stroke)
                done.append(stroke)
            assert world.info()["used"] == model.used, (world.info(), model.used)
            check_pool(world.download(), CHAIN_DEPTH, np.concatenate(done))


def run_two_heights_world(ort, depth, capacity, h, k):
    from test_voxel_builder import check_pool
    rec = two_heights_record(depth, h, k)
    with ort.World(empty_tree(depth), capacity=capacity) as world:
        world.edit(rec)
        assert world.info()["used"] == depth + 1          # one node short: id 1 handed back as an interior node
        check_pool(world.download(), depth, rec)
        assert world.at(rec[:, :3]).tolist() == [h]


def run_two_heights_builders(ort, depth, capacity, h, k, use_gpu, threads=0):
    rec = two_heights_record(depth, h, k)
    tree = run_builders(ort, depth, rec, use_gpu, threads, capacity)
    assert tree.n_nodes == depth and tree.at(*rec[0, :3].tolist()) == h
