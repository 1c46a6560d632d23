"""Terrain builder binding (och_build_terrain in liboch_gpu.so).

Builds the demo world of ORT/test_och_h_octree.cpp:561-787 (heightmap from
simplex noise, grass/dirt cap, simplex tunnels) as a hash-consed DAG in
parallel, breadth-first ordered.  Returns the node pool in the reference's
h_octree layout (1-based, root 1) or och::octree layout (0-based, root 0).
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ._lib import DiffStats, EditParams, HostPool, OchError, TerrainParams, VoxelParams, call
from ._marshal import host_array, host_pool_result, nodes_arg, records_arg, struct_dict


@dataclass
class NodePool:
    nodes: np.ndarray            # (n, 8) uint32
    root: int
    depth: int
    index_base: int
    solid_voxels: int = 0
    voxel_hist: list = field(default_factory=list)
    tree_nodes: int = 0
    build_seconds: float = 0.0

    @property
    def n_nodes(self) -> int:
        return self.nodes.shape[0]

    def at(self, x: int, y: int, z: int) -> int:
        """h_octree::at (ORT/och_h_octree.h:239-258)."""
        return call("och_pool_at", self.nodes.ctypes.data, self.root, self.depth, self.index_base, x, y, z)

    def read_box(self, lo, hi, dtype=np.uint8) -> np.ndarray:
        """The voxels of the box lo <= (x, y, z) < hi as a dense (nz, ny, nx) array indexed [z, y, x]
        (och_pool_read_box), the form build_voxels takes a grid in.  The box may reach outside the tree:
        cells there read 0.  dtype is np.uint8 or np.uint32; OchError INVALID names an id that uint8
        cannot hold."""
        lo, hi, shape, kind = _read_box_args(lo, hi, dtype, "NodePool.read_box")
        nodes, ptr, n = nodes_arg(self.nodes)
        grid = np.zeros(shape, dtype)
        # an empty grid still names a buffer: the call refuses NULL before it looks at the box
        target = grid if grid.size else np.zeros(1, dtype)
        call("och_pool_read_box", ptr, n, int(self.root), int(self.depth), int(self.index_base),
             lo, hi, kind, target.ctypes.data, grid.nbytes)
        return grid

    def diff(self, other: "NodePool", records: bool = True):
        """The voxels that differ between this pool and `other` (same depth and index_base), as
        (records, stats) (och_pool_diff): an (n, 4) np.uint32 array of (x, y, z, id under other) in
        ascending Morton order, id 0 where the voxel is gone, and {"n", "pairs", "box_lo", "box_hi"}.
        Applied to this pool's content with edit_voxels the records give other's.  records=False gives
        None and the stats."""
        if not isinstance(other, NodePool):
            raise ValueError(f"NodePool.diff: a NodePool, not {type(other).__name__}")
        if (other.depth, other.index_base) != (self.depth, self.index_base):
            raise ValueError(f"NodePool.diff: depth {other.depth} / index_base {other.index_base} against depth "
                             f"{self.depth} / index_base {self.index_base}")
        a, a_ptr, a_n = nodes_arg(self.nodes)
        b, b_ptr, b_n = (a, a_ptr, a_n) if other.nodes is self.nodes else nodes_arg(other.nodes)
        st = DiffStats()
        args = (a_ptr, a_n, int(self.root), b_ptr, b_n, int(other.root), int(self.depth), int(self.index_base))
        call("och_pool_diff", *args, None, 0, C.byref(st))
        out = None
        if records:
            out = np.zeros((st.n, 4), np.uint32)
            if st.n:
                call("och_pool_diff", *args, out.ctypes.data, st.n, C.byref(st))
        return out, struct_dict(st)

    # -- linearised node-pool file: a 64-byte header, then the
    # n x 8 little-endian uint32 slots exactly as och_gpu_pool_create takes them.
    # The reference rebuilds its world on every start (ORT/test_och_h_octree.cpp:822);
    # a depth-12 build takes ~30 s even in parallel, a load is one read.
    # Version 2: the CRC-32 covers the header fields (depth, index base, root,
    # node count) and then the slots; version-1 files (slots only) still load.
    _MAGIC = b"OCHPOOL\0"
    _HEADER = struct.Struct("<8sIiiIQI")   # magic, version, depth, index_base, root, n_nodes, crc32
    _VERSION = 2

    @classmethod
    def _crc(cls, version, depth, base, root, n, slots) -> int:
        crc = 0
        if version >= 2:
            crc = zlib.crc32(struct.pack("<IiiIQ", version, depth, base, root, n))
        return zlib.crc32(slots, crc)

    def save(self, path) -> None:
        nodes = np.ascontiguousarray(self.nodes, dtype="<u4").reshape(-1, 8)
        n = nodes.shape[0]
        crc = self._crc(self._VERSION, self.depth, self.index_base, self.root, n, memoryview(nodes).cast("B"))
        head = self._HEADER.pack(self._MAGIC, self._VERSION, self.depth, self.index_base, self.root, n, crc)
        with open(path, "wb") as f:
            f.write(head.ljust(64, b"\0"))
            f.write(memoryview(nodes).cast("B"))

    @classmethod
    def load(cls, path, mmap: bool = False, verify: bool = True) -> "NodePool":
        """Read a pool file.  Raises ValueError on a bad magic/version, a size
        that does not match the header, a depth / index base / root outside
        their ranges, or (verify=True) a checksum mismatch.  mmap=True maps the
        slots read-only instead of reading them."""
        path = Path(path)
        size = path.stat().st_size
        with open(path, "rb") as f:
            raw = f.read(64)
        if len(raw) < 64:
            raise ValueError(f"{path}: truncated header")
        magic, ver, depth, base, root, n, crc = cls._HEADER.unpack(raw[:cls._HEADER.size])
        if magic != cls._MAGIC or ver not in (1, 2):
            raise ValueError(f"{path}: not a version-1/2 node-pool file")
        if size != 64 + n * 32:
            raise ValueError(f"{path}: {size} bytes, header says {n} nodes ({64 + n * 32} bytes)")
        if not 1 <= depth <= 22 or base not in (0, 1):
            raise ValueError(f"{path}: depth {depth} / index base {base} out of range")
        # h_octree: root 0 = empty tree, else 1..n; och::octree: root 0 of n >= 1 nodes
        if (base == 1 and root > n) or (base == 0 and (root != 0 or n == 0)):
            raise ValueError(f"{path}: root {root} outside a {n}-node pool (index base {base})")
        if mmap:
            nodes = np.memmap(path, dtype="<u4", mode="r", offset=64, shape=(n, 8))
        else:
            nodes = np.fromfile(path, dtype="<u4", offset=64, count=n * 8).reshape(n, 8)
        if verify and cls._crc(ver, depth, base, root, n, memoryview(np.ascontiguousarray(nodes)).cast("B")) != crc:
            raise ValueError(f"{path}: checksum mismatch")
        return cls(np.asarray(nodes, dtype=np.uint32), root, depth, base)


def _read_box_args(lo, hi, dtype, who: str):
    """(lo, hi as int32[3], the (nz, ny, nx) shape, the grid kind) of a read_box call."""
    if np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.uint32)):
        raise ValueError(f"{who}: dtype is np.uint8 or np.uint32, not {np.dtype(dtype)}")
    corners = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = np.asarray(v)
        if v.shape != (3,) or v.dtype.kind not in "iu":
            raise ValueError(f"{who}: {name} is three integers (x, y, z), not {v.dtype} of shape {v.shape}")
        v = v.astype(np.int64)
        if v.min() < -(1 << 31) or v.max() >= 1 << 31:
            raise ValueError(f"{who}: {name} outside int32")
        corners.append(v)
    if (corners[1] < corners[0]).any():
        raise ValueError(f"{who}: hi {tuple(corners[1].tolist())} lies below lo {tuple(corners[0].tolist())}")
    nx, ny, nz = (int(n) for n in corners[1] - corners[0])
    kind = VOXELS_GRID_U8 if np.dtype(dtype) == np.dtype(np.uint8) else VOXELS_GRID_U32
    return ((C.c_int32 * 3)(*corners[0].tolist()), (C.c_int32 * 3)(*corners[1].tolist()), (nz, ny, nx), kind)


def build_terrain(depth: int, tunnels: bool = True, dedup: bool = True, rand_kind: str = "glibc",
                  threads: int = 0, use_gpu: bool = False) -> NodePool:
    """The demo world as a node pool.  use_gpu=True voxelises (and, for a DAG,
    hash-conses) on the current GPU (och_terrain_params.use_gpu; raises
    OchError OCH_E_NODEV without one); the pool is the same either way."""
    params = TerrainParams(int(depth), int(tunnels), int(dedup), 1 if rand_kind == "msvc" else 0,
                           int(threads), int(bool(use_gpu)))
    return _build("och_build_terrain", params)


def _build(name: str, params) -> NodePool:
    hp = HostPool()
    call(name, C.byref(params), C.byref(hp))
    return NodePool(*host_pool_result(hp))


VOXELS_LIST, VOXELS_GRID_U8, VOXELS_GRID_U32 = 0, 1, 2


def _capacity(capacity, who: str) -> int:
    if not 0 <= int(capacity) <= 0xFFFFFFFF:
        raise ValueError(f"{who}: capacity {capacity} outside uint32")
    return int(capacity)


def build_voxels(voxels, depth: int | None = None, use_gpu: bool = False, threads: int = 0, capacity: int = 0) -> NodePool:
    """A DAG from the caller's voxels (och_build_voxels), the same canonical pool whatever the path,
    the record order or the input kind.

    voxels is an (n, 4) integer array of (x, y, z, id) records that act as successive set() calls (a
    later record replaces an earlier one, id 0 removes, coordinates outside the tree are ignored; depth
    is required), or a cubic 3-D uint8 / uint32 array indexed [z, y, x] with a power-of-two side (the
    depth follows from the side).  A numpy array is host memory; a CUDA torch tensor (int32 / uint32
    records) is read where it lies, on the current device, and needs use_gpu=True.  capacity = node ids
    to reserve, 0 = the exact bound."""
    voxels = host_array(voxels)
    on_device = hasattr(voxels, "is_cuda")
    if not on_device:
        voxels = np.asarray(voxels)
    if on_device or (voxels.ndim == 2 and voxels.shape[1] == 4):
        voxels, ptr, n, on_device = records_arg(voxels, "build_voxels", use_gpu=use_gpu)
        kind = VOXELS_LIST
    elif voxels.ndim == 3:
        side = voxels.shape[0]
        if voxels.shape != (side, side, side) or side < 2 or side & (side - 1):
            raise ValueError(f"build_voxels: a grid is cubic with a power-of-two side >= 2, not {voxels.shape}")
        if voxels.dtype not in (np.uint8, np.uint32):
            raise ValueError(f"build_voxels: a grid holds uint8 or uint32 ids, not {voxels.dtype}")
        if depth is not None and 1 << int(depth) != side:
            raise ValueError(f"build_voxels: depth {depth} does not match a grid of side {side}")
        depth = side.bit_length() - 1
        voxels = np.ascontiguousarray(voxels)
        kind, ptr, n = (VOXELS_GRID_U8 if voxels.dtype == np.uint8 else VOXELS_GRID_U32), voxels.ctypes.data, 0
    else:
        raise ValueError(f"build_voxels: an (n, 4) record list or a cubic 3-D grid, not shape {voxels.shape}")
    if depth is None:
        raise ValueError("build_voxels: a record list needs depth")
    params = VoxelParams(int(depth), kind, ptr, int(n), int(on_device), int(bool(use_gpu)), int(threads),
                         _capacity(capacity, "build_voxels"))
    return _build("och_build_voxels", params)


def edit_voxels(tree, voxels, use_gpu: bool = False, threads: int = 0, capacity: int = 0) -> NodePool:
    """A batch of voxel edits applied to an existing world (och_edit_voxels): the canonical pool of the
    tree's voxels after the records, the pool build_voxels gives for those voxels followed by the
    records, slot for slot, whatever the path.

    tree is a NodePool with index_base 1 or a (nodes, root, depth) tuple in that form; it need not be
    canonical (an Editor's nodes() will do: only what the root reaches is read).  voxels is a record
    list as build_voxels takes it, on the host or, with use_gpu=True, a CUDA tensor; no records
    canonicalise the tree.  capacity = node ids to reserve, 0 = the reachable nodes + the rows of the
    records' own tree + 1."""
    if isinstance(tree, NodePool):
        if tree.index_base != 1:
            raise OchError(-1, "och_edit_voxels", "a pool with index_base 1 (h_octree form), not an och::octree pool")
        tree = (tree.nodes, tree.root, tree.depth)
    nodes, root, depth = tree
    nodes, nodes_ptr, n_nodes = nodes_arg(nodes)
    voxels, ptr, n, on_device = records_arg(voxels, "edit_voxels", use_gpu=use_gpu)
    if not 0 <= int(root) <= 0xFFFFFFFF:
        raise ValueError(f"edit_voxels: root {root} outside uint32")
    params = EditParams(nodes_ptr, n_nodes, int(root), int(depth), ptr, int(n), int(on_device),
                        int(bool(use_gpu)), int(threads), _capacity(capacity, "edit_voxels"))
    return _build("och_edit_voxels", params)


def box_records(lo, hi, id: int) -> np.ndarray:
    """The (n, 4) uint32 records (x, y, z, id) of the box lo <= (x, y, z) < hi, x fastest, then y, then z:
    one brush stroke for edit_voxels (the reference's is box_records(c - 20, c + 20, v)).  An empty box
    gives (0, 4).  A coordinate below 0 wraps to one outside any tree, which an edit ignores."""
    if not 0 <= int(id) <= 0xFFFFFFFF:
        raise ValueError(f"box_records: id {id} outside uint32")
    lo, hi = np.asarray(lo, np.int64).reshape(3), np.asarray(hi, np.int64).reshape(3)
    nx, ny, nz = (int(v) for v in np.maximum(hi - lo, 0))
    rec = np.empty((nz, ny, nx, 4), np.uint32)
    rec[..., 0] = (lo[0] + np.arange(nx)).astype(np.uint32)[None, None, :]
    rec[..., 1] = (lo[1] + np.arange(ny)).astype(np.uint32)[None, :, None]
    rec[..., 2] = (lo[2] + np.arange(nz)).astype(np.uint32)[:, None, None]
    rec[..., 3] = int(id)
    return rec.reshape(-1, 4)


def _box_args(lo, hi, who: str):
    """(lo, hi as int32[3]) of a box stroke, checked as read_box checks its corners."""
    return _read_box_args(lo, hi, np.uint8, who)[:2]


def box_cubes(lo, hi, depth: int):
    """The maximal aligned cubes of the box lo <= (x, y, z) < hi clipped to a tree of `depth`
    (och_box_cubes, host only): (keys, heights, cubes_per_height, cells_per_height).  keys[i] is cube i's
    Morton key at height heights[i] (side 2^h, corner = the key's coordinates times 2^h), in ascending
    height and ascending key within a height; cubes_per_height[h] counts them and cells_per_height[H]
    the cells of side 2^H that straddle the box, both np.uint64 of length depth + 1.  What
    World.fill_box writes and rebuilds: its stats' cubes and cells are the two sums."""
    lo, hi = _box_args(lo, hi, "box_cubes")
    cubes, cells, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
    call("och_box_cubes", lo, hi, int(depth), None, None, 0, cubes, cells, C.byref(n))
    keys, heights = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint8)
    if n.value:
        call("och_box_cubes", lo, hi, int(depth), keys.ctypes.data, heights.ctypes.data, n.value, cubes, cells, C.byref(n))
    return keys, heights, np.array(cubes[:int(depth) + 1], np.uint64), np.array(cells[:int(depth) + 1], np.uint64)


BALL_RANGE = 1 << 24      # |centre2[a]| and the diameter at most (include/och_gpu.h)


def _ball_args(centre2, diameter, who: str):
    """(centre2 as int32[3], diameter) of a ball, refused as the library refuses them."""
    try:
        c2 = list(centre2)
    except TypeError:
        raise ValueError(f"{who}: centre2 is three integers, not {centre2!r}") from None
    if len(c2) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in c2):
        raise ValueError(f"{who}: centre2 is three integers, not {centre2!r}")
    if isinstance(diameter, bool) or not isinstance(diameter, (int, np.integer)):
        raise ValueError(f"{who}: diameter is an integer, not {diameter!r}")
    if any(abs(int(v)) > BALL_RANGE for v in c2) or not 0 <= int(diameter) <= BALL_RANGE:
        raise ValueError(f"{who}: |centre2| and diameter are at most 2^24, diameter at least 0, not {centre2!r}, {diameter!r}")
    return (C.c_int32 * 3)(*(int(v) for v in c2)), int(diameter)


def sphere_records(centre2, diameter: int, id: int) -> np.ndarray:
    """The (n, 4) uint32 records (x, y, z, id) of a ball: the voxels (x, y, z) with
    (2x+1-centre2[0])^2 + (2y+1-centre2[1])^2 + (2z+1-centre2[2])^2 <= diameter^2 (centre2 is twice the
    centre, diameter counts voxels; all integers), those inside the ball's axis box
    ceil((centre2 - diameter - 1) / 2) <= (x, y, z) < floor((centre2 + diameter - 1) / 2) + 1, unclipped, in
    box_records' order: what World.fill_sphere is held to.  A coordinate below 0 wraps as box_records' do."""
    if isinstance(id, bool) or not isinstance(id, (int, np.integer)) or not 0 <= int(id) <= 0xFFFFFFFF:
        raise ValueError(f"sphere_records: id is an integer inside uint32, not {id!r}")
    c2, d = _ball_args(centre2, diameter, "sphere_records")
    c2 = np.array(c2[:], np.int64)
    lo, hi = (c2 - d) >> 1, ((c2 + d - 1) >> 1) + 1          # ceil((n - 1) / 2) = floor(n / 2)
    off = [(2 * np.arange(lo[a], max(hi[a], lo[a]), dtype=np.int64) + 1 - c2[a]) ** 2 for a in range(3)]
    z, y, x = np.nonzero(off[2][:, None, None] + off[1][None, :, None] + off[0][None, None, :] <= d * d)
    rec = np.empty((x.size, 4), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = (lo[0] + x).astype(np.uint32), (lo[1] + y).astype(np.uint32), (lo[2] + z).astype(np.uint32)
    rec[:, 3] = int(id)
    return rec


def sphere_cubes(centre2, diameter: int, depth: int):
    """The maximal aligned cubes of a ball (sphere_records says which voxels) clipped to a tree of `depth`
    (och_sphere_cubes, host only), in box_cubes' return shape: (keys, heights, cubes_per_height,
    cells_per_height).  What World.fill_sphere writes and rebuilds.  There are no closed forms: the counts
    come from the walk, whose cost follows the ball's surface."""
    c2, d = _ball_args(centre2, diameter, "sphere_cubes")
    cubes, cells, n = (C.c_uint64 * 22)(), (C.c_uint64 * 22)(), C.c_uint64()
    call("och_sphere_cubes", c2, d, int(depth), None, None, 0, cubes, cells, C.byref(n))
    keys, heights = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint8)
    if n.value:
        call("och_sphere_cubes", c2, d, int(depth), keys.ctypes.data, heights.ctypes.data, n.value, cubes, cells, C.byref(n))
    return keys, heights, np.array(cubes[:int(depth) + 1], np.uint64), np.array(cells[:int(depth) + 1], np.uint64)


def occupied_box(nodes: np.ndarray, root: int, depth: int, index_base: int = 1):
    """Bounding box of the pool's voxels (och_pool_occupied_box): (lo, hi) in
    voxel units, voxel (x, y, z) inside iff lo <= (x, y, z) < hi; lo = hi = 0
    for a pool without voxels.  The kernels' cull box (OCH_OPT_CULL)."""
    nodes, ptr, n = nodes_arg(nodes)
    lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    call("och_pool_occupied_box", ptr, n, int(root), int(depth), int(index_base), lo, hi)
    return tuple(lo), tuple(hi)


def pack_pool(nodes: np.ndarray, root: int, depth: int, index_base: int = 1):
    """The packed device layout of a pool (och_pool_pack): (packed nodes, packed root)."""
    nodes, ptr, n_nodes = nodes_arg(nodes)
    n, r = C.c_uint32(), C.c_uint32()
    call("och_pool_pack", ptr, n_nodes, int(root), int(depth), int(index_base), None, 0, C.byref(n), C.byref(r))
    out = np.zeros((n.value, 8), np.uint32)
    call("och_pool_pack", ptr, n_nodes, int(root), int(depth), int(index_base), out.ctypes.data, n.value, C.byref(n),
         C.byref(r))
    return out, r.value
