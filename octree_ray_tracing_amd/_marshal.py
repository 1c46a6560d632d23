"""The marshalling steps of the wrappers over the C ABI, each said once.

tracer, frame, builder, world and editor turn Python values into what include/och_gpu.h takes
(a camera array, a node table, a record list) and what it fills in back
into Python values (a stats struct, a host pool).  A step that more than one wrapper needs lives
here or nowhere: a size rule of the ABI that changes is changed in this file.  Nothing here
launches anything; torch is imported only where a device tensor is at hand.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import Camera, call


# -- device buffers

def _dev_ptr(t) -> int:
    """Device pointer of a torch tensor (or an int already)."""
    if isinstance(t, int):
        return t
    if not t.is_cuda:
        raise ValueError("expected a device tensor")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return t.data_ptr()


def _nbytes(t):
    """The bytes a tensor holds; None for a raw pointer, whose size nobody here knows."""
    if hasattr(t, "numel") and hasattr(t, "element_size"):
        return t.numel() * t.element_size()
    return None


def _need(t, nbytes: int, what: str):
    """A device buffer passed as a tensor must hold what the launch writes or
    reads: the C ABI takes bare pointers (as the reference's interface takes
    references), so the sizes are checked here.  Raw pointers pass unchecked."""
    have = _nbytes(t)
    if have is not None and have < nbytes:
        raise ValueError(f"{what}: the buffer holds {have} B, the launch needs {nbytes} B")


def capacity_of(buf, bytes_per_pixel: int, given) -> int:
    """The capacity_pixels argument of a render entry: what the caller gave, else what the tensor holds."""
    if given is not None:
        return int(given)
    if _nbytes(buf) is None:
        raise ValueError("a raw pointer needs capacity_pixels")
    return _nbytes(buf) // bytes_per_pixel


# -- cameras

def views(cams):
    """One camera or a list of equal-size ones as (pointer to the och_camera array, n, first camera).
    The pointer keeps the array alive."""
    cams = cams if isinstance(cams, (list, tuple)) else [cams]
    arr = (Camera * len(cams))(*cams)
    return C.cast(arr, C.c_void_p), len(cams), cams[0] if cams else None


# -- host tables

def nodes_arg(nodes, null_if_empty: bool = False):
    """A node table as (the (n, 8) uint32 array to keep alive, its address, n); null_if_empty: no rows
    are passed as NULL."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    return nodes, None if null_if_empty and not nodes.size else nodes.ctypes.data, nodes.shape[0]


def palette_arg(rgba):
    """A palette as (array to keep alive, its address, voxel ids): 6 colours per id."""
    rgba = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
    if rgba.size % 6:
        raise ValueError("palette must hold 6 colours per voxel id")
    return rgba, rgba.ctypes.data, rgba.size // 6


def rcp_lut_arg(lut):
    """An RCPPS table as (array to keep alive, its address, log2 of its entries)."""
    lut = np.ascontiguousarray(lut, np.uint32)
    return lut, lut.ctypes.data, int(round(math.log2(lut.size)))


# -- voxel records

def host_array(x):
    """A CPU torch tensor is host memory: numpy's view of it.  Anything else as it is."""
    return x.numpy() if hasattr(x, "is_cuda") and not x.is_cuda else x


def records_arg(voxels, who: str, device: int | None = None, use_gpu: bool = True):
    """An (n, 4) record list as (what to keep alive, address, n, on_device).  A numpy array (or a CPU
    tensor) is host memory, of any integer width.  A CUDA tensor (int32 / uint32) is read where it lies:
    it must be on `device` (None: the current device), the callee must be using the GPU, and its writes
    are complete on return, because the callee reads on a stream of its own."""
    voxels = host_array(voxels)
    if not hasattr(voxels, "is_cuda"):
        voxels = np.asarray(voxels)
        if voxels.ndim != 2 or voxels.shape[1] != 4:
            raise ValueError(f"{who}: an (n, 4) record list, not shape {voxels.shape}")
        if voxels.dtype.kind not in "iu":
            raise ValueError(f"{who}: records are integers, not {voxels.dtype}")
        if voxels.dtype.itemsize != 4:
            wide = voxels.astype(np.int64)
            if wide.size and not (0 <= wide[:, 3].min() and wide[:, 3].max() <= 0xFFFFFFFF):
                raise ValueError(f"{who}: a voxel id outside uint32")
            outside = ((wide[:, :3] < 0) | (wide[:, :3] > 0xFFFFFFFF)).any(axis=1)
            wide[outside, :3] = 0xFFFFFFFF         # outside any tree: ignored
            voxels = wide.astype(np.uint32)
        voxels = np.ascontiguousarray(voxels).view(np.uint32)
        return voxels, voxels.ctypes.data, voxels.shape[0], False
    if not use_gpu:
        raise ValueError(f"{who}: a device tensor needs use_gpu=True")
    import torch

    if voxels.dim() != 2 or voxels.shape[1] != 4 or voxels.dtype not in (torch.int32, torch.uint32):
        raise ValueError(f"{who}: a device list is an (n, 4) int32 / uint32 tensor, not "
                         f"{tuple(voxels.shape)} {voxels.dtype}")
    want = torch.cuda.current_device() if device is None else device
    if voxels.device.index != want:
        where = f"the current device is {want}" if device is None else f"the world on device {want}"
        raise ValueError(f"{who}: the tensor is on {voxels.device}, {where}")
    voxels = voxels.contiguous()
    torch.cuda.current_stream(voxels.device).synchronize()
    return voxels, voxels.data_ptr(), voxels.shape[0], True


def u32_arg(v, who: str, what: str) -> int:
    """A voxel id (or another uint32 argument) as an int; a bool, a float or a value outside uint32 is refused."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFFFFFF:
        raise ValueError(f"{who}: {what} is an integer inside uint32, not {v!r}")
    return int(v)


def when_arg(when, who: str) -> int:
    """The predicate of a conditional stroke: WHEN_IS (0) or WHEN_IS_NOT (1)."""
    if isinstance(when, bool) or not isinstance(when, (int, np.integer)) or int(when) not in (0, 1):
        raise ValueError(f"{who}: when is WHEN_IS (0) or WHEN_IS_NOT (1), not {when!r}")
    return int(when)


def select_records(grid, origin, id, when, match, mask=None) -> np.ndarray:
    """The records of a conditional stroke, on the host: (x, y, z, id) for every voxel v of a dense grid
    (indexed [z, y, x], read_box's layout, its lo as `origin`) with v == match (WHEN_IS) or v != match
    (WHEN_IS_NOT), optionally only where the boolean `mask` of the grid's shape holds.  An (n, 4) np.uint32
    array in the grid's own order; a coordinate below 0 wraps as box_records' do.  What World.paint_box
    and paint_sphere are held to: edit() of these records leaves the same world."""
    id = u32_arg(id, "select_records", "id")
    match = u32_arg(match, "select_records", "match")
    when = when_arg(when, "select_records")
    grid = np.asarray(host_array(grid))
    if grid.ndim != 3 or grid.dtype.kind not in "iu":
        raise ValueError(f"select_records: a dense (nz, ny, nx) integer grid, not shape {grid.shape} {grid.dtype}")
    origin = [int(v) for v in origin]
    if len(origin) != 3:
        raise ValueError(f"select_records: origin is (x, y, z), not {origin!r}")
    hit = (grid.astype(np.int64) & 0xFFFFFFFF == match) != bool(when)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != grid.shape or mask.dtype != np.bool_:
            raise ValueError(f"select_records: mask is a boolean array of the grid's shape {grid.shape}, not "
                             f"{mask.shape} {mask.dtype}")
        hit &= mask
    z, y, x = np.nonzero(hit)
    out = np.empty((x.size, 4), np.int64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x + origin[0], y + origin[1], z + origin[2], id
    return (out & 0xFFFFFFFF).astype(np.uint32)


# -- what the library fills in

def struct_dict(st) -> dict:
    """A stats struct as a dict in field order: an array field as a tuple."""
    out = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        out[name] = tuple(v) if isinstance(v, C.Array) else v
    return out


def host_pool_result(hp) -> tuple:
    """NodePool's fields from an och_host_pool the library filled: the nodes are copied and the
    library's buffer is freed, whatever happens."""
    try:
        n = hp.n_nodes
        arr = np.ctypeslib.as_array(hp.nodes, shape=(n * 8,)).reshape(n, 8).copy()
    finally:
        call("och_host_pool_free", C.byref(hp))
    return arr, hp.root, hp.depth, hp.index_base, hp.solid_voxels, list(hp.voxel_hist), hp.tree_nodes, hp.build_seconds


# -- handles

class Handle:
    """The owner of one library object: `_h` (a c_void_p, NULL once closed) and `_destroy`, the name of
    the entry that frees it.  close() may be called twice; __del__ closes and swallows."""
    _destroy: str

    def _live(self) -> bool:
        return bool(getattr(self, "_h", None) and self._h.value)

    def close(self):
        if self._live():
            call(self._destroy, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScopedHandle(Handle):
    """A Handle that a with-statement closes."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
