"""A world that stays on the GPU between brush strokes (och_world_* in include/och_gpu.h).

The demo's brush keys (ORT/test_och_h_octree.cpp:397-433) call ``tree.set`` 64 000 times and redraw;
here a stroke is ``world.edit(box_records(...))`` followed by ``world.flush(pool)`` before the next
frame.  Only the stroke's new nodes are made and published: the store is append-only, so frames in
flight stay valid and nothing of the pool travels to the host and back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import HostPool, OchError, call
from ._marshal import ScopedHandle, host_array, host_pool_result, nodes_arg, records_arg, struct_dict, u32_arg, when_arg
from .builder import VOXELS_GRID_U8, NodePool, _ball_args, _box_args, _capacity, _read_box_args
from .tracer import HOctree


class World(ScopedHandle):
    """A 1-based DAG resident on one GPU: edit() applies a record list as edit_voxels would, make_pool()
    and flush() show it, download() gives the canonical pool, compact() drops what strokes left behind;
    fill_box() and restore_box() set or restore a whole box at a cost that follows its surface;
    fill_sphere() and restore_sphere() do the same for a ball;
    paint_box() and paint_sphere() change only the voxels that are, or are not, one id (paint, fill-under, replace);
    at() and read_box() ask it what it holds without a download, tighten() makes its box exact;
    snapshot(), checkout() and release() remember and restore earlier states (UndoStack, below), diff()
    gives what changed between two of them."""
    _destroy = "och_world_destroy"

    def __init__(self, tree, capacity: int | None = None, device: int = -1):
        """tree is a NodePool with index_base 1 or a (nodes, root, depth) tuple in that form, as edit_voxels
        takes it (no nodes or root 0: an empty world to paint into).  capacity = node ids to reserve for the
        world's life, id 0 included; None = twice the reachable nodes + 64 * depth."""
        self._h = C.c_void_p()
        if isinstance(tree, NodePool):
            if tree.index_base != 1:
                raise OchError(-1, "och_world_create", "a pool with index_base 1 (h_octree form), not an och::octree pool")
            tree = (tree.nodes, tree.root, tree.depth)
        nodes, root, depth = tree
        nodes, ptr, n = nodes_arg(nodes, null_if_empty=True)
        if not 0 <= int(root) <= 0xFFFFFFFF:
            raise ValueError(f"World: root {root} outside uint32")
        self.depth = int(depth)
        call("och_world_create", ptr, n, int(root), self.depth,
             _capacity(capacity or 0, "World"), int(device), C.byref(self._h))
        self.device = self.info()["device"]

    @property
    def closed(self) -> bool:
        return not self._live()

    def _open(self, who: str):
        if self.closed:
            raise ValueError(f"World.{who}: the world is closed")
        return self._h

    def info(self) -> dict:
        """och_world_stats: capacity, used, root, depth, device, strokes, generation, box_lo, box_hi."""
        st = _lib.WorldStats()
        call("och_world_info", self._open("info"), C.byref(st))
        return struct_dict(st)

    def edit(self, records) -> None:
        """One stroke: an (n, 4) record list as edit_voxels takes it, a numpy array or a CUDA tensor
        (int32 / uint32) on the world's device.  OchError CAPACITY leaves the world unchanged:
        compact() and retry."""
        if getattr(records, "is_cuda", False):
            self._open("edit")                    # a closed world refuses before a device tensor is touched
        records, ptr, n, on_device = records_arg(records, "World.edit", device=self.device)
        call("och_world_edit", self._open("edit"), ptr, n, int(on_device))

    def make_pool(self) -> HOctree:
        """A device pool of the current world on the world's device (och_world_pool_create); the caller
        closes it.  It has no host mirror: update() and Editor.flush() on it raise OchError INVALID."""
        h = C.c_void_p()
        call("och_world_pool_create", self._open("make_pool"), C.byref(h))
        return HOctree._adopt(h, self.depth)

    def flush(self, pool) -> None:
        """Publish the strokes since this pool's last flush; complete on return."""
        call("och_world_flush", self._open("flush"), pool._h)

    def download(self) -> NodePool:
        """The canonical pool of the world's voxels with its statistics, as build_voxels / edit_voxels
        return it for the same content.  The world is unchanged."""
        hp = HostPool()
        call("och_world_download", self._open("download"), C.byref(hp))
        return NodePool(*host_pool_result(hp))

    def at(self, coords):
        """The voxels at (n, 3) coordinates (x, y, z) under the current root, unflushed strokes included
        (och_world_at); a coordinate outside the tree gives 0.  An integer array gives np.uint32 of shape
        (n,); an int32 CUDA tensor on the world's device is read where it lies and gives an int32 CUDA
        tensor holding the ids' bits.  Complete on return."""
        coords = host_array(coords)
        if hasattr(coords, "is_cuda"):
            import torch

            if coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int32:
                raise ValueError(f"World.at: device coordinates are an (n, 3) int32 tensor, not "
                                 f"{tuple(coords.shape)} {coords.dtype}")
            h = self._open("at")
            if coords.device.index != self.device:
                raise ValueError(f"World.at: the tensor is on {coords.device}, the world on device {self.device}")
            coords = coords.contiguous()
            ids = torch.empty(coords.shape[0], dtype=torch.int32, device=coords.device)
            torch.cuda.current_stream(coords.device).synchronize()       # the query reads on the world's stream
            call("och_world_at", h, coords.data_ptr(), coords.shape[0], ids.data_ptr(), 1)
            return ids
        coords = np.asarray(coords)
        if coords.ndim != 2 or coords.shape[1] != 3:
            raise ValueError(f"World.at: an (n, 3) coordinate list, not shape {coords.shape}")
        if coords.dtype.kind not in "iu":
            raise ValueError(f"World.at: coordinates are integers, not {coords.dtype}")
        if coords.dtype != np.int32:
            wide = coords.astype(np.int64) if coords.dtype != np.uint64 else coords
            if wide.size and (int(wide.min()) < -(1 << 31) or int(wide.max()) >= 1 << 31):
                raise ValueError("World.at: a coordinate outside int32")
            coords = wide.astype(np.int32)
        coords = np.ascontiguousarray(coords)
        ids = np.zeros(coords.shape[0], np.uint32)
        call("och_world_at", self._open("at"), coords.ctypes.data if coords.size else None, coords.shape[0],
             ids.ctypes.data if ids.size else None, 0)
        return ids

    def read_box(self, lo, hi, dtype=np.uint8, device: bool = False):
        """The voxels of the box lo <= (x, y, z) < hi under the current root as a dense (nz, ny, nx)
        array indexed [z, y, x] (och_world_read_box): NodePool.read_box of the download, byte for byte,
        without the download.  dtype is np.uint8 or np.uint32.  device=True leaves the grid on the
        world's device as a CUDA tensor (uint8, or int32 holding the ids' bits).  Complete on return."""
        lo, hi, shape, kind = _read_box_args(lo, hi, dtype, "World.read_box")
        h = self._open("read_box")
        if device:
            import torch

            dev = torch.device("cuda", self.device)
            grid = torch.empty(shape, dtype=torch.uint8 if kind == VOXELS_GRID_U8 else torch.int32, device=dev)
            target = grid if grid.numel() else torch.empty(1, dtype=grid.dtype, device=dev)
            torch.cuda.current_stream(dev).synchronize()                  # the allocation's stream before the world's
            call("och_world_read_box", h, lo, hi, kind, target.data_ptr(), grid.numel() * grid.element_size(), 1)
            return grid
        grid = np.zeros(shape, dtype)
        target = grid if grid.size else np.zeros(1, dtype)
        call("och_world_read_box", h, lo, hi, kind, target.ctypes.data, grid.nbytes, 0)
        return grid

    def tighten(self):
        """Make the world's box exact (och_world_tighten): (box_lo, box_hi), hi exclusive, both (0, 0, 0)
        for a world without voxels.  The next flush of each pool publishes it; later strokes grow it again."""
        call("och_world_tighten", self._open("tighten"))
        info = self.info()
        return info["box_lo"], info["box_hi"]

    def compact(self) -> None:
        """Drop what the root no longer reaches (och_world_compact): generation + 1, every pool is
        rewritten whole by its next flush."""
        call("och_world_compact", self._open("compact"))

    # -- history (och_world_snapshot / _checkout / _release / _snapshots / _diff)

    @staticmethod
    def _handle(s, who: str) -> int:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
            raise ValueError(f"World.{who}: a snapshot is an integer handle, not {type(s).__name__}")
        if not 0 <= int(s) < 1 << 64:
            raise ValueError(f"World.{who}: handle {s} outside uint64")
        return int(s)

    def snapshot(self) -> int:
        """Remember the current root: a handle (1, 2, ... per world, never reused) that checkout() and
        diff() take, live until release() or close().  O(1); compact() keeps what live snapshots reach."""
        s = C.c_uint64()
        call("och_world_snapshot", self._open("snapshot"), C.byref(s))
        return s.value

    def checkout(self, s: int) -> None:
        """Make snapshot s the current state again (undo / redo): root, mask and the box the world had
        then.  O(1), nothing is launched; flush() publishes it.  Strokes afterwards branch off."""
        h = self._open("checkout")
        call("och_world_checkout", h, self._handle(s, "checkout"))

    def release(self, s: int) -> None:
        """Forget snapshot s; what only it reached goes with the next compact()."""
        h = self._open("release")
        call("och_world_release", h, self._handle(s, "release"))

    def snapshots(self) -> list:
        """The live handles in ascending order."""
        h = self._open("snapshots")
        n = _lib._u32()
        call("och_world_snapshots", h, None, 0, C.byref(n))
        ids = (C.c_uint64 * max(n.value, 1))()
        call("och_world_snapshots", h, ids, n.value, C.byref(n))
        return [int(v) for v in ids[:n.value]]

    def diff(self, a: int, b: int = 0, device: bool = False, records: bool = True):
        """The voxels that differ between snapshots a and b (0: the current state), as (records, stats)
        (och_world_diff): NodePool.diff of the two downloads without a download, at a cost that follows
        the change.  records is an (n, 4) np.uint32 array of (x, y, z, id under b) in ascending Morton
        order, id 0 where the voxel is gone -- what edit() takes to turn a's content into b's; with
        device=True an int32 CUDA tensor on the world's device holding the same bits; with records=False
        None.  stats is {"n", "pairs", "box_lo", "box_hi"}.  Complete on return."""
        h = self._open("diff")
        a, b = self._handle(a, "diff"), self._handle(b, "diff")
        st = _lib.DiffStats()
        call("och_world_diff", h, a, b, None, 0, 0, C.byref(st))      # the summary sizes the output
        if not records:
            return None, struct_dict(st)
        n = int(st.n)
        if device:
            import torch

            dev = torch.device("cuda", self.device)
            out = torch.empty((n, 4), dtype=torch.int32, device=dev)
            if n:
                torch.cuda.current_stream(dev).synchronize()              # the allocation's stream before the world's
                call("och_world_diff", h, a, b, out.data_ptr(), n, 1, C.byref(st))
            return out, struct_dict(st)
        out = np.zeros((n, 4), np.uint32)
        if n:
            call("och_world_diff", h, a, b, out.ctypes.data, n, 0, C.byref(st))
        return out, struct_dict(st)

    # -- regions (och_world_fill_box / och_world_restore_box)

    def fill_box(self, lo, hi, id: int) -> dict:
        """One stroke: every voxel of the box lo <= (x, y, z) < hi becomes id (0 removes), as
        edit(box_records(lo, hi, id)) would leave the world, without a record (och_world_fill_box): a cube of
        side 2^h inside the box is one child word, only the cells that straddle its faces get new nodes.
        The part of the box outside the tree is ignored.  Returns {"cubes", "cells", "new_ids", "lo", "hi"}:
        box_cubes' two totals, the ids consumed and the clipped box.  OchError CAPACITY leaves the world
        unchanged: compact() and retry."""
        h = self._open("fill_box")
        lo, hi = _box_args(lo, hi, "World.fill_box")
        if isinstance(id, bool) or not isinstance(id, (int, np.integer)) or not 0 <= int(id) <= 0xFFFFFFFF:
            raise ValueError(f"World.fill_box: id is an integer inside uint32, not {id!r}")
        st = _lib.RegionStats()
        call("och_world_fill_box", h, lo, hi, int(id), C.byref(st))
        return struct_dict(st)

    def restore_box(self, s: int, lo, hi) -> dict:
        """One stroke: inside the box the content of snapshot s, outside it the current content
        (och_world_restore_box): undo for a region.  The cost follows what differs inside the box.  Returns
        fill_box's dict; cubes and cells count only what differs."""
        h = self._open("restore_box")
        s = self._handle(s, "restore_box")
        lo, hi = _box_args(lo, hi, "World.restore_box")
        st = _lib.RegionStats()
        call("och_world_restore_box", h, s, lo, hi, C.byref(st))
        return struct_dict(st)

    # -- balls (och_world_fill_sphere / och_world_restore_sphere)

    def fill_sphere(self, centre2, diameter: int, id: int) -> dict:
        """One stroke: every voxel of the ball becomes id (0 removes), as edit(sphere_records(centre2,
        diameter, id)) would leave the world, without a record (och_world_fill_sphere).  centre2 is twice the
        centre in voxels, diameter counts voxels, both integers; sphere_records says which voxels those are.
        Returns fill_box's dict: sphere_cubes' two totals, the ids consumed and the ball's clipped axis box."""
        h = self._open("fill_sphere")
        c2, d = _ball_args(centre2, diameter, "World.fill_sphere")
        if isinstance(id, bool) or not isinstance(id, (int, np.integer)) or not 0 <= int(id) <= 0xFFFFFFFF:
            raise ValueError(f"World.fill_sphere: id is an integer inside uint32, not {id!r}")
        st = _lib.RegionStats()
        call("och_world_fill_sphere", h, c2, d, int(id), C.byref(st))
        return struct_dict(st)

    def restore_sphere(self, s: int, centre2, diameter: int) -> dict:
        """One stroke: inside the ball the content of snapshot s, outside it the current content
        (och_world_restore_sphere): restore_box for a round brush.  Returns fill_box's dict; cubes and cells
        count only what differs."""
        h = self._open("restore_sphere")
        s = self._handle(s, "restore_sphere")
        c2, d = _ball_args(centre2, diameter, "World.restore_sphere")
        st = _lib.RegionStats()
        call("och_world_restore_sphere", h, s, c2, d, C.byref(st))
        return struct_dict(st)

    # -- conditional strokes (och_world_paint_box / och_world_paint_sphere)

    def paint_box(self, lo, hi, id: int, when: int = _lib.WHEN_IS_NOT, match: int = 0) -> dict:
        """One stroke: inside the box lo <= (x, y, z) < hi a voxel v becomes id where v != match (when =
        WHEN_IS_NOT) or v == match (WHEN_IS), and stays otherwise, as edit(select_records(...)) of the box's
        grid would leave the world, without reading it (och_world_paint_box).  The defaults paint the solid
        voxels; (WHEN_IS, 0) fills only the empty ones; (WHEN_IS, m) replaces material m, with id 0 erases
        it; (WHEN_IS_NOT, m) with id 0 keeps only m.  The cost follows the box's surface and the distinct
        nodes under it.  Returns {"cubes", "cells", "nodes", "new_ids", "lo", "hi"}.  OchError CAPACITY
        leaves the world unchanged: compact() and retry."""
        h = self._open("paint_box")
        lo, hi = _box_args(lo, hi, "World.paint_box")
        id, match = u32_arg(id, "World.paint_box", "id"), u32_arg(match, "World.paint_box", "match")
        when = when_arg(when, "World.paint_box")
        st = _lib.PaintStats()
        call("och_world_paint_box", h, lo, hi, when, match, id, C.byref(st))
        return struct_dict(st)

    def paint_sphere(self, centre2, diameter: int, id: int, when: int = _lib.WHEN_IS_NOT, match: int = 0) -> dict:
        """paint_box for a round brush (och_world_paint_sphere): centre2 and diameter as fill_sphere takes
        them, the predicate and the returned dict as paint_box'."""
        h = self._open("paint_sphere")
        c2, d = _ball_args(centre2, diameter, "World.paint_sphere")
        id, match = u32_arg(id, "World.paint_sphere", "id"), u32_arg(match, "World.paint_sphere", "match")
        when = when_arg(when, "World.paint_sphere")
        st = _lib.PaintStats()
        call("och_world_paint_sphere", h, c2, d, when, match, id, C.byref(st))
        return struct_dict(st)


class UndoStack:
    """Undo and redo over a World's snapshots.  The stack snapshots the world as it is when made;
    push() after every stroke.  undo() and redo() are checkouts (O(1); flush() shows them) and return
    whether they moved.  A push after an undo releases the abandoned branch; beyond `limit` entries
    the oldest is released."""

    def __init__(self, world: World, limit: int = 64):
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 2:
            raise ValueError(f"UndoStack: limit is an integer of at least 2 (a state to go back to), not {limit!r}")
        self.world, self.limit = world, int(limit)
        self._entries = [world.snapshot()]
        self._at = 0

    @property
    def entries(self) -> list:
        """The stack's handles, oldest first."""
        return list(self._entries)

    @property
    def current(self) -> int:
        return self._entries[self._at]

    def push(self) -> int:
        """Remember the world as it is now, after a stroke; the new handle."""
        s = self.world.snapshot()
        for dead in self._entries[self._at + 1:]:
            self.world.release(dead)
        del self._entries[self._at + 1:]
        self._entries.append(s)
        while len(self._entries) > self.limit:
            self.world.release(self._entries.pop(0))
        self._at = len(self._entries) - 1
        return s

    def undo(self) -> bool:
        if self._at == 0:
            return False
        self.world.checkout(self._entries[self._at - 1])
        self._at -= 1
        return True

    def redo(self) -> bool:
        if self._at + 1 >= len(self._entries):
            return False
        self.world.checkout(self._entries[self._at + 1])
        self._at += 1
        return True
