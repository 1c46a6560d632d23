"""Host-side mirror of the reference's tracer interface over the C ABI.

Reference (ORT/ = Octree_Ray_Tracing/):
  och::h_octree<L, D>::sse_trace(ox, oy, oz, dx, dy, dz, dir&, voxel&, t&)   ORT/och_h_octree.h:292-452
  och::octree::sse_trace(...)                                              ORT/och_octree.cpp:167-325
  tree_camera::update_position / trace_pixel                               ORT/test_och_h_octree.cpp:64-138
  tree_window::update_image                                                ORT/test_och_h_octree.cpp:437-457

`HOctree` / `Octree` wrap a device-resident node pool (`och_gpu_pool`).  Every
compute call runs the gfx950 kernels in liboch_gpu.so; nothing here computes
a hit on the CPU.
"""
from __future__ import annotations

import ctypes as C
import enum
import math

import numpy as np

from . import _lib
from ._lib import Camera, Light, OchError, call
from ._marshal import (ScopedHandle, _dev_ptr, _need, capacity_of, nodes_arg, palette_arg, rcp_lut_arg, struct_dict,
                       views)


class Direction(enum.IntEnum):
    """och::direction (ORT/och_tree_helper.h:7-18)."""
    x_pos = 0
    y_pos = 1
    z_pos = 2
    x_neg = 3
    y_neg = 4
    z_neg = 5
    exit = 6
    inside = 7
    error = 8


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _event_handle(e):
    """A hipEvent_t as an int: a raw handle, a ctypes c_void_p, or an object with ``h``."""
    if e is None:
        return None
    h = getattr(e, "h", e)
    return h.value if hasattr(h, "value") else int(h)


def host_rcp_lut() -> np.ndarray:
    """This host's RCPPS (_mm_rcp_ps, ORT/och_h_octree.h:316) as a 2^k table."""
    buf = np.empty(1 << 23, np.uint32)
    k = C.c_int()
    call("och_host_rcp_lut", _np_ptr(buf), C.byref(k))
    return buf[: 1 << k.value].copy()


def rcp_from_lut(xbits: int, lut: np.ndarray) -> int:
    lut, ptr, log2_entries = rcp_lut_arg(lut)
    return call("och_rcp_from_lut", xbits, ptr, log2_entries)


def rcp_lut_error(lut: np.ndarray) -> float:
    """Largest relative error of an RCPPS table over [-2, -1) (och_rcp_lut_error)."""
    lut, ptr, log2_entries = rcp_lut_arg(lut)
    e = C.c_double()
    call("och_rcp_lut_error", ptr, log2_entries, C.byref(e))
    return e.value


def device_list() -> list[int]:
    """HIP indices of the visible gfx950 devices (och_device_list)."""
    n = C.c_int()
    call("och_device_list", None, 0, C.byref(n))
    arr = (C.c_int * max(n.value, 1))()
    call("och_device_list", C.cast(arr, C.c_void_p), n.value, C.byref(n))
    return list(arr[:n.value])


def device_count() -> int:
    n = C.c_int()
    call("och_device_count", C.byref(n))
    return n.value


def camera(pos=(1.5, 1.5, 1.5), yaw: float = 0.0, pitch: float = 0.0, fov: float = 1.25,
           width: int = 640, height: int = 360) -> Camera:
    """tree_camera state -> per-frame uniforms (ORT/test_och_h_octree.cpp:53-55, :87-115).
    yaw = camera.dir.x, pitch = camera.dir.y."""
    cam = Camera()
    call("och_camera_setup", float(pos[0]), float(pos[1]), float(pos[2]), float(yaw), float(pitch),
         float(fov), int(width), int(height), C.byref(cam))
    return cam


def light_check(light: Light) -> None:
    """Raises OchError (OCH_E_INVALID) for a light a lit render would refuse (och_light_check, host only)."""
    call("och_light_check", C.byref(light))


class GpuPool(ScopedHandle):
    """A node pool resident in HBM on one device, traced by the gfx950 kernels."""
    _destroy = "och_gpu_pool_destroy"

    def __init__(self, nodes: np.ndarray, root: int, depth: int, index_base: int = 1,
                 miss_t: float | None = None, device: int = -1):
        nodes, ptr, n = nodes_arg(nodes)
        if miss_t is None:
            miss_t = math.inf if index_base == 1 else 0.0
        self.depth, self.index_base, self.miss_t = int(depth), int(index_base), float(miss_t)
        self._h = C.c_void_p()
        call("och_gpu_pool_create", ptr, n, int(root), int(depth),
             int(index_base), float(miss_t), int(device), C.byref(self._h))
        self._palette_n = 0

    @classmethod
    def _adopt(cls, handle, depth: int, index_base: int = 1, miss_t: float = math.inf):
        """The Python side of a pool the library made itself (World.make_pool); it owns the handle."""
        pool = cls.__new__(cls)
        pool.depth, pool.index_base, pool.miss_t = int(depth), int(index_base), float(miss_t)
        pool._h = handle
        pool._palette_n = 0
        return pool

    # -- configuration
    def info(self) -> dict:
        inf = _lib.PoolInfo()
        call("och_gpu_pool_info", self._h, C.byref(inf))
        return struct_dict(inf)

    def get_root(self) -> int:
        return self.info()["root"]

    def set_rcp_lut(self, lut: np.ndarray):
        if np.size(lut) < 2 or np.size(lut) & (np.size(lut) - 1):
            raise ValueError("RCPPS table size must be a power of two")
        lut, ptr, log2_entries = rcp_lut_arg(lut)
        call("och_gpu_set_rcp_lut", self._h, ptr, log2_entries)

    def set_palette(self, rgba: np.ndarray):
        rgba, ptr, n = palette_arg(rgba)
        call("och_gpu_set_palette", self._h, ptr, n)
        self._palette_n = n

    def set_stream(self, stream):
        """Enqueue _dev work on a caller stream (torch.cuda.Stream or raw handle)."""
        handle = getattr(stream, "cuda_stream", stream)
        call("och_gpu_set_stream", self._h, C.c_void_p(handle))

    def update(self, first: int, nodes: np.ndarray, root: int):
        nodes, ptr, n = nodes_arg(nodes)
        call("och_gpu_pool_update", self._h, int(first), n, ptr, int(root))

    # och_option (include/och_gpu.h); ids 0, 2, 3, 7, 9, 12, 13 were retired arms
    OPTIONS = {"block": 1, "layout": 4, "tile_order": 5, "bounce_compact": 6, "cull": 8, "timing": 10, "plan": 11,
               "split": 14, "split_segs": 15, "split_level": 16}
    READ_ONLY = {"split_tiles": 17}

    def set_option(self, name: str, value: int):
        """Launch options (och_gpu_set_option): block, layout, tile_order, bounce_compact, cull
        (1 = rays proven to miss the voxels' bounding box skip the walk; exact), timing, plan."""
        call("och_gpu_set_option", self._h, self.OPTIONS[name], int(value))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        call("och_gpu_get_option", self._h, self.OPTIONS.get(name) or self.READ_ONLY[name], C.byref(v))
        return v.value

    def set_stamp_buffer(self, stamps, capacity_waves: int):
        """Per-wave residency records (diagnostics); stamps = device int64 tensor or None."""
        call("och_gpu_set_stamp_buffer", self._h, None if stamps is None else _dev_ptr(stamps), int(capacity_waves))

    def occupancy(self, kind: int = 0) -> int:
        """HIP's workgroups-per-CU answer: 0 render grid, 2 trace grid."""
        v = C.c_int()
        call("och_gpu_occupancy", self._h, int(kind), C.byref(v))
        return v.value

    def synchronize(self):
        call("och_gpu_synchronize", self._h)

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        call("och_gpu_last_kernel_ms", self._h, C.byref(ms))
        return ms.value

    def set_launch_events(self, start, stop):
        """The next trace/render launch records these HIP events (raw hipEvent_t
        handles, or objects with an ``h`` handle) through its own dispatch."""
        call("och_gpu_set_launch_events", self._h, _event_handle(start), _event_handle(stop))

    # -- tracing (reference signature)
    def sse_trace(self, ox, oy, oz, dx, dy, dz):
        """h_octree::sse_trace: returns (Direction, voxel, t)."""
        d, v, t = C.c_int32(), C.c_uint32(), C.c_float()
        call("och_gpu_trace", self._h, float(ox), float(oy), float(oz), float(dx), float(dy), float(dz),
             C.byref(d), C.byref(v), C.byref(t))
        return Direction(d.value), v.value, t.value

    def trace_batch(self, origins, dirs, width: int | None = None):
        """Host arrays in, host arrays out (synchronous).  origins (3,) or (n,3).
        width: the rays are a row-major image that many rays wide (a camera's
        rays, x + y * W): traced 8x8 tiles per wave (och_gpu_trace_batch_image)."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        origins = np.ascontiguousarray(origins, np.float32)
        stride = 0 if origins.size == 3 else 3
        n = dirs.shape[0]
        hd, hv, ht = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n, np.float32)
        if width:
            call("och_gpu_trace_batch_image", self._h, _np_ptr(origins), stride, _np_ptr(dirs), n, int(width),
                 _np_ptr(hd), _np_ptr(hv), _np_ptr(ht))
        else:
            call("och_gpu_trace_batch", self._h, _np_ptr(origins), stride, _np_ptr(dirs), n,
                 _np_ptr(hd), _np_ptr(hv), _np_ptr(ht))
        return hd, hv, ht

    def trace_batch_dev(self, origins, dirs, hit_dir, hit_voxel, hit_time, push=None, n=None):
        """Device buffers (torch tensors), asynchronous on the pool's stream."""
        self._batch("och_gpu_trace_batch_dev", origins, dirs, n, (), (hit_dir, hit_voxel, hit_time), push)

    def trace_batch_tiled_dev(self, origins, dirs, width: int, hit_dir, hit_voxel, hit_time, push=None, n=None):
        """trace_batch_dev for rays laid out as a row-major image `width` wide: one 8x8 tile of
        neighbouring rays per wavefront (och_gpu_trace_batch_tiled_dev); records in the caller's order."""
        self._batch("och_gpu_trace_batch_tiled_dev", origins, dirs, n, (int(width),), (hit_dir, hit_voxel, hit_time),
                    push)

    def plan_batch_tiled(self, origins, dirs, width: int, n=None):
        """Plan the launch order of tiled batches of this geometry (och_gpu_plan_batch_tiled); used with
        set_option("tile_order", 2).  Synchronous."""
        self._batch("och_gpu_plan_batch_tiled", origins, dirs, n, (int(width),))

    def trace_bounce_batch_dev(self, origins, dirs, hit_dir, hit_voxel, hit_time, bounce_dir, bounce_voxel,
                               bounce_time, push=None, n=None):
        """Config 5: primary + one mirrored secondary ray per hit (device tensors, async)."""
        self._batch("och_gpu_trace_bounce_batch_dev", origins, dirs, n, (),
                    (hit_dir, hit_voxel, hit_time, bounce_dir, bounce_voxel, bounce_time), push)

    def _batch(self, name, origins, dirs, n, width, records=None, push=None):
        """A batch entry's call: n rays (default: what dirs holds) from one shared origin (stride 0) or one
        each, `width` spliced in where the entry takes one; records: the buffers the launch writes, followed
        by push (None: no such buffer), for an entry that has them."""
        if n is None:
            n = dirs.numel() // 3
        stride = 0 if origins.numel() == 3 else 3
        outs = ()
        if records is not None:
            self._need_batch(origins, dirs, n, stride, (*records, push))
            outs = (*[_dev_ptr(r) for r in records], None if push is None else _dev_ptr(push))
        call(name, self._h, _dev_ptr(origins), stride, _dev_ptr(dirs), int(n), *width, *outs)

    @staticmethod
    def _need_batch(origins, dirs, n, stride, outs):
        _need(origins, 12 * (int(n) if stride else 1), "origins")
        _need(dirs, 12 * int(n), "dirs")
        for o in outs:
            if o is not None:
                _need(o, 4 * int(n), "hit records")

    @staticmethod
    def _frame_views(cams, row_chunk):
        """views(cams) and the row chunk, by default the whole frame as one chunk."""
        arr, n, first = views(cams)
        return arr, n, first, int(first.height if row_chunk is None else row_chunk)

    def _need_frames(self, buf, n, first, row_chunk, n_shards, bytes_per_pixel, what):
        """A shard's slices hold whole row chunks: n views of slice_rows rows each."""
        _need(buf, n * self.slice_rows(first.height, row_chunk, int(n_shards)) * first.width * bytes_per_pixel, what)

    # -- frame path
    def raygen_dev(self, cam: Camera, dirs):
        _need(dirs, 12 * cam.width * cam.height, "dirs")
        call("och_gpu_raygen_dev", self._h, C.byref(cam), _dev_ptr(dirs))

    def render(self, cam: Camera) -> np.ndarray:
        """update_position + update_image: RGBA8 (olc::Pixel) frame, H x W uint32."""
        out = np.empty((cam.height, cam.width), np.uint32)
        call("och_gpu_render", self._h, C.byref(cam), _np_ptr(out))
        return out

    def render_dev(self, cam: Camera, rgba_slice, row_chunk: int | None = None, shard: int = 0,
                   n_shards: int = 1):
        row_chunk = int(cam.height if row_chunk is None else row_chunk)
        self._need_frames(rgba_slice, 1, cam, row_chunk, n_shards, 4, "rgba_slice")
        call("och_gpu_render_dev", self._h, C.byref(cam), _dev_ptr(rgba_slice), row_chunk,
             int(shard), int(n_shards))

    def render_views_dev(self, cams, rgba_slices, row_chunk: int | None = None, shard: int = 0, n_shards: int = 1):
        """Several equal-size cameras in one launch; rgba_slices holds the views' slices back to back."""
        self._plain_views("och_gpu_render_views_dev", cams, rgba_slices, 4, "rgba_slices", row_chunk, shard, n_shards)

    def _plain_views(self, name, cams, buf, bytes_per_pixel, what, row_chunk, shard, n_shards, *bounce):
        arr, n, first, row_chunk = self._frame_views(cams, row_chunk)
        self._need_frames(buf, n, first, row_chunk, n_shards, bytes_per_pixel, what)
        call(name, self._h, arr, n, _dev_ptr(buf), row_chunk, int(shard), int(n_shards), *bounce)

    def render_ssaa(self, cam: Camera, s: int) -> np.ndarray:
        """The frame of `cam` (the sample grid's camera: width and height multiples of s = 2, 4 or 8)
        supersampled s x s: (H / s, W / s) uint32, each byte the rounded mean of its block's samples
        (och_gpu_render_ssaa; frame.box_downsample states the definition on the host)."""
        return self._ssaa("och_gpu_render_ssaa", cam, None, s)

    def _ssaa(self, name, cam, light, s):
        s = int(s)
        out = np.empty((cam.height // s, cam.width // s) if s > 0 else (0, 0), np.uint32)
        call(name, self._h, C.byref(cam), *self._lit(light), s, _np_ptr(out), out.size)
        return out

    @staticmethod
    def _lit(light) -> tuple:
        """The light a lit entry takes after its cameras, spliced into the unlit entry's arguments."""
        return () if light is None else (C.byref(light),)

    def render_ssaa_views_dev(self, cams, s: int, rgba, capacity_pixels: int | None = None):
        """Several equal-size sample-grid cameras supersampled s x s in one launch (och_gpu_render_ssaa_views_dev):
        rgba (a device tensor of 4-byte words, or a raw pointer with capacity_pixels) receives the views'
        (H / s) x (W / s) frames back to back.  Asynchronous on the pool's stream."""
        self._ssaa_views("och_gpu_render_ssaa_views_dev", cams, None, s, rgba, capacity_pixels)

    def _ssaa_views(self, name, cams, light, s, rgba, capacity_pixels):
        arr, n, first = views(cams)
        s = int(s)
        if s in (2, 4, 8) and n:                 # any other s the library refuses before it touches rgba
            _need(rgba, 4 * n * (first.width // s) * (first.height // s), "rgba")
        capacity_pixels = capacity_of(rgba, 4, capacity_pixels)
        call(name, self._h, arr, n, *self._lit(light), s, _dev_ptr(rgba), capacity_pixels)

    def render_lit(self, cam: Camera, light: Light) -> np.ndarray:
        """The frame of `cam` with every face hit shaded by sun shadow and ambient occlusion
        (och_gpu_render_lit; frame.shade_lit states the shade on the host): H x W uint32."""
        out = np.empty((cam.height, cam.width), np.uint32)
        call("och_gpu_render_lit", self._h, C.byref(cam), C.byref(light), _np_ptr(out), out.size)
        return out

    def _lit_views(self, name, cams, light, buf, bytes_per_pixel, capacity_pixels, row_chunk, shard, n_shards):
        arr, n, first, row_chunk = self._frame_views(cams, row_chunk)
        self._need_frames(buf, n, first, row_chunk, n_shards, bytes_per_pixel, name)
        capacity_pixels = capacity_of(buf, bytes_per_pixel, capacity_pixels)
        call(name, self._h, arr, n, C.byref(light), _dev_ptr(buf), capacity_pixels, row_chunk, int(shard),
             int(n_shards))

    def render_lit_views_dev(self, cams, light: Light, rgba_slices, capacity_pixels: int | None = None,
                             row_chunk: int | None = None, shard: int = 0, n_shards: int = 1):
        """render_views_dev's slices, lit (och_gpu_render_lit_views_dev): rgba_slices is a device tensor of
        4-byte words, or a raw pointer with capacity_pixels.  Asynchronous on the pool's stream."""
        self._lit_views("och_gpu_render_lit_views_dev", cams, light, rgba_slices, 4, capacity_pixels, row_chunk, shard,
                        n_shards)

    def render_lit_masks_views_dev(self, cams, light: Light, mask_slices, capacity_pixels: int | None = None,
                                   row_chunk: int | None = None, shard: int = 0, n_shards: int = 1):
        """The lit frame's mask bytes, one per pixel, laid out as the RGBA8 slices
        (och_gpu_render_lit_masks_views_dev): bits 0..3 AO ray k occluded, bit 4 shadowed, bit 5
        self-shadowed, 0x80 not a face hit."""
        self._lit_views("och_gpu_render_lit_masks_views_dev", cams, light, mask_slices, 1, capacity_pixels, row_chunk,
                        shard, n_shards)

    # Lit codes (include/och_gpu.h): the lit frame's exchange format, one int16
    # per pixel = OCH_CODE_* byte | mask byte << 8; shade_lit_unshard_dev yields
    # the RGBA8 frames render_lit_views_dev writes (frame.shade_lit_codes on the host).
    @staticmethod
    def _need_lit_codes(buf, what):
        if hasattr(buf, "element_size") and buf.element_size() != 2:
            raise ValueError(f"{what}: lit codes are 2-byte elements (int16), not {buf.element_size()}-byte ones")

    def render_lit_codes_views_dev(self, cams, light: Light, code_slices, capacity_pixels: int | None = None,
                                   row_chunk: int | None = None, shard: int = 0, n_shards: int = 1):
        """render_codes_views_dev's slices, lit (och_gpu_render_lit_codes_views_dev): code_slices is a device
        tensor of int16, or a raw pointer with capacity_pixels.  Asynchronous on the pool's stream."""
        self._need_lit_codes(code_slices, "code_slices")
        self._lit_views("och_gpu_render_lit_codes_views_dev", cams, light, code_slices, 2, capacity_pixels, row_chunk,
                        shard, n_shards)

    def shade_lit_unshard_dev(self, gathered_codes, frames, width: int, height: int, row_chunk: int, n_shards: int,
                              light: Light, n_views: int = 1):
        """Gathered lit codes [n_shards][n_views][rows][W] -> RGBA8 frames [n_views][H][W] under light's
        two weights (och_gpu_shade_lit_unshard_views_dev)."""
        self._need_lit_codes(gathered_codes, "gathered_codes")
        rows = self.slice_rows(height, row_chunk, n_shards)
        _need(gathered_codes, 2 * n_shards * n_views * rows * width, "gathered_codes")
        _need(frames, 4 * n_views * height * width, "frames")
        call("och_gpu_shade_lit_unshard_views_dev", self._h, _dev_ptr(gathered_codes), _dev_ptr(frames), int(width),
             int(height), int(row_chunk), int(n_shards), int(n_views), C.byref(light))

    def render_lit_steps_dev(self, cams, light: Light, frames, streams, n_steps: int, events=None,
                             row_chunk: int | None = None):
        """render_steps_dev with every frame a lit frame (och_gpu_render_lit_steps_dev)."""
        self._steps("och_gpu_render_lit_steps_dev", cams, light, frames, streams, n_steps, events, row_chunk)

    def render_lit_ssaa(self, cam: Camera, light: Light, s: int) -> np.ndarray:
        """The lit frame of `cam` (the sample grid's camera, as for render_ssaa) supersampled s x s:
        (H / s, W / s) uint32, every sample shaded as render_lit shades it, then the rounded mean
        (och_gpu_render_lit_ssaa; box_downsample(shade_lit(...)) states it on the host)."""
        return self._ssaa("och_gpu_render_lit_ssaa", cam, light, s)

    def render_lit_ssaa_views_dev(self, cams, light: Light, s: int, rgba, capacity_pixels: int | None = None):
        """Several equal-size sample-grid cameras, lit and supersampled s x s in one launch
        (och_gpu_render_lit_ssaa_views_dev): rgba (a device tensor of 4-byte words, or a raw pointer with
        capacity_pixels) receives the views' (H / s) x (W / s) frames back to back.  Asynchronous on the
        pool's stream."""
        self._ssaa_views("och_gpu_render_lit_ssaa_views_dev", cams, light, s, rgba, capacity_pixels)

    def render_steps_dev(self, cams, frames, streams, n_steps: int, events=None, row_chunk: int | None = None,
                         bounce: bool = False):
        """n_steps whole frames of these cameras issued by the library's own loop
        (och_gpu_render_steps_dev): frame k on streams[k % B] into frames[k % B],
        B = len(frames) = len(streams); events = n_steps (start, stop) pairs of HIP
        events (raw handles or objects with ``h``) recorded by each frame's dispatch."""
        self._steps("och_gpu_render_steps_dev", cams, None, frames, streams, n_steps, events, row_chunk,
                    int(bool(bounce)))

    def _steps(self, name, cams, light, frames, streams, n_steps, events, row_chunk, *bounce):
        if len(frames) != len(streams) or not frames:
            raise ValueError("one stream per frame buffer")
        arr, n, first, row_chunk = self._frame_views(cams, row_chunk)
        sp = (C.c_void_p * len(streams))(*[getattr(s_, "cuda_stream", s_) for s_ in streams])
        for f in frames:
            self._need_frames(f, n, first, row_chunk, 1, 4, "frames")
        fp = (C.c_void_p * len(frames))(*[_dev_ptr(f) for f in frames])
        e0 = e1 = None
        if events is not None:
            if len(events) != n_steps:
                raise ValueError("one event pair per step")
            e0 = (C.c_void_p * n_steps)(*[_event_handle(a) for a, _ in events])
            e1 = (C.c_void_p * n_steps)(*[_event_handle(b) for _, b in events])
        call(name, self._h, arr, n, *self._lit(light), int(n_steps), sp, fp, len(frames), e0, e1, row_chunk, *bounce)

    def plan_views(self, cams, row_chunk: int | None = None, shard: int = 0, n_shards: int = 1):
        """Plan the launch order of frames of this geometry (och_gpu_plan_views); used with
        set_option("tile_order", 2).  Synchronous."""
        arr, n, _, row_chunk = self._frame_views(cams, row_chunk)
        call("och_gpu_plan_views", self._h, arr, n, row_chunk, int(shard), int(n_shards))

    def render_bounce_views_dev(self, cams, rgba_slices, row_chunk: int | None = None, shard: int = 0,
                                n_shards: int = 1):
        """Config 5 frames: one bounce per hit pixel, shaded (see och_gpu_render_bounce_views_dev)."""
        self._plain_views("och_gpu_render_bounce_views_dev", cams, rgba_slices, 4, "rgba_slices", row_chunk, shard,
                          n_shards)

    # Row deal (och_gpu_set_row_deal): which shard renders each row chunk.
    def set_row_deal(self, height: int, row_chunk: int, n_shards: int, chunk_shard=None):
        """chunk_shard[g] = shard of row chunk g (None = round-robin) for frames of this geometry."""
        if chunk_shard is None:
            call("och_gpu_set_row_deal", self._h, int(height), int(row_chunk), int(n_shards), None)
            return
        deal = np.ascontiguousarray(chunk_shard, np.int32).reshape(-1)
        if deal.size != -(-int(height) // int(row_chunk)):
            raise ValueError("one shard per row chunk expected")
        call("och_gpu_set_row_deal", self._h, int(height), int(row_chunk), int(n_shards), _np_ptr(deal))

    def slice_rows(self, height: int, row_chunk: int, n_shards: int) -> int:
        """Rows per slice for this geometry under the pool's deal (och_gpu_slice_rows)."""
        v = C.c_int()
        call("och_gpu_slice_rows", self._h, int(height), int(row_chunk), int(n_shards), C.byref(v))
        return v.value

    def chunk_costs(self, cams, row_chunk: int) -> np.ndarray:
        """Per-row-chunk cost of these views from one timed render (och_gpu_chunk_costs)."""
        arr, n, first = views(cams)
        out = np.empty(-(-first.height // int(row_chunk)), np.float32)
        call("och_gpu_chunk_costs", self._h, arr, n, int(row_chunk), _np_ptr(out))
        return out

    def unshard_dev(self, gathered, frame, width: int, height: int, row_chunk: int, n_shards: int, n_views: int = 1):
        rows = self.slice_rows(height, row_chunk, n_shards)
        _need(gathered, 4 * n_shards * n_views * rows * width, "gathered")
        _need(frame, 4 * n_views * height * width, "frame")
        call("och_gpu_unshard_views_dev", self._h, _dev_ptr(gathered), _dev_ptr(frame), int(width), int(height),
             int(row_chunk), int(n_shards), int(n_views))

    # Indexed-colour frames (include/och_gpu.h OCH_CODE_*): one byte per pixel,
    # the multi-GPU exchange format; shade_unshard_dev yields the RGBA8 frames.
    CODE_MAX_VOXELS = 20

    def render_codes_views_dev(self, cams, code_slices, row_chunk: int | None = None, shard: int = 0,
                               n_shards: int = 1, bounce: bool = False):
        self._plain_views("och_gpu_render_codes_views_dev", cams, code_slices, 1, "code_slices", row_chunk, shard,
                          n_shards, int(bool(bounce)))

    def shade_unshard_dev(self, gathered_codes, frames, width: int, height: int, row_chunk: int, n_shards: int,
                          n_views: int = 1):
        rows = self.slice_rows(height, row_chunk, n_shards)
        _need(gathered_codes, n_shards * n_views * rows * width, "gathered_codes")
        _need(frames, 4 * n_views * height * width, "frames")
        call("och_gpu_shade_unshard_views_dev", self._h, _dev_ptr(gathered_codes), _dev_ptr(frames), int(width),
             int(height), int(row_chunk), int(n_shards), int(n_views))


def shard_rows(height: int, row_chunk: int, n_shards: int) -> int:
    return call("och_shard_rows", int(height), int(row_chunk), int(n_shards))


def deal_chunks(costs, n_shards: int, weights=None) -> np.ndarray:
    """och_deal_chunks: row chunks dealt longest-first onto the least loaded shard per weight."""
    costs = np.ascontiguousarray(costs, np.float32).reshape(-1)
    out = np.empty(costs.size, np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w is not None and w.size != n_shards:
        raise ValueError("one weight per shard expected")
    call("och_deal_chunks", _np_ptr(costs), costs.size, int(n_shards), None if w is None else _np_ptr(w), _np_ptr(out))
    return out


# The display rank's share of the row chunks (it also shades the whole frame),
# per world size and exchange, from tools/proxy_rank.py sweeps of every shard
# (profiles/r04/r04e/, r04f/): with the gather to rank 0 the
# other ranks receive nothing, so the display rank takes a smaller share.
# rank 0's deal weight by exchange and world size (tools/proxy_rank.py sweeps,
# DESIGN.md §5); N = 8 all-gather 0.5 since round 5's faster kernel made the
# display rank's whole-frame shade a larger part of its step (profiles/r05/r05al/)
DISPLAY_WEIGHTS = {"gather": {2: 0.9, 4: 0.7, 8: 0.5}, "all_gather": {2: 0.9, 4: 0.8, 8: 0.5}}


def display_weight(world: int, exchange: str = "all_gather") -> float:
    """Default deal weight of rank 0 (the display rank) at this world size,
    for the exchange configs[3] names (the all-gather) unless told otherwise."""
    table = DISPLAY_WEIGHTS.get(exchange, DISPLAY_WEIGHTS["all_gather"])
    if world in table:
        return table[world]
    return max(0.5, 1.0 - (0.0625 if exchange == "gather" else 0.05) * world)


# The heavy-tile split by world size (bench.py sweeps): at N = 1
# the costliest tiles only (T 80: +1.2 % over the 20-step window, -0.4 %
# sustained, a lone frame 0.19 -> 0.16 ms; profiles/r06/r06ah/), off at N = 2 and
# 4 (a tie), T 60 from N = 8, whose half-size launches end on their tails.
# split_defaults takes the entry of the nearest listed world size at or below
# the asked one (so N = 4 takes N = 2's, N = 16 takes N = 8's).
SPLIT_DEFAULTS = {1: {"split": 80, "split_segs": 4, "split_level": 6}, 2: {"split": 0},
                  8: {"split": 60, "split_segs": 4, "split_level": 6}}


def split_defaults(world: int) -> dict:
    """Pool options of the heavy-tile split at this world size ({"split": 0} = off)."""
    best = {"split": 0}
    for w, opts in sorted(SPLIT_DEFAULTS.items()):
        if world >= w:
            best = dict(opts)
    return best


class HOctree(GpuPool):
    """och::h_octree's table on the GPU: 1-based, miss t = +INF (ORT/och_h_octree.h:429)."""

    def __init__(self, nodes, root, depth, device: int = -1):
        super().__init__(nodes, root, depth, index_base=1, miss_t=math.inf, device=device)


class Octree(GpuPool):
    """och::octree's table on the GPU: 0-based, root 0, miss t = 0 (ORT/och_octree.cpp:302)."""

    def __init__(self, nodes, depth, device: int = -1):
        super().__init__(nodes, 0, depth, index_base=0, miss_t=0.0, device=device)
