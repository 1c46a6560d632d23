"""What the Python wrappers hand to the C ABI, as a transcript (tests/golden/binding_calls.json).

`call` is replaced by a recorder in every module of the package that imports it, so nothing here loads or launches the
library: every public wrapper that can run without a device is driven once per path through its
marshalling, and the entry names, the normalised argument values and the wrappers' return values are
compared with the fixture, followed by one input per Python-side refusal with the exception's type
and text.  The fixture was written from the wrappers as they stood before their marshalling steps
were gathered in _marshal.py (`python tests/test_binding_calls_host.py --write`); a difference is a
change of behaviour.

Normalisation: ints, None and strings as they are, floats by repr; a c_void_p by value, or by the
bytes of the ctypes array it was cast from (the camera array dies with the call); ctypes arrays by
element, arrays of structs by their bytes; byref(x) by x's bytes, a struct that holds addresses by
field; an address handed over as an int by the name the test gave that host array ("host:nodes"), "host:?" for one the wrapper made.
och_gpu_slice_rows is answered (och_shard_rows' round-robin rule) but not compared: a wrapper may
ask it as often as it likes.  The device-tensor paths that synchronise a torch stream are left to the
GPU suite."""
import ctypes as C
import json
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

FIXTURE = Path(__file__).resolve().parent / "golden" / "binding_calls.json"
UNCOMPARED = {"och_gpu_slice_rows"}
W, H, VIEWS, ROW_CHUNK, SHARD, N_SHARDS = 24, 20, 2, 8, 1, 3
SLICE_ROWS = 8                                                # ceil(ceil(20 / 8) / 3) * 8
POOL_NODES = np.array([[2, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]], np.uint32)
_NODES_BUF = (C.c_uint32 * 16)(*POOL_NODES.reshape(-1).tolist())


class Dev:
    """A stand-in device tensor: what _dev_ptr, _need and the capacity rule ask of one."""
    is_cuda = True

    def __init__(self, ptr, numel, size=4, contiguous=True):
        self.ptr, self.n, self.size, self.contiguous = ptr, numel, size, contiguous

    def is_contiguous(self):
        return self.contiguous

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n

    def element_size(self):
        return self.size


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class OtherDevice:
    """A torch.device that is not the world's."""
    index = 1

    def __str__(self):
        return "cuda:1"


def fill_struct(st):
    """Distinct values in every field, so a dict made of the struct shows which field went where."""
    for i, (name, kind) in enumerate(st._fields_):
        if issubclass(kind, C.Array):
            getattr(st, name)[:] = [10 * (i + 1) + k for k in range(kind._length_)]
        elif not issubclass(kind, C._Pointer):
            setattr(st, name, i + 1)


class Recorder:
    def __init__(self, prototypes):
        self.prototypes, self.calls, self.names, self.keep = prototypes, [], {}, []

    def host(self, name, arr):
        """Name a host array of the test's, so its address is recognised among the arguments."""
        self.names[arr.ctypes.data] = name
        self.keep.append(arr)
        return arr

    def norm(self, a, kind):
        if a is None or isinstance(a, str):
            return a
        if isinstance(a, (bool, int, np.integer)):
            a = int(a)
            if kind is C.c_void_p and a >= 1 << 32:
                return "host:" + self.names.get(a, "?")
            return a
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, C.c_void_p):
            src = [o for o in (a._objects or {}).values() if isinstance(o, C.Array)]
            return {"bytes": bytes(src[0]).hex()} if src else a.value
        if isinstance(a, C.Array):
            return {"bytes": bytes(a).hex()} if issubclass(a._type_, C.Structure) else list(a)
        if hasattr(a, "_obj"):
            return {"byref": self.pointee(a._obj)}
        raise TypeError(f"an argument of type {type(a).__name__}")

    def pointee(self, x):
        """What byref(x) points to: bytes, or a struct by field where a field holds an address."""
        if not isinstance(x, C.Structure) or not any(k is C.c_void_p or issubclass(k, C._Pointer) for _, k in x._fields_):
            return bytes(x).hex()
        fields = []
        for name, kind in x._fields_:
            v = getattr(x, name)
            if issubclass(kind, C._Pointer):
                v = bool(v)
            fields.append([name, list(v) if isinstance(v, C.Array) else self.norm(v, kind)])
        return fields

    def __call__(self, name, *args):
        kinds = self.prototypes[name][1]
        assert len(args) == len(kinds), (name, len(args), len(kinds))
        if name not in UNCOMPARED:
            self.calls.append([name] + [self.norm(a, k) for a, k in zip(args, kinds)])
        return self.answer(name, args)

    def answer(self, name, args):
        """The host queries a wrapper needs an answer from; everything else returns 0 (OCH_OK)."""
        def out(i):
            return args[i]._obj
        if name in ("och_gpu_slice_rows", "och_shard_rows"):
            height, row_chunk, n_shards = args[-4:-1] if name == "och_gpu_slice_rows" else args
            rows = -(-(-(-height // row_chunk)) // n_shards) * row_chunk
            if name == "och_shard_rows":
                return rows
            out(4).value = rows
        elif name in ("och_gpu_pool_create", "och_editor_create", "och_world_create", "och_frame_group_create",
                      "och_comm_create"):
            out(-1).value = 0x1000
        elif name == "och_world_pool_create":
            out(1).value = 0x2000
        elif name in ("och_gpu_pool_info", "och_editor_info", "och_world_info", "och_world_fill_box",
                      "och_world_restore_box"):
            fill_struct(out(-1))
        elif name in ("och_world_diff", "och_pool_diff"):
            fill_struct(out(-1))
            out(-1).n = 2
        elif name in ("och_build_terrain", "och_build_voxels", "och_edit_voxels", "och_world_download"):
            hp = out(1)
            fill_struct(hp)
            hp.nodes, hp.n_nodes = C.cast(_NODES_BUF, C.POINTER(C.c_uint32)), 2
        elif name == "och_editor_nodes":
            C.cast(C.pointer(out(1)), C.POINTER(C.c_void_p))[0] = C.addressof(_NODES_BUF)
            out(2).value, out(3).value = 2, 1
        elif name == "och_world_snapshots":
            out(3).value = 2
            if args[1] is not None:
                args[1][0], args[1][1] = 1, 3
        elif name == "och_world_snapshot":
            out(1).value = 5
        elif name == "och_pool_pack":
            out(7).value, out(8).value = 2, 1
        elif name == "och_box_cubes":
            out(8).value = 2
        elif name == "och_device_list":
            out(2).value = 2
            if args[0] is not None:
                next(iter(o for o in args[0]._objects.values() if isinstance(o, C.Array)))[0:2] = [0, 1]
        elif name == "och_device_count":
            out(0).value = 2
        elif name == "och_host_rcp_lut":
            out(1).value = 3
        elif name == "och_rcp_lut_error":
            out(2).value = 0.25
        elif name in ("och_gpu_get_option", "och_gpu_occupancy"):
            out(-1).value = 4
        elif name == "och_gpu_last_kernel_ms":
            out(1).value = 0.5
        elif name == "och_gpu_trace":
            out(7).value, out(8).value, out(9).value = 1, 2, 0.5
        elif name in ("och_editor_at", "och_pool_at", "och_rcp_from_lut"):
            return 7
        return 0


def shown(v):
    """A wrapper's return value as JSON: a dict by its items in order, an array by type and shape
    (wrappers hand out np.empty buffers the library would have filled)."""
    from octree_ray_tracing_amd.builder import NodePool
    if isinstance(v, NodePool):
        return {"NodePool": [v.nodes.tolist(), shown(v.root), shown(v.depth), shown(v.index_base), shown(v.solid_voxels),
                             shown(v.voxel_hist), shown(v.tree_nodes), shown(v.build_seconds)]}
    if isinstance(v, np.ndarray):
        return {"array": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, dict):
        return {"dict": [[k, shown(x)] for k, x in v.items()]}
    if isinstance(v, (list, tuple)):
        return [shown(x) for x in v]
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, (bool, int, np.integer)):
        return [type(v).__name__, int(v)]
    if v is None or isinstance(v, str):
        return v
    return type(v).__name__


def make_camera(Camera, k=0):
    cam = Camera()
    cam.pos[:] = [1.5, 1.25 + 0.125 * k, 1.5]
    cam.rot[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cam.fov_factor, cam.aspect, cam.view_x, cam.view_y = 1.25, W / H, 0.5, 0.25
    cam.width, cam.height = W, H
    return cam


def transcript(monkeypatch):
    """Drive the wrappers under the recorder: {"calls": [...], "refusals": [...]}."""
    import octree_ray_tracing_amd as ort
    from octree_ray_tracing_amd import _lib, builder, editor, frame, tracer, world
    from octree_ray_tracing_amd._lib import Camera, Light

    rec = Recorder(_lib.PROTOTYPES)
    real = _lib.call
    for name, m in list(sys.modules.items()):             # the modules import `call` by name: every copy of it
        if name.startswith(ort.__name__ + ".") and getattr(m, "call", None) is real:
            monkeypatch.setattr(m, "call", rec)
    assert all(getattr(m, "call") is rec for m in (tracer, frame, world, builder, editor))
    entries, refusals, made = [], [], []

    def drive(label, fn, *a, **kw):
        first = len(rec.calls)
        r = fn(*a, **kw)
        entries.append({"wrapper": label, "calls": rec.calls[first:], "returns": shown(r)})
        return r

    def refuse(label, fn, *a, **kw):
        first = len(rec.calls)
        with pytest.raises((ValueError, RuntimeError)) as e:
            fn(*a, **kw)
        refusals.append({"wrapper": label, "type": type(e.value).__name__, "text": str(e.value),
                         "calls_before": rec.calls[first:]})

    nodes = rec.host("nodes", POOL_NODES.copy())
    cams = [make_camera(Camera, k) for k in range(VIEWS)]
    cam = cams[0]
    light = Light(sun_dir=(0.5, 1.0, 0.25), ao_reach=4.0)
    events = [(0xE00 + 2 * k, Obj(h=C.c_void_p(0xE01 + 2 * k))) for k in range(3)]
    streams = [0x500, Obj(cuda_stream=0x501)]
    try:
        # -- tracer: module functions
        drive("host_rcp_lut", tracer.host_rcp_lut)
        lut = rec.host("lut", np.arange(8, dtype=np.uint32))
        drive("rcp_from_lut", tracer.rcp_from_lut, 0x3F800000, lut)
        drive("rcp_lut_error", tracer.rcp_lut_error, lut)
        drive("rcp_lut_error/6 entries", tracer.rcp_lut_error, rec.host("lut6", np.arange(6, dtype=np.uint32)))
        drive("device_list", tracer.device_list)
        drive("device_count", tracer.device_count)
        drive("camera", tracer.camera, (1.5, 1.25, 1.0), 0.3, -0.6, 1.25, W, H)
        drive("light_check", tracer.light_check, light)
        drive("shard_rows", tracer.shard_rows, H, ROW_CHUNK, N_SHARDS)
        costs = rec.host("costs", np.array([3, 1, 2], np.float32))
        drive("deal_chunks", tracer.deal_chunks, costs, 2)
        drive("deal_chunks/weights", tracer.deal_chunks, costs, 2, rec.host("weights", np.array([1, 0.5], np.float32)))

        # -- GpuPool
        pool = drive("GpuPool", tracer.GpuPool, nodes, 1, 3)
        made.append(pool)
        for label, fn in (("HOctree", lambda: tracer.HOctree(nodes, 1, 3, device=1)),
                          ("Octree", lambda: tracer.Octree(nodes, 3)),
                          ("GpuPool/0-based", lambda: tracer.GpuPool(nodes.reshape(-1), 0, 3, index_base=0))):
            p = drive(label, fn)
            made.append(p)
            entries[-1]["returns"] = [p.depth, p.index_base, repr(p.miss_t)]
            drive(label + ".close", p.close)
            drive(label + ".close twice", p.close)
        drive("info", pool.info)
        drive("get_root", pool.get_root)
        drive("set_rcp_lut", pool.set_rcp_lut, lut)
        palette = rec.host("palette", np.arange(12, dtype=np.uint32))
        drive("set_palette", pool.set_palette, palette.reshape(2, 6))
        entries[-1]["returns"] = pool._palette_n
        drive("set_stream/handle", pool.set_stream, 0x500)
        drive("set_stream/object", pool.set_stream, streams[1])
        drive("update", pool.update, 1, nodes[1:], 1)
        drive("set_option", pool.set_option, "tile_order", 2)
        drive("get_option", pool.get_option, "plan")
        drive("get_option/read-only", pool.get_option, "split_tiles")
        drive("set_stamp_buffer/None", pool.set_stamp_buffer, None, 0)
        drive("set_stamp_buffer", pool.set_stamp_buffer, Dev(0x7000, 64, 8), 64)
        drive("occupancy", pool.occupancy, 2)
        drive("synchronize", pool.synchronize)
        drive("last_kernel_ms", pool.last_kernel_ms)
        drive("set_launch_events/None", pool.set_launch_events, None, None)
        drive("set_launch_events", pool.set_launch_events, *events[0])
        drive("sse_trace", pool.sse_trace, 1.5, 1.5, 1.5, 0, 0, -1)

        n = 5
        origin = rec.host("origin", np.array([1.5, 1.5, 1.5], np.float32))
        origins = rec.host("origins", np.full((n, 3), 1.5, np.float32))
        dirs = rec.host("dirs", np.ones((n, 3), np.float32))
        drive("trace_batch", pool.trace_batch, origin, dirs)
        drive("trace_batch/per-ray origins", pool.trace_batch, origins, dirs)
        drive("trace_batch/width", pool.trace_batch, origin, dirs, width=5)
        d_origin, d_origins, d_dirs = Dev(0x8000, 3), Dev(0x8100, 3 * n), Dev(0x8200, 3 * n)
        hits = [Dev(0x8300 + 0x100 * k, n) for k in range(7)]
        drive("trace_batch_dev", pool.trace_batch_dev, d_origin, d_dirs, *hits[:3])
        drive("trace_batch_dev/push, n, per-ray origins", pool.trace_batch_dev, d_origins, d_dirs, *hits[:3], push=hits[6], n=4)
        drive("trace_batch_dev/raw pointers", pool.trace_batch_dev, d_origin, d_dirs, 0x8300, 0x8400, 0x8500)
        drive("trace_batch_tiled_dev", pool.trace_batch_tiled_dev, d_origin, d_dirs, 5, *hits[:3])
        drive("trace_batch_tiled_dev/push, n", pool.trace_batch_tiled_dev, d_origins, d_dirs, 2, *hits[:3], push=hits[6], n=4)
        drive("plan_batch_tiled", pool.plan_batch_tiled, d_origin, d_dirs, 5)
        drive("plan_batch_tiled/n, per-ray origins", pool.plan_batch_tiled, d_origins, d_dirs, 2, n=4)
        drive("trace_bounce_batch_dev", pool.trace_bounce_batch_dev, d_origin, d_dirs, *hits[:6])
        drive("trace_bounce_batch_dev/push, n", pool.trace_bounce_batch_dev, d_origins, d_dirs, *hits[:6], push=hits[6], n=4)

        whole = Dev(0x9000, W * H)
        wholes = Dev(0x9000, VIEWS * W * H)
        slices = Dev(0xA000, VIEWS * SLICE_ROWS * W)
        sharded = dict(row_chunk=ROW_CHUNK, shard=SHARD, n_shards=N_SHARDS)
        drive("raygen_dev", pool.raygen_dev, cam, Dev(0x9000, 3 * W * H))
        drive("render", pool.render, cam)
        drive("render_dev", pool.render_dev, cam, whole)
        drive("render_dev/sharded", pool.render_dev, cam, Dev(0xA000, SLICE_ROWS * W), **sharded)
        drive("render_dev/raw pointer", pool.render_dev, cam, 0xA000, **sharded)
        for name in ("render_views_dev", "render_bounce_views_dev", "render_codes_views_dev"):
            fn, size = getattr(pool, name), 1 if "codes" in name else 4
            drive(name, fn, cams, Dev(0x9000, VIEWS * W * H, size))
            drive(name + "/sharded, tuple", fn, tuple(cams), Dev(0xA000, VIEWS * SLICE_ROWS * W, size), **sharded)
            drive(name + "/raw pointer", fn, cams, 0xA000, **sharded)
        drive("render_codes_views_dev/bounce", pool.render_codes_views_dev, cams, Dev(0xA000, VIEWS * SLICE_ROWS * W, 1),
              bounce=True, **sharded)
        for name, lit in (("render_ssaa", ()), ("render_lit_ssaa", (light,))):
            drive(name, getattr(pool, name), cam, *lit, 2)
            drive(name + "/s 0", getattr(pool, name), cam, *lit, 0)
        for name, lit in (("render_ssaa_views_dev", ()), ("render_lit_ssaa_views_dev", (light,))):
            fn = getattr(pool, name)
            drive(name, fn, cams, *lit, 2, Dev(0x9000, VIEWS * (W // 2) * (H // 2)))
            drive(name + "/larger buffer of bytes", fn, cams, *lit, 4, Dev(0x9000, 1001, 1))
            drive(name + "/raw pointer", fn, cams, *lit, 2, 0x9000, capacity_pixels=VIEWS * W * H)
            drive(name + "/tensor and capacity", fn, cams, *lit, 2, wholes, capacity_pixels=7)
            drive(name + "/s 3", fn, cams, *lit, 3, Dev(0x9000, 1))
        drive("render_lit", pool.render_lit, cam, light)
        for name, size in (("render_lit_views_dev", 4), ("render_lit_masks_views_dev", 1), ("render_lit_codes_views_dev", 2)):
            fn = getattr(pool, name)
            drive(name, fn, cams, light, Dev(0x9000, VIEWS * W * H, size))
            drive(name + "/sharded, tuple", fn, tuple(cams), light, Dev(0xA000, VIEWS * SLICE_ROWS * W + 1, size), **sharded)
            drive(name + "/raw pointer", fn, cams, light, 0xA000, capacity_pixels=VIEWS * SLICE_ROWS * W, **sharded)
            drive(name + "/tensor and capacity", fn, cams, light, Dev(0x9000, VIEWS * W * H, size), 7)
        gathered = dict(width=W, height=H, row_chunk=ROW_CHUNK, n_shards=N_SHARDS, n_views=VIEWS)
        for name, size, lit in (("unshard_dev", 4, {}), ("shade_unshard_dev", 1, {}), ("shade_lit_unshard_dev", 2, {"light": light})):
            fn = getattr(pool, name)
            drive(name, fn, Dev(0xB000, N_SHARDS * VIEWS * SLICE_ROWS * W, size), wholes, **gathered, **lit)
            drive(name + "/raw pointers", fn, 0xB000, 0x9000, **gathered, **lit)
        frames = [Dev(0x9000, VIEWS * W * H), Dev(0xC000, VIEWS * W * H)]
        for name, lit in (("render_steps_dev", ()), ("render_lit_steps_dev", (light,))):
            fn = getattr(pool, name)
            drive(name, fn, cams, *lit, frames, streams, 3)
            padded = [Dev(f.ptr, VIEWS * 24 * W) for f in frames]           # whole row chunks: 24 rows for 20
            drive(name + "/events, row_chunk", fn, tuple(cams), *lit, padded, streams, 3, events=events, row_chunk=ROW_CHUNK)
            drive(name + "/raw pointers", fn, cams, *lit, [0x9000], [0x500], 1)
        drive("render_steps_dev/bounce", pool.render_steps_dev, cams, frames, streams, 2, bounce=True)
        drive("plan_views", pool.plan_views, cams)
        drive("plan_views/sharded", pool.plan_views, cams, **sharded)
        drive("set_row_deal/round-robin", pool.set_row_deal, H, ROW_CHUNK, N_SHARDS)
        drive("set_row_deal", pool.set_row_deal, H, ROW_CHUNK, N_SHARDS, rec.host("deal", np.array([0, 2, 1], np.int32)))
        drive("slice_rows", pool.slice_rows, H, ROW_CHUNK, N_SHARDS)
        drive("chunk_costs", pool.chunk_costs, cams, ROW_CHUNK)
        drive("chunk_costs/one camera", pool.chunk_costs, cam, ROW_CHUNK)

        # -- GpuPool refusals
        cpu = Obj(is_cuda=False)
        refuse("_dev_ptr/host tensor", pool.raygen_dev, cam, cpu)
        refuse("_dev_ptr/not contiguous", pool.set_stamp_buffer, Dev(0x7000, 64, 8, contiguous=False), 64)
        refuse("_need", pool.raygen_dev, cam, Dev(0x9000, 3 * W * H - 1))
        refuse("set_rcp_lut/not a power of two", pool.set_rcp_lut, np.arange(6, dtype=np.uint32))
        refuse("set_rcp_lut/one entry", pool.set_rcp_lut, np.arange(1, dtype=np.uint32))
        refuse("set_palette", pool.set_palette, np.arange(7, dtype=np.uint32))
        refuse("trace_batch_dev/short origins", pool.trace_batch_dev, Dev(0x8100, 3 * n - 1), d_dirs, *hits[:3])
        refuse("trace_batch_dev/short dirs", pool.trace_batch_dev, d_origin, d_dirs, *hits[:3], n=n + 1)
        refuse("trace_batch_tiled_dev/short push", pool.trace_batch_tiled_dev, d_origin, d_dirs, 5, *hits[:3], push=Dev(0x8900, n - 1))
        refuse("trace_bounce_batch_dev/short record", pool.trace_bounce_batch_dev, d_origin, d_dirs, *hits[:5], Dev(0x8900, n - 1))
        refuse("render_dev/short slice", pool.render_dev, cam, Dev(0xA000, SLICE_ROWS * W - 1), **sharded)
        refuse("render_views_dev/short slices", pool.render_views_dev, cams, Dev(0xA000, VIEWS * SLICE_ROWS * W - 1), **sharded)
        refuse("render_bounce_views_dev/short slices", pool.render_bounce_views_dev, cams, Dev(0x9000, VIEWS * W * H - 1))
        refuse("render_codes_views_dev/short slices", pool.render_codes_views_dev, cams, Dev(0x9000, VIEWS * W * H - 1, 1))
        for name, lit in (("render_ssaa_views_dev", ()), ("render_lit_ssaa_views_dev", (light,))):
            fn = getattr(pool, name)
            refuse(name + "/short buffer", fn, cams, *lit, 2, Dev(0x9000, VIEWS * (W // 2) * (H // 2) - 1))
            refuse(name + "/raw pointer without capacity", fn, cams, *lit, 2, 0x9000)
            refuse(name + "/host tensor", fn, cams, *lit, 2, cpu, capacity_pixels=7)
        for name, size in (("render_lit_views_dev", 4), ("render_lit_masks_views_dev", 1), ("render_lit_codes_views_dev", 2)):
            fn = getattr(pool, name)
            refuse(name + "/short slices", fn, cams, light, Dev(0xA000, VIEWS * SLICE_ROWS * W - 1, size), **sharded)
            refuse(name + "/raw pointer without capacity", fn, cams, light, 0xA000, **sharded)
        refuse("render_lit_codes_views_dev/4-byte elements", pool.render_lit_codes_views_dev, cams, light, wholes)
        refuse("shade_lit_unshard_dev/1-byte elements", pool.shade_lit_unshard_dev, Dev(0xB000, 1 << 20, 1), wholes, **gathered, light=light)
        refuse("shade_lit_unshard_dev/short codes", pool.shade_lit_unshard_dev, Dev(0xB000, 5, 2), wholes, **gathered, light=light)
        refuse("shade_lit_unshard_dev/short frames", pool.shade_lit_unshard_dev, 0xB000, Dev(0x9000, 5), **gathered, light=light)
        refuse("unshard_dev/short gathered", pool.unshard_dev, Dev(0xB000, 5), wholes, **gathered)
        refuse("unshard_dev/short frame", pool.unshard_dev, 0xB000, Dev(0x9000, 5), **gathered)
        refuse("shade_unshard_dev/short codes", pool.shade_unshard_dev, Dev(0xB000, 5, 1), wholes, **gathered)
        refuse("shade_unshard_dev/short frames", pool.shade_unshard_dev, 0xB000, Dev(0x9000, 5), **gathered)
        for name, lit in (("render_steps_dev", ()), ("render_lit_steps_dev", (light,))):
            fn = getattr(pool, name)
            refuse(name + "/streams and frames differ", fn, cams, *lit, frames, streams[:1], 3)
            refuse(name + "/no frames", fn, cams, *lit, [], [], 3)
            refuse(name + "/short frame", fn, cams, *lit, [frames[0], Dev(0xC000, 5)], streams, 3)
            refuse(name + "/host frame", fn, cams, *lit, [frames[0], cpu], streams, 3)
            refuse(name + "/events and steps differ", fn, cams, *lit, frames, streams, 2, events=events)
        refuse("set_row_deal", pool.set_row_deal, H, ROW_CHUNK, N_SHARDS, [0, 1])
        refuse("deal_chunks", tracer.deal_chunks, costs, 2, [1.0, 0.5, 0.25])
        drive("GpuPool.close", pool.close)

        # -- frame: RcclComm, FrameGroup, ShardedSteps
        uid = bytes(range(128))
        drive("RcclComm.unique_id", frame.RcclComm.unique_id)
        entries[-1]["returns"] = None
        comm = drive("RcclComm", frame.RcclComm, uid, 2, 1, 0)
        made.append(comm)
        entries[-1]["returns"] = [comm.n_ranks, comm.rank, comm.device, comm.handle.value]
        send, recv = Dev(0xA000, VIEWS * SLICE_ROWS * W, 1), Dev(0xB000, 2 * VIEWS * SLICE_ROWS * W, 1)
        drive("RcclComm.all_gather", comm.all_gather, send, recv, streams[1])
        drive("RcclComm.gather", comm.gather, send, recv, streams[1])
        drive("RcclComm.gather/not the root", comm.gather, Dev(0xA000, 48, 2), None, streams[1], root=1)
        drive("RcclComm.available", frame.RcclComm.available)
        drive("RcclComm.abort", comm.abort)
        refuse("RcclComm/short id", frame.RcclComm, uid[:5], 2, 1, 0)

        group = drive("FrameGroup", frame.FrameGroup, nodes, 1, 3, devices=[0, 1])
        made.append(group)
        entries[-1]["returns"] = [group.n, group._h.value]
        g2 = drive("FrameGroup/every device, 0-based", frame.FrameGroup, nodes, 0, 3, index_base=0)
        made.append(g2)
        entries[-1]["returns"] = [g2.n, g2._h.value]
        drive("FrameGroup/every device, 0-based.close", g2.close)
        drive("FrameGroup.set_palette", group.set_palette, palette)
        drive("FrameGroup.set_option", group.set_option, "plan", 1)
        drive("FrameGroup.plan", group.plan, cams)
        drive("FrameGroup.plan/one camera, row_chunk", group.plan, cam, row_chunk=4)
        drive("FrameGroup.render", group.render, cams)
        entries[-1]["returns"] = list(group._shape)
        drive("FrameGroup.render/bounce", group.render, tuple(cams), row_chunk=4, bounce=True)
        drive("FrameGroup.render/lit, one camera", group.render, cam, light=light)
        entries[-1]["returns"] = list(group._shape)
        drive("FrameGroup.render_steps", group.render_steps, cams, 5)
        drive("FrameGroup.render_steps/bounce", group.render_steps, cams, 5, n_buffers=2, row_chunk=4, bounce=True)
        drive("FrameGroup.render_steps/lit", group.render_steps, cam, 5, light=light)
        entries[-1]["returns"] = list(group._shape)
        drive("FrameGroup.synchronize", group.synchronize)
        drive("FrameGroup.download", group.download, 1)
        refuse("FrameGroup.set_palette", group.set_palette, np.arange(7, dtype=np.uint32))
        refuse("FrameGroup.render/lit and bounce", group.render, cams, bounce=True, light=light)
        refuse("FrameGroup.render_steps/lit and bounce", group.render_steps, cams, 5, bounce=True, light=light)
        drive("FrameGroup.close", group.close)

        issued = []

        def native(status):
            def fn(*args):
                kinds = _lib.PROTOTYPES["och_gpu_render_sharded_steps_dev"][1]
                issued.append([rec.norm(a, k) for a, k in zip(args, kinds)])
                return status
            return fn
        fake_lib = Obj(och_gpu_render_sharded_steps_dev=native(0), och_gpu_render_lit_sharded_steps_dev=native(1),
                       och_last_error=lambda: b"what the library said")
        monkeypatch.setattr(frame, "load", lambda: fake_lib)
        spool = tracer.GpuPool._adopt(C.c_void_p(0x3000), 3)
        made.append(spool)

        def sharded_frames(rank, shade="all", mode="all_gather", lit=None, **kw):
            return [Obj(comm=comm, indexed=True, direct=False, light=lit, pool=spool, exchange_mode=mode, shade=shade,
                        rank=rank, row_chunk=ROW_CHUNK, slice=Dev(0xA000 + k, 1), gathered=Dev(0xB000 + k, 1),
                        frames=Dev(0x9000 + k, 1), **kw) for k in range(2)]
        sstreams = [Obj(cuda_stream=0x500), Obj(cuda_stream=0x501)]
        for label, frames_, kw, prep in (
                ("all_gather", sharded_frames(1), {}, (3,)),
                ("all_gather/events, bounce", sharded_frames(1), {"bounce": True}, (2, [0xE00, 0xE02], [0xE01, 0xE03])),
                ("display", sharded_frames(1, shade="display"), {}, (3,)),
                ("display/rank 0", sharded_frames(0, shade="display"), {}, (3,)),
                ("gather", sharded_frames(1, shade="display", mode="gather"), {}, (3,)),
                ("gather/override, rank 0, one camera", sharded_frames(0, shade="display"), {"exchange": "gather"}, (3,))):
            steps = frame.ShardedSteps(frames_, sstreams, comm, cam if "one camera" in label else cams, **kw)
            issue = steps.prepare(*prep)
            before = len(issued)
            issue()
            issue()
            entries.append({"wrapper": "ShardedSteps/" + label, "calls": issued[before:],
                            "returns": [steps.mode, steps.exchange, steps.n_views]})
        lit_steps = frame.ShardedSteps(sharded_frames(1, lit=light), sstreams, comm, cams)
        before = len(issued)
        refuse("ShardedSteps/the library refuses", lit_steps.prepare(3))
        refusals[-1]["calls_before"] = issued[before:]
        other = Obj(n_ranks=2, rank=1)
        refuse("ShardedSteps/streams and frames differ", frame.ShardedSteps, sharded_frames(1), sstreams[:1], comm, cams)
        refuse("ShardedSteps/another comm", frame.ShardedSteps, sharded_frames(1), sstreams, other, cams)
        mixed = sharded_frames(1)
        mixed[1].light = light
        refuse("ShardedSteps/two lights", frame.ShardedSteps, mixed, sstreams, comm, cams)
        refuse("ShardedSteps/lit and bounce", frame.ShardedSteps, sharded_frames(1, lit=light), sstreams, comm, cams, bounce=True)
        refuse("ShardedSteps/exchange", frame.ShardedSteps, sharded_frames(1), sstreams, comm, cams, exchange="display")
        refuse("ShardedSteps/gather without display", frame.ShardedSteps, sharded_frames(1), sstreams, comm, cams, exchange="gather")
        drive("RcclComm.close", comm.close)
        drive("RcclComm.abort/closed", comm.abort)

        # -- frame: host definitions and ShardedFrame's argument checks
        refuse("box_downsample/s", frame.box_downsample, np.zeros((4, 4), np.uint32), 3)
        refuse("box_downsample/shape", frame.box_downsample, np.zeros((4, 6), np.uint32), 4)
        refuse("shade_lit", frame.shade_lit, np.zeros((4, 6), np.uint32), np.zeros((4, 5), np.uint8), light)
        refuse("code_table", frame.code_table, np.zeros(7, np.uint32))
        refuse("shade_lit_codes", frame.shade_lit_codes, np.zeros(4, np.uint32), palette, light)
        fpool = tracer.GpuPool._adopt(C.c_void_p(0x3000), 3)
        made.append(fpool)
        refuse("ShardedFrame/shade", frame.ShardedFrame, fpool, W, H, shade="rank 0")
        refuse("ShardedFrame/comm of another rank", frame.ShardedFrame, fpool, W, H, comm=other)
        refuse("ShardedFrame/exchange", frame.ShardedFrame, fpool, W, H, exchange="scatter")
        refuse("ShardedFrame/gather without comm", frame.ShardedFrame, fpool, W, H, exchange="gather", shade="display")
        lit_frame = frame.ShardedFrame.__new__(frame.ShardedFrame)
        lit_frame.light = light
        refuse("ShardedFrame.render_local/lit and bounce", lit_frame.render_local, cams, bounce=True)

        # -- editor
        ed = drive("Editor", editor.Editor, nodes, 1, 3)
        made.append(ed)
        entries[-1]["returns"] = [ed.depth, ed._h.value]
        e2 = drive("Editor/capacity", editor.Editor, nodes.reshape(-1), 1, 3, capacity=100)
        made.append(e2)
        drive("Editor/capacity.close", e2.close)
        drive("Editor.set", ed.set, 1, 2, 3, 4)
        drive("Editor.at", ed.at, 1, 2, 3)
        drive("Editor.stats", ed.stats)
        drive("Editor.root", lambda: ed.root)
        drive("Editor.nodes", ed.nodes)
        mirror = drive("Editor.make_pool", ed.make_pool, device=1)
        made.append(mirror)
        drive("Editor.flush", ed.flush, mirror)
        drive("Editor.make_pool's pool.close", mirror.close)
        drive("Editor.close", ed.close)

        # -- builder
        host_pool = builder.NodePool(nodes, 1, 3, 1)
        drive("NodePool.at", host_pool.at, 1, 2, 3)
        drive("NodePool.read_box", host_pool.read_box, (0, 1, 2), (4, 4, 4))
        drive("NodePool.read_box/uint32, empty", host_pool.read_box, [0, 1, 2], [0, 4, 4], np.uint32)
        drive("NodePool.diff", host_pool.diff, builder.NodePool(rec.host("other nodes", POOL_NODES.copy()), 2, 3, 1))
        drive("NodePool.diff/itself, no records", host_pool.diff, host_pool, records=False)
        drive("build_terrain", builder.build_terrain, 4)
        drive("build_terrain/options", builder.build_terrain, 5, tunnels=False, dedup=False, rand_kind="msvc", threads=3, use_gpu=True)
        records = rec.host("records", np.array([[0, 0, 0, 1], [1, 2, 3, 0]], np.uint32))
        wide = np.array([[0, 0, 0, 1], [-1, 2, 1 << 40, 0]], np.int64)
        grid8, grid32 = rec.host("grid8", np.zeros((4, 4, 4), np.uint8)), rec.host("grid32", np.zeros((2, 2, 2), np.uint32))
        drive("build_voxels/records", builder.build_voxels, records, depth=3)
        drive("build_voxels/int64 records, options", builder.build_voxels, wide, depth=3, use_gpu=True, threads=2, capacity=100)
        drive("build_voxels/int32 records", builder.build_voxels, records.view(np.int32), 3)
        drive("build_voxels/no records", builder.build_voxels, np.zeros((0, 4), np.uint8), 3)
        drive("build_voxels/grid u8", builder.build_voxels, grid8)
        drive("build_voxels/grid u32, depth", builder.build_voxels, grid32, depth=1)
        drive("edit_voxels", builder.edit_voxels, host_pool, records)
        drive("edit_voxels/tuple, int64 records, options", builder.edit_voxels, (nodes.reshape(-1), 2, 3), wide, use_gpu=True, threads=2,
              capacity=100)
        drive("box_records", builder.box_records, (0, 0, 0), (2, 1, 1), 5)
        drive("box_cubes", builder.box_cubes, (0, 0, 0), (4, 4, 4), 3)
        drive("occupied_box", builder.occupied_box, nodes, 1, 3)
        drive("occupied_box/0-based", builder.occupied_box, nodes.reshape(-1), 0, 3, index_base=0)
        drive("pack_pool", builder.pack_pool, nodes, 1, 3)
        device_list_ = Obj(is_cuda=True)
        zero_based = builder.NodePool(nodes, 0, 3, 0)
        refuse("NodePool.diff/not a pool", host_pool.diff, nodes)
        refuse("NodePool.diff/another depth", host_pool.diff, builder.NodePool(nodes, 1, 4, 1))
        refuse("NodePool.read_box/dtype", host_pool.read_box, (0, 0, 0), (1, 1, 1), np.int16)
        refuse("NodePool.read_box/floats", host_pool.read_box, (0.0, 0, 0), (1, 1, 1))
        refuse("NodePool.read_box/two numbers", host_pool.read_box, (0, 0, 0), (1, 1))
        refuse("NodePool.read_box/outside int32", host_pool.read_box, (0, 0, 0), (1, 1, 1 << 31))
        refuse("NodePool.read_box/hi below lo", host_pool.read_box, (0, 2, 0), (1, 1, 1))
        refuse("box_cubes/hi below lo", builder.box_cubes, (0, 2, 0), (1, 1, 1), 3)
        refuse("box_records/id", builder.box_records, (0, 0, 0), (1, 1, 1), -1)
        refuse("build_voxels/device list without use_gpu", builder.build_voxels, device_list_, depth=3)
        refuse("build_voxels/floats", builder.build_voxels, np.zeros((2, 4), np.float32), depth=3)
        refuse("build_voxels/id outside uint32", builder.build_voxels, np.array([[0, 0, 0, 1 << 32]], np.int64), depth=3)
        refuse("build_voxels/grid not cubic", builder.build_voxels, np.zeros((4, 4, 2), np.uint8))
        refuse("build_voxels/grid side", builder.build_voxels, np.zeros((3, 3, 3), np.uint8))
        refuse("build_voxels/grid dtype", builder.build_voxels, np.zeros((4, 4, 4), np.int32))
        refuse("build_voxels/grid and depth", builder.build_voxels, grid8, depth=3)
        refuse("build_voxels/shape", builder.build_voxels, np.zeros((5, 3), np.uint32), depth=3)
        refuse("build_voxels/no depth", builder.build_voxels, records)
        refuse("build_voxels/capacity", builder.build_voxels, records, depth=3, capacity=1 << 32)
        refuse("build_voxels/shape before depth and capacity", builder.build_voxels, np.zeros(4, np.uint32), capacity=-1)
        refuse("edit_voxels/0-based pool", builder.edit_voxels, zero_based, records)
        refuse("edit_voxels/device list without use_gpu", builder.edit_voxels, host_pool, device_list_)
        refuse("edit_voxels/shape", builder.edit_voxels, host_pool, grid8)
        refuse("edit_voxels/floats", builder.edit_voxels, host_pool, np.zeros((2, 4), np.float64))
        refuse("edit_voxels/root", builder.edit_voxels, (nodes, -1, 3), records)
        refuse("edit_voxels/capacity", builder.edit_voxels, host_pool, records, capacity=-1)
        refuse("edit_voxels/records before root", builder.edit_voxels, (nodes, -1, 3), np.zeros((5, 3), np.uint32))

        # -- world
        wd = drive("World", world.World, host_pool)
        made.append(wd)
        entries[-1]["returns"] = [wd.depth, wd.device, wd._h.value, wd.closed]
        w2 = drive("World/empty, capacity, device", world.World, (np.zeros((0, 8), np.uint32), 0, 4), capacity=1000, device=1)
        made.append(w2)
        drive("World/empty, capacity, device.close", w2.close)
        entries[-1]["returns"] = w2.closed
        drive("World.info", wd.info)
        drive("World.edit", wd.edit, records)
        drive("World.edit/int64 records", wd.edit, wide)
        drive("World.edit/no records", wd.edit, np.zeros((0, 4), np.int32))
        wpool = drive("World.make_pool", wd.make_pool)
        made.append(wpool)
        entries[-1]["returns"] = [type(wpool).__name__, wpool._h.value, wpool.depth, wpool.index_base, repr(wpool.miss_t)]
        drive("World.flush", wd.flush, wpool)
        drive("World.make_pool's pool.close", wpool.close)
        drive("World.download", wd.download)
        coords = rec.host("coords", np.array([[0, 0, 0], [1, 2, 3]], np.int32))
        drive("World.at", wd.at, coords)
        drive("World.at/int64", wd.at, np.array([[0, 0, 0], [1, 2, -3]], np.int64))
        drive("World.at/uint64", wd.at, np.array([[0, 0, 7]], np.uint64))
        drive("World.at/nothing", wd.at, np.zeros((0, 3), np.int32))
        drive("World.read_box", wd.read_box, (0, 1, 2), (4, 4, 4))
        drive("World.read_box/uint32, empty", wd.read_box, [0, 1, 2], [0, 4, 4], np.uint32)
        drive("World.tighten", wd.tighten)
        drive("World.compact", wd.compact)
        drive("World.snapshot", wd.snapshot)
        drive("World.checkout", wd.checkout, 5)
        drive("World.release", wd.release, np.uint64(5))
        drive("World.snapshots", wd.snapshots)
        drive("World.diff", wd.diff, 1)
        drive("World.diff/two snapshots, no records", wd.diff, 1, 3, records=False)
        drive("World.fill_box", wd.fill_box, (0, 1, 2), (4, 4, 4), 7)
        drive("World.restore_box", wd.restore_box, 3, (0, 1, 2), (4, 4, 4))
        stack = drive("UndoStack", world.UndoStack, wd, limit=2)
        drive("UndoStack.push", stack.push)
        drive("UndoStack.push/beyond the limit", stack.push)
        drive("UndoStack.undo", stack.undo)
        drive("UndoStack.undo/at the bottom", stack.undo)
        drive("UndoStack.redo", stack.redo)
        drive("UndoStack.redo/at the top", stack.redo)
        entries[-1]["returns"] = [stack.entries, stack.current]

        import torch
        bad_shape = Obj(is_cuda=True, dim=lambda: 3, shape=(2, 2, 4), dtype=torch.int32)
        elsewhere = Obj(is_cuda=True, dim=lambda: 2, dtype=torch.int32, device=OtherDevice())
        refuse("World/0-based pool", world.World, zero_based)
        refuse("World/root", world.World, (nodes, -1, 3))
        refuse("World/capacity", world.World, host_pool, capacity=1 << 32)
        refuse("World.edit/shape", wd.edit, np.zeros((5, 3), np.uint32))
        refuse("World.edit/floats", wd.edit, np.zeros((5, 4), np.float32))
        refuse("World.edit/id outside uint32", wd.edit, np.array([[0, 0, 0, -1]], np.int64))
        refuse("World.edit/device list of another shape", wd.edit, bad_shape)
        elsewhere.shape = (2, 4)
        refuse("World.edit/device list on another device", wd.edit, elsewhere)
        refuse("World.at/shape", wd.at, np.zeros((5, 4), np.int32))
        refuse("World.at/floats", wd.at, np.zeros((5, 3), np.float32))
        refuse("World.at/outside int32", wd.at, np.array([[0, 0, 1 << 31]], np.int64))
        refuse("World.at/device coordinates of another type", wd.at, Obj(is_cuda=True, dim=lambda: 2, shape=(2, 3), dtype=torch.int64))
        elsewhere.shape = (2, 3)
        refuse("World.at/device coordinates on another device", wd.at, elsewhere)
        refuse("World.read_box/dtype", wd.read_box, (0, 0, 0), (1, 1, 1), np.int16)
        refuse("World.read_box/hi below lo", wd.read_box, (0, 2, 0), (1, 1, 1))
        for name in ("checkout", "release"):
            refuse(f"World.{name}/not an integer", getattr(wd, name), 1.0)
            refuse(f"World.{name}/bool", getattr(wd, name), True)
            refuse(f"World.{name}/outside uint64", getattr(wd, name), -1)
        refuse("World.diff/handle", wd.diff, 1, "current")
        refuse("World.fill_box/box", wd.fill_box, (0, 2, 0), (1, 1, 1), 7)
        refuse("World.fill_box/id", wd.fill_box, (0, 0, 0), (1, 1, 1), 1 << 32)
        refuse("World.fill_box/bool id", wd.fill_box, (0, 0, 0), (1, 1, 1), True)
        refuse("World.restore_box/handle before box", wd.restore_box, None, (0, 2, 0), (1, 1, 1))
        refuse("World.restore_box/box", wd.restore_box, 3, (0, 0), (1, 1, 1))
        refuse("UndoStack/limit", world.UndoStack, wd, limit=1)
        drive("World.close", wd.close)
        entries[-1]["returns"] = wd.closed
        # a closed world: the order of the checks
        refuse("closed World.edit/shape comes first", wd.edit, np.zeros((5, 3), np.uint32))
        refuse("closed World.edit/records", wd.edit, records)
        refuse("closed World.edit/device list untouched", wd.edit, Obj(is_cuda=True))
        refuse("closed World.at/shape comes first", wd.at, np.zeros((5, 4), np.int32))
        refuse("closed World.at/coordinates", wd.at, coords)
        refuse("closed World.at/device type comes first", wd.at, Obj(is_cuda=True, dim=lambda: 2, shape=(2, 3), dtype=torch.int64))
        refuse("closed World.at/device coordinates", wd.at, elsewhere)
        refuse("closed World.read_box/box comes first", wd.read_box, (0, 2, 0), (1, 1, 1))
        refuse("closed World.read_box", wd.read_box, (0, 0, 0), (1, 1, 1))
        refuse("closed World.fill_box/closed comes first", wd.fill_box, (0, 2, 0), (1, 1, 1), 7)
        refuse("closed World.restore_box/closed comes first", wd.restore_box, None, (0, 0, 0), (1, 1, 1))
        refuse("closed World.checkout/closed comes first", wd.checkout, None)
        refuse("closed World.diff/closed comes first", wd.diff, None)
        for name in ("info", "make_pool", "download", "tighten", "compact", "snapshot", "snapshots"):
            refuse("closed World." + name, getattr(wd, name))
        refuse("closed World.flush", wd.flush, None)
    finally:
        for o in made:                       # nothing made here holds a handle the library could be asked to destroy
            o._h = C.c_void_p()
    return {"calls": entries, "refusals": refusals}


def pool_file_refusals(tmp_path):
    """NodePool.load's refusals (the file format's, not the C ABI's), the path left out of the text."""
    from octree_ray_tracing_amd.builder import NodePool
    good = tmp_path / "good.pool"
    NodePool(POOL_NODES, 1, 3, 1).save(good)
    raw = good.read_bytes()
    fmt = NodePool._HEADER

    def header(**kw):
        f = dict(zip(("magic", "version", "depth", "base", "root", "n", "crc"), fmt.unpack(raw[:fmt.size])))
        f.update(kw)
        return fmt.pack(*f.values()).ljust(64, b"\0")
    cases = {"truncated": raw[:40], "magic": header(magic=b"NOTAPOOL") + raw[64:], "version": header(version=3) + raw[64:],
             "size": raw[:-4], "depth": header(depth=23) + raw[64:], "base": header(base=2) + raw[64:],
             "root": header(root=3) + raw[64:], "0-based root": header(base=0, root=1) + raw[64:],
             "checksum": raw[:-1] + struct.pack("B", raw[-1] ^ 1)}
    out = []
    for label, data in cases.items():
        path = tmp_path / "bad.pool"
        path.write_bytes(data)
        with pytest.raises(ValueError) as e:
            NodePool.load(path)
        out.append({"wrapper": "NodePool.load/" + label, "type": "ValueError", "text": str(e.value).replace(str(path), "<path>")})
    return out


def whole_transcript(monkeypatch, tmp_path):
    t = transcript(monkeypatch)
    t["refusals"] += pool_file_refusals(tmp_path)
    return json.loads(json.dumps(t))


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    with pytest.MonkeyPatch.context() as mp:
        return whole_transcript(mp, tmp_path_factory.mktemp("pools"))


@pytest.fixture(scope="module")
def want():
    return json.loads(FIXTURE.read_text())


def test_every_wrapper_is_driven_once_per_label(got, want):
    for part in ("calls", "refusals"):
        labels = [e["wrapper"] for e in got[part]]
        assert labels == [e["wrapper"] for e in want[part]]
        assert len(set(labels)) == len(labels)


def test_what_reaches_the_library(got, want):
    for g, w in zip(got["calls"], want["calls"]):
        assert g["calls"] == w["calls"], g["wrapper"]


def test_what_the_wrappers_return(got, want):
    for g, w in zip(got["calls"], want["calls"]):
        assert g["returns"] == w["returns"], g["wrapper"]


def test_refusals(got, want):
    """Same input, same exception type, same text, and the same calls made before the refusal."""
    for g, w in zip(got["refusals"], want["refusals"]):
        assert g == w, g["wrapper"]


def test_the_recorder_stands_in_for_the_library(got):
    """Nothing was launched: the transcript names only entries of the binding's table."""
    import octree_ray_tracing_amd as ort
    names = {c[0] for e in got["calls"] for c in e["calls"] if isinstance(c[0], str)}
    assert names <= set(ort._lib.exported_symbols())
    assert len(names) > 100


if __name__ == "__main__" and "--write" in sys.argv:
    import tempfile
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    with pytest.MonkeyPatch.context() as mp, tempfile.TemporaryDirectory() as tmp:
        FIXTURE.write_text(json.dumps(whole_transcript(mp, Path(tmp)), indent=0, separators=(",", ":")) + "\n")
    print(f"wrote {FIXTURE}")
