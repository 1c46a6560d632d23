"""octree_ray_tracing_amd -- MI355X-native sparse-voxel-octree ray caster.

The hot path (Laine-Karras SVO/SVDAG traversal of the reference's
h_octree::sse_trace / octree::sse_trace, its camera ray generator and its
per-pixel shading loop) runs as hand-written gfx950 HIP kernels in
liboch_gpu.so behind the C ABI of include/och_gpu.h.  This package is the
host-side mirror of the reference interface over that ABI.
"""
from ._lib import LIGHT_AO, LIGHT_SUN, WHEN_IS, WHEN_IS_NOT, Light, OchError, library_path, load
from ._marshal import select_records
from .builder import (NodePool, box_cubes, box_records, build_terrain, build_voxels, edit_voxels, occupied_box, pack_pool,
                      sphere_cubes, sphere_records)
from .editor import Editor
from .frame import FrameGroup, RcclComm, ShardedFrame, ShardedSteps, box_downsample, code_table, shade_lit, shade_lit_codes
from .tracer import (Direction, GpuPool, HOctree, Octree, camera, deal_chunks, display_weight, device_count, device_list, host_rcp_lut,
                     light_check, rcp_from_lut, rcp_lut_error, shard_rows, split_defaults)
from .voxels import VoxelData, VoxelDataError
from .world import UndoStack, World

__all__ = ["LIGHT_AO", "LIGHT_SUN", "WHEN_IS", "WHEN_IS_NOT", "select_records", "Light", "light_check", "shade_lit", "shade_lit_codes", "code_table", "OchError", "library_path", "load", "NodePool", "build_terrain", "build_voxels", "edit_voxels", "box_records", "box_cubes", "sphere_records", "sphere_cubes", "occupied_box", "pack_pool", "Editor", "FrameGroup", "RcclComm", "ShardedFrame", "ShardedSteps", "box_downsample", "Direction", "GpuPool",
           "HOctree", "Octree", "camera", "deal_chunks", "display_weight", "device_count", "device_list", "host_rcp_lut", "rcp_from_lut", "rcp_lut_error", "shard_rows", "split_defaults",
           "VoxelData", "VoxelDataError", "World", "UndoStack"]
