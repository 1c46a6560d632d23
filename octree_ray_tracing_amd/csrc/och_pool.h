// och_pool.h -- the pool object as och_pool.cpp (which owns it), och_api.cpp
// (which launches on it) and och_rcp.cpp see it, and the few helpers these files
// call in each other.  Private to the three; the rest of the host layer reaches
// a pool through och_internal.h's och::pool_* and the C ABI.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "och_host.h"

namespace och {

// One cost-planned launch order (och_gpu_plan_views, och_gpu_plan_batch_tiled)
// and the launch it was planned for (frame_key, batch_key).
struct LaunchPlan {
    DevBuf<uint32_t> order;         // OCH_OPT_TILE_ORDER = 2
    DevBuf<uint32_t> order_xcd;     // OCH_OPT_TILE_ORDER = 3: grouped per XCD
    uint32_t blocks = 0;            // entries of the current plan (its launch's grid)
    std::vector<uint32_t> h_order, h_order_xcd;   // the host's copies: tile tables bake them in (use_tiles)
    uint64_t serial = 0;            // och_gpu_pool::plan_serial when the plan was made (tile-table keys)
    int64_t key[9] = {};
    // no plan until a new one is in place: later launches run in natural order
    void invalidate() { key[0] = -1; }
    bool matches(const int64_t k[9]) const { return order.d && std::memcmp(k, key, sizeof key) == 0; }
};

// The primary plan's split form (OCH_OPT_SPLIT, plan_split): the heavy tiles'
// split waves first, then the plan's other workgroups, and the waves' task
// rows; valid with plans[0]'s key while params matches the options it was
// made with
struct SplitPlan {
    DevBuf<uint32_t> order, tasks;
    std::vector<uint32_t> h_order, h_tasks;       // the host's copies (use_tiles)
    uint32_t n = 0, extra = 0, tiles = 0;
    int params[3] = {0, 0, 0};      // threshold, segments, level
    void invalidate() { n = extra = tiles = params[0] = params[1] = params[2] = 0; }
};

// One camera launch as the kernels run it (och::plan::tile_table), on the
// device, and the launch it was made for.  The pool keeps the last few: a frame
// loop's geometry, sharding and plan stay the same from frame to frame, so
// after the first frame a launch only looks its table up.
struct TileTable {
    DevBuf<uint64_t> d;
    uint32_t n = 0, grid = 0, block = 0;
    int64_t key[12] = {};
    uint64_t used = 0;              // och_gpu_pool::tile_clock at the last launch; 0 = empty
};

}  // namespace och

// ------------------------------------------------------------ pool object

struct och_gpu_pool {
    int device = 0;
    och::DevBuf<uint32_t> d_nodes;  // with one padding node in front for 1-based pools
    uint32_t n_nodes = 0;           // nodes in d_nodes
    uint32_t root = 0;
    int depth = 0;
    int index_base = 1;
    float miss_t = INFINITY;
    och::DevBuf<uint32_t> d_lut;    // .d: the pool has an RCPPS table
    int lut_log2 = 0;
    uint32_t rcp_xlo = 0, rcp_xspan = 0;   // DevPool::rcp_xlo / rcp_xspan of the uploaded table
    double lut_error = INFINITY;    // maximum relative error of the table (lut_max_rel_error)
    och::DevBuf<uint32_t> d_palette;
    uint32_t n_voxels = 0;
    och::DevBuf<uint32_t> d_code_table;  // .d: OCH_CODE_* -> RGBA8 (256 words), when n_voxels <= OCH_CODE_MAX_VOXELS
    hipStream_t own_stream = nullptr;
    hipStream_t ext_stream = nullptr;
    bool use_ext = false;           // och_gpu_set_stream called: ext_stream (NULL = null stream)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool timed = false;
    // schedule (och_gpu_set_option)
    int opt_block = 64;
    uint64_t *stamps = nullptr;
    uint32_t stamp_cap = 0;
    // host mirror of the uploaded nodes (user numbering), for validating edits
    std::vector<uint32_t> mirror;
    // packed layout (see och_internal.h DevPool)
    och::DevBuf<uint32_t> d_packed; // .d: a packed layout exists
    uint32_t packed_root = 0;
    uint32_t packed_nodes = 0;
    bool packed_by_slot = false;    // d_packed numbered like d_nodes (editor flushes)
    uint64_t serial = 0;            // process-unique, never reused (och::pool_serial)
    uint64_t last_writer = 0;       // editor id of the last och::pool_commit, 0 otherwise
    bool torn = false;              // a failed editor flush left the slots half written (och::pool_mark_torn)
    // A world's pool (och::pool_create_for_world): the world's id (0: an ordinary pool), and what
    // och_world_flush last wrote, ids [0, world_published) of generation world_generation.  Such a
    // pool has no mirror: och_gpu_pool_update and the editor's writes refuse it.
    uint64_t world = 0, world_generation = 0;
    uint32_t world_published = 0;
    int opt_layout = 1;
    int opt_tile_order = 0;
    int opt_bounce_compact = 1;
    int opt_cull = 1;
    int opt_timing = 1;                        // OCH_OPT_TIMING
    int opt_plan = 10;                         // OCH_OPT_PLAN (shape of och_gpu_plan_views' order)
    int opt_split = 0;                         // OCH_OPT_SPLIT: heavy-tile threshold, % of the costliest tile (0 off)
    int opt_split_segs = 4;                    // OCH_OPT_SPLIT_SEGS: lanes per heavy tile's ray (2, 4, 8, 16)
    int opt_split_level = 6;                   // OCH_OPT_SPLIT_LEVEL: the level whose cells are the segments
    hipEvent_t next_ev_start = nullptr;        // och_gpu_set_launch_events: the next launch's events
    hipEvent_t next_ev_stop = nullptr;
    // bounding box of the pool's voxels (voxel units, [lo, hi)), for the cull
    bool box_any = false;
    int32_t box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    // host-call staging
    och::DevBuf<char> scratch;
    // editor flush staging (och::pool_scatter_slots): pinned host + device, grown on demand
    uint32_t *h_stage = nullptr;
    size_t stage_words = 0;
    och::DevBuf<uint32_t> d_stage;
    // cost-planned launch orders (och_gpu_plan_views, OCH_OPT_TILE_ORDER = 2)
    // [0] primary frames (grid kernel), [1] config-5 frames (bounce kernel),
    // [2] tiled trace batches (och_gpu_plan_batch_tiled)
    och::LaunchPlan plans[3];
    och::SplitPlan split;
    uint64_t plan_serial = 0;                 // counts the plans made (och_gpu_plan_views)
    och::TileTable tile_tables[8];            // camera launches' tile tables (use_tiles), least recently used out first
    uint64_t tile_clock = 0;
    // row deal (och_gpu_set_row_deal): for frames of deal_h rows in chunks of
    // deal_chunk over deal_n shards, chunk g belongs to a chosen shard instead
    // of g % n; slices hold deal_max chunks (the largest shard's, the rest padded)
    int deal_h = 0, deal_chunk = 0, deal_n = 0, deal_max = 0;
    uint64_t deal_serial = 0;                 // changes with every deal (plan keys)
    och::DevBuf<int32_t> d_chunk_map;         // [deal_n][deal_max] global chunk, -1 = padding
    std::vector<int32_t> h_chunk_map;         // and the host's copy (tile tables)
    och::DevBuf<int32_t> d_owner;             // [n_chunks] shard << 16 | local chunk
    std::vector<int32_t> deal_table;          // the chunk -> shard table as set
    bool deal_for(int H, int rc, int n) const { return deal_n && H == deal_h && rc == deal_chunk && n == deal_n; }
    int slice_rows(int H, int rc, int n) const { return deal_for(H, rc, n) ? deal_max * rc : och_shard_rows(H, rc, n); }

    hipStream_t stream() const { return use_ext ? ext_stream : own_stream; }

    // No packed layout: launches walk the raw one until a new one is in place.
    hipError_t drop_packed()
    {
        packed_nodes = 0;
        packed_by_slot = false;
        return d_packed.release();
    }

    och::Schedule schedule() const
    {
        och::Schedule sc = {};          // no order, no cost output, no split, no events
        sc.block = opt_block;
        sc.tile_order = opt_tile_order;
        sc.bounce_compact = opt_bounce_compact;
        sc.stamps = stamps;
        sc.stamp_cap = stamp_cap;
        return sc;
    }

    och::DevPool dev() const
    {
        och::DevPool p;
        const bool pk = opt_layout == 1 && d_packed.d;
        p.nodes = pk ? d_packed.d : d_nodes.d;
        p.n_slots = 8u * (pk ? packed_nodes : n_nodes);
        p.packed = pk ? 1 : 0;
        p.lut = d_lut.d;
        p.rcp_xlo = rcp_xlo;
        p.rcp_xspan = rcp_xspan;
        p.root = pk ? packed_root : root;
        p.depth = depth;
        p.lut_shift = 23 - lut_log2;
        uint32_t mb;
        std::memcpy(&mb, &miss_t, 4);
        p.miss_bits = mb;
        p.half_voxel = std::ldexp(1.0F, -(depth + 1));
        p.dim_lo = 1u << (23 - depth);
        p.dim_span = (1u << 22) - p.dim_lo;
        // 1 + k / 2^depth is an exact float for depth <= 22
        p.cull = box_any ? opt_cull : 0;
        p.cam_cull = lut_error <= och::kCameraCullRcpError ? 1 : 0;
        for (int a = 0; a < 3; ++a) {
            p.cull_lo[a] = 1.0F + std::ldexp((float)box_lo[a], -depth);
            p.cull_hi[a] = 1.0F + std::ldexp((float)box_hi[a], -depth);
        }
        return p;
    }
};

namespace och {

// och_pool.cpp
int ensure_scratch(och_gpu_pool *p, size_t bytes);
int check_ready(const och_gpu_pool *p);

// och_rcp.cpp: this host's RCPPS as a table (made once), and a table's error
struct HostRcp {
    int status = OCH_OK;
    int log2_entries = 0;
    std::vector<uint32_t> lut;
    std::string error;
};

const HostRcp &host_rcp();
double lut_max_rel_error(const uint32_t *lut, int log2_entries);

}  // namespace och
