// och_api.cpp -- the C ABI (include/och_gpu.h): pools, RCPPS capture, camera
// constants, synchronous and asynchronous trace / render entry points.
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "och_host.h"

using och::check_views;
using och::DevBuf;
using och::DeviceGuard;
using och::fail;

namespace {

constexpr uint32_t kIdLimit = 1u << 24;   // packed ids are 24 bits

thread_local std::string g_error;

}  // namespace

int och::fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return status;
}

namespace {

thread_local const char *t_entry = nullptr;     // outermost C-ABI entry of this thread

// The first pending HIP error a launcher cleared since the last reset, process
// wide (the frame group issues from one thread per device), and how many.
struct Discarded {
    std::mutex m;
    int code = 0;
    int count = 0;
    std::string what;
};

Discarded &discarded()
{
    static Discarded d;
    return d;
}

// ------------------------------------------------------------ RCPPS capture

inline uint32_t rcpps_native(uint32_t x)
{
    const __m128 r = _mm_rcp_ps(_mm_castsi128_ps(_mm_set1_epi32((int)x)));
    return (uint32_t)_mm_cvtsi128_si32(_mm_castps_si128(r));
}

struct HostRcp {
    int status = OCH_OK;
    int log2_entries = 0;
    std::vector<uint32_t> lut;
    std::string error;
};

const HostRcp &host_rcp()
{
    static HostRcp cap;
    static std::once_flag once;
    std::call_once(once, [] {
        const uint32_t n = 1u << 23;
        std::vector<uint32_t> full(n);
        for (uint32_t m = 0; m < n; m += 4) {
            const __m128i x = _mm_set_epi32((int)(0xBF800000u | (m + 3)), (int)(0xBF800000u | (m + 2)),
                                            (int)(0xBF800000u | (m + 1)), (int)(0xBF800000u | m));
            _mm_storeu_si128((__m128i *)&full[m], _mm_castps_si128(_mm_rcp_ps(_mm_castsi128_ps(x))));
        }
        // Smallest k such that the result only depends on the top k mantissa bits.
        int k = 23;
        for (int cand = 8; cand <= 23; ++cand) {
            const uint32_t block = 1u << (23 - cand);
            bool ok = true;
            for (uint32_t m = 0; m < n && ok; ++m) ok = full[m] == full[m & ~(block - 1)];
            if (ok) { k = cand; break; }
        }
        cap.log2_entries = k;
        cap.lut.resize(1u << k);
        for (uint32_t i = 0; i < (1u << k); ++i) cap.lut[i] = full[(size_t)i << (23 - k)];
        // Check the exponent model on every exponent (negative inputs, as the tracer uses).
        for (uint32_t e = 0; e < 256 && cap.status == OCH_OK; ++e)
            for (uint32_t m = 0; m < n; m += (e == 127 ? 1u : 997u)) {
                const uint32_t x = 0x80000000u | (e << 23) | m;
                if (e == 255 && m) continue;   // NaN payload handling is not used by the tracer
                const uint32_t want = rcpps_native(x);
                const uint32_t got = och_rcp_from_lut(x, cap.lut.data(), k);
                if (want != got) {
                    cap.status = OCH_E_RCP_MODEL;
                    char buf[160];
                    snprintf(buf, sizeof buf, "host RCPPS(0x%08x) = 0x%08x, table model gives 0x%08x", x, want, got);
                    cap.error = buf;
                    break;
                }
            }
    });
    return cap;
}

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

}  // namespace

// ------------------------------------------------------------ pool object

struct och_gpu_pool {
    int device = 0;
    DevBuf<uint32_t> d_nodes;       // with one padding node in front for 1-based pools
    uint32_t n_nodes = 0;           // nodes in d_nodes
    uint32_t root = 0;
    int depth = 0;
    int index_base = 1;
    float miss_t = INFINITY;
    DevBuf<uint32_t> d_lut;         // .d: the pool has an RCPPS table
    int lut_log2 = 0;
    uint32_t rcp_xlo = 0, rcp_xspan = 0;   // DevPool::rcp_xlo / rcp_xspan of the uploaded table
    double lut_error = INFINITY;    // maximum relative error of the table (lut_max_rel_error)
    DevBuf<uint32_t> d_palette;
    uint32_t n_voxels = 0;
    DevBuf<uint32_t> d_code_table;  // .d: OCH_CODE_* -> RGBA8 (256 words), when n_voxels <= OCH_CODE_MAX_VOXELS
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
    DevBuf<uint32_t> d_packed;      // .d: a packed layout exists
    uint32_t packed_root = 0;
    uint32_t packed_nodes = 0;
    bool packed_by_slot = false;    // d_packed numbered like d_nodes (editor flushes)
    uint64_t serial = 0;            // process-unique, never reused (och::pool_serial)
    uint64_t last_writer = 0;       // editor id of the last och::pool_commit, 0 otherwise
    bool torn = false;              // a failed editor flush left the slots half written (och::pool_mark_torn)
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
    DevBuf<char> scratch;
    // editor flush staging (och::pool_scatter_slots): pinned host + device, grown on demand
    uint32_t *h_stage = nullptr;
    size_t stage_words = 0;
    DevBuf<uint32_t> d_stage;
    // cost-planned launch orders (och_gpu_plan_views, OCH_OPT_TILE_ORDER = 2)
    // [0] primary frames (grid kernel), [1] config-5 frames (bounce kernel),
    // [2] tiled trace batches (och_gpu_plan_batch_tiled)
    LaunchPlan plans[3];
    SplitPlan split;
    uint64_t plan_serial = 0;                 // counts the plans made (och_gpu_plan_views)
    TileTable tile_tables[8];                 // camera launches' tile tables (use_tiles), least recently used out first
    uint64_t tile_clock = 0;
    // row deal (och_gpu_set_row_deal): for frames of deal_h rows in chunks of
    // deal_chunk over deal_n shards, chunk g belongs to a chosen shard instead
    // of g % n; slices hold deal_max chunks (the largest shard's, the rest padded)
    int deal_h = 0, deal_chunk = 0, deal_n = 0, deal_max = 0;
    uint64_t deal_serial = 0;                 // changes with every deal (plan keys)
    DevBuf<int32_t> d_chunk_map;              // [deal_n][deal_max] global chunk, -1 = padding
    std::vector<int32_t> h_chunk_map;         // and the host's copy (tile tables)
    DevBuf<int32_t> d_owner;                  // [n_chunks] shard << 16 | local chunk
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

namespace {

int ensure_scratch(och_gpu_pool *p, size_t bytes)
{
    OCH_HIP(p->scratch.reserve(bytes));
    return OCH_OK;
}

// Launches refuse a pool that a failed editor flush left half written: its
// slots may name nodes that were never uploaded.
int check_ready(const och_gpu_pool *p)
{
    if (p->torn)
        return fail(OCH_E_INVALID, "pool left half written by a failed och_editor_flush: flush the editor again");
    if (!p->d_lut.d) return fail(OCH_E_RCP_MODEL, "no RCPPS table on this pool (call och_gpu_set_rcp_lut)");
    return OCH_OK;
}

// Walk every reachable (node, level) pair once and check that interior slots
// name nodes inside the pool, so no kernel can read out of bounds.
int validate_pool(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int base)
{
    if (depth < 1 || depth > 22) return fail(OCH_E_INVALID, "depth %d outside 1..22", depth);
    if (n_nodes == 0) return fail(OCH_E_INVALID, "empty node array");
    if ((uint64_t)n_nodes + 1 >= (1ull << 29)) return fail(OCH_E_INVALID, "pool of %u nodes exceeds 2^29", n_nodes);
    auto in_range = [&](uint32_t v) { return base == 1 ? (v >= 1 && v <= n_nodes) : (v < n_nodes); };
    if (base == 1 && root == 0) return OCH_OK;   // empty h_octree: every ray misses
    if (!in_range(root)) return fail(OCH_E_INVALID, "root %u outside the pool", root);
    std::vector<uint32_t> seen(n_nodes, 0);
    std::vector<uint32_t> cur{root}, next;
    seen[root - base] |= 1u << 1;
    for (int level = 1; level < depth; ++level) {
        next.clear();
        for (uint32_t v : cur) {
            const uint32_t *c = nodes + (size_t)(v - base) * 8;
            for (int k = 0; k < 8; ++k) {
                if (!c[k]) continue;
                if (!in_range(c[k]) || (base == 0 && c[k] == 0))
                    return fail(OCH_E_INVALID, "node %u (level %d) slot %d names %u, outside the pool", v, level, k, c[k]);
                uint32_t &s = seen[c[k] - base];
                if (!(s & (1u << (level + 1)))) {
                    s |= 1u << (level + 1);
                    next.push_back(c[k]);
                }
            }
        }
        cur.swap(next);
    }
    return OCH_OK;
}

}  // namespace

// Bounding box of the voxels: one post-order walk over the (node, level)
// pairs, each box memoised in node-local voxel units (a DAG shares subtrees;
// a node the caller's table shares between levels gets one entry per level).
bool och::occupied_box(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int base, int32_t lo[3],
                       int32_t hi[3])
{
    struct Box {
        int32_t lo[3], hi[3];
        bool empty() const { return lo[0] >= hi[0]; }
    };
    if ((base == 1 && root == 0) || n_nodes == 0) return false;
    std::vector<uint8_t> memo_level(n_nodes, 0);     // level + 1 of memo[i], 0 = none
    std::vector<Box> memo(n_nodes);
    std::unordered_map<uint64_t, Box> extra;
    auto walk = [&](auto &self, uint32_t v, int level) -> Box {
        const uint32_t i = v - base;
        const uint64_t key = ((uint64_t)i << 5) | (uint64_t)level;
        if (memo_level[i] == level + 1) return memo[i];
        if (memo_level[i]) {
            auto it = extra.find(key);
            if (it != extra.end()) return it->second;
        }
        Box b{{INT32_MAX, INT32_MAX, INT32_MAX}, {INT32_MIN, INT32_MIN, INT32_MIN}};
        const int32_t half = 1 << (depth - level - 1);   // a child's size in voxels
        const uint32_t *c = nodes + (size_t)i * 8;
        for (int k = 0; k < 8; ++k) {
            if (!c[k]) continue;
            Box cb{{0, 0, 0}, {1, 1, 1}};                // leaf level: the voxel itself
            if (level + 1 < depth) {
                cb = self(self, c[k], level + 1);
                if (cb.empty()) continue;
            }
            for (int a = 0; a < 3; ++a) {
                const int32_t off = ((k >> a) & 1) * half;
                b.lo[a] = std::min(b.lo[a], off + cb.lo[a]);
                b.hi[a] = std::max(b.hi[a], off + cb.hi[a]);
            }
        }
        if (b.lo[0] == INT32_MAX) b = Box{{0, 0, 0}, {0, 0, 0}};
        if (!memo_level[i]) {
            memo_level[i] = (uint8_t)(level + 1);
            memo[i] = b;
        } else {
            extra.emplace(key, b);
        }
        return b;
    };
    const Box b = walk(walk, root, 0);
    if (b.empty()) return false;
    for (int a = 0; a < 3; ++a) {
        lo[a] = b.lo[a];
        hi[a] = b.hi[a];
    }
    return true;
}

namespace {

void set_box(och_gpu_pool *p, const uint32_t *nodes, uint32_t n_nodes)
{
    p->box_any = och::occupied_box(nodes, n_nodes, p->root, p->depth, p->index_base, p->box_lo, p->box_hi);
}

// Packed layout: every reachable (node, level) pair gets a breadth-first id
// (1-based; 0 is a zero padding node).  Interior slots become
// child_id | child_mask << 24, leaf-level slots keep the voxel ids.  A node
// the caller's table shares between levels (h_octree hash-conses by content
// alone) is simply emitted once per level.  Returns false when more than
// 2^24 - 1 ids would be needed.
bool pack_pool(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int base,
               std::vector<uint32_t> &out, uint32_t &packed_root)
{
    auto mask_of = [&](uint32_t v) {
        const uint32_t *c = nodes + (size_t)(v - base) * 8;
        uint32_t m = 0;
        for (int k = 0; k < 8; ++k) m |= (uint32_t)(c[k] != 0) << k;
        return m;
    };
    out.assign(8, 0u);                               // padding node 0
    if (base == 1 && root == 0) {
        packed_root = 0;
        return true;
    }
    // id of (v, level): first_level[v] / first_id[v] hold the common case, a
    // map holds the rare extra levels.
    std::vector<uint8_t> first_level(n_nodes, 0);
    std::vector<uint32_t> first_id(n_nodes, 0);
    std::unordered_map<uint64_t, uint32_t> extra;
    std::vector<uint32_t> order_v;
    std::vector<uint8_t> order_l;
    uint32_t next = 1;
    auto id_of = [&](uint32_t v, int level, bool create) -> uint32_t {
        const uint32_t i = v - base;
        if (first_level[i] == level) return first_id[i];
        if (first_level[i] == 0) {
            if (!create) return 0;
            first_level[i] = (uint8_t)level;
            first_id[i] = next;
            order_v.push_back(v);
            order_l.push_back((uint8_t)level);
            return next++;
        }
        const uint64_t key = ((uint64_t)i << 5) | (uint64_t)level;
        auto it = extra.find(key);
        if (it != extra.end()) return it->second;
        if (!create) return 0;
        extra.emplace(key, next);
        order_v.push_back(v);
        order_l.push_back((uint8_t)level);
        return next++;
    };
    id_of(root, 1, true);
    for (size_t q = 0; q < order_v.size(); ++q) {        // breadth-first: order grows as we go
        const int level = order_l[q];
        if (level >= depth) continue;
        const uint32_t *c = nodes + (size_t)(order_v[q] - base) * 8;
        for (int k = 0; k < 8; ++k)
            if (c[k]) id_of(c[k], level + 1, true);
        if (next > kIdLimit) return false;
    }
    out.resize((size_t)next * 8, 0u);
    for (size_t q = 0; q < order_v.size(); ++q) {
        const uint32_t v = order_v[q];
        const int level = order_l[q];
        const uint32_t *c = nodes + (size_t)(v - base) * 8;
        uint32_t *o = out.data() + (q + 1) * 8;
        for (int k = 0; k < 8; ++k) {
            if (!c[k]) continue;
            o[k] = level == depth ? c[k] : (id_of(c[k], level + 1, false) | (mask_of(c[k]) << 24));
        }
    }
    packed_root = 1u | (mask_of(root) << 24);
    return true;
}

int upload_packed(och_gpu_pool *p, const uint32_t *nodes, uint32_t n_nodes)
{
    std::vector<uint32_t> packed;
    uint32_t proot = 0;
    OCH_HIP(p->drop_packed());
    if (!pack_pool(nodes, n_nodes, p->root, p->depth, p->index_base, packed, proot))
        return OCH_OK;   // raw only
    OCH_HIP(p->d_packed.upload(packed));
    p->packed_root = proot;
    p->packed_nodes = (uint32_t)(packed.size() / 8);
    return OCH_OK;
}

// Largest relative error |r * x - 1| of the table model over x in [-2, -1):
// entry k serves the mantissa bin [k, k + 1) / 2^L, so the extremes are at
// the bin's ends.  Non-finite or zero entries count as an infinite error.
double lut_max_rel_error(const uint32_t *lut, int log2_entries)
{
    const uint32_t n = 1u << log2_entries;
    double worst = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        float r;
        std::memcpy(&r, &lut[k], 4);
        if (!std::isfinite(r) || r == 0.0F) return INFINITY;
        const double lo = -(1.0 + (double)k / n), hi = -(1.0 + (double)(k + 1) / n);
        worst = std::max({worst, std::fabs((double)r * lo - 1.0), std::fabs((double)r * hi - 1.0)});
    }
    return worst;
}

int upload_lut(och_gpu_pool *p, const uint32_t *lut, int log2_entries)
{
    if (!lut || log2_entries < 1 || log2_entries > 23) return fail(OCH_E_INVALID, "bad RCPPS table");
    OCH_HIP(p->d_lut.release());       // no table until the new one is in place
    // The device table holds every entry + (127 << 23): the kernels' RCPPS of
    // x = -|d| is then entry - (x's exponent bits) wherever the model's result
    // exponent ent_e + 127 - e stays in 1..254 and the entry is negative -- for
    // e in [max(1, max_e - 127), min_e + 126] over this table's entries (och_kernels.hip
    // rcpps); other x, and every x of a table with a non-negative entry, take
    // the model itself.
    const uint32_t n = 1u << log2_entries;
    std::vector<uint32_t> adj(n);
    int min_e = 255, max_e = 0;
    bool negative = true;
    for (uint32_t k = 0; k < n; ++k) {
        const int e = (int)((lut[k] >> 23) & 0xFFu);
        min_e = std::min(min_e, e);
        max_e = std::max(max_e, e);
        negative = negative && (lut[k] >> 31) != 0;
        adj[k] = lut[k] + (127u << 23);
    }
    const int e_lo = std::max(1, max_e - 127), e_hi = std::min(254, min_e + 126);
    p->rcp_xlo = (uint32_t)e_lo << 23;
    p->rcp_xspan = negative && e_hi >= e_lo ? (uint32_t)(e_hi - e_lo + 1) << 23 : 0u;
    OCH_HIP(p->d_lut.upload(adj));
    p->lut_log2 = log2_entries;
    // camera_proven_miss budgets the table's error; a coarser table leaves
    // every camera ray to the exact ray_cull
    p->lut_error = lut_max_rel_error(lut, log2_entries);
    return OCH_OK;
}

}  // namespace

extern "C" {

OCH_API int och_abi_version(void) { return OCH_GPU_ABI_VERSION; }

OCH_API const char *och_last_error(void) { return g_error.c_str(); }

OCH_API int och_discarded_error(int *hip_error, int *count, char *what, size_t what_cap, int reset)
{
    auto &d = discarded();
    std::lock_guard<std::mutex> lk(d.m);
    if (hip_error) *hip_error = d.code;
    if (count) *count = d.count;
    if (what && what_cap) snprintf(what, what_cap, "%s", d.what.c_str());
    if (reset) {
        d.code = d.count = 0;
        d.what.clear();
    }
    return OCH_OK;
}

OCH_API int och_device_list(int *devices, int capacity, int *count)
{
    if (!count || (capacity > 0 && !devices)) return fail(OCH_E_INVALID, "NULL argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    int gfx950 = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) {
            if (gfx950 < capacity) devices[gfx950] = i;
            ++gfx950;
        }
    }
    *count = gfx950;
    return OCH_OK;
}

OCH_API int och_device_count(int *count)
{
    if (!count) return fail(OCH_E_INVALID, "count is NULL");
    return och_device_list(nullptr, 0, count);
}

OCH_API uint32_t och_rcp_from_lut(uint32_t x, const uint32_t *lut, int log2_entries)
{
    const uint32_t sign = x & 0x80000000u, e = (x >> 23) & 0xFFu;
    if (e == 0) return sign | 0x7F800000u;
    if (e == 0xFFu) return (x & 0x7FFFFFu) ? (x | 0x400000u) : sign;
    const uint32_t ent = lut[(x & 0x7FFFFFu) >> (23 - log2_entries)];
    const int ne = (int)((ent >> 23) & 0xFFu) + 127 - (int)e;
    return ne <= 0 ? sign : (sign | ((uint32_t)ne << 23) | (ent & 0x7FFFFFu));
}

OCH_API int och_rcp_lut_error(const uint32_t *lut, int log2_entries, double *max_rel_error)
{
    if (!lut || !max_rel_error || log2_entries < 1 || log2_entries > 23) return fail(OCH_E_INVALID, "bad RCPPS table");
    *max_rel_error = lut_max_rel_error(lut, log2_entries);
    return OCH_OK;
}

OCH_API int och_host_rcp_lut(uint32_t *lut, int *log2_entries)
{
    const HostRcp &c = host_rcp();
    if (c.status != OCH_OK) return fail(c.status, "%s", c.error.c_str());
    if (lut) std::memcpy(lut, c.lut.data(), c.lut.size() * sizeof(uint32_t));
    if (log2_entries) *log2_entries = c.log2_entries;
    return OCH_OK;
}

OCH_API int och_gpu_pool_create(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                                float miss_t, int device, och_gpu_pool **out)
{
    if (!nodes || !out) return fail(OCH_E_INVALID, "nodes/out is NULL");
    if (index_base != 0 && index_base != 1) return fail(OCH_E_INVALID, "index_base must be 0 or 1");
    *out = nullptr;
    int st = validate_pool(nodes, n_nodes, root, depth, index_base);
    if (st != OCH_OK) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(OCH_E_NODEV, "no HIP device visible");
    if (device < 0) OCH_HIP(hipGetDevice(&device));
    if (device >= ndev) return fail(OCH_E_NODEV, "device %d of %d", device, ndev);
    DeviceGuard g(device);
    if (!g.ok) return fail(OCH_E_HIP, "hipSetDevice(%d) failed", device);

    och_gpu_pool *p = new och_gpu_pool;
    static std::atomic<uint64_t> next_serial{1};
    p->serial = next_serial.fetch_add(1);
    p->device = device;
    p->depth = depth;
    p->index_base = index_base;
    p->miss_t = miss_t;
    p->root = root;
    p->n_nodes = n_nodes + (uint32_t)index_base;   // padding node 0 for 1-based pools
    auto bail = [&](int s) { och_gpu_pool_destroy(p); return s; };
    if (p->d_nodes.reserve((size_t)p->n_nodes * 8) != hipSuccess)
        return bail(fail(OCH_E_NOMEM, "hipMalloc(%zu) failed", (size_t)p->n_nodes * 32));
    if (index_base == 1 && hipMemset(p->d_nodes.d, 0, 32) != hipSuccess) return bail(fail(OCH_E_HIP, "hipMemset failed"));
    if (hipMemcpy(p->d_nodes.d + 8 * index_base, nodes, (size_t)n_nodes * 32, hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(OCH_E_HIP, "node upload failed"));
    p->mirror.assign(nodes, nodes + (size_t)n_nodes * 8);
    set_box(p, nodes, n_nodes);
    st = upload_packed(p, nodes, n_nodes);
    if (st != OCH_OK) return bail(st);
    if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess ||
        // timing only: no system-scope release at the timed kernel's end
        hipEventCreateWithFlags(&p->ev_start, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_stop, hipEventDisableSystemFence) != hipSuccess)
        return bail(fail(OCH_E_HIP, "stream/event creation failed"));
    const HostRcp &rc = host_rcp();
    if (rc.status == OCH_OK) {
        st = upload_lut(p, rc.lut.data(), rc.log2_entries);
        if (st != OCH_OK) return bail(st);
    }
    // A host whose RCPPS does not fit the model leaves the pool without a table:
    // tracing then fails with OCH_E_RCP_MODEL until och_gpu_set_rcp_lut is called.
    *out = p;
    return OCH_OK;
}

OCH_API int och_gpu_pool_destroy(och_gpu_pool *p)
{
    if (!p) return OCH_OK;
    DeviceGuard g(p->device);
    if (p->own_stream) (void)hipStreamSynchronize(p->own_stream);
    if (p->use_ext) (void)hipStreamSynchronize(p->ext_stream);
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    // all device memory is held in DevBufs, freed by delete below (on the pool's device: g)
    if (p->ev_start) (void)hipEventDestroy(p->ev_start);
    if (p->ev_stop) (void)hipEventDestroy(p->ev_stop);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    delete p;
    return OCH_OK;
}

OCH_API int och_gpu_pool_info(const och_gpu_pool *p, och_pool_info *info)
{
    if (!p || !info) return fail(OCH_E_INVALID, "pool/info is NULL");
    info->device_bytes = (uint64_t)p->n_nodes * 32;
    info->n_nodes = p->n_nodes;
    info->root = p->root;
    info->depth = p->depth;
    info->index_base = p->index_base;
    info->miss_t = p->miss_t;
    info->rcp_log2_entries = p->d_lut.d ? p->lut_log2 : 0;
    info->device = p->device;
    return OCH_OK;
}

OCH_API int och_gpu_pool_update(och_gpu_pool *p, uint32_t first, uint32_t count, const uint32_t *nodes, uint32_t root)
{
    OCH_ENTRY();
    if (!p || (count && !nodes)) return fail(OCH_E_INVALID, "pool/nodes is NULL");
    if (p->torn) return fail(OCH_E_INVALID, "pool left half written by a failed och_editor_flush: flush the editor again");
    const uint32_t n_user = p->n_nodes - (uint32_t)p->index_base;
    const uint32_t lo = p->index_base == 1 ? 1u : 0u;
    if (count && (first < lo || (uint64_t)first - lo + count > n_user))
        return fail(OCH_E_INVALID, "update [%u, +%u) outside the pool", first, count);
    // Apply to the host mirror and re-validate everything reachable from the
    // new root before any byte reaches the device (h_octree::set keeps the
    // pool consistent, ORT/och_h_octree.h:176-237; a bad edit must not fault).
    const size_t off = (size_t)(first - lo) * 8;
    std::vector<uint32_t> saved(p->mirror.begin() + off, p->mirror.begin() + off + (size_t)count * 8);
    std::memcpy(p->mirror.data() + off, nodes, (size_t)count * 32);
    const int st = validate_pool(p->mirror.data(), n_user, root, p->depth, p->index_base);
    if (st != OCH_OK) {
        std::memcpy(p->mirror.data() + off, saved.data(), saved.size() * 4);
        return st;
    }
    // slots are rewritten in place: kernels of frames in flight on any stream
    // may still walk them (as the editor's flush)
    int ds = och::pool_drain(p);
    if (ds != OCH_OK) return ds;
    DeviceGuard g(p->device);
    if (count)
        OCH_HIP(hipMemcpyAsync(p->d_nodes.d + 8 * (size_t)(first - lo + p->index_base), p->mirror.data() + off,
                               (size_t)count * 32, hipMemcpyHostToDevice, p->stream()));
    OCH_HIP(hipStreamSynchronize(p->stream()));
    p->root = root;
    p->last_writer = 0;
    set_box(p, p->mirror.data(), n_user);
    return upload_packed(p, p->mirror.data(), n_user);
}

}  // extern "C"

int och::report(int status, const char *msg) { return fail(status, "%s", msg); }

// ------------------------------------------------------------ discarded errors


och::EntryScope::EntryScope(const char *name) : prev(t_entry)
{
    if (!t_entry) t_entry = name;
}

och::EntryScope::~EntryScope() { t_entry = prev; }

void och::clear_pending_error(const char *launcher)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return;
    Discarded &d = discarded();
    std::lock_guard<std::mutex> lk(d.m);
    if (d.count++ == 0) {
        char buf[320];
        snprintf(buf, sizeof buf, "%s (%d) pending at %s, cleared by %s", hipGetErrorName(e), (int)e,
                 t_entry ? t_entry : "an internal call", launcher);
        d.code = (int)e;
        d.what = buf;
    }
}

uint64_t och::pool_serial(const och_gpu_pool *p) { return p ? p->serial : 0; }
void *och::pool_stream(const och_gpu_pool *p) { return p ? static_cast<void *>(p->stream()) : nullptr; }
int och::pool_palette_size(const och_gpu_pool *p, int *n)
{
    if (!p || !n) return fail(OCH_E_INVALID, "NULL argument");
    *n = (int)p->n_voxels;
    return OCH_OK;
}
uint64_t och::pool_last_writer(const och_gpu_pool *p) { return p ? p->last_writer : 0; }

int och::pool_drain(och_gpu_pool *p)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    DeviceGuard g(p->device);
    // Every stream, not just the pool's: bench and frame code rotate the pool
    // over several streams with frames in flight, and a kernel still walking a
    // slot that is rewritten in place could read a torn DAG.
    OCH_HIP(hipDeviceSynchronize());
    return OCH_OK;
}

int och::pool_write_slots(och_gpu_pool *p, uint32_t first, uint32_t count, const uint32_t *raw,
                          const uint32_t *packed, bool full)
{
    if (!p || p->index_base != 1 || (count && !raw)) return fail(OCH_E_INVALID, "bad editor flush");
    if ((uint64_t)first + count > p->n_nodes || (full && (first != 0 || count != p->n_nodes)))
        return fail(OCH_E_INVALID, "editor window [%u, +%u) outside the pool", first, count);
    if (packed && p->n_nodes > kIdLimit) return fail(OCH_E_INVALID, "packed ids exceed 24 bits");
    if (packed && !full && (!p->d_packed.d || !p->packed_by_slot))
        return fail(OCH_E_INVALID, "packed buffer is not in editor numbering");
    DeviceGuard g(p->device);
    p->last_writer = 0;                 // until pool_commit: a failed flush forces a full rewrite
    // mirror and raw device slots: slot 0 is the padding node, never written
    const uint32_t lo = first ? first : 1;
    const uint32_t skip = lo - first;
    if (count > skip) {
        const size_t n = (size_t)(count - skip) * 8;
        std::memcpy(p->mirror.data() + (size_t)(lo - 1) * 8, raw + (size_t)skip * 8, n * 4);
        OCH_HIP(hipMemcpy(p->d_nodes.d + (size_t)lo * 8, raw + (size_t)skip * 8, n * 4, hipMemcpyHostToDevice));
    }
    if (!packed) return OCH_OK;
    if (full && (!p->d_packed.d || !p->packed_by_slot || p->packed_nodes != p->n_nodes)) {
        OCH_HIP(p->drop_packed());
        OCH_HIP(p->d_packed.reserve((size_t)p->n_nodes * 8));
        p->packed_nodes = p->n_nodes;
        p->packed_by_slot = true;
    }
    if (count)
        OCH_HIP(hipMemcpy(p->d_packed.d + (size_t)first * 8, packed, (size_t)count * 32, hipMemcpyHostToDevice));
    return OCH_OK;
}

int och::pool_scatter_slots(och_gpu_pool *p, const uint32_t *ids, uint32_t count, const uint32_t *raw,
                            const uint32_t *packed)
{
    if (!p || p->index_base != 1 || (count && (!ids || !raw))) return fail(OCH_E_INVALID, "bad editor flush");
    if (packed && (!p->d_packed.d || !p->packed_by_slot))
        return fail(OCH_E_INVALID, "packed buffer is not in editor numbering");
    if (count == 0) return OCH_OK;
    for (uint32_t i = 0; i < count; ++i)
        if (ids[i] == 0 || ids[i] >= p->n_nodes) return fail(OCH_E_INVALID, "editor slot %u outside the pool", ids[i]);
    DeviceGuard g(p->device);
    p->last_writer = 0;                 // until pool_commit
    // staging: [ids | raw | packed]
    const size_t words = (size_t)count * (packed ? 17 : 9);
    const size_t cap = std::max<size_t>(words, 1 << 16);
    if (words > p->stage_words) {
        if (p->h_stage) OCH_HIP(hipHostFree(p->h_stage));
        p->h_stage = nullptr;
        p->stage_words = 0;
        OCH_HIP(hipHostMalloc(&p->h_stage, cap * 4, hipHostMallocDefault));
        p->stage_words = cap;
    }
    OCH_HIP(p->d_stage.reserve(cap));
    std::memcpy(p->h_stage, ids, (size_t)count * 4);
    std::memcpy(p->h_stage + count, raw, (size_t)count * 32);
    if (packed) std::memcpy(p->h_stage + 9 * (size_t)count, packed, (size_t)count * 32);
    for (uint32_t i = 0; i < count; ++i)       // host mirror (user numbering, slot s at row s - 1)
        std::memcpy(p->mirror.data() + (size_t)(ids[i] - 1) * 8, raw + (size_t)i * 8, 32);
    const hipStream_t s = p->stream();
    uint32_t *stage = p->d_stage.d;
    OCH_HIP(hipMemcpyAsync(stage, p->h_stage, words * 4, hipMemcpyHostToDevice, s));
    OCH_HIP(och::launch_scatter_slots(stage, stage + count, packed ? stage + 9 * (size_t)count : nullptr,
                                      count, p->d_nodes.d, packed ? p->d_packed.d : nullptr, s));
    OCH_HIP(hipStreamSynchronize(s));
    return OCH_OK;
}

int och::pool_commit(och_gpu_pool *p, uint32_t root, uint32_t packed_root, bool packed, uint64_t writer,
                     const int32_t *box_lo, const int32_t *box_hi)
{
    if (!p || p->index_base != 1) return fail(OCH_E_INVALID, "bad editor flush");
    if (packed && (!p->d_packed.d || !p->packed_by_slot))
        return fail(OCH_E_INVALID, "packed buffer is not in editor numbering");
    DeviceGuard g(p->device);
    if (!packed) OCH_HIP(p->drop_packed());
    p->root = root;
    p->packed_root = packed ? packed_root : 0;
    p->box_any = box_lo && box_hi;
    for (int a = 0; a < 3; ++a) {
        p->box_lo[a] = p->box_any ? box_lo[a] : 0;
        p->box_hi[a] = p->box_any ? box_hi[a] : 0;
    }
    p->last_writer = writer;
    p->torn = false;
    return OCH_OK;
}

int och::pool_mark_torn(och_gpu_pool *p)
{
    if (!p) return OCH_E_INVALID;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    (void)p->drop_packed();
    p->packed_root = 0;
    p->root = 0;
    p->box_any = false;
    p->last_writer = 0;
    p->torn = true;
    return OCH_OK;
}

// ------------------------------------------------------------ launch planning
// The pure planners: vectors and integers in and out, no HIP call, no pool; external
// linkage, so that a host program can call them (tests/test_plan_host.py pins them).
namespace och {
namespace plan {

// The stable costliest-first permutation of the workgroups.
std::vector<uint32_t> by_cost(const std::vector<uint32_t> &costs)
{
    std::vector<uint32_t> order(costs.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return costs[a] > costs[b]; });
    return order;
}

// The launch order from the costliest-first list (OCH_OPT_PLAN): 0 = all
// workgroups costliest first; P in 1..99 = the costliest P % first, then the
// rest in natural order (the tails a frame ends on start early, while the bulk
// keeps the raster order's mix of sky and terrain tiles); 100 = alternate the
// costliest and the cheapest left.  Default 10: with frames in flight, every
// frame starting all its costly tiles at once cost 3.5 % over long runs
// (profiles/r03/ab/plan_*).
void shape(std::vector<uint32_t> &order, int mode)
{
    const size_t n = order.size();
    if (mode <= 0 || n < 2) return;
    std::vector<uint32_t> out;
    out.reserve(n);
    if (mode >= 100) {
        for (size_t i = 0, j = n - 1; i <= j && j < n; ++i, --j) {
            out.push_back(order[i]);
            if (j != i) out.push_back(order[j]);
            if (j == 0) break;
        }
    } else {
        const size_t head = n * (size_t)mode / 100;
        std::vector<uint8_t> taken(n, 0);
        for (size_t i = 0; i < head; ++i) {
            out.push_back(order[i]);
            taken[order[i]] = 1;
        }
        for (uint32_t b = 0; b < n; ++b)
            if (!taken[b]) out.push_back(b);
    }
    order.swap(out);
}

// Grouped per XCD (OCH_OPT_TILE_ORDER = 3): workgroup slot i runs on XCD
// i % 8, so deal 64x64-pixel supertiles over the XCDs (each XCD's L2 then
// holds the nodes of its own neighbouring tiles) and keep the costliest-
// first order within each XCD's list.  Workgroup b starts at tile b * (block / 64).
std::vector<uint32_t> group_by_xcd(const std::vector<uint32_t> &order, uint32_t tiles_x, uint32_t tiles_y, uint32_t block)
{
    const uint32_t stx = (tiles_x + 7) / 8, sty = (tiles_y + 7) / 8;
    std::vector<std::vector<uint32_t>> lists(8);
    for (uint32_t b : order) {
        const uint32_t tile = b * (block / 64), view = tile / (tiles_x * tiles_y), t = tile % (tiles_x * tiles_y);
        const uint32_t super = (view * sty + (t / tiles_x) / 8) * stx + (t % tiles_x) / 8;
        lists[super % 8].push_back(b);
    }
    std::vector<uint32_t> grouped;
    grouped.reserve(order.size());
    std::vector<size_t> at(8, 0);
    while (grouped.size() < order.size())
        for (uint32_t x = 0; x < 8 && grouped.size() < order.size(); ++x) {
            uint32_t from = x;
            if (at[x] == lists[x].size())       // this XCD's list ran dry: the fullest other list
                for (uint32_t y = 0; y < 8; ++y)
                    if (lists[y].size() - at[y] > lists[from].size() - at[from]) from = y;
            grouped.push_back(lists[from][at[from]++]);
        }
    return grouped;
}

// A split tile's rays longer than this % of its longest walk over
// OCH_OPT_SPLIT_SEGS lanes; the others take one lane and walk whole
// (tools/split_model.c: 30 % keeps the critical path of splitting every ray
// and adds almost no work).
constexpr int kSplitRayPct = 30;

// The split form of a primary plan (OCH_OPT_SPLIT).  The tiles
// whose planning cost reaches opt_split % of the costliest one's are split:
// one counting render gives every pixel's walked PUSHes, a tile's rays longer
// than kSplitRayPct % of its longest get opt_split_segs lanes each (segment
// lanes), the others one, and its rays are packed, costliest first, into
// waves of 64 lanes with every lane of a ray in one wave (their records merge
// through that wave's LDS).  Rows of d_split_tasks: the tile, then 64 lane
// tasks (pixel | seg << 6 | log2(S) << 10, ~0 idle).  The order: the split
// waves (1 << 31 | row), then the plan's other workgroups in its order.
// Block 64 only (workgroup = tile), packed layout, tiles < 2^24, and a split
// level above the leaves; otherwise no split plan.

// One tile's waves, 64 lane tasks each, from its pixels' PUSHes (-1: outside the frame).
std::vector<uint32_t> pack_split_tile(const int cnt[64], int S)
{
    const int log2s = __builtin_ctz((unsigned)S), mx = std::max(0, *std::max_element(cnt, cnt + 64));
    auto long_ray = [&](int l) { return cnt[l] * 100 > kSplitRayPct * mx; };
    std::vector<std::pair<int, int>> rays;                  // (estimated lane cost, pixel)
    for (int l = 0; l < 64; ++l)
        if (cnt[l] >= 0) rays.push_back({long_ray(l) ? cnt[l] / S : cnt[l], l});
    std::stable_sort(rays.begin(), rays.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<uint32_t> waves, used;                      // 64 words per wave, idle at first; lanes taken
    for (const auto &r : rays) {
        const uint32_t l = (uint32_t)r.second, lanes = long_ray(r.second) ? (uint32_t)S : 1u;
        size_t w = 0;
        while (w < used.size() && used[w] + lanes > 64) ++w;
        if (w == used.size()) {
            used.push_back(0);
            waves.resize(waves.size() + 64, ~0u);
        }
        for (uint32_t s = 0; s < lanes; ++s)
            waves[w * 64 + used[w]++] = l | s << 6 | (uint32_t)(lanes > 1 ? log2s : 0) << 10;
    }
    return waves;
}

struct Split {
    std::vector<uint32_t> order, tasks;
    uint32_t tiles = 0, extra = 0;      // heavy tiles; waves - heavy tiles
};

// The heavy tiles (pct % of the costliest, at most max(1, n / 16): a bound on the
// planner's work), their waves, and the split order; push: slices of rows x W.
Split split_order(const std::vector<uint16_t> &push, int W, int rows, const std::vector<uint32_t> &by_cost,
                  const std::vector<uint32_t> &order, const std::vector<uint32_t> &c, int pct, int S)
{
    Split sp;
    const uint32_t n = (uint32_t)order.size();
    if (pct <= 0 || n == 0) return sp;
    const double thr = (double)c[by_cost[0]] * pct / 100.0;
    const uint32_t cap = std::max(1u, n / 16);
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, per_view = tiles_x * (uint32_t)((rows + 7) / 8);
    std::vector<uint8_t> heavy(n, 0);
    for (uint32_t k = 0; k < n && k < cap && (double)c[by_cost[k]] >= thr; ++k, ++sp.tiles) {
        const uint32_t t = by_cost[k];
        heavy[t] = 1;
        const uint32_t view = t / per_view, tt = t % per_view, ty = tt / tiles_x, tx = tt % tiles_x;
        int cnt[64];
        for (int l = 0; l < 64; ++l) {
            const uint32_t col = tx * 8 + (uint32_t)(l % 8), srow = ty * 8 + (uint32_t)(l / 8);
            cnt[l] = col < (uint32_t)W && srow < (uint32_t)rows ? push[((size_t)view * rows + srow) * W + col] : -1;
        }
        const std::vector<uint32_t> waves = pack_split_tile(cnt, S);
        for (size_t w = 0; w < waves.size(); w += 64) {
            sp.order.push_back(0x80000000u | (uint32_t)(sp.tasks.size() / 65));
            sp.tasks.push_back(t);
            sp.tasks.insert(sp.tasks.end(), waves.begin() + w, waves.begin() + w + 64);
        }
    }
    sp.extra = (uint32_t)sp.order.size() - sp.tiles;
    for (uint32_t b : order)
        if (!heavy[b]) sp.order.push_back(b);
    return sp;
}

// A workgroup's time spread over its per_block tiles (natural 8x8-tile order), a
// tile's over its 8 rows, summed per chunk of row_chunk rows (och_gpu_chunk_costs).
std::vector<float> spread_chunk_costs(const std::vector<uint32_t> &c, int n_views, int W, int H, uint32_t per_block,
                                      int row_chunk)
{
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, tiles_y = (uint32_t)(H + 7) / 8;
    const uint32_t tiles = (uint32_t)n_views * tiles_x * tiles_y;
    std::vector<double> acc((H + row_chunk - 1) / row_chunk, 0.0);
    for (uint32_t b = 0; b < c.size(); ++b)
        for (uint32_t t = b * per_block; t < std::min(tiles, (b + 1) * per_block); ++t) {
            const uint32_t ty = (t % (tiles_x * tiles_y)) / tiles_x;
            const int r0 = (int)ty * 8, r1 = std::min(H, r0 + 8);
            for (int r = r0; r < r1; ++r) acc[r / row_chunk] += (double)c[b] / per_block / (r1 - r0);
        }
    return std::vector<float>(acc.begin(), acc.end());
}

}  // namespace plan
}  // namespace och

int och::check_views(const och_camera *cams, int n_views)
{
    for (int v = 0; v < n_views; ++v)
        if (cams[v].width != cams[0].width || cams[v].height != cams[0].height || cams[v].width <= 0 || cams[v].height <= 0)
            return fail(OCH_E_INVALID, "views must share one positive width and height");
    return OCH_OK;
}

namespace {

int tiled_args(const och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs, uint32_t n,
               uint32_t width)
{
    if (!p || (n && (!origin || !dirs))) return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (width == 0) return fail(OCH_E_INVALID, "width must be positive");
    const uint64_t rows = ((uint64_t)n + width - 1) / width;
    if ((uint64_t)((width + 7) / 8) * ((rows + 7) / 8) * 64 >= (1ull << 32))
        return fail(OCH_E_INVALID, "batch of %u rays %u wide too large", n, width);
    return check_ready(p);
}

// The key of a tiled batch's launch plan: the geometry and the block size.
void batch_key(const och_gpu_pool *p, uint32_t n, uint32_t width, int64_t key[9])
{
    const int64_t k[9] = {n, width, p->opt_block, 0, 0, 0, 0, 0, 0};
    std::memcpy(key, k, sizeof k);
}

// The key of a frame's launch plan: the geometry, the sharding, the block
// size, config 5's compaction and the row deal the frame was made for.
void frame_key(const och_gpu_pool *p, const och::DevFrame &f, bool bounce, int64_t key[9])
{
    const int64_t k[9] = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards, p->opt_block,
                          bounce ? p->opt_bounce_compact : 0, f.chunk_map ? (int64_t)p->deal_serial : 0};
    std::memcpy(key, k, sizeof k);
}

// The frame of n_views checked views (check_views) as the kernels take it,
// with this shard's slice height and, under a row deal, its chunk map.
och::DevFrame make_frame(const och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *out, uint8_t *codes,
                         int row_chunk, int shard, int n_shards)
{
    och::DevFrame f;
    for (int v = 0; v < n_views; ++v) f.cams[v] = cams[v];
    f.n_views = n_views;
    f.palette = p->d_palette.d;
    f.n_voxels = p->n_voxels;
    f.out = out;
    f.codes = codes;
    f.row_chunk = row_chunk;
    f.shard = shard;
    f.n_shards = n_shards;
    f.slice_rows = p->slice_rows(cams[0].height, row_chunk, n_shards);
    const bool dealt = p->deal_for(cams[0].height, row_chunk, n_shards);
    f.chunk_map = dealt ? p->d_chunk_map.d + (size_t)shard * p->deal_max : nullptr;
    return f;
}

// A planning render: launch(sc) in natural order, sc.cost naming n_words words preset to
// 0xFFFFFFFF that every launched workgroup overwrites with its duration; c receives them.
// frame: the camera frame the launch renders (bounce: by the config-5 kernel), for its tile table.
int use_tiles(och_gpu_pool *p, const och::DevFrame &f, bool bounce, och::Schedule &sc);

template <class Launch>
int cost_render(och_gpu_pool *p, uint32_t *cost, uint32_t n_words, std::vector<uint32_t> &c, Launch launch,
                const och::DevFrame *frame = nullptr, bool bounce = false)
{
    och::Schedule sc = p->schedule();
    sc.tile_order = 0;
    sc.cost = cost;
    if (frame)
        if (int ts = use_tiles(p, *frame, bounce, sc)) return ts;
    OCH_HIP(hipMemsetAsync(cost, 0xFF, (size_t)n_words * 4, p->stream()));
    OCH_HIP(launch(sc));
    c.resize(n_words);
    OCH_HIP(hipMemcpyAsync(c.data(), cost, (size_t)n_words * 4, hipMemcpyDeviceToHost, p->stream()));
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

extern "C" {   // the render path's pieces, defined with the entries below inside extern "C": declared so here
och::Schedule timed_schedule(och_gpu_pool *p, int &st);
int timed_done(och_gpu_pool *p, const och::Schedule &sc, bool launched);
void use_plan(const och_gpu_pool *p, const och::DevFrame &f, bool bounce, bool split, och::Schedule &sc);
}

// One camera launch of frame f: the schedule with the launch's timing, the plan of
// this geometry (split: its split form too), the tile table, the launch, the timing's
// end.  CAMERA_LAUNCH's launch expression takes the schedule as `sc`; a failure names it.
template <class Launch>
int camera_launch(och_gpu_pool *p, const och::DevFrame &f, bool bounce, bool split, const char *what, Launch launch)
{
    int ts;
    och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    use_plan(p, f, bounce, split, sc);
    if (int us = use_tiles(p, f, bounce, sc)) return us;
    const hipError_t e = launch(sc);
    if (e != hipSuccess) return fail(OCH_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return timed_done(p, sc, true);
}
#define CAMERA_LAUNCH(p, f, bounce, split, call) \
    camera_launch(p, f, bounce, split, #call, [&](const och::Schedule &sc) { return call; })

// A host form: render(scratch) into the pool's scratch (pixels words and `spare`
// bytes), then the pixels to the caller's rgba, complete on return.
template <class Render>
int to_host(och_gpu_pool *p, size_t pixels, size_t spare, uint32_t *rgba, Render render)
{
    DeviceGuard g(p->device);
    int st = ensure_scratch(p, pixels * 4 + spare);
    if (st != OCH_OK) return st;
    st = render(reinterpret_cast<uint32_t *>(p->scratch.d));
    if (st != OCH_OK) return st;
    OCH_HIP(hipMemcpyAsync(rgba, p->scratch.d, pixels * 4, hipMemcpyDeviceToHost, p->stream()));
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

}  // namespace

extern "C" {

OCH_API int och_gpu_set_rcp_lut(och_gpu_pool *p, const uint32_t *lut, int log2_entries)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    DeviceGuard g(p->device);
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return upload_lut(p, lut, log2_entries);
}

OCH_API int och_gpu_set_palette(och_gpu_pool *p, const uint32_t *rgba, uint32_t n_voxels)
{
    if (!p || (n_voxels && !rgba)) return fail(OCH_E_INVALID, "pool/palette is NULL");
    DeviceGuard g(p->device);
    OCH_HIP(hipStreamSynchronize(p->stream()));
    OCH_HIP(p->d_palette.release());
    OCH_HIP(p->d_code_table.release());   // no code table unless this palette fits the codes
    p->n_voxels = 0;
    if (n_voxels <= OCH_CODE_MAX_VOXELS) {
        // Indexed-colour frames: trace_pixel's colour per code
        // (ORT/test_och_h_octree.cpp:76-84), then config 5's blocked (halved) variants.
        std::vector<uint32_t> t(256, 0xFFFF00FFu);
        for (uint32_t c = 0; c < 6 * n_voxels; ++c) t[c] = rgba[c];
        t[OCH_CODE_INSIDE] = 0xFF07193Fu;
        t[OCH_CODE_SKY] = 0xFFFEBF00u;
        for (uint32_t c = 0; c < OCH_CODE_BLOCKED; ++c)
            t[c | OCH_CODE_BLOCKED] = ((t[c] >> 1) & 0x007F7F7Fu) | (t[c] & 0xFF000000u);
        OCH_HIP(p->d_code_table.upload(t));
    }
    if (!n_voxels) return OCH_OK;
    OCH_HIP(p->d_palette.reserve((size_t)n_voxels * 6));
    OCH_HIP(hipMemcpy(p->d_palette.d, rgba, (size_t)n_voxels * 6 * 4, hipMemcpyHostToDevice));
    p->n_voxels = n_voxels;
    return OCH_OK;
}

OCH_API int och_gpu_set_stream(och_gpu_pool *p, void *stream)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    p->ext_stream = (hipStream_t)stream;
    p->use_ext = true;
    return OCH_OK;
}

// Option ids retired in round 5 (measured slower on every scene, DESIGN.md
// §8): 0 schedule (persistent / refill), 2 waves per CU, 3 refill, 7 chunk
// tiles, 9 merge, 12 per-node skip, 13 column cull.  Their ids stay unused.
static int retired_option(int option)
{
    return fail(OCH_E_INVALID, "option %d was retired (the grid schedule alone remains; DESIGN.md section 8)", option);
}

OCH_API int och_gpu_set_option(och_gpu_pool *p, int option, int value)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    switch (option) {
    case OCH_OPT_BLOCK:
        if (value < 64 || value > 1024 || value % 64) return fail(OCH_E_INVALID, "block %d", value);
        p->opt_block = value;
        return OCH_OK;
    case OCH_OPT_LAYOUT:
        if (value != 0 && value != 1) return fail(OCH_E_INVALID, "layout must be 0 or 1");
        if (value == 1 && !p->d_packed.d) return fail(OCH_E_INVALID, "pool too large for the packed layout");
        p->opt_layout = value;
        return OCH_OK;
    case OCH_OPT_TILE_ORDER:
        if (value < 0 || value > 3) return fail(OCH_E_INVALID, "tile order must be 0..3");
        p->opt_tile_order = value;
        return OCH_OK;
    case OCH_OPT_BOUNCE_COMPACT:
        if (value < 0 || value > 2) return fail(OCH_E_INVALID, "bounce compaction must be 0, 1 or 2");
        p->opt_bounce_compact = value;
        return OCH_OK;
    case OCH_OPT_CULL:
        if (value < 0 || value > 2) return fail(OCH_E_INVALID, "cull must be 0, 1 or 2");
        p->opt_cull = value;
        return OCH_OK;
    case OCH_OPT_TIMING:
        if (value < 0 || value > 2) return fail(OCH_E_INVALID, "timing must be 0, 1 or 2");
        p->opt_timing = value;
        return OCH_OK;
    case OCH_OPT_PLAN:
        if (value < 0 || value > 100) return fail(OCH_E_INVALID, "plan shape must be 0..100");
        p->opt_plan = value;
        return OCH_OK;
    case OCH_OPT_SPLIT:
        if (value < 0 || value > 100) return fail(OCH_E_INVALID, "split threshold must be 0..100 (%% of the costliest tile)");
        p->opt_split = value;
        return OCH_OK;
    case OCH_OPT_SPLIT_SEGS:
        if (value != 2 && value != 4 && value != 8 && value != 16) return fail(OCH_E_INVALID, "split segments must be 2, 4, 8 or 16");
        p->opt_split_segs = value;
        return OCH_OK;
    case OCH_OPT_SPLIT_LEVEL:
        if (value < 1 || value > 21) return fail(OCH_E_INVALID, "split level must be 1..21");
        p->opt_split_level = value;
        return OCH_OK;
    case OCH_OPT_SPLIT_TILES:
        return fail(OCH_E_INVALID, "OCH_OPT_SPLIT_TILES is read-only");
    case 0: case 2: case 3: case 7: case 9: case 12: case 13:
        return retired_option(option);
    default:
        return fail(OCH_E_INVALID, "unknown option %d", option);
    }
}

OCH_API int och_gpu_get_option(const och_gpu_pool *p, int option, int *value)
{
    if (!p || !value) return fail(OCH_E_INVALID, "NULL argument");
    switch (option) {
    case OCH_OPT_BLOCK: *value = p->opt_block; return OCH_OK;
    case OCH_OPT_LAYOUT: *value = (p->opt_layout == 1 && p->d_packed.d) ? 1 : 0; return OCH_OK;
    case OCH_OPT_TILE_ORDER: *value = p->opt_tile_order; return OCH_OK;
    case OCH_OPT_BOUNCE_COMPACT: *value = p->opt_bounce_compact; return OCH_OK;
    case OCH_OPT_CULL: *value = p->opt_cull; return OCH_OK;
    case OCH_OPT_TIMING: *value = p->opt_timing; return OCH_OK;
    case OCH_OPT_PLAN: *value = p->opt_plan; return OCH_OK;
    case OCH_OPT_SPLIT: *value = p->opt_split; return OCH_OK;
    case OCH_OPT_SPLIT_SEGS: *value = p->opt_split_segs; return OCH_OK;
    case OCH_OPT_SPLIT_LEVEL: *value = p->opt_split_level; return OCH_OK;
    case OCH_OPT_SPLIT_TILES: *value = (int)p->split.tiles; return OCH_OK;
    case 0: case 2: case 3: case 7: case 9: case 12: case 13:
        return retired_option(option);
    default: return fail(OCH_E_INVALID, "unknown option %d", option);
    }
}

OCH_API int och_gpu_occupancy(const och_gpu_pool *p, int kind, int *blocks_per_cu)
{
    if (!p || !blocks_per_cu) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    OCH_HIP(och::occupancy_blocks_per_cu(kind, p->opt_block, p->depth, blocks_per_cu));
    return OCH_OK;
}

OCH_API int och_gpu_set_stamp_buffer(och_gpu_pool *p, uint64_t *stamps, uint32_t capacity_waves)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    p->stamps = capacity_waves ? stamps : nullptr;
    p->stamp_cap = stamps ? capacity_waves : 0;
    return OCH_OK;
}

namespace {

// Per-launch timing of the traversal kernel (OCH_OPT_TIMING).  1 (default):
// the dispatch itself records the pool's events (hipExtLaunchKernel, no
// packets of its own); 2: hipEventRecord before and after the launch (two
// marker packets, each with a system-scope release: ~10 us of idle GPU
// between two launches of a stream); 0: none.  Events handed
// over by och_gpu_set_launch_events take the place of the pool's for one launch.
och::Schedule timed_schedule(och_gpu_pool *p, int &st)
{
    och::Schedule sc = p->schedule();
    st = OCH_OK;
    if (p->next_ev_start || p->next_ev_stop) {
        sc.ev_start = p->next_ev_start;
        sc.ev_stop = p->next_ev_stop;
        p->next_ev_start = p->next_ev_stop = nullptr;
    } else if (p->opt_timing == 1) {
        sc.ev_start = p->ev_start;
        sc.ev_stop = p->ev_stop;
    } else if (p->opt_timing == 2 && hipEventRecord(p->ev_start, p->stream()) != hipSuccess) {
        st = fail(OCH_E_HIP, "hipEventRecord: %s", hipGetErrorString(hipGetLastError()));
    }
    return sc;
}

// After the launch: och_gpu_last_kernel_ms reads the pool's events only if
// this launch recorded them (n = 0 launches nothing).
int timed_done(och_gpu_pool *p, const och::Schedule &sc, bool launched)
{
    if (sc.ev_start == p->ev_start && sc.ev_start) {
        p->timed = launched;
    } else if (!sc.ev_start && !sc.ev_stop && p->opt_timing == 2) {
        OCH_HIP(hipEventRecord(p->ev_stop, p->stream()));
        p->timed = true;
    } else {
        p->timed = false;
    }
    return OCH_OK;
}

// A frame loop points the pool at each frame's stream and hands each launch its events; when
// it ends, also after a failure, the pool's own stream is back and no event waits for a launch.
struct FrameLoopScope {
    och_gpu_pool *const p;
    const bool had_ext = p->use_ext;
    const hipStream_t prev = p->ext_stream;
    ~FrameLoopScope()
    {
        p->next_ev_start = p->next_ev_stop = nullptr;
        p->ext_stream = prev;
        p->use_ext = had_ext;
    }
    void frame(void *stream, void *const *start_events, void *const *stop_events, int k)
    {
        p->ext_stream = static_cast<hipStream_t>(stream);
        p->use_ext = true;
        if (start_events) {
            p->next_ev_start = static_cast<hipEvent_t>(start_events[k]);
            p->next_ev_stop = static_cast<hipEvent_t>(stop_events[k]);
        }
    }
};

}  // namespace

OCH_API int och_gpu_set_launch_events(och_gpu_pool *p, void *start_event, void *stop_event)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    p->next_ev_start = static_cast<hipEvent_t>(start_event);
    p->next_ev_stop = static_cast<hipEvent_t>(stop_event);
    return OCH_OK;
}

OCH_API int och_gpu_synchronize(och_gpu_pool *p)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    DeviceGuard g(p->device);
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_last_kernel_ms(och_gpu_pool *p, float *ms)
{
    if (!p || !ms) return fail(OCH_E_INVALID, "pool/ms is NULL");
    if (!p->timed)
        return fail(OCH_E_INVALID, "the last launch on this pool was not timed (none yet, n = 0, OCH_OPT_TIMING 0, "
                                   "or the caller's events)");
    DeviceGuard g(p->device);
    OCH_HIP(hipEventSynchronize(p->ev_stop));
    OCH_HIP(hipEventElapsedTime(ms, p->ev_start, p->ev_stop));
    return OCH_OK;
}

OCH_API int och_gpu_trace_batch_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                    uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time,
                                    uint32_t *push_count)
{
    OCH_ENTRY();
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    int ts;
    const och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    OCH_HIP(och::launch_trace_batch(p->dev(), origin, origin_stride, dirs, n, hit_dir, hit_voxel,
                                    reinterpret_cast<uint32_t *>(hit_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_trace_bounce_batch_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                           uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time,
                                           int32_t *bounce_dir, uint32_t *bounce_voxel, float *bounce_time,
                                           uint32_t *push_count)
{
    OCH_ENTRY();
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time || !bounce_dir || !bounce_voxel ||
                     !bounce_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    int ts;
    const och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    OCH_HIP(och::launch_trace_bounce_batch(p->dev(), origin, origin_stride, dirs, n, hit_dir, hit_voxel,
                                           reinterpret_cast<uint32_t *>(hit_time), bounce_dir, bounce_voxel,
                                           reinterpret_cast<uint32_t *>(bounce_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_trace_batch_tiled_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                          uint32_t n, uint32_t width, int32_t *hit_dir, uint32_t *hit_voxel,
                                          float *hit_time, uint32_t *push_count)
{
    OCH_ENTRY();
    if (int st = tiled_args(p, origin, origin_stride, dirs, n, width)) return st;
    if (n && (!hit_dir || !hit_voxel || !hit_time)) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    int ts;
    och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    if (p->opt_tile_order >= 2 && p->plans[2].order.d) {
        int64_t key[9];
        batch_key(p, n, width, key);
        if (p->plans[2].matches(key)) {
            sc.order = p->plans[2].order.d;
            sc.order_n = p->plans[2].blocks;
        }
    }
    OCH_HIP(och::launch_trace_batch_tiled(p->dev(), origin, origin_stride, dirs, n, width, hit_dir, hit_voxel,
                                          reinterpret_cast<uint32_t *>(hit_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_plan_batch_tiled(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                     uint32_t n, uint32_t width)
{
    OCH_ENTRY();
    if (int st = tiled_args(p, origin, origin_stride, dirs, n, width)) return st;
    if (n == 0) return OCH_OK;
    DeviceGuard g(p->device);
    const uint32_t tiles = ((width + 7) / 8) * (uint32_t)(((n + width - 1) / width + 7) / 8);
    const uint32_t max_blocks = (uint32_t)(((uint64_t)tiles * 64 + p->opt_block - 1) / p->opt_block);
    const size_t out_bytes = (((size_t)n * 4 + 255) & ~(size_t)255);
    int st = ensure_scratch(p, 3 * out_bytes + (size_t)max_blocks * 4);
    if (st != OCH_OK) return st;
    char *base = p->scratch.d;
    std::vector<uint32_t> c;
    st = cost_render(p, reinterpret_cast<uint32_t *>(base + 3 * out_bytes), max_blocks, c, [&](const och::Schedule &sc) {
        return och::launch_trace_batch_tiled(p->dev(), origin, origin_stride, dirs, n, width,
                                             reinterpret_cast<int32_t *>(base), reinterpret_cast<uint32_t *>(base + out_bytes),
                                             reinterpret_cast<uint32_t *>(base + 2 * out_bytes), nullptr, sc, p->stream());
    });
    if (st != OCH_OK) return st;
    const std::vector<uint32_t> order = och::plan::by_cost(c);
    LaunchPlan &plan = p->plans[2];
    plan.invalidate();                        // no plan until the new one is in place (a failure below leaves none)
    if (int ds = och::pool_drain(p)) return ds;   // launches in flight on other streams may read the old order
    OCH_HIP(plan.order.upload(order));
    batch_key(p, n, width, plan.key);
    plan.blocks = max_blocks;
    return OCH_OK;
}

namespace {

// Host rays in, host records out, synchronous: the rays staged in the pool's
// scratch, traced by the array kernel (width 0) or as a `width`-wide image of
// 8x8 tiles (och_gpu_trace_batch_tiled_dev), the records copied back.
int host_batch(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs, uint32_t n, uint32_t width,
               int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time)
{
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (n == 0) return OCH_OK;
    DeviceGuard g(p->device);
    const size_t n_orig = origin_stride ? (size_t)n * 3 : 3;
    const size_t b_orig = (n_orig * 4 + 255) & ~(size_t)255;
    const size_t b_dirs = ((size_t)n * 12 + 255) & ~(size_t)255;
    const size_t b_out = ((size_t)n * 4 + 255) & ~(size_t)255;
    int st = ensure_scratch(p, b_orig + b_dirs + 3 * b_out);
    if (st != OCH_OK) return st;
    char *base = p->scratch.d;
    float *d_orig = reinterpret_cast<float *>(base);
    float *d_dirs = reinterpret_cast<float *>(base + b_orig);
    int32_t *d_dir = reinterpret_cast<int32_t *>(base + b_orig + b_dirs);
    uint32_t *d_vox = reinterpret_cast<uint32_t *>(base + b_orig + b_dirs + b_out);
    float *d_t = reinterpret_cast<float *>(base + b_orig + b_dirs + 2 * b_out);
    hipStream_t s = p->stream();
    OCH_HIP(hipMemcpyAsync(d_orig, origin, n_orig * 4, hipMemcpyHostToDevice, s));
    OCH_HIP(hipMemcpyAsync(d_dirs, dirs, (size_t)n * 12, hipMemcpyHostToDevice, s));
    st = width ? och_gpu_trace_batch_tiled_dev(p, d_orig, origin_stride, d_dirs, n, width, d_dir, d_vox, d_t, nullptr)
               : och_gpu_trace_batch_dev(p, d_orig, origin_stride, d_dirs, n, d_dir, d_vox, d_t, nullptr);
    if (st != OCH_OK) return st;
    OCH_HIP(hipMemcpyAsync(hit_dir, d_dir, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipMemcpyAsync(hit_voxel, d_vox, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipMemcpyAsync(hit_time, d_t, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipStreamSynchronize(s));
    return OCH_OK;
}

}  // namespace

OCH_API int och_gpu_trace_batch(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time)
{
    OCH_ENTRY();
    return host_batch(p, origin, origin_stride, dirs, n, 0, hit_dir, hit_voxel, hit_time);
}

OCH_API int och_gpu_trace_batch_image(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                      uint32_t n, uint32_t width, int32_t *hit_dir, uint32_t *hit_voxel,
                                      float *hit_time)
{
    OCH_ENTRY();
    if (width == 0) return fail(OCH_E_INVALID, "width must be positive");
    return host_batch(p, origin, origin_stride, dirs, n, width, hit_dir, hit_voxel, hit_time);
}

OCH_API int och_gpu_trace(och_gpu_pool *p, float ox, float oy, float oz, float dx, float dy, float dz,
                          int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time)
{
    OCH_ENTRY();
    if (!hit_direction || !hit_voxel || !hit_time) return fail(OCH_E_INVALID, "NULL output");
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    return och_gpu_trace_batch(p, o, 0, d, 1, hit_direction, hit_voxel, hit_time);
}

OCH_API int och_camera_setup(float px, float py, float pz, float yaw, float pitch, float fov, int width, int height,
                             och_camera *cam)
{
    if (!cam || width <= 0 || height <= 0) return fail(OCH_E_INVALID, "bad camera arguments");
    // ORT/test_och_h_octree.cpp:89-115, evaluated in float exactly as written.
    cam->pos[0] = px;
    cam->pos[1] = py;
    cam->pos[2] = pz;
    cam->aspect = (float)width / (float)height;
    cam->view_x = 2.0F / (float)width;
    cam->view_y = 2.0F / (float)height;
    cam->fov_factor = 1 / tanf(fov / 2);
    const float sin_a = 0, cos_a = 1;
    const float sin_b = sinf(yaw), cos_b = cosf(yaw);
    const float sin_c = sinf(pitch), cos_c = cosf(pitch);
    cam->rot[0] = cos_a * cos_b;
    cam->rot[1] = cos_a * sin_b * sin_c - sin_a * cos_c;
    cam->rot[2] = cos_a * sin_b * cos_c + sin_a * sin_c;
    cam->rot[3] = sin_a * cos_b;
    cam->rot[4] = sin_a * sin_b * sin_c + cos_a * cos_c;
    cam->rot[5] = sin_a * sin_b * cos_c - cos_a * sin_c;
    cam->rot[6] = -sin_b;
    cam->rot[7] = cos_b * sin_c;
    cam->rot[8] = cos_b * cos_c;
    cam->width = width;
    cam->height = height;
    return OCH_OK;
}

OCH_API int och_gpu_raygen_dev(och_gpu_pool *p, const och_camera *cam, float *dirs)
{
    OCH_ENTRY();
    if (!p || !cam || !dirs) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_raygen(*cam, dirs, p->stream()));
    return OCH_OK;
}

OCH_API int och_shard_rows(int height, int row_chunk, int n_shards)
{
    if (height <= 0 || row_chunk <= 0 || n_shards <= 0) return 0;
    const int chunks = (height + row_chunk - 1) / row_chunk;
    return ((chunks + n_shards - 1) / n_shards) * row_chunk;
}

namespace {

// The launch order of frame f under OCH_OPT_TILE_ORDER 2 / 3: the pool's plan
// (och_gpu_plan_views) when it was made for this geometry, else none (natural
// order).  split: the launch can run the plan's split form (the grid kernel);
// without it the order stays an unsplit permutation of the frame's grid.
void use_plan(const och_gpu_pool *p, const och::DevFrame &f, bool bounce, bool split, och::Schedule &sc)
{
    const LaunchPlan &plan = p->plans[bounce ? 1 : 0];
    if (p->opt_tile_order < 2 || !plan.order.d) return;
    int64_t key[9];
    frame_key(p, f, bounce, key);
    if (!plan.matches(key)) return;
    sc.order = p->opt_tile_order == 3 ? plan.order_xcd.d : plan.order.d;
    sc.order_n = plan.blocks;
    // the plan's split form, while the options it was made with hold
    const SplitPlan &sp = p->split;
    if (split && !bounce && p->opt_tile_order == 2 && sp.n && p->dev().packed && p->opt_split == sp.params[0] &&
        p->opt_split_segs == sp.params[1] && p->opt_split_level == sp.params[2]) {
        sc.order = sp.order.d;
        sc.order_n = sp.n;
        sc.split_extra = sp.extra;
        sc.split_tasks = sp.tasks.d;
        sc.split_level = (uint32_t)p->opt_split_level;
    }
}

// The tile table of frame f's launch under sc (after use_plan): the pool's
// table of this geometry, block size and launch order, made and uploaded when
// the pool holds none.  Nothing in it depends on the cameras.  bounce: the
// config-5 kernel's launch (its own block size).
int use_tiles(och_gpu_pool *p, const och::DevFrame &f, bool bounce, och::Schedule &sc)
{
    const int block = bounce ? std::max(och::kBounceBlock, sc.block) : sc.block;
    const LaunchPlan &plan = p->plans[bounce ? 1 : 0];
    // the launch order: the split plan's, the plan's (whole, or grouped per XCD), or none
    const std::vector<uint32_t> *order = nullptr, *tasks = nullptr;
    int mode = sc.tile_order == 1 ? 1 : 0;
    if (sc.split_tasks) {
        order = &p->split.h_order;
        tasks = &p->split.h_tasks;
        mode = 4;
    } else if (sc.order) {
        mode = p->opt_tile_order == 3 ? 3 : 2;
        order = mode == 3 ? &plan.h_order_xcd : &plan.h_order;
    }
    const int64_t key[12] = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards,
                             f.slice_rows, block, mode, f.chunk_map ? (int64_t)p->deal_serial : 0,
                             order ? (int64_t)plan.serial : 0, bounce ? 1 : 0};
    TileTable *t = nullptr, *oldest = &p->tile_tables[0];
    for (TileTable &c : p->tile_tables) {
        if (c.used && std::memcmp(c.key, key, sizeof key) == 0) t = &c;
        if (c.used < oldest->used) oldest = &c;
    }
    if (!t) {
        och::plan::TileGeometry g = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards,
                                     f.slice_rows, block, mode == 1 ? 1 : 0, nullptr};
        if (f.chunk_map) g.chunk_map = p->h_chunk_map.data() + (size_t)f.shard * p->deal_max;
        std::vector<uint64_t> table;
        uint32_t grid = 0;
        // a plan of another grid (stale, or for another block size) is not this launch's: natural order
        const uint32_t blocks = (uint32_t)(((uint64_t)f.n_views * ((f.cams[0].width + 7) / 8) * ((f.slice_rows + 7) / 8) * 64 +
                                            block - 1) / block);
        if (order && mode != 4 && order->size() != blocks) order = nullptr;
        const char *why = "";
        if (int st = och::plan::tile_table(g, order ? order->data() : nullptr, order ? (uint32_t)order->size() : 0u,
                                           tasks ? tasks->data() : nullptr, tasks ? (uint32_t)tasks->size() : 0u, table,
                                           grid, &why))
            return fail(st, "tile table of a %d x %d frame, %d views: %s", g.width, g.height, g.n_views, why);
        t = oldest;
        if (t->used) {                          // launches in flight on other streams may read the table it replaces
            t->used = 0;
            if (int ds = och::pool_drain(p)) return ds;
        }
        OCH_HIP(t->d.upload(table));
        t->n = (uint32_t)table.size();
        t->grid = grid;
        t->block = (uint32_t)block;
        std::memcpy(t->key, key, sizeof key);
    }
    t->used = ++p->tile_clock;
    sc.tiles = t->d.d;
    sc.tiles_n = t->n;
    sc.tiles_grid = t->grid;
    sc.tiles_block = t->block;
    return OCH_OK;
}

// `what` (code frames of some kind) needs the code table of a palette small enough for 1-byte codes.
static int needs_code_palette(const och_gpu_pool *p, const char *what)
{
    if (p->n_voxels > OCH_CODE_MAX_VOXELS || !p->d_code_table.d)
        return fail(OCH_E_INVALID, "%s need a palette (och_gpu_set_palette) of at most %d voxel ids", what,
                    OCH_CODE_MAX_VOXELS);
    return OCH_OK;
}

// The shape of a sharded frame: the views, the sharding triple, one size, a token per pixel.
static int frame_args(const och_camera *cams, int n_views, int row_chunk, int shard, int n_shards)
{
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (row_chunk <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards)
        return fail(OCH_E_INVALID, "bad sharding (%d, %d, %d)", row_chunk, shard, n_shards);
    if (int vs = och::check_views(cams, n_views)) return vs;
    if ((uint64_t)cams[0].width * cams[0].height * n_views >= (1ull << 32)) return fail(OCH_E_INVALID, "frame too large");
    return OCH_OK;
}

// A frame loop's arguments: the window, its events, a frame per buffer.
static int loop_args(int n_steps, int n_buffers, void *const *start_events, void *const *stop_events, uint32_t *const *frames)
{
    if (n_steps < 0 || n_buffers < 1) return fail(OCH_E_INVALID, "n_steps %d / n_buffers %d", n_steps, n_buffers);
    if ((start_events == nullptr) != (stop_events == nullptr))
        return fail(OCH_E_INVALID, "start_events and stop_events: both or neither");
    for (int b = 0; b < n_buffers; ++b)
        if (!frames[b]) return fail(OCH_E_INVALID, "frames[%d] is NULL", b);
    return OCH_OK;
}

// What the three unshard entries refuse (table: the entry shades through the code table).
static int unshard_args(const och_gpu_pool *p, const void *gathered, const uint32_t *frames, int width, int height,
                        int row_chunk, int n_shards, int n_views, bool table)
{
    if (!p || !gathered || !frames || width <= 0 || height <= 0 || row_chunk <= 0 || n_shards <= 0 || n_views < 1)
        return fail(OCH_E_INVALID, "bad unshard arguments");
    if (table && !p->d_code_table.d)
        return fail(OCH_E_INVALID, "no code table: set a palette of at most %d voxel ids", OCH_CODE_MAX_VOXELS);
    return OCH_OK;
}

// The host forms' refusal before the staging buffer is sized; the device form checks again.
static int host_capacity(size_t capacity_pixels, int width, int height, size_t &pixels)
{
    pixels = (size_t)width * (size_t)height;
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "rgba holds %zu pixels, %d x %d need %zu", capacity_pixels, width, height, pixels);
    return OCH_OK;
}

int render_views(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices, int row_chunk, int shard,
                 int n_shards, bool bounce, uint8_t *code_slices = nullptr)
{
    if (!p || !cams || (!rgba_slices && !code_slices)) return fail(OCH_E_INVALID, "NULL argument");
    if (int cs = code_slices ? needs_code_palette(p, "indexed-colour frames") : OCH_OK) return cs;
    if (int fs = frame_args(cams, n_views, row_chunk, shard, n_shards)) return fs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    const och::DevFrame f = make_frame(p, cams, n_views, rgba_slices, code_slices, row_chunk, shard, n_shards);
    if (code_slices) return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render_codes(p->dev(), f, sc, bounce, p->stream()));
    if (bounce) return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render_bounce(p->dev(), f, sc, p->stream()));
    return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render(p->dev(), f, sc, p->stream()));
}

// What the four supersampled entries refuse of s, the views and the sample grid
// (the host forms pass their one camera).
static int ssaa_args(const och_camera *cams, int n_views, int s)
{
    if (s != 2 && s != 4 && s != 8) return fail(OCH_E_INVALID, "samples per axis %d: must be 2, 4 or 8", s);
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (int vs = och::check_views(cams, n_views)) return vs;
    if (cams[0].width % s || cams[0].height % s)
        return fail(OCH_E_INVALID, "sample grid %d x %d is not a multiple of %d", cams[0].width, cams[0].height, s);
    return OCH_OK;
}

// och_gpu_render_ssaa_views_dev (light null) and och_gpu_render_lit_ssaa_views_dev behind
// their NULL and light checks.  Every refusal comes before anything is written or launched.
static int render_ssaa_views(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light, int s,
                             uint32_t *rgba, size_t capacity_pixels)
{
    if (int as = ssaa_args(cams, n_views, s)) return as;
    const int Ws = cams[0].width, Hs = cams[0].height;
    if ((uint64_t)Ws * Hs * n_views >= (1ull << 32)) return fail(OCH_E_INVALID, "frame too large");
    const size_t pixels = (size_t)n_views * (Ws / s) * (Hs / s);
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "rgba holds %zu pixels, %d views of %d x %d need %zu", capacity_pixels, n_views, Ws / s,
                    Hs / s, pixels);
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // the sample grid as the 1-sample render's whole frame: its plan, never the split form
    const och::DevFrame f = make_frame(p, cams, n_views, rgba, nullptr, Hs, 0, 1);
    if (light)
        return CAMERA_LAUNCH(p, f, false, false,
                             och::launch_render_lit_ssaa(p->dev(), f, sc, *light, s == 2 ? 1 : s == 4 ? 2 : 3, p->stream()));
    return CAMERA_LAUNCH(p, f, false, false, och::launch_render_ssaa(p->dev(), f, sc, s == 2 ? 1 : s == 4 ? 2 : 3, p->stream()));
}

// The primary plan's split form (och::plan::split_order has the whole story):
// the counting render, the split order and task rows, their upload.
int plan_split(och_gpu_pool *p, const och::DevFrame &f, const std::vector<uint32_t> &by_cost,
               const std::vector<uint32_t> &order, const std::vector<uint32_t> &c)
{
    SplitPlan &sp = p->split;
    sp.invalidate();
    const uint32_t n = (uint32_t)order.size();
    if (p->opt_split <= 0 || p->opt_block != 64 || !p->dev().packed || p->opt_split_level >= p->depth || n == 0 ||
        n >= (1u << 24))
        return OCH_OK;
    // every pixel's walked PUSHes (one counting render of the planned frame)
    std::vector<uint16_t> push((size_t)f.n_views * f.slice_rows * f.cams[0].width);
    DevBuf<uint16_t> d_push;
    OCH_HIP(d_push.reserve(push.size()));
    och::Schedule sc = p->schedule();
    sc.tile_order = 0;
    if (int us = use_tiles(p, f, false, sc)) return us;
    // The counting render writes only the frame's pixels: rows past the height in
    // the last chunk and padding chunks keep the cleared 0, a ray without a PUSH,
    // so the plan does not depend on what the allocation held.
    hipError_t e = hipMemsetAsync(d_push.d, 0, push.size() * 2, p->stream());
    if (e == hipSuccess) e = och::launch_render_push(p->dev(), f, sc, d_push.d, p->stream());
    if (e == hipSuccess) e = hipMemcpyAsync(push.data(), d_push.d, push.size() * 2, hipMemcpyDeviceToHost, p->stream());
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream());
    (void)d_push.release();
    if (e != hipSuccess) return fail(OCH_E_HIP, "split plan: counting render: %s", hipGetErrorString(e));
    const och::plan::Split s = och::plan::split_order(push, f.cams[0].width, f.slice_rows, by_cost, order, c, p->opt_split,
                                                      p->opt_split_segs);
    if (s.tiles == 0) return OCH_OK;
    OCH_HIP(sp.order.upload(s.order));
    OCH_HIP(sp.tasks.upload(s.tasks));
    sp.h_order = s.order;
    sp.h_tasks = s.tasks;
    sp.n = (uint32_t)s.order.size();
    sp.extra = s.extra;
    sp.tiles = s.tiles;
    sp.params[0] = p->opt_split;
    sp.params[1] = p->opt_split_segs;
    sp.params[2] = p->opt_split_level;
    return OCH_OK;
}

}  // namespace

OCH_API int och_gpu_plan_views(och_gpu_pool *p, const och_camera *cams, int n_views, int row_chunk, int shard,
                               int n_shards)
{
    OCH_ENTRY();
    if (!p || !cams) return fail(OCH_E_INVALID, "NULL argument");
    if (n_views < 1 || n_views > OCH_MAX_VIEWS || row_chunk <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards)
        return fail(OCH_E_INVALID, "bad plan arguments");
    if (int vs = check_views(cams, n_views)) return vs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // One planning render per kernel (primary grid, config-5 bounce) into
    // scratch in natural order, timing every workgroup.
    const int W = cams[0].width, rows = p->slice_rows(cams[0].height, row_chunk, n_shards);
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, tiles_y = (uint32_t)(rows + 7) / 8;
    const size_t frame_bytes = (size_t)n_views * rows * W * 4;
    const uint32_t max_blocks = (uint32_t)((size_t)n_views * tiles_y * tiles_x) + 1024;
    int st = ensure_scratch(p, frame_bytes + (size_t)max_blocks * 4);
    if (st != OCH_OK) return st;
    uint32_t *cost = reinterpret_cast<uint32_t *>(p->scratch.d + frame_bytes);
    const och::DevFrame f = make_frame(p, cams, n_views, reinterpret_cast<uint32_t *>(p->scratch.d), nullptr, row_chunk,
                                       shard, n_shards);
    for (int which = 0; which < 2; ++which) {
        LaunchPlan &plan = p->plans[which];
        std::vector<uint32_t> c;
        st = cost_render(p, cost, max_blocks, c, [&](const och::Schedule &sc) {
            return which ? och::launch_render_bounce(p->dev(), f, sc, p->stream())
                         : och::launch_render(p->dev(), f, sc, p->stream());
        }, &f, which != 0);
        if (st != OCH_OK) return st;
        c.resize(std::find(c.begin(), c.end(), 0xFFFFFFFFu) - c.begin());   // launched blocks wrote a cost
        if (c.empty()) {
            plan.invalidate();                   // no plan: later launches run in natural order
            return fail(OCH_E_INVALID, "planning render wrote no workgroup costs (kernel without cost output?)");
        }
        const std::vector<uint32_t> by_cost = och::plan::by_cost(c);
        std::vector<uint32_t> order = by_cost;
        och::plan::shape(order, p->opt_plan);
        const uint32_t block = (uint32_t)(which ? std::max(och::kBounceBlock, p->opt_block) : p->opt_block);
        const std::vector<uint32_t> grouped = och::plan::group_by_xcd(order, tiles_x, tiles_y, block);
        plan.invalidate();                    // no plan until the new one is in place (a failure below leaves none)
        if (int ds = och::pool_drain(p)) return ds;   // launches in flight on other streams may read the old order
        OCH_HIP(plan.order.upload(order));
        OCH_HIP(plan.order_xcd.upload(grouped));
        plan.h_order = order;
        plan.h_order_xcd = grouped;
        plan.serial = ++p->plan_serial;
        if (which == 0)
            if (int ss = plan_split(p, f, by_cost, order, c)) return ss;
        frame_key(p, f, which != 0, plan.key);
        plan.blocks = (uint32_t)order.size();
    }
    return OCH_OK;
}

OCH_API int och_gpu_set_row_deal(och_gpu_pool *p, int height, int row_chunk, int n_shards, const int32_t *chunk_shard)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    if (!chunk_shard && !p->deal_n) return OCH_OK;                      // round-robin already
    if (chunk_shard && p->deal_for(height, row_chunk, n_shards) && row_chunk > 0 &&
        std::equal(p->deal_table.begin(), p->deal_table.end(), chunk_shard))
        return OCH_OK;                                                  // this deal already (plans stay valid)
    // Validate the new deal and build its tables on the host first: a bad
    // call leaves the pool's current deal in place.
    std::vector<int32_t> map, owner;
    int n_chunks = 0, max_chunks = 1;
    if (chunk_shard) {
        if (height <= 0 || row_chunk <= 0 || n_shards <= 0 || n_shards > 32767)
            return fail(OCH_E_INVALID, "bad row deal geometry (%d, %d, %d)", height, row_chunk, n_shards);
        n_chunks = (height + row_chunk - 1) / row_chunk;
        std::vector<std::vector<int32_t>> mine(n_shards);
        for (int c = 0; c < n_chunks; ++c) {
            if (chunk_shard[c] < 0 || chunk_shard[c] >= n_shards)
                return fail(OCH_E_INVALID, "chunk %d dealt to shard %d of %d", c, chunk_shard[c], n_shards);
            mine[chunk_shard[c]].push_back(c);
        }
        for (const auto &m : mine) max_chunks = std::max(max_chunks, (int)m.size());
        if (max_chunks > 65535) return fail(OCH_E_INVALID, "more than 65535 chunks for one shard");
        map.assign((size_t)n_shards * max_chunks, -1);
        owner.assign(n_chunks, 0);
        for (int sh = 0; sh < n_shards; ++sh)
            for (size_t l = 0; l < mine[sh].size(); ++l) {
                map[(size_t)sh * max_chunks + l] = mine[sh][l];
                owner[mine[sh][l]] = (sh << 16) | (int32_t)l;
            }
    }
    DeviceGuard g(p->device);
    DevBuf<int32_t> d_map, d_own;             // the new tables; after the swap below, the old ones (freed on return)
    if (chunk_shard) {
        hipError_t e = d_map.upload(map);
        if (e == hipSuccess) e = d_own.upload(owner);
        if (e != hipSuccess) return fail(OCH_E_HIP, "row deal tables: %s", hipGetErrorString(e));
    }
    // frames in flight may still read the old tables; on failure the new ones
    // are freed and the old deal stays
    const hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return fail(OCH_E_HIP, "row deal: hipDeviceSynchronize: %s", hipGetErrorString(se));
    p->d_chunk_map.swap(d_map);
    p->d_owner.swap(d_own);
    p->h_chunk_map.swap(map);
    ++p->deal_serial;
    if (!chunk_shard) {                        // back to round-robin
        p->deal_n = p->deal_h = p->deal_chunk = p->deal_max = 0;
        p->deal_table.clear();
        return OCH_OK;
    }
    p->deal_h = height;
    p->deal_chunk = row_chunk;
    p->deal_n = n_shards;
    p->deal_max = max_chunks;
    p->deal_table.assign(chunk_shard, chunk_shard + n_chunks);
    return OCH_OK;
}

OCH_API int och_gpu_slice_rows(const och_gpu_pool *p, int height, int row_chunk, int n_shards, int *rows)
{
    if (!p || !rows) return fail(OCH_E_INVALID, "NULL argument");
    *rows = p->slice_rows(height, row_chunk, n_shards);
    return OCH_OK;
}

OCH_API int och_gpu_chunk_costs(och_gpu_pool *p, const och_camera *cams, int n_views, int row_chunk, float *costs)
{
    OCH_ENTRY();
    if (!p || !cams || !costs || row_chunk <= 0) return fail(OCH_E_INVALID, "bad chunk-cost arguments");
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (int vs = check_views(cams, n_views)) return vs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // one whole-frame render, natural 8x8-tile order, every workgroup timed
    const int W = cams[0].width, H = cams[0].height;
    // tiles per workgroup exactly as launch_as sizes the grid kernel's grid
    const uint32_t tiles = (uint32_t)n_views * ((uint32_t)(W + 7) / 8) * ((uint32_t)(H + 7) / 8),
                   per_block = (uint32_t)p->opt_block / 64;
    const uint32_t n_blocks = (tiles + per_block - 1) / per_block;
    const size_t frame_bytes = ((size_t)n_views * H * W * 4 + 255) & ~(size_t)255;
    int st = ensure_scratch(p, frame_bytes + (size_t)n_blocks * 4);
    if (st != OCH_OK) return st;
    const och::DevFrame f = make_frame(p, cams, n_views, reinterpret_cast<uint32_t *>(p->scratch.d), nullptr, H, 0, 1);
    // The grid kernel writes the costs: every launched workgroup overwrites its 0xFFFFFFFF, so a
    // block the launch did not cover is caught below instead of being read as
    // uninitialised scratch.
    std::vector<uint32_t> c;
    st = cost_render(p, reinterpret_cast<uint32_t *>(p->scratch.d + frame_bytes), n_blocks, c,
                     [&](const och::Schedule &sc) { return och::launch_render(p->dev(), f, sc, p->stream()); }, &f);
    if (st != OCH_OK) return st;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (c[b] == 0xFFFFFFFFu) return fail(OCH_E_INVALID, "chunk-cost render left workgroup %u untimed", b);
    const std::vector<float> spread = och::plan::spread_chunk_costs(c, n_views, W, H, per_block, row_chunk);
    std::copy(spread.begin(), spread.end(), costs);
    return OCH_OK;
}

OCH_API int och_deal_chunks(const float *costs, int n_chunks, int n_shards, const float *weights, int32_t *chunk_shard)
{
    if (!costs || !chunk_shard || n_chunks <= 0 || n_shards <= 0) return fail(OCH_E_INVALID, "bad deal arguments");
    std::vector<double> w(n_shards, 1.0);
    double w_sum = 0.0, w_max = 0.0;
    for (int s = 0; s < n_shards; ++s) {
        if (weights) w[s] = weights[s];
        if (!(w[s] > 0.0)) return fail(OCH_E_INVALID, "shard %d weight %g is not positive", s, w[s]);
        w_sum += w[s];
        w_max = std::max(w_max, w[s]);
    }
    // a shard holds at most its weighted share of the chunks plus two, which
    // bounds the padding of the equal-size slices an all-gather needs
    const int cap = (int)std::ceil(n_chunks * w_max / w_sum) + 2;
    std::vector<int> order(n_chunks);
    for (int k = 0; k < n_chunks; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return costs[a] > costs[b]; });
    std::vector<double> load(n_shards, 0.0);
    std::vector<int> count(n_shards, 0);
    for (int k : order) {             // longest processing time first, onto the least loaded shard (per weight)
        int best = -1;
        double best_score = 0.0;
        for (int s = 0; s < n_shards; ++s) {
            if (count[s] >= cap) continue;
            const double score = (load[s] + std::max(0.0f, costs[k])) / w[s];
            if (best < 0 || score < best_score || (score == best_score && count[s] < count[best])) {
                best = s;
                best_score = score;
            }
        }
        chunk_shard[k] = best;
        load[best] += std::max(0.0f, costs[k]);
        ++count[best];
    }
    return OCH_OK;
}

OCH_API int och_gpu_render_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices,
                                     int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    return render_views(p, cams, n_views, rgba_slices, row_chunk, shard, n_shards, false);
}

OCH_API int och_gpu_render_bounce_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices,
                                            int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    return render_views(p, cams, n_views, rgba_slices, row_chunk, shard, n_shards, true);
}

OCH_API int och_gpu_render_ssaa_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, int s, uint32_t *rgba,
                                          size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cams || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    return render_ssaa_views(p, cams, n_views, nullptr, s, rgba, capacity_pixels);
}

OCH_API int och_light_check(const och_light *l)
{
    if (!l) return fail(OCH_E_INVALID, "light is NULL");
    if (l->flags & ~(OCH_LIGHT_SUN | OCH_LIGHT_AO)) return fail(OCH_E_INVALID, "unknown light flags 0x%x", l->flags);
    if (l->flags & OCH_LIGHT_SUN) {
        const float *s = l->sun_dir;
        if (!std::isfinite(s[0]) || !std::isfinite(s[1]) || !std::isfinite(s[2]))
            return fail(OCH_E_INVALID, "sun_dir is not finite");
        if (s[0] == 0.0F && s[1] == 0.0F && s[2] == 0.0F) return fail(OCH_E_INVALID, "sun_dir is zero");
    }
    if ((l->flags & OCH_LIGHT_AO) && !(std::isfinite(l->ao_reach) && l->ao_reach > 0.0F))
        return fail(OCH_E_INVALID, "ao_reach %g: must be finite and > 0", (double)l->ao_reach);
    if (l->sun_shade < 0 || l->sun_shade > 256) return fail(OCH_E_INVALID, "sun_shade %d outside 0..256", l->sun_shade);
    if (l->ao_shade < 0 || l->ao_shade > 64) return fail(OCH_E_INVALID, "ao_shade %d outside 0..64", l->ao_shade);
    if (l->sun_shade + 4 * l->ao_shade > 256)
        return fail(OCH_E_INVALID, "sun_shade %d + 4 * ao_shade %d exceeds 256", l->sun_shade, l->ao_shade);
    return OCH_OK;
}

}  // extern "C"

namespace {

// och_gpu_render_lit_views_dev / _lit_masks_views_dev / _lit_codes_views_dev:
// exactly one of rgba, masks and codes.
int render_lit_views(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light, uint32_t *rgba,
                     uint8_t *masks, size_t capacity_pixels, int row_chunk, int shard, int n_shards,
                     uint16_t *codes = nullptr)
{
    // every refusal comes before anything is written or launched
    if (!p || !cams || !light || (!rgba && !masks && !codes)) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int cs = codes ? needs_code_palette(p, "lit codes") : OCH_OK) return cs;
    if (int fs = frame_args(cams, n_views, row_chunk, shard, n_shards)) return fs;
    const int W = cams[0].width, H = cams[0].height;
    const size_t pixels = (size_t)n_views * p->slice_rows(H, row_chunk, n_shards) * W;
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "the buffer holds %zu pixels, %d slices of %d x %d need %zu", capacity_pixels, n_views,
                    W, p->slice_rows(H, row_chunk, n_shards), pixels);
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    const och::DevFrame f = make_frame(p, cams, n_views, rgba, nullptr, row_chunk, shard, n_shards);
    // the primary render's plan of this grid, never its split form
    if (codes) return CAMERA_LAUNCH(p, f, false, false, och::launch_render_lit_codes(p->dev(), f, sc, *light, codes, p->stream()));
    return CAMERA_LAUNCH(p, f, false, false, och::launch_render_lit(p->dev(), f, sc, *light, masks, p->stream()));
}

}  // namespace

extern "C" {

OCH_API int och_gpu_render_lit_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                         uint32_t *rgba_slices, size_t capacity_pixels, int row_chunk, int shard,
                                         int n_shards)
{
    OCH_ENTRY();
    if (!rgba_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, rgba_slices, nullptr, capacity_pixels, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_render_lit_masks_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views,
                                               const och_light *light, uint8_t *mask_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    if (!mask_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, nullptr, mask_slices, capacity_pixels, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_render_lit_codes_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views,
                                               const och_light *light, uint16_t *code_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    if (!code_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, nullptr, nullptr, capacity_pixels, row_chunk, shard, n_shards,
                            code_slices);
}

OCH_API int och_gpu_shade_lit_unshard_views_dev(och_gpu_pool *p, const uint16_t *gathered, uint32_t *frames, int width,
                                                int height, int row_chunk, int n_shards, int n_views,
                                                const och_light *light)
{
    OCH_ENTRY();
    if (int ls = och_light_check(light)) return ls;
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, true)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_shade_lit_unshard(gathered, frames, p->d_code_table.d, width, height, row_chunk, n_shards,
                                          p->slice_rows(height, row_chunk, n_shards), n_views,
                                          p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr,
                                          light->sun_shade, light->ao_shade, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_render_lit(och_gpu_pool *p, const och_camera *cam, const och_light *light, uint32_t *rgba,
                               size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int vs = och::check_views(cam, 1)) return vs;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width, cam->height, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *o) { return och_gpu_render_lit_views_dev(p, cam, 1, light, o, pixels, cam->height, 0, 1); });
}

OCH_API int och_gpu_render_lit_ssaa_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                              int s, uint32_t *rgba, size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cams || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;      // before the s check
    return render_ssaa_views(p, cams, n_views, light, s, rgba, capacity_pixels);
}

OCH_API int och_gpu_render_lit_ssaa(och_gpu_pool *p, const och_camera *cam, const och_light *light, int s, uint32_t *rgba,
                                    size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int as = ssaa_args(cam, 1, s)) return as;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width / s, cam->height / s, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *o) { return och_gpu_render_lit_ssaa_views_dev(p, cam, 1, light, s, o, pixels); });
}

OCH_API int och_gpu_render_steps_dev(och_gpu_pool *p, const och_camera *cams, int n_views, int n_steps,
                                     void *const *streams, uint32_t *const *frames, int n_buffers,
                                     void *const *start_events, void *const *stop_events, int row_chunk, int bounce)
{
    OCH_ENTRY();
    if (!p || !cams || !streams || !frames) return fail(OCH_E_INVALID, "NULL argument");
    if (int as = loop_args(n_steps, n_buffers, start_events, stop_events, frames)) return as;
    // The frame loop of update_image (ORT/test_och_h_octree.cpp:437-457), one
    // launch per frame, issued here rather than by the caller's interpreter.
    // The pool's stream is restored afterwards, also after a failure.
    FrameLoopScope loop{p};
    int st = OCH_OK;
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        loop.frame(streams[b], start_events, stop_events, k);
        st = render_views(p, cams, n_views, frames[b], row_chunk, 0, 1, bounce != 0);
    }
    return st;
}

OCH_API int och_gpu_render_lit_steps_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                         int n_steps, void *const *streams, uint32_t *const *frames, int n_buffers,
                                         void *const *start_events, void *const *stop_events, int row_chunk)
{
    OCH_ENTRY();
    if (!p || !cams || !light || !streams || !frames) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int as = loop_args(n_steps, n_buffers, start_events, stop_events, frames)) return as;
    if (int vs = och::check_views(cams, n_views)) return vs;
    // och_gpu_render_steps_dev's loop, each frame a lit frame as one shard
    const size_t pixels = (size_t)n_views * (size_t)cams[0].width * (size_t)cams[0].height;
    FrameLoopScope loop{p};
    int st = OCH_OK;
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        loop.frame(streams[b], start_events, stop_events, k);
        st = render_lit_views(p, cams, n_views, light, frames[b], nullptr, pixels, row_chunk, 0, 1);
    }
    return st;
}

}  // extern "C"

int och::sharded_steps(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views, int n_steps,
                       void *const *streams, uint8_t *const *slices, uint8_t *const *gathered, uint32_t *const *frames,
                       int n_buffers, void *const *start_events, void *const *stop_events, int row_chunk, int bounce,
                       int exchange, bool codes, const och_light *light)
{
    if (!p || !comm || !cams || !streams || !slices) return fail(OCH_E_INVALID, "NULL argument");
    if (light && bounce) return fail(OCH_E_INVALID, "lit and bounce together are out of scope");
    if (light)
        if (int ls = och_light_check(light)) return ls;
    if (n_steps < 0 || n_buffers < 1) return fail(OCH_E_INVALID, "n_steps %d / n_buffers %d", n_steps, n_buffers);
    if (n_views < 1 || n_views > OCH_MAX_VIEWS || row_chunk <= 0) return fail(OCH_E_INVALID, "bad views / row_chunk");
    if (exchange < OCH_EXCHANGE_ALL_GATHER || exchange > OCH_EXCHANGE_GATHER)
        return fail(OCH_E_INVALID, "unknown exchange %d", exchange);
    if ((start_events == nullptr) != (stop_events == nullptr))
        return fail(OCH_E_INVALID, "start_events and stop_events: both or neither");
    int n_ranks = 0, rank = 0, device = -1;
    if (int cs = och::comm_ranks(comm, &n_ranks, &rank, &device)) return cs;
    if (device != p->device) return fail(OCH_E_INVALID, "communicator on device %d, pool on device %d", device, p->device);
    const bool receives = exchange != OCH_EXCHANGE_GATHER || rank == 0;
    const bool shades = exchange == OCH_EXCHANGE_ALL_GATHER || rank == 0;
    // Everything a frame needs is checked before the first is queued: a rank
    // that stops part way leaves its peers' collectives without a partner.
    for (int b = 0; b < n_buffers; ++b) {
        if (!slices[b]) return fail(OCH_E_INVALID, "slices[%d] is NULL", b);
        if (receives && (!gathered || !gathered[b])) return fail(OCH_E_INVALID, "rank %d needs gathered[%d]", rank, b);
        if (shades && (!frames || !frames[b])) return fail(OCH_E_INVALID, "rank %d needs frames[%d]", rank, b);
    }
    if (int vs = check_views(cams, n_views)) return vs;
    if (codes && shades && !p->d_code_table.d)
        return fail(OCH_E_INVALID, "no code table: set a palette of at most %d voxel ids", OCH_CODE_MAX_VOXELS);
    // lit codes: the rendering rank needs the palette too (render_lit_views would refuse mid-window)
    if (int cs = codes && light ? needs_code_palette(p, "lit codes") : OCH_OK) return cs;
    const int W = cams[0].width, H = cams[0].height;
    const size_t pixels = (size_t)n_views * p->slice_rows(H, row_chunk, n_ranks) * W;
    const size_t bytes = pixels * (codes ? (light ? 2 : 1) : 4);
    DeviceGuard g(p->device);
    // Per frame: render -> exchange -> shade, all on the frame's stream, so
    // the three are ordered on the device and the host never waits.  A
    // buffer set is reused only behind the previous frame on its stream.
    int st = OCH_OK;
    bool issued = false;                     // a collective of this window is queued
    FrameLoopScope loop{p};
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        const hipStream_t s = static_cast<hipStream_t>(streams[b]);
        loop.frame(streams[b], start_events, stop_events, k);
        if (light)
            st = render_lit_views(p, cams, n_views, light, codes ? nullptr : reinterpret_cast<uint32_t *>(slices[b]),
                                  nullptr, pixels, row_chunk, rank, n_ranks,
                                  codes ? reinterpret_cast<uint16_t *>(slices[b]) : nullptr);
        else
            st = render_views(p, cams, n_views, codes ? nullptr : reinterpret_cast<uint32_t *>(slices[b]), row_chunk,
                              rank, n_ranks, bounce != 0, codes ? slices[b] : nullptr);
        if (st == OCH_OK) {
            st = exchange == OCH_EXCHANGE_GATHER
                     ? och::comm_gather(comm, slices[b], receives ? gathered[b] : nullptr, bytes, 0, s)
                     : och::comm_all_gather(comm, slices[b], gathered[b], bytes, s);
            issued = issued || st == OCH_OK;
        }
        if (st == OCH_OK && shades)
            st = !codes ? och_gpu_unshard_views_dev(p, reinterpret_cast<const uint32_t *>(gathered[b]), frames[b], W, H,
                                                    row_chunk, n_ranks, n_views)
                 : light ? och_gpu_shade_lit_unshard_views_dev(p, reinterpret_cast<const uint16_t *>(gathered[b]),
                                                               frames[b], W, H, row_chunk, n_ranks, n_views, light)
                         : och_gpu_shade_unshard_views_dev(p, gathered[b], frames[b], W, H, row_chunk, n_ranks, n_views);
    }
    if (st != OCH_OK && issued) {
        // The peers' collectives of this window can no longer all complete.
        // Aborting here does not unblock the peers: their callers must abort
        // theirs (bench.py's watchdog, or the process exiting).  A failure
        // before this rank queued any collective leaves the communicator as
        // it was (every rank failing alike keeps a consistent one).
        och::comm_abort(comm);               // leaves the error text alone
        return fail(st, "%s (communicator aborted: the window stopped part way)", och_last_error());
    }
    return st;
}

extern "C" {

OCH_API int och_gpu_render_sharded_steps_dev(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views,
                                             int n_steps, void *const *streams, uint8_t *const *slices,
                                             uint8_t *const *gathered, uint32_t *const *frames, int n_buffers,
                                             void *const *start_events, void *const *stop_events, int row_chunk,
                                             int bounce, int exchange)
{
    OCH_ENTRY();
    return och::sharded_steps(p, comm, cams, n_views, n_steps, streams, slices, gathered, frames, n_buffers, start_events,
                              stop_events, row_chunk, bounce, exchange, true, nullptr);
}

OCH_API int och_gpu_render_lit_sharded_steps_dev(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views,
                                                 int n_steps, void *const *streams, uint8_t *const *slices,
                                                 uint8_t *const *gathered, uint32_t *const *frames, int n_buffers,
                                                 void *const *start_events, void *const *stop_events, int row_chunk,
                                                 const och_light *light, int exchange)
{
    OCH_ENTRY();
    if (!light) return fail(OCH_E_INVALID, "light is NULL");
    return och::sharded_steps(p, comm, cams, n_views, n_steps, streams, slices, gathered, frames, n_buffers, start_events,
                              stop_events, row_chunk, 0, exchange, true, light);
}

OCH_API int och_gpu_render_codes_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint8_t *code_slices,
                                           int row_chunk, int shard, int n_shards, int bounce)
{
    OCH_ENTRY();
    if (!code_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_views(p, cams, n_views, nullptr, row_chunk, shard, n_shards, bounce != 0, code_slices);
}

OCH_API int och_gpu_shade_unshard_views_dev(och_gpu_pool *p, const uint8_t *gathered, uint32_t *frames, int width,
                                            int height, int row_chunk, int n_shards, int n_views)
{
    OCH_ENTRY();
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, true)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_shade_unshard(gathered, frames, p->d_code_table.d, width, height, row_chunk, n_shards,
                                      p->slice_rows(height, row_chunk, n_shards), n_views,
                                      p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_render_dev(och_gpu_pool *p, const och_camera *cam, uint32_t *rgba_slice, int row_chunk, int shard,
                               int n_shards)
{
    OCH_ENTRY();
    if (!cam) return fail(OCH_E_INVALID, "NULL camera");
    return och_gpu_render_views_dev(p, cam, 1, rgba_slice, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_unshard_views_dev(och_gpu_pool *p, const uint32_t *gathered, uint32_t *frames, int width,
                                      int height, int row_chunk, int n_shards, int n_views)
{
    OCH_ENTRY();
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, false)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_unshard(gathered, frames, width, height, row_chunk, n_shards,
                                p->slice_rows(height, row_chunk, n_shards), n_views,
                                p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_unshard_dev(och_gpu_pool *p, const uint32_t *gathered, uint32_t *frame, int width, int height,
                                int row_chunk, int n_shards)
{
    OCH_ENTRY();
    return och_gpu_unshard_views_dev(p, gathered, frame, width, height, row_chunk, n_shards, 1);
}

OCH_API int och_gpu_render(och_gpu_pool *p, const och_camera *cam, uint32_t *rgba)
{
    OCH_ENTRY();
    if (!p || !cam || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    // no capacity argument, and a scratch of exactly the frame
    return to_host(p, (size_t)cam->width * cam->height, 0, rgba,
                   [&](uint32_t *scratch) { return och_gpu_render_dev(p, cam, scratch, cam->height, 0, 1); });
}

OCH_API int och_gpu_render_ssaa(och_gpu_pool *p, const och_camera *cam, int s, uint32_t *rgba, size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int as = ssaa_args(cam, 1, s)) return as;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width / s, cam->height / s, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *scratch) { return och_gpu_render_ssaa_views_dev(p, cam, 1, s, scratch, pixels); });
}

OCH_API int och_pool_pack(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                          uint32_t *out, uint32_t out_capacity, uint32_t *out_nodes, uint32_t *out_root)
{
    if (!nodes || !out_nodes || !out_root) return fail(OCH_E_INVALID, "NULL argument");
    int st = validate_pool(nodes, n_nodes, root, depth, index_base);
    if (st != OCH_OK) return st;
    std::vector<uint32_t> packed;
    uint32_t proot = 0;
    if (!pack_pool(nodes, n_nodes, root, depth, index_base, packed, proot))
        return fail(OCH_E_CAPACITY, "more than 2^24 - 1 (node, level) pairs");
    *out_nodes = (uint32_t)(packed.size() / 8);
    *out_root = proot;
    if (out) {
        if (out_capacity < *out_nodes) return fail(OCH_E_CAPACITY, "output holds %u nodes, %u needed", out_capacity, *out_nodes);
        std::memcpy(out, packed.data(), packed.size() * 4);
    }
    return OCH_OK;
}

OCH_API int och_pool_occupied_box(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                                  int32_t lo[3], int32_t hi[3])
{
    if (!nodes || !lo || !hi) return fail(OCH_E_INVALID, "NULL argument");
    if (index_base != 0 && index_base != 1) return fail(OCH_E_INVALID, "index_base must be 0 or 1");
    const int st = validate_pool(nodes, n_nodes, root, depth, index_base);
    if (st != OCH_OK) return st;
    if (!och::occupied_box(nodes, n_nodes, root, depth, index_base, lo, hi))
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
    return OCH_OK;
}

OCH_API uint32_t och_pool_at(const uint32_t *nodes, uint32_t root, int depth, int index_base, int x, int y, int z)
{
    // h_octree::at (ORT/och_h_octree.h:239-258) with the child digit of z_encode_16.
    if (!nodes || (index_base == 1 && root == 0)) return 0;
    uint32_t cur = root;
    for (int l = depth - 1; l >= 0; --l) {
        const int c = ((x >> l) & 1) | (((y >> l) & 1) << 1) | (((z >> l) & 1) << 2);
        const uint32_t nx = nodes[(size_t)(cur - index_base) * 8 + c];
        if (l == 0 || !nx) return nx;
        cur = nx;
    }
    return 0;
}

}  // extern "C"
