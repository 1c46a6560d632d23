// och_pool.cpp -- the pool as an object, and what belongs to no pool: the error
// text and the discarded-error record, the ABI version and device list; pool
// validation, packing and upload; create / destroy / info / update; the editor's
// hooks (och::pool_*); every och_gpu_set_* / get_option setting except the row
// deal; the host-only och_pool_* entries.  Nothing here launches a trace or a
// render: that is och_api.cpp.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <unordered_map>

#include "och_pool.h"

using och::DeviceGuard;
using och::fail;
using och::host_rcp;
using och::HostRcp;
using och::lut_max_rel_error;

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

int och::report(int status, const char *msg) { return fail(status, "%s", msg); }

OCH_API const char *och_last_error(void) { return g_error.c_str(); }

// ------------------------------------------------------------ discarded errors

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

}  // namespace

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

// ------------------------------------------------------------ version, devices

OCH_API int och_abi_version(void) { return OCH_GPU_ABI_VERSION; }

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

// ------------------------------------------------------------ validation, packing, upload

namespace och {

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

}  // namespace och

namespace {

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

// A pool object of n_nodes device nodes, nothing allocated yet.
och_gpu_pool *pool_new(int device, int depth, int index_base, float miss_t, uint32_t n_nodes)
{
    och_gpu_pool *p = new och_gpu_pool;
    static std::atomic<uint64_t> next_serial{1};
    p->serial = next_serial.fetch_add(1);
    p->device = device;
    p->depth = depth;
    p->index_base = index_base;
    p->miss_t = miss_t;
    p->n_nodes = n_nodes;
    return p;
}

// What every pool has besides its nodes: its stream, the timing events and this host's RCPPS table.
int pool_equip(och_gpu_pool *p)
{
    if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess ||
        // timing only: no system-scope release at the timed kernel's end
        hipEventCreateWithFlags(&p->ev_start, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_stop, hipEventDisableSystemFence) != hipSuccess)
        return fail(OCH_E_HIP, "stream/event creation failed");
    // A host whose RCPPS does not fit the model leaves the pool without a table:
    // tracing then fails with OCH_E_RCP_MODEL until och_gpu_set_rcp_lut is called.
    const HostRcp &rc = host_rcp();
    return rc.status == OCH_OK ? upload_lut(p, rc.lut.data(), rc.log2_entries) : OCH_OK;
}

}  // namespace

// ------------------------------------------------------------ create, destroy, info, update

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

    och_gpu_pool *p = pool_new(device, depth, index_base, miss_t, n_nodes + (uint32_t)index_base);   // padding node 0 for 1-based pools
    p->root = root;
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
    st = pool_equip(p);
    if (st != OCH_OK) return bail(st);
    *out = p;
    return OCH_OK;
}

// A world's pool (och_world.h): capacity slots in both layouts, the packed one
// (capacity <= 2^24) numbered like the slots, nothing in them yet and no host
// mirror; och_world_flush fills it.  The caller has the device current.
int och::pool_create_for_world(int device, int depth, uint32_t capacity, uint64_t world, och_gpu_pool **out)
{
    och_gpu_pool *p = pool_new(device, depth, 1, INFINITY, capacity);
    p->world = world;
    auto bail = [&](int s) { och_gpu_pool_destroy(p); return s; };
    if (p->d_nodes.reserve((size_t)capacity * 8) != hipSuccess ||
        (capacity <= kIdLimit && p->d_packed.reserve((size_t)capacity * 8) != hipSuccess))
        return bail(fail(OCH_E_NOMEM, "hipMalloc(%zu) failed", (size_t)capacity * 32));
    if (hipMemset(p->d_nodes.d, 0, 32) != hipSuccess || (p->d_packed.d && hipMemset(p->d_packed.d, 0, 32) != hipSuccess))
        return bail(fail(OCH_E_HIP, "hipMemset failed"));
    if (p->d_packed.d) {
        p->packed_nodes = capacity;
        p->packed_by_slot = true;
    }
    const int st = pool_equip(p);
    if (st != OCH_OK) return bail(st);
    *out = p;
    return OCH_OK;
}

int och::pool_world_view(och_gpu_pool *p, uint64_t world, WorldPoolView *v)
{
    if (!p || !v || !world || p->world != world) return fail(OCH_E_INVALID, "the pool was not made from this world");
    v->raw = p->d_nodes.d;
    v->packed = p->packed_by_slot ? p->d_packed.d : nullptr;
    v->n_nodes = p->n_nodes;
    v->generation = &p->world_generation;
    v->published = &p->world_published;
    return OCH_OK;
}

uint64_t och::pool_world(const och_gpu_pool *p) { return p ? p->world : 0; }

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
    if (p->world) return fail(OCH_E_INVALID, "a world's pool has no host mirror: it is written by och_world_flush alone");
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

// ------------------------------------------------------------ the editor's hooks (och_internal.h)

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
    if (!p || p->index_base != 1 || p->world || (count && !raw)) return fail(OCH_E_INVALID, "bad editor flush");
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
    if (!p || p->index_base != 1 || p->world || (count && (!ids || !raw))) return fail(OCH_E_INVALID, "bad editor flush");
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

// ------------------------------------------------------------ settings

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

namespace {

// Option ids retired in round 5 (measured slower on every scene, DESIGN.md
// §8): 0 schedule (persistent / refill), 2 waves per CU, 3 refill, 7 chunk
// tiles, 9 merge, 12 per-node skip, 13 column cull.  Their ids stay unused.
static int retired_option(int option)
{
    return fail(OCH_E_INVALID, "option %d was retired (the grid schedule alone remains; DESIGN.md section 8)", option);
}

}  // namespace

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

OCH_API int och_gpu_set_stamp_buffer(och_gpu_pool *p, uint64_t *stamps, uint32_t capacity_waves)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    p->stamps = capacity_waves ? stamps : nullptr;
    p->stamp_cap = stamps ? capacity_waves : 0;
    return OCH_OK;
}

OCH_API int och_gpu_set_launch_events(och_gpu_pool *p, void *start_event, void *stop_event)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    p->next_ev_start = static_cast<hipEvent_t>(start_event);
    p->next_ev_stop = static_cast<hipEvent_t>(stop_event);
    return OCH_OK;
}

// ------------------------------------------------------------ host-only pool entries

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

int och::read_box_cells(const char *who, const int32_t lo[3], const int32_t hi[3], int kind, const void *grid,
                        size_t capacity_bytes, uint64_t *cells)
{
    *cells = 0;
    if (!lo || !hi || !grid) return fail(OCH_E_INVALID, "%s: NULL argument", who);
    if (kind != OCH_VOXELS_GRID_U8 && kind != OCH_VOXELS_GRID_U32)
        return fail(OCH_E_INVALID, "%s: kind must be OCH_VOXELS_GRID_U8 or OCH_VOXELS_GRID_U32", who);
    uint64_t n[3];
    for (int a = 0; a < 3; ++a) {
        if (hi[a] < lo[a]) return fail(OCH_E_INVALID, "%s: hi[%d] = %d lies below lo[%d] = %d", who, a, hi[a], a, lo[a]);
        n[a] = (uint64_t)((int64_t)hi[a] - (int64_t)lo[a]);
    }
    if (!n[0] || !n[1] || !n[2]) return OCH_OK;
    // n[0] * n[1] * n[2] <= room without forming a product that could pass 64 bits
    const uint64_t room = (uint64_t)capacity_bytes / (kind == OCH_VOXELS_GRID_U8 ? 1u : 4u);
    if (n[0] > room || n[1] > room / n[0] || n[2] > room / n[0] / n[1])
        return fail(OCH_E_INVALID, "%s: a box of %llu x %llu x %llu cells does not fit %zu bytes", who,
                    (unsigned long long)n[0], (unsigned long long)n[1], (unsigned long long)n[2], capacity_bytes);
    *cells = n[0] * n[1] * n[2];
    return OCH_OK;
}

namespace {

// och_pool_read_box's walk: only the nodes that meet the box (clipped to the
// tree) are visited, so empty space costs nothing beyond the zeroed grid.
struct BoxReader {
    const uint32_t *nodes;
    int base;
    int64_t clo[3], chi[3], lo[3];
    uint64_t nx, ny;
    bool u8;
    void *grid;
    uint32_t over = 0;   // the first id met that a u8 cell cannot hold

    // node v at height h with its corner at o: its children have side 1 << h
    void walk(uint32_t v, int h, const int64_t o[3])
    {
        const uint32_t *c = nodes + (size_t)(v - (uint32_t)base) * 8;
        const int64_t s = (int64_t)1 << h;
        for (int k = 0; k < 8 && !over; ++k) {
            if (!c[k]) continue;
            const int64_t p[3] = {o[0] + (k & 1) * s, o[1] + ((k >> 1) & 1) * s, o[2] + ((k >> 2) & 1) * s};
            if (p[0] >= chi[0] || p[0] + s <= clo[0] || p[1] >= chi[1] || p[1] + s <= clo[1] || p[2] >= chi[2] ||
                p[2] + s <= clo[2])
                continue;
            if (h) {
                walk(c[k], h - 1, p);
                continue;
            }
            const size_t at = ((size_t)(p[2] - lo[2]) * ny + (size_t)(p[1] - lo[1])) * nx + (size_t)(p[0] - lo[0]);
            if (!u8)
                static_cast<uint32_t *>(grid)[at] = c[k];
            else if (c[k] <= 255u)
                static_cast<uint8_t *>(grid)[at] = (uint8_t)c[k];
            else
                over = c[k];
        }
    }
};

}  // namespace

OCH_API int och_pool_read_box(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                              const int32_t lo[3], const int32_t hi[3], int kind, void *grid, size_t capacity_bytes)
{
    if (!nodes) return fail(OCH_E_INVALID, "och_pool_read_box: NULL argument");
    if (index_base != 0 && index_base != 1) return fail(OCH_E_INVALID, "och_pool_read_box: index_base must be 0 or 1");
    uint64_t cells = 0;
    if (const int cs = och::read_box_cells("och_pool_read_box", lo, hi, kind, grid, capacity_bytes, &cells)) return cs;
    if (const int vs = validate_pool(nodes, n_nodes, root, depth, index_base)) return vs;
    if (!cells) return OCH_OK;
    BoxReader r{};
    r.nodes = nodes;
    r.base = index_base;
    r.u8 = kind == OCH_VOXELS_GRID_U8;
    r.grid = grid;
    std::memset(grid, 0, (size_t)cells * (r.u8 ? 1 : 4));
    const int64_t dim = (int64_t)1 << depth;
    bool meets = !(index_base == 1 && root == 0);
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = lo[a];
        r.clo[a] = std::max<int64_t>(lo[a], 0);
        r.chi[a] = std::min<int64_t>(hi[a], dim);
        meets = meets && r.clo[a] < r.chi[a];
    }
    r.nx = (uint64_t)((int64_t)hi[0] - lo[0]);
    r.ny = (uint64_t)((int64_t)hi[1] - lo[1]);
    const int64_t origin[3] = {0, 0, 0};
    if (meets) r.walk(root, depth - 1, origin);
    if (r.over) return fail(OCH_E_INVALID, "och_pool_read_box: voxel id %u does not fit a u8 grid", r.over);
    return OCH_OK;
}

namespace {

// och_pool_diff's walk: both trees at once, child digits ascending, so the
// differing voxels come out in ascending Morton order.  An absent side reads
// zeros all the way down; an all-zero node on one side is no node either.
struct PoolDiffer {
    const uint32_t *na, *nb;
    int base;
    bool same_array;     // both arguments are one array: equal ids are equal subtrees
    uint32_t *out;       // null: count only
    uint64_t n = 0, pairs = 0;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};

    // the position at height h with its corner at o; has_a / has_b: a node is there
    void walk(bool has_a, uint32_t a, bool has_b, uint32_t b, int h, const uint32_t o[3])
    {
        static const uint32_t zeros[8] = {0};
        const uint32_t *ca = has_a ? na + (size_t)(a - (uint32_t)base) * 8 : zeros;
        const uint32_t *cb = has_b ? nb + (size_t)(b - (uint32_t)base) * 8 : zeros;
        const uint32_t s = 1u << h;
        ++pairs;
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t wa = ca[k], wb = cb[k];
            const uint32_t p[3] = {o[0] + (k & 1u) * s, o[1] + ((k >> 1) & 1u) * s, o[2] + ((k >> 2) & 1u) * s};
            if (h) {
                if ((!wa && !wb) || (same_array && wa == wb)) continue;
                walk(wa != 0, wa, wb != 0, wb, h - 1, p);
            } else if (wa != wb) {
                if (out) {
                    uint32_t *r = out + n * 4;
                    r[0] = p[0], r[1] = p[1], r[2] = p[2], r[3] = wb;
                }
                for (int ax = 0; ax < 3; ++ax) {
                    lo[ax] = std::min(lo[ax], p[ax]);
                    hi[ax] = std::max(hi[ax], p[ax]);
                }
                ++n;
            }
        }
    }
};

}  // namespace

OCH_API int och_pool_diff(const uint32_t *nodes_a, uint32_t n_a, uint32_t root_a, const uint32_t *nodes_b, uint32_t n_b,
                          uint32_t root_b, int depth, int index_base, void *records, uint64_t capacity, och_diff_stats *stats)
{
    if (!stats) return fail(OCH_E_INVALID, "och_pool_diff: stats is NULL");
    if (!nodes_a || !nodes_b) return fail(OCH_E_INVALID, "och_pool_diff: NULL argument");
    if (index_base != 0 && index_base != 1) return fail(OCH_E_INVALID, "och_pool_diff: index_base must be 0 or 1");
    if (depth < 1 || depth > 21)
        return fail(OCH_E_INVALID, "och_pool_diff: depth must be 1..21 (a record's Morton key has 3 * depth bits)");
    if (const int vs = validate_pool(nodes_a, n_a, root_a, depth, index_base)) return vs;
    if (const int vs = validate_pool(nodes_b, n_b, root_b, depth, index_base)) return vs;
    const bool has_a = !(index_base == 1 && root_a == 0), has_b = !(index_base == 1 && root_b == 0);
    const uint32_t origin[3] = {0, 0, 0};
    PoolDiffer count{nodes_a, nodes_b, index_base, nodes_a == nodes_b, nullptr};
    const bool equal_roots = count.same_array && has_a == has_b && (!has_a || root_a == root_b);
    if ((has_a || has_b) && !equal_roots) count.walk(has_a, root_a, has_b, root_b, depth - 1, origin);
    if (count.n >= (1ull << 31)) return fail(OCH_E_INVALID, "och_pool_diff: the differing voxels number 2^31 or more");
    och_diff_stats ds;
    std::memset(&ds, 0, sizeof ds);
    ds.n = count.n;
    ds.pairs = count.pairs;
    for (int a = 0; a < 3 && count.n; ++a) {
        ds.box_lo[a] = (int32_t)count.lo[a];
        ds.box_hi[a] = (int32_t)count.hi[a] + 1;
    }
    *stats = ds;
    if (!records || !count.n) return OCH_OK;
    if (count.n > capacity)
        return fail(OCH_E_CAPACITY, "och_pool_diff: %llu records, the buffer holds %llu", (unsigned long long)count.n,
                    (unsigned long long)capacity);
    PoolDiffer write{nodes_a, nodes_b, index_base, nodes_a == nodes_b, static_cast<uint32_t *>(records)};
    write.walk(has_a, root_a, has_b, root_b, depth - 1, origin);
    return OCH_OK;
}

och::BoxCubes och::box_cube_counts(const int32_t lo[3], const int32_t hi[3], int depth)
{
    BoxCubes c;
    const int64_t dim = (int64_t)1 << depth;
    int64_t l[3], h[3];
    bool any = true;
    for (int a = 0; a < 3; ++a) {
        l[a] = std::max<int64_t>(lo[a], 0);
        h[a] = std::min<int64_t>(hi[a], dim);
        any = any && l[a] < h[a];
    }
    if (!any) return c;
    c.any = true;
    uint64_t in[23];   // prod in_a by height, 0 .. depth + 1
    for (int H = 0; H <= depth + 1; ++H) {
        uint64_t touch = 1, inside = 1;
        for (int a = 0; a < 3; ++a) {
            const int64_t s = (int64_t)1 << H;
            touch *= (uint64_t)(((h[a] + s - 1) >> H) - (l[a] >> H));
            inside *= (uint64_t)std::max<int64_t>(0, (h[a] >> H) - ((l[a] + s - 1) >> H));
        }
        in[H] = inside;
        if (H <= depth) c.cells[H] = touch - inside;
    }
    for (int H = 0; H <= depth; ++H) {
        c.cubes[H] = in[H] - 8 * in[H + 1];
        c.n_cubes += c.cubes[H];
        c.n_cells += c.cells[H];
        if (c.cubes[H]) c.top = H;
    }
    for (int a = 0; a < 3; ++a) {
        c.lo[a] = (int32_t)l[a];
        c.hi[a] = (int32_t)h[a];
    }
    return c;
}

OCH_API int och_box_cubes(const int32_t lo[3], const int32_t hi[3], int depth, uint64_t *keys, uint8_t *heights,
                          uint64_t capacity, uint64_t cubes_per_height[22], uint64_t cells_per_height[22], uint64_t *count)
{
    if (!lo || !hi) return fail(OCH_E_INVALID, "och_box_cubes: lo or hi is NULL");
    if (!count) return fail(OCH_E_INVALID, "och_box_cubes: count is NULL");
    if (depth < 1 || depth > 21) return fail(OCH_E_INVALID, "och_box_cubes: depth must be 1..21 (a Morton key has 3 * depth bits)");
    if ((keys == nullptr) != (heights == nullptr) || (!keys && capacity))
        return fail(OCH_E_INVALID, "och_box_cubes: keys and heights go together, and capacity counts their entries");
    const och::BoxCubes c = och::box_cube_counts(lo, hi, depth);
    if (cubes_per_height) std::copy(c.cubes, c.cubes + 22, cubes_per_height);
    if (cells_per_height) std::copy(c.cells, c.cells + 22, cells_per_height);
    *count = c.n_cubes;
    if (!keys || !c.n_cubes) return OCH_OK;
    if (c.n_cubes > capacity)
        return fail(OCH_E_CAPACITY, "och_box_cubes: %llu cubes, the buffers hold %llu", (unsigned long long)c.n_cubes,
                    (unsigned long long)capacity);
    // top-down, a level's straddling cells in Morton order, child digits ascending: each height's
    // cubes come out in ascending Morton order; height h's go to [first[h], first[h] + cubes[h])
    uint64_t first[22] = {0}, at[22] = {0};
    for (int h = 1; h <= depth; ++h) first[h] = at[h] = first[h - 1] + c.cubes[h - 1];
    struct Cell {
        uint64_t key;
        int32_t o[3];
    };
    auto emit = [&](int h, uint64_t key) {
        keys[at[h]] = key;
        heights[at[h]++] = (uint8_t)h;
    };
    if (c.top == depth) {   // the whole tree
        emit(depth, 0);
        return OCH_OK;
    }
    std::vector<Cell> front{{0, {0, 0, 0}}}, next;
    for (int H = depth; H >= 1 && !front.empty(); --H) {
        const int32_t s = (int32_t)1 << (H - 1);
        next.clear();
        for (const Cell &f : front)
            for (int k = 0; k < 8; ++k) {
                const Cell ch{f.key << 3 | (uint64_t)k, {f.o[0] + (k & 1) * s, f.o[1] + ((k >> 1) & 1) * s, f.o[2] + ((k >> 2) & 1) * s}};
                bool inside = true, outside = false;
                for (int a = 0; a < 3; ++a) {
                    inside = inside && c.lo[a] <= ch.o[a] && ch.o[a] + s <= c.hi[a];
                    outside = outside || ch.o[a] >= c.hi[a] || ch.o[a] + s <= c.lo[a];
                }
                if (inside)
                    emit(H - 1, ch.key);
                else if (!outside)
                    next.push_back(ch);
            }
        front.swap(next);
    }
    for (int h = 0; h <= depth; ++h)
        if (at[h] != first[h] + c.cubes[h]) return fail(OCH_E_INVALID, "och_box_cubes: the walk and the closed forms disagree");
    return OCH_OK;
}

och::BoxCubes och::ball_cube_walk(const int32_t c2[3], uint32_t diameter, int depth, uint64_t *keys, uint8_t *heights, uint64_t capacity)
{
    BoxCubes c;
    c.any = ball_axis_box(c2, diameter, depth, c.lo, c.hi);
    if (!c.any) return c;
    const Ball B = make_ball(c2, diameter);
    struct Cell {
        uint64_t key;
        int32_t o[3];
    };
    // top-down, a level's straddling cells in Morton order, child digits ascending: each height's
    // cubes come out in ascending Morton order; with `at`, height h's go to keys[at[h]...]
    const auto walk = [&](uint64_t *at) {
        const Cell root{0, {0, 0, 0}};
        const int rc = ball_class(B, root.o, depth);
        if (rc == 2) {   // the whole tree
            if (at) {
                keys[at[depth]] = 0;
                heights[at[depth]++] = (uint8_t)depth;
            } else {
                c.cubes[depth] = 1;
            }
        }
        if (rc != 1) return;
        std::vector<Cell> front{root}, next;
        for (int H = depth; H >= 1 && !front.empty(); --H) {
            const int32_t s = (int32_t)1 << (H - 1);
            if (!at) c.cells[H] = front.size();
            next.clear();
            for (const Cell &f : front)
                for (int k = 0; k < 8; ++k) {
                    const Cell ch{f.key << 3 | (uint64_t)k, {f.o[0] + (k & 1) * s, f.o[1] + ((k >> 1) & 1) * s, f.o[2] + ((k >> 2) & 1) * s}};
                    const int cc = ball_class(B, ch.o, H - 1);
                    if (cc == 1) {
                        next.push_back(ch);
                    } else if (cc == 2 && at) {
                        keys[at[H - 1]] = ch.key;
                        heights[at[H - 1]++] = (uint8_t)(H - 1);
                    } else if (cc == 2) {
                        ++c.cubes[H - 1];
                    }
                }
            front.swap(next);
        }
    };
    walk(nullptr);
    for (int H = 0; H <= depth; ++H) {
        c.n_cubes += c.cubes[H];
        c.n_cells += c.cells[H];
        if (c.cubes[H]) c.top = H;
    }
    if (keys && c.n_cubes && c.n_cubes <= capacity) {
        uint64_t at[22] = {0};
        for (int h = 1; h <= depth; ++h) at[h] = at[h - 1] + c.cubes[h - 1];
        walk(at);
    }
    return c;
}

OCH_API int och_sphere_cubes(const int32_t centre2[3], uint32_t diameter, int depth, uint64_t *keys, uint8_t *heights,
                             uint64_t capacity, uint64_t cubes_per_height[22], uint64_t cells_per_height[22], uint64_t *count)
{
    if (!centre2) return fail(OCH_E_INVALID, "och_sphere_cubes: centre2 is NULL");
    if (!count) return fail(OCH_E_INVALID, "och_sphere_cubes: count is NULL");
    if (depth < 1 || depth > 21) return fail(OCH_E_INVALID, "och_sphere_cubes: depth must be 1..21 (a Morton key has 3 * depth bits)");
    if ((keys == nullptr) != (heights == nullptr) || (!keys && capacity))
        return fail(OCH_E_INVALID, "och_sphere_cubes: keys and heights go together, and capacity counts their entries");
    if (const char *range = och::ball_range_error(centre2, diameter)) return fail(OCH_E_INVALID, "och_sphere_cubes: %s", range);
    const och::BoxCubes c = och::ball_cube_walk(centre2, diameter, depth, keys, heights, capacity);
    if (cubes_per_height) std::copy(c.cubes, c.cubes + 22, cubes_per_height);
    if (cells_per_height) std::copy(c.cells, c.cells + 22, cells_per_height);
    *count = c.n_cubes;
    if (keys && c.n_cubes > capacity)
        return fail(OCH_E_CAPACITY, "och_sphere_cubes: %llu cubes, the buffers hold %llu", (unsigned long long)c.n_cubes,
                    (unsigned long long)capacity);
    return OCH_OK;
}
