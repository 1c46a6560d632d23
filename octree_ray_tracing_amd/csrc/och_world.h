// och_world.h -- the resident world (och_world_*): a DAG that stays on one GPU
// between brush strokes.  Included by och_builder.cpp only, after
// och_voxel_edit.h, whose steps it runs over a store that outlives the call:
//   create   -- upload, reach and adopt (edit_upload, edit_reach, edit_adopt),
//               once; the store, its table and the root stay on the device.
//   edit     -- records and levels (edit_records, edit_levels) against that
//               store, then the root is replaced.  Nothing of the pool is
//               uploaded, reached, adopted, renumbered, counted or downloaded.
//   flush    -- the ids handed out since a pool's last flush, copied (raw
//               layout) and packed (k_world_pack) on the device, then the
//               roots and the box through och::pool_commit.
//   download -- renumber_gpu + pool_stats_gpu from the current root.
//   compact  -- renumber_gpu, then the renumbered pool adopted into a fresh
//               store (its levels are contiguous id ranges: no reach).
//
// Append-only.  alloc_node writes only ids nobody has seen yet and k_settle
// only finishes table slots claimed in the same level, so a stroke changes no
// row that any earlier root reaches: a frame in flight that walks a pool from
// an earlier root reads only ids below that flush's `used`, a later flush
// writes only ids at or above it, and no device-wide wait is needed before
// publishing.  Store and pool meet only across dispatch boundaries (the flush
// ends in a synchronise of the world's stream; a launch takes its root by
// value, after that), which is all the per-XCD L2s ask for (k_intern's rule,
// och_dag.h).
//
// Capacity is checked before anything is interned: a stroke that ran out of
// ids half way would leave table slots that went back to 0 behind probes that
// already passed them; a later equal row would be interned twice and the
// downloaded pool would no longer be canonical.  The bound, used + the level
// counts of the stroke's unique keys, allows one id per row of the records'
// own tree: a row allocates at most one id (its claimant's), so no intern of
// an admitted stroke can fail, and the answer depends on the records alone.
//
// Said once, here, for this file, och_world_read.h and och_world_history.h:
//   the state        -- WorldSnapshot (root, child mask, box): och_world::now,
//                       copied by a snapshot, assigned by a checkout.
//   the box          -- six words on the device (kNoBox, box_reduce), lo / hi
//                       exclusive on the host (WorldBox, box_decode, box_union).
//   an entry         -- world_call: the usable check, the world's device, the
//                       body, its status to the caller (who reports what, and
//                       when a HIP failure breaks the world).
//   a host array     -- world_stage (its place on the device) and
//                       world_read_back (queue, synchronise, then look).
//   the rest         -- row_mask, WorldHead / world_read_head, world_install
//                       (a compaction's end), world_phase (the trace's timer).
//
// Out of scope: worlds replicated across GPUs, frame groups and the sharded
// paths; 0-based pools; depth 22.  Reading the world back (at, a box to a grid,
// the exact box after removals) is och_world_read.h, with what stays out of
// scope there; remembering earlier roots (snapshot, checkout, the diff of two
// roots) is och_world_history.h; strokes whose shape is a box or a ball (fill,
// clear, restore from a snapshot) are och_world_region.h, those conditional on
// the old voxel (paint, fill-under, replace) och_world_paint.h.
#pragma once
#include <map>
#include <memory>

#include "och_host.h"
#include "och_voxel_edit.h"

namespace {

// Words of a store's head (GpuStore.next; [0] the id counter, [1] overflow,
// the tree-node counters from word 64) that a world uses: the current root
// and its child mask, and the stroke's box (min x y z, max x y z, inclusive).
constexpr int kHeadRoot = 8, kHeadBox = 16, kHeadWords = 22;

// The child mask of a row: bit k set where child word k is not 0.
__device__ inline uint32_t row_mask(const uint32_t *__restrict__ row)
{
    const uint4 *rec = reinterpret_cast<const uint4 *>(row);
    const uint4 a = rec[0], b = rec[1];
    return (uint32_t)(a.x != 0) | (uint32_t)(a.y != 0) << 1 | (uint32_t)(a.z != 0) << 2 | (uint32_t)(a.w != 0) << 3 |
           (uint32_t)(b.x != 0) << 4 | (uint32_t)(b.y != 0) << 5 | (uint32_t)(b.z != 0) << 6 | (uint32_t)(b.w != 0) << 7;
}

// The stroke's result into the head, for one read-back with the id counter.
__global__ __launch_bounds__(64) void k_world_root(GpuStore S, const uint32_t *__restrict__ new_root, uint32_t *__restrict__ head)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t r = *new_root;
    head[kHeadRoot] = r;
    head[kHeadRoot + 1] = r && r < S.cap ? row_mask(S.nodes + (size_t)r * 8) : 0u;
}

// A box on the device: six words, min x y z then max x y z, inclusive; kNoBox
// while it holds no voxel.  box_decode (below) is the host's reading of it.
constexpr uint32_t kNoBox[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0};

// A wavefront's voxels into `box`, this lane's at Morton key `key()` if it
// `has` one: the minima and maxima in registers, then six atomics by the first
// lane of a wavefront that holds a voxel (`some`: the caller knows that it does).
template <class Key>
__device__ inline void box_reduce(bool has, Key key, bool some, uint32_t *__restrict__ box)
{
    uint32_t lo[3] = {kNoBox[0], kNoBox[1], kNoBox[2]}, hi[3] = {kNoBox[3], kNoBox[4], kNoBox[5]};
    if (has) {
        const uint64_t k = key();
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = compact3(k >> a);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor(lo[a], o));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor(hi[a], o));
        }
    if ((threadIdx.x & 63u) == 0 && (some || lo[0] != kNoBox[0])) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(box + a, lo[a]);
            atomicMax(box + 3 + a, hi[a]);
        }
    }
}

// The box of the stroke's voxels, from its m unique keys and their ids (id 0
// is a removal: no voxel).  box: kNoBox before.
__global__ __launch_bounds__(256) void k_world_box(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ words,
                                                   uint32_t m, uint32_t *__restrict__ box)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool has = i < m && words[i];
    const uint64_t key = has ? keys[i] : 0ull;   // loaded here, not in the helper: the instructions the kernel always had
    box_reduce(has, [&] { return key; }, false, box);
}

// The packed layout numbered like the store, ids [lo, hi): thread q is child
// word q & 7 of id lo + q / 8.  An interior word becomes child | mask(child) << 24
// (the child's row is an earlier dispatch's), a leaf-level word stays as it is.
__global__ __launch_bounds__(256) void k_world_pack(GpuStore S, uint32_t lo, uint32_t hi, uint32_t *__restrict__ packed)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)(hi - lo) * 8) return;
    const uint32_t id = lo + (uint32_t)(q >> 3);
    const size_t at = (size_t)id * 8 + (q & 7u);
    uint32_t w = S.nodes[at];
    if (w && w < S.cap && S.level[id] != 0) w |= row_mask(S.nodes + (size_t)w * 8) << 24;
    packed[at] = w;
}

// list[i] = first + i
__global__ __launch_bounds__(256) void k_world_iota(uint32_t *__restrict__ list, uint32_t n, uint32_t first)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) list[i] = first + i;
}

constexpr uint32_t kWorldIdLimit = 1u << 24;           // packed ids are 24 bits
constexpr uint32_t kWorldCapLimit = (1u << 29) - 1;    // a pool's n_nodes + 1 stays below 2^29 (och_gpu_pool_create)

}  // namespace

// A box as the host keeps it: lo inclusive, hi exclusive; all 0 without a voxel.
struct WorldBox {
    bool any = false;
    int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};

// A state of the world: a root of the append-only store with its child mask
// and the box of its voxels.  The world's current one (och_world::now), and
// what a snapshot keeps of it (och_world_history.h): a copy.
struct WorldSnapshot {
    uint32_t root = 0, root_mask = 0;
    WorldBox box;
};

struct och_world {
    int device = 0, depth = 0;
    uint64_t id = 0;                  // process-unique, never reused: the mark on this world's pools
    bool broken = false;
    hipStream_t st = nullptr;
    std::unique_ptr<GpuScope> store_scope, work_scope;   // both on st, which the world owns
    GpuStore S{};
    EditWork W;                       // for W.n_cap records and as many rows, grown on demand and kept
    void *d_upload = nullptr;         // W.n_cap host records' way to the device
    uint32_t used = 1;
    WorldSnapshot now;                // the current state
    uint64_t strokes = 0, generation = 0;
    // och_world_read.h: freed after the destructor's body, the stream gone by then (hipFree waits for the device)
    och::DevBuf<uint8_t> d_read;      // a host grid's, or host coordinates' and ids', way through the device
    och::DevBuf<ulonglong2> d_lbox;   // the local boxes of ids [1, boxed) of generation lbox_generation
    uint32_t boxed = 1;
    uint64_t lbox_generation = 0;
    // och_world_history.h: the live snapshots by handle (ascending; handles start at 1 and are never
    // reused) and the diff's frontier, count and scan buffers for diff_cap pairs a level, kept
    std::map<uint64_t, WorldSnapshot> snapshots;
    uint64_t next_snapshot = 1;
    // a checkout changed now.root and now.root_mask on the host only: the next stroke, which starts from
    // the head's root word, uploads them first (from head_up, which outlives the copy)
    bool head_stale = false;
    uint32_t head_up[2] = {0, 0};
    och::DevBuf<uint8_t> d_diff;
    uint32_t diff_cap = 0;
    size_t diff_temp_bytes = 0;
    // och_world_region.h: a region stroke's cubes, frontiers, counts and scan storage, sized by its box, kept
    och::DevBuf<uint8_t> d_region;
    // och_world_paint.h: a conditional stroke's map (the distinct nodes under the shape, their sort and scan), kept
    och::DevBuf<uint8_t> d_paint;

    uint32_t *head() const { return S.next; }
    ~och_world()
    {
        work_scope.reset();           // each synchronises st before it frees
        store_scope.reset();
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

PhaseTimer world_phase(const och_world &w) { return PhaseTimer{"world ", 4, w.st}; }

// The host's reading of a device box.
WorldBox box_decode(const uint32_t box[6])
{
    WorldBox b;
    b.any = box[0] != kNoBox[0];
    for (int a = 0; a < 3 && b.any; ++a) {
        b.lo[a] = (int32_t)box[a];
        b.hi[a] = (int32_t)box[3 + a] + 1;
    }
    return b;
}

void box_union(WorldBox &into, const WorldBox &b)
{
    if (!b.any) return;
    for (int a = 0; a < 3; ++a) {
        into.lo[a] = into.any ? std::min(into.lo[a], b.lo[a]) : b.lo[a];
        into.hi[a] = into.any ? std::max(into.hi[a], b.hi[a]) : b.hi[a];
    }
    into.any = true;
}

// Where a call's array of `bytes` stands on the device: a device array is its
// own place, a host array's is the world's staging buffer, grown when it has
// to be (nullptr: no memory for it).
void *world_stage(och_world &w, const void *array, size_t bytes, bool on_device)
{
    if (on_device) return const_cast<void *>(array);
    return w.d_read.reserve(bytes) == hipSuccess ? w.d_read.d : nullptr;
}

// A copy to the host; one of no bytes is left out.
struct ReadBack {
    void *to;
    const void *from;
    size_t bytes;
};

// Queue the copies, then synchronise the stream whatever they returned: the
// destinations may be the caller's frame's, and nothing writes there once it
// has gone.  Fails if a copy or the synchronise failed.
int world_read_back(och_world &w, std::initializer_list<ReadBack> copies)
{
    hipError_t ce = hipSuccess;
    for (const ReadBack &c : copies)
        if (ce == hipSuccess && c.bytes) ce = hipMemcpyAsync(c.to, c.from, c.bytes, hipMemcpyDeviceToHost, w.st);
    const hipError_t se = hipStreamSynchronize(w.st);
    return ce == hipSuccess && se == hipSuccess ? OCH_OK : OCH_E_HIP;
}

// A store's head after the last dispatch on it: the ids in use, the root and
// its mask, the device box.
struct WorldHead {
    uint32_t used = 0, root = 0, mask = 0, box[6] = {0};
};

int world_read_head(och_world &w, const GpuStore &S, WorldHead *H)
{
    uint32_t h[kHeadWords] = {0};
    if (const int rs = world_read_back(w, {{h, S.next, sizeof h}})) return rs;
    if (h[1] & 4u) return och::report(OCH_E_HIP, "och_world: a row outside its level");
    if (h[1]) return och::report(OCH_E_HIP, "och_world: the store overflowed after its capacity check");
    H->used = std::min(h[0], S.cap);
    H->root = h[kHeadRoot];
    H->mask = h[kHeadRoot + 1];
    std::memcpy(H->box, h + kHeadBox, sizeof H->box);
    return OCH_OK;
}

// Work buffers for n records: kept while they suffice, else replaced by larger ones.
int world_reserve(och_world &w, uint32_t n)
{
    size_t need = 0;
    if (const int ts = edit_temp_bytes(n, w.depth, w.st, &need)) return ts;
    if (n <= w.W.n_cap && need <= w.W.temp_bytes) return OCH_OK;
    uint32_t cap = 4096;
    while (cap < n) cap <<= 1;
    w.work_scope.reset();
    w.W = EditWork{};
    w.d_upload = nullptr;
    w.work_scope.reset(new GpuScope(w.st));
    GpuScope &G = *w.work_scope;
    int st = edit_work_records(G, w.W, cap, w.depth);
    if (st == OCH_OK) st = edit_work_rows(G, w.W, cap);   // a level's rows never outnumber the keys
    if (st == OCH_OK && !G.alloc(&w.d_upload, (size_t)cap * 16)) st = OCH_E_NOMEM;
    if (st == OCH_OK && w.W.temp_bytes < need) st = OCH_E_NOMEM;
    if (st != OCH_OK) {
        w.work_scope.reset();
        w.W = EditWork{};
        w.d_upload = nullptr;
    }
    return st;
}

int world_edit(och_world &w, const void *records, uint32_t n, bool on_device)
{
    const hipStream_t st = w.st;
    PhaseTimer phase = world_phase(w);
    if (const int rs = world_reserve(w, n)) return rs;
    const void *d_in = records;
    if (!on_device) {
        GPU_TRY(hipMemcpyAsync(w.d_upload, records, (size_t)n * 16, hipMemcpyHostToDevice, st));
        d_in = w.d_upload;
    }
    if (!phase("upload")) return OCH_E_HIP;
    uint32_t m = 0;
    uint64_t counts[kMaxVoxelDepth] = {0}, rows_total = 0;
    if (const int es = edit_records(st, w.W, static_cast<const uint32_t *>(d_in), n, w.depth, phase, m, counts, rows_total))
        return es;
    if (!m) {   // every record outside the tree
        ++w.strokes;
        return OCH_OK;
    }
    // before anything is interned: see the head of this file
    if ((uint64_t)w.used + rows_total > w.S.cap) return report_build(OCH_E_CAPACITY, "och_world", "");
    uint32_t *head = w.head();
    if (w.head_stale) {
        w.head_up[0] = w.now.root;
        w.head_up[1] = w.now.root_mask;
        GPU_TRY(hipMemcpyAsync(head + kHeadRoot, w.head_up, sizeof w.head_up, hipMemcpyHostToDevice, st));
        w.head_stale = false;
    }
    GPU_TRY(hipMemcpyAsync(head + kHeadBox, kNoBox, sizeof kNoBox, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_world_box, blocks(m), dim3(256), 0, st, w.W.keys[0], w.W.words[0], m, head + kHeadBox);
    GPU_TRY(hipGetLastError());
    const uint32_t *d_new = nullptr;
    if (const int ls = edit_levels(st, w.W, w.S, head + kHeadRoot, m, counts, w.depth, &d_new)) return ls;
    hipLaunchKernelGGL(k_world_root, dim3(1), dim3(64), 0, st, w.S, d_new, head);
    GPU_TRY(hipGetLastError());
    WorldHead H;
    if (const int hs = world_read_head(w, w.S, &H)) return hs;
    if (!phase("levels")) return OCH_E_HIP;
    if (phase.on)
        std::fprintf(stderr, "[och_build] world: %u records, %u keys, %u new ids, %u of %u used\n", n, m, H.used - w.used, H.used,
                     w.S.cap);
    w.used = H.used;
    w.now.root = H.root;
    w.now.root_mask = H.mask;
    box_union(w.now.box, box_decode(H.box));
    ++w.strokes;
    return OCH_OK;
}

// A fresh store of `cap` ids holding the 1-based pool R names (reached, on the
// device), in a scope of its own on the world's stream; T takes the adoption's
// rows.  H: the store's head after the adoption.
int world_adopt(och_world &w, GpuScope &T, const EditReach &R, uint32_t cap, std::unique_ptr<GpuScope> &scope, GpuStore &S,
                WorldHead *H)
{
    scope.reset(new GpuScope(w.st));
    if (const int cs = gpu_store_create(*scope, cap, false, S)) return cs;
    EditWork TW;
    if (const int ws = edit_work_rows(T, TW, R.widest())) return ws;
    if (const int as = edit_adopt(w.st, R, S, TW, w.depth)) return as;
    hipLaunchKernelGGL(k_world_root, dim3(1), dim3(64), 0, w.st, S, R.d_map + R.root, S.next);
    GPU_TRY(hipGetLastError());
    return world_read_head(w, S, H);
}

// A compaction's end: the freshly adopted store becomes the world's.  Nothing
// of the world has changed before; the old store goes with `scope`, after a
// synchronise of the stream.
void world_install(och_world &w, std::unique_ptr<GpuScope> &scope, const GpuStore &S, const WorldHead &H)
{
    w.store_scope.swap(scope);
    w.S = S;
    w.used = H.used;
    w.now.root = H.root;
    w.now.root_mask = H.mask;
    w.head_stale = false;   // the new store's head holds the adopted root (k_world_root)
    ++w.generation;
}

int world_create(och_world &w, const uint32_t *nodes, uint32_t n_nodes, uint32_t root, uint32_t capacity)
{
    GPU_TRY(hipStreamCreateWithFlags(&w.st, hipStreamNonBlocking));
    PhaseTimer phase = world_phase(w);
    GpuScope T(w.st);
    EditReach R;
    if (const int us = edit_upload(T, R, nodes, n_nodes, root)) return us;
    if (const int rs = edit_reach(w.st, R, w.depth)) return rs;
    if (!phase("reach")) return OCH_E_HIP;
    const uint64_t cap = capacity ? capacity : 2 * R.reach + 64ull * (uint64_t)w.depth;
    if (cap < R.reach + 1) return OCH_E_CAPACITY;
    if (cap >= kWorldCapLimit) return och::report(OCH_E_INVALID, "och_world_create: a capacity of 2^29 - 1 ids or more");
    WorldHead H;
    if (const int as = world_adopt(w, T, R, (uint32_t)cap, w.store_scope, w.S, &H)) return as;
    if (!phase("adopt")) return OCH_E_HIP;
    w.used = H.used;
    w.now.root = H.root;
    w.now.root_mask = H.mask;
    w.now.box.any = och::occupied_box(nodes, n_nodes, root, w.depth, 1, w.now.box.lo, w.now.box.hi);
    phase("box");
    return OCH_OK;
}

int world_compact(och_world &w)
{
    PhaseTimer phase = world_phase(w);
    GpuScope T(w.st);
    EditReach R;
    if (w.now.root) {
        DevicePool dev;
        uint32_t n = 0;
        if (const int rs = renumber_gpu(w.S, w.used, w.now.root, w.depth, T, nullptr, &n, false, &dev)) return rs;
        // the renumbered pool's depths are id ranges: lv_cnt as the reach would give them, the ids as a list
        R.d_pool = const_cast<uint32_t *>(dev.nodes);
        R.n_nodes = n;
        R.root = 1;
        if (!T.alloc(&R.d_map, ((size_t)n + 1) * 4) || !T.alloc(&R.d_order, (size_t)n * 4)) return OCH_E_NOMEM;
        GPU_TRY(hipMemsetAsync(R.d_map, 0, 4, w.st));
        hipLaunchKernelGGL(k_world_iota, blocks(n), dim3(256), 0, w.st, R.d_order, n, 1u);
        GPU_TRY(hipGetLastError());
        uint32_t off = 0;
        for (size_t l = 0; l < dev.level_counts.size() && l < (size_t)w.depth && off < n; ++l) {
            R.lv_off[l] = off;
            R.lv_cnt[l] = std::min(dev.level_counts[l], n - off);
            off += R.lv_cnt[l];
        }
        R.reach = n;
        if (!phase("renumber")) return OCH_E_HIP;
    } else {
        if (!T.alloc(&R.d_map, 4)) return OCH_E_NOMEM;
        GPU_TRY(hipMemsetAsync(R.d_map, 0, 4, w.st));
    }
    std::unique_ptr<GpuScope> scope;
    GpuStore S;
    WorldHead H;
    if (const int as = world_adopt(w, T, R, w.S.cap, scope, S, &H)) return as;
    if (!phase("adopt")) return OCH_E_HIP;
    if (phase.on) std::fprintf(stderr, "[och_build] world: compacted %u ids to %u\n", w.used, H.used);
    world_install(w, scope, S, H);
    return OCH_OK;
}

int world_flush(och_world &w, och_gpu_pool *pool)
{
    och::WorldPoolView v;
    if (const int vs = och::pool_world_view(pool, w.id, &v)) return vs;
    if (v.n_nodes != w.S.cap) return och::report(OCH_E_INVALID, "och_world_flush: the pool was not made from this world");
    const bool whole = *v.generation != w.generation;
    // ids of another generation: launches in flight may walk the slots about to change
    if (whole && *v.published)
        if (const int ds = och::pool_drain(pool)) return ds;
    const uint32_t lo = whole ? 0u : *v.published, hi = w.used;
    PhaseTimer phase = world_phase(w);
    int st = OCH_OK;
    if (hi > lo) {
        if (hipMemcpyAsync(v.raw + (size_t)lo * 8, w.S.nodes + (size_t)lo * 8, (size_t)(hi - lo) * 32, hipMemcpyDeviceToDevice,
                           w.st) != hipSuccess)
            st = OCH_E_HIP;
        if (st == OCH_OK && v.packed) {
            hipLaunchKernelGGL(k_world_pack, blocks((size_t)(hi - lo) * 8), dim3(256), 0, w.st, w.S, lo, hi, v.packed);
            if (hipGetLastError() != hipSuccess) st = OCH_E_HIP;
        }
    }
    // complete on return: the launch that takes the new root starts after its nodes are there
    if (st == OCH_OK && hipStreamSynchronize(w.st) != hipSuccess) st = OCH_E_HIP;
    if (st == OCH_OK)
        st = och::pool_commit(pool, w.now.root, w.now.root ? w.now.root | w.now.root_mask << 24 : 0u, v.packed != nullptr, 0,
                              w.now.box.any ? w.now.box.lo : nullptr, w.now.box.any ? w.now.box.hi : nullptr);
    if (st != OCH_OK) {
        // below `published` nothing was written, so the pool still shows its last flush -- unless it was being rewritten
        if (whole && *v.published) (void)och::pool_mark_torn(pool);
        return st;
    }
    *v.published = hi;
    *v.generation = w.generation;
    phase("flush");
    return OCH_OK;
}

// och_world_history.h: the compaction of a world with live snapshots (what any of them reaches stays).
int world_compact_history(och_world &w);

int world_usable(const och_world *w, const char *who)
{
    if (!w) return och::report(OCH_E_INVALID, (std::string(who) + ": world is NULL").c_str());
    if (w->broken)
        return och::report(OCH_E_INVALID, (std::string(who) + ": the world is broken (an earlier call failed in HIP)").c_str());
    return OCH_OK;
}

constexpr bool kBreaks = true, kStays = false;       // what a HIP failure does to the world
constexpr bool kPoolTexts = true, kOwnTexts = false;

// An entry that works on the device, around its body: the usable check, the
// world's device current, then the body's status.  HIP, NOMEM and NODEV come
// back bare and get their text here, under `report_as`; every other failure
// was reported where it was found.  kBreaks: the entry writes the store, so a
// HIP failure leaves it unknown and the world refuses every later call; an
// entry that only reads, or builds beside the store, leaves the world usable.
// kPoolTexts (flush): only HIP is bare, the rest is the pool layer's, reported.
template <class Body>
int world_call(och_world *w, const char *entry, const char *report_as, bool breaks, bool pool_texts, Body body)
{
    if (const int us = world_usable(w, entry)) return us;
    och::DeviceGuard g(w->device);
    if (!g.ok) return report_build(OCH_E_HIP, "och_world", "");
    const int st = body();
    if (st == OCH_E_HIP && breaks) w->broken = true;
    const bool bare = st == OCH_E_HIP || (!pool_texts && (st == OCH_E_NOMEM || st == OCH_E_NODEV));
    return bare ? report_build(st, report_as, "allocation failed") : st;
}

}  // namespace

OCH_API int och_world_create(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, uint32_t capacity, int device,
                             och_world **out)
{
    if (!out) return och::report(OCH_E_INVALID, "och_world_create: out is NULL");
    *out = nullptr;
    if (depth < 1 || depth > kMaxVoxelDepth)
        return och::report(OCH_E_INVALID, "och_world_create: depth must be 1..21 (a Morton key of 3 * depth bits and the "
                                          "out-of-range bit fill 64 bits)");
    if (!nodes && n_nodes) return och::report(OCH_E_INVALID, "och_world_create: nodes is null");
    if (root > n_nodes) return och::report(OCH_E_INVALID, "och_world_create: root lies past the pool's end");
    int ndev = 0;
    if (!gpu_present() || hipGetDeviceCount(&ndev) != hipSuccess) return report_build(OCH_E_NODEV, "och_world", "");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return report_build(OCH_E_HIP, "och_world", "");
    if (device >= ndev) return report_build(OCH_E_NODEV, "och_world", "");
    och::DeviceGuard g(device);
    if (!g.ok) return report_build(OCH_E_HIP, "och_world", "");
    static std::atomic<uint64_t> next_id{1};
    och_world *w = new och_world;
    w->id = next_id.fetch_add(1);
    w->device = device;
    w->depth = depth;
    const int st = world_create(*w, nodes, n_nodes, root, capacity);
    if (st != OCH_OK) {
        delete w;
        return st == OCH_E_INVALID ? st : report_build(st, "och_world", "allocation failed");
    }
    *out = w;
    return OCH_OK;
}

OCH_API int och_world_destroy(och_world *w)
{
    if (!w) return OCH_OK;
    och::DeviceGuard g(w->device);
    delete w;
    return OCH_OK;
}

OCH_API int och_world_info(const och_world *w, och_world_stats *info)
{
    if (!info) return och::report(OCH_E_INVALID, "och_world_info: info is NULL");
    if (const int us = world_usable(w, "och_world_info")) return us;
    info->capacity = w->S.cap;
    info->used = w->used;
    info->root = w->now.root;
    info->depth = w->depth;
    info->device = w->device;
    info->strokes = w->strokes;
    info->generation = w->generation;
    std::memcpy(info->box_lo, w->now.box.lo, sizeof info->box_lo);   // all 0 without a voxel
    std::memcpy(info->box_hi, w->now.box.hi, sizeof info->box_hi);
    return OCH_OK;
}

OCH_API int och_world_edit(och_world *w, const void *records, uint64_t n, int on_device)
{
    if (n >= (1ull << 31)) return och::report(OCH_E_INVALID, "och_world_edit: a list holds fewer than 2^31 records");
    if (!records && n) return och::report(OCH_E_INVALID, "och_world_edit: records is null");
    if (!n) return world_usable(w, "och_world_edit");
    return world_call(w, "och_world_edit", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_edit(*w, records, (uint32_t)n, on_device != 0); });
}

OCH_API int och_world_pool_create(och_world *w, och_gpu_pool **out)
{
    if (!out) return och::report(OCH_E_INVALID, "och_world_pool_create: out is NULL");
    *out = nullptr;
    return world_call(w, "och_world_pool_create", "och_world", kStays, kPoolTexts, [&] {
        och_gpu_pool *pool = nullptr;
        if (const int cs = och::pool_create_for_world(w->device, w->depth, w->S.cap, w->id, &pool)) return cs;
        och::WorldPoolView v;
        int st = och::pool_world_view(pool, w->id, &v);
        if (st == OCH_OK) {
            *v.generation = w->generation;   // nothing published: the first flush writes ids [0, used)
            st = world_flush(*w, pool);
        }
        if (st == OCH_OK)
            *out = pool;
        else
            (void)och_gpu_pool_destroy(pool);
        return st;
    });
}

OCH_API int och_world_flush(och_world *w, och_gpu_pool *pool)
{
    return world_call(w, "och_world_flush", "och_world", kStays, kPoolTexts, [&] {
        if (!pool) return och::report(OCH_E_INVALID, "och_world_flush: pool is NULL");
        return world_flush(*w, pool);
    });
}

OCH_API int och_world_download(och_world *w, och_host_pool *out)
{
    if (!out) return och::report(OCH_E_INVALID, "och_world_download: out is NULL");
    return world_call(w, "och_world_download", "och_world", kStays, kOwnTexts, [&] {
        const auto t_start = std::chrono::steady_clock::now();
        PhaseTimer phase = world_phase(*w);
        BuildStats vs;
        uint32_t root = w->now.root, n_out = 0;
        uint32_t *nodes = nullptr;
        int st = OCH_OK;
        if (!root) {
            st = empty_pool(&nodes, &n_out, root);
        } else {
            GpuScope T(w->st);
            DevicePool dev;
            st = renumber_gpu(w->S, w->used, root, w->depth, T, &nodes, &n_out, phase.on, &dev);
            if (st == OCH_OK && (st = pool_stats_gpu(T, dev, n_out, w->depth, vs)) != OCH_OK) std::free(nodes);
        }
        if (st != OCH_OK) return st;
        phase("download");
        return finish_pool(out, nodes, n_out, root, 1, w->depth, vs, t_start);
    });
}

OCH_API int och_world_compact(och_world *w)
{
    // the old store is replaced only once the new one is whole: a failure leaves the world as it was
    return world_call(w, "och_world_compact", "och_world", kStays, kOwnTexts,
                      [&] { return w->snapshots.empty() ? world_compact(*w) : world_compact_history(*w); });
}
