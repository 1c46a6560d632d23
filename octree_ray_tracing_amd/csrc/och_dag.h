// och_dag.h -- what every builder of och_builder.cpp shares: the canonical DAG
// as a store of (level, 8 child words) -> node id, on the host (NodeStore) and
// on the GPU (GpuStore and the k_intern* / k_settle kernels), its breadth-first
// renumbering on either (renumber, renumber_gpu and the k_bfs_* kernels), and
// the small steps around a build: the scope that owns a GPU build's buffers
// and stream, the empty pool, the phase timer, the status texts and the fill
// of the caller's och_host_pool.
//
// A node belongs to exactly one level (the level is part of the key): the
// reference's table may share one slot between a leaf-level node and an
// interior node whose child indices happen to spell the same 8 words --
// harmless for tracing, impossible to renumber.
//
// Included by och_builder.cpp only (one translation unit, hence the unnamed
// namespace): the terrain builder there, the voxel builder (och_voxel_build.h)
// and, on top of that one, the batch editor (och_voxel_edit.h) are written on
// top of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "och_hash.h"
#include "och_internal.h"

namespace {

// Zeroed, lazily backed; transparent huge pages where the kernel allows them
// (the hash table and the leaf map are probed at random: fewer TLB misses).
template <class T>
T *map_zeroed(size_t count)
{
    void *p = mmap(nullptr, count * sizeof(T), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) return nullptr;
    (void)madvise(p, count * sizeof(T), MADV_HUGEPAGE);
    return static_cast<T *>(p);
}

template <class T>
void unmap(T *p, size_t count)
{
    if (p) munmap(p, count * sizeof(T));
}

void parallel_for(int threads, uint64_t n, const std::function<void(uint64_t, int)> &fn)
{
    std::atomic<uint64_t> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            for (;;) {
                const uint64_t i = next.fetch_add(1, std::memory_order_relaxed);
                if (i >= n) break;
                fn(i, t);
            }
        });
    for (auto &th : pool) th.join();
}

using och_hash::node_hash;

// Lock-free interning of (level, 8 child words) -> node id.  Ids are handed
// out by one atomic counter; a lost insert race leaves an unused id behind
// (dropped by the breadth-first renumbering).
struct NodeStore {
    uint32_t cap = 0;
    uint32_t *nodes = nullptr;             // cap x 8
    uint8_t *level = nullptr;              // height above the voxels of each id
    std::atomic<uint32_t> next{1};         // id 0 = empty
    std::atomic<uint32_t> *table = nullptr;
    uint64_t table_mask = 0;
    std::atomic<uint32_t> *leaf_ids = nullptr;   // direct map of 3-bit-per-voxel leaf codes
    std::atomic<bool> full{false};
    bool dedup = true;

    bool init(uint32_t capacity, bool dd)
    {
        cap = capacity;
        dedup = dd;
        nodes = map_zeroed<uint32_t>((size_t)cap * 8);
        level = map_zeroed<uint8_t>(cap);
        if (!nodes || !level) return false;
        if (dedup) {
            uint64_t ts = 1;
            while (ts < (uint64_t)cap * 2) ts <<= 1;
            table_mask = ts - 1;
            table = map_zeroed<std::atomic<uint32_t>>(ts);
            leaf_ids = map_zeroed<std::atomic<uint32_t>>(1u << 24);
            if (!table || !leaf_ids) return false;
        }
        return true;
    }
    void release()
    {
        unmap(nodes, (size_t)cap * 8);
        unmap(level, cap);
        unmap(table, table_mask + 1);
        unmap(leaf_ids, (size_t)1 << 24);
        nodes = nullptr;
        level = nullptr;
        table = nullptr;
        leaf_ids = nullptr;
    }

    uint32_t alloc(const uint32_t *c, int h)
    {
        const uint32_t id = next.fetch_add(1, std::memory_order_relaxed);
        if (id >= cap) {
            full.store(true, std::memory_order_relaxed);
            return 0;
        }
        std::memcpy(nodes + (size_t)id * 8, c, 32);
        level[id] = (uint8_t)h;
        return id;
    }

    // The leaf-level node c through the direct map, code = its 3 bits per child.
    uint32_t claim_leaf(uint32_t code, const uint32_t *c)
    {
        std::atomic<uint32_t> &slot = leaf_ids[code];
        uint32_t id = slot.load(std::memory_order_acquire);
        if (id) return id;
        const uint32_t mine = alloc(c, 0);
        if (!mine) return 0;
        if (slot.compare_exchange_strong(id, mine, std::memory_order_acq_rel)) return mine;
        return id;
    }

    // A leaf-level node given as its code (3 bits per child, child k at bits 3k).
    uint32_t intern_code(uint32_t code)
    {
        uint32_t c[8];
        for (int k = 0; k < 8; ++k) c[k] = (code >> (3 * k)) & 7u;
        return dedup ? claim_leaf(code, c) : alloc(c, 0);
    }

    uint32_t intern(const uint32_t *c, int h)
    {
        if (!dedup) return alloc(c, h);
        if (h == 0) {
            uint32_t code = 0;
            bool small = true;
            for (int k = 0; k < 8; ++k) {
                small &= c[k] < 8;
                code |= (c[k] & 7u) << (3 * k);
            }
            if (small) return claim_leaf(code, c);
        }
        uint64_t i = node_hash(c, h) & table_mask;
        uint32_t mine = 0;
        for (;;) {
            uint32_t id = table[i].load(std::memory_order_acquire);
            if (!id) {
                if (!mine) {
                    mine = alloc(c, h);
                    if (!mine) return 0;
                }
                if (table[i].compare_exchange_strong(id, mine, std::memory_order_acq_rel)) return mine;
            }
            if (level[id] == h && std::memcmp(nodes + (size_t)id * 8, c, 32) == 0) return id;
            i = (i + 1) & table_mask;
        }
    }
};

// Levels h0 .. h1 - 1 above a grid of ids of side n = 2^(h1 - h0), index
// (z * n + y) * n + x, in place: every level turns the 2x2x2 blocks of its grid
// into the nodes of a grid of half the side, down to the one node returned.
uint32_t reduce_grid(NodeStore &ns, int h0, int h1, std::vector<uint32_t> &ids, uint64_t &tree_nodes)
{
    int n = 1 << (h1 - h0);
    for (int h = h0; h < h1; ++h) {
        const int m = n / 2;
        // nodes of eight equal children (solid stone) repeat: the last one per
        // level skips the hash table (a DAG only; an expanded tree shares nothing)
        uint32_t last_child = 0, last_id = 0;
        for (int z = 0; z < m; ++z)
            for (int y = 0; y < m; ++y)
                for (int x = 0; x < m; ++x) {
                    uint32_t c[8];
                    bool any = false, same = true;
                    for (int k = 0; k < 8; ++k) {
                        const int cx = 2 * x + (k & 1), cy = 2 * y + ((k >> 1) & 1), cz = 2 * z + ((k >> 2) & 1);
                        c[k] = ids[((size_t)cz * n + cy) * n + cx];
                        any |= c[k] != 0;
                        same &= c[k] == c[0];
                    }
                    uint32_t id = 0;
                    if (any) {
                        if (same && ns.dedup && c[0] == last_child) {
                            id = last_id;
                        } else {
                            id = ns.intern(c, h);
                            if (same) last_child = c[0], last_id = id;
                        }
                        ++tree_nodes;
                    }
                    ids[((size_t)z * m + y) * m + x] = id;   // safe: writes trail reads
                }
        n = m;
    }
    return ids[0];
}

// An empty world: one zero node, root 0.  *out: malloc'd, as renumber().
int empty_pool(uint32_t **out, uint32_t *n_out, uint32_t &root)
{
    root = 0;
    *n_out = 1;
    *out = static_cast<uint32_t *>(std::calloc(8, 4));
    return *out ? OCH_OK : OCH_E_NOMEM;
}

// Breadth-first renumbering of a node store (ids 1 .. used - 1, records of 8
// child words, level[id] = height above the voxels): level by level from the
// root, children in slot order; 1-based (h_octree, slot 0 never used) or
// 0-based octree.  *out: malloc'd n_out x 8 words (one zero node when empty).
int renumber(const uint32_t *store, const uint8_t *level, uint32_t used, uint32_t root, int depth, int base,
             uint32_t **out, uint32_t *n_out)
{
    if (!root) return empty_pool(out, n_out, root);
    std::vector<uint32_t> newid(used, 0);
    std::vector<uint32_t> order;
    order.reserve(1024);
    std::vector<uint32_t> lv{root};
    newid[root] = (uint32_t)base;
    order.push_back(root);
    for (int l = 1; l < depth; ++l) {
        std::vector<uint32_t> nxt;
        for (uint32_t v : lv) {
            const uint32_t *c = store + (size_t)v * 8;
            for (int k = 0; k < 8; ++k)
                if (c[k] && !(newid[c[k]] || c[k] == root)) {
                    newid[c[k]] = (uint32_t)(order.size() + base);
                    order.push_back(c[k]);
                    nxt.push_back(c[k]);
                }
        }
        lv.swap(nxt);
    }
    *n_out = (uint32_t)order.size();
    uint32_t *nodes = static_cast<uint32_t *>(std::calloc((size_t)*n_out * 8, 4));
    if (!nodes) return OCH_E_NOMEM;
    for (size_t i = 0; i < order.size(); ++i) {
        const uint32_t v = order[i];
        const uint32_t *c = store + (size_t)v * 8;
        const bool leaf = level[v] == 0;
        for (int k = 0; k < 8; ++k) nodes[i * 8 + k] = (leaf || !c[k]) ? c[k] : newid[c[k]];
    }
    *out = nodes;
    return OCH_OK;
}

// ------------------------------------------------------------ around a build

// What a build counts besides its pool (och_host_pool's statistics).
struct BuildStats {
    uint64_t hist[8] = {0};   // voxels per id 0..7
    uint64_t tree_nodes = 0;  // nodes of the expanded tree
    uint64_t solid = 0;       // voxels of any id but 0
};

// OCH_BUILD_TRACE=1: phase times on stderr, "[och_build] <prefix><phase> <seconds> s",
// each since the line before.  With a stream a phase ends in a synchronise of
// it (tracing only); false when that fails.
struct PhaseTimer {
    const char *prefix;
    int digits;
    hipStream_t sync = nullptr;
    bool on = std::getenv("OCH_BUILD_TRACE") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();

    bool operator()(const char *name)
    {
        if (!on) return true;
        if (sync && hipStreamSynchronize(sync) != hipSuccess) return false;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[och_build] %s%-10s %8.*f s\n", prefix, name, digits,
                     std::chrono::duration<double>(now - last).count());
        last = now;
        return true;
    }
};

// A failed build's status with its text: `who` names the builder, `nomem` what it could not allocate.
int report_build(int status, const char *who, const char *nomem)
{
    if (status == OCH_E_NODEV) return och::report(status, "use_gpu: no HIP device");
    const std::string what = status == OCH_E_CAPACITY ? "node capacity exhausted" : status == OCH_E_NOMEM ? nomem : "HIP error";
    return och::report(status, (std::string(who) + ": " + what).c_str());
}

// The renumbered pool and the build's statistics into the caller's och_host_pool.
int finish_pool(och_host_pool *out, uint32_t *nodes, uint32_t n_out, uint32_t root, int base, int depth,
                const BuildStats &stats, std::chrono::steady_clock::time_point t_start)
{
    out->nodes = nodes;
    out->n_nodes = n_out;
    out->root = root ? (uint32_t)base : 0;
    out->depth = depth;
    out->index_base = base;
    out->tree_nodes = stats.tree_nodes;
    for (int k = 0; k < 8; ++k) out->voxel_hist[k] = stats.hist[k];
    out->solid_voxels = stats.solid;
    out->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return OCH_OK;
}

// ------------------------------------------------------------ a GPU build's scope

#define GPU_TRY(expr)                               \
    do {                                            \
        if ((expr) != hipSuccess) return OCH_E_HIP; \
    } while (0)

// A HIP device to build on.  Clears the thread's pending HIP error: a stale
// error of an earlier HIP call (another library's) is not this build's.
bool gpu_present()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return false;
    (void)hipGetLastError();
    return true;
}

// The device buffers and the one stream of a GPU build on the current device:
// when the scope ends the stream is synchronised and destroyed and the buffers
// are freed, whatever the build returned.  A scope that borrows its stream (a
// world's, och_world.h) synchronises it and leaves it to its owner.
struct GpuScope {
    hipStream_t st = nullptr;
    bool own_stream = true;
    std::vector<void *> bufs;

    GpuScope() = default;
    GpuScope(const GpuScope &) = delete;
    GpuScope &operator=(const GpuScope &) = delete;
    ~GpuScope()
    {
        if (st) {
            (void)hipStreamSynchronize(st);
            if (own_stream) (void)hipStreamDestroy(st);
        }
        for (void *p : bufs) (void)hipFree(p);
    }
    explicit GpuScope(hipStream_t borrowed) : st(borrowed), own_stream(false) {}
    int open()
    {
        if (!gpu_present()) return OCH_E_NODEV;
        GPU_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return OCH_OK;
    }
    // At least 4 bytes, so that an empty input still names a buffer.
    template <class T>
    bool alloc(T **p, size_t bytes)
    {
        if (hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(bytes, 4)) != hipSuccess) return false;
        bufs.push_back(*p);
        return true;
    }
};

dim3 blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// ------------------------------------------------------------ GPU hash-consing
//
// A DAG build (dedup) with use_gpu interns on the GPU as well; the host only
// renumbers.  Leaf-level nodes are interned by their 24-bit code through a
// direct map (k_intern_codes).  Every level above is one pair of dispatches
// over all its nodes:
//   k_intern -- each node gathers its eight child ids (written by an earlier
//               dispatch); empty nodes stop there.  The rest probe one open-
//               addressing table shared by all levels.  An empty slot is
//               claimed by compare-and-swap with the node's own index (kCand |
//               index) and the claimant allocates the node's id and writes its
//               record.  A node meeting a claimed slot compares its children
//               with the claimant's, gathered again from the same earlier
//               dispatch's ids; a slot holding a finished id is compared with
//               that node's record, written by an earlier dispatch.
//   k_settle -- each node takes its id (its own or its claimant's) and each
//               claimant turns its slot into the finished id.
// No dispatch reads what another workgroup writes in the same dispatch except
// through the atomics, so the per-XCD L2s need no coherence beyond dispatch
// boundaries.  Ids come from one counter in claim order and differ from run to
// run; the breadth-first renumbering makes the pool identical to the host
// build's, slot for slot.

constexpr uint32_t kCand = 0x80000000u;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct GpuStore {
    uint32_t *nodes;                 // cap x 8 child words
    uint8_t *level;                  // height above the voxels of each id
    uint32_t *next;                  // id counter, starts at 1 (0 = empty)
    uint32_t *table;                 // tmask + 1 slots: 0, kCand | node index (this level), or an id
    uint32_t *leaf_id;               // 2^24 leaf codes -> id
    uint32_t *overflow;              // 1: capacity exhausted, 2: table exhausted, 4: a row outside its level (k_vox_rows, k_edit_rows)
    unsigned long long *tree_nodes;  // kCounters partial counts of expanded-tree nodes, 128 B apart
    uint32_t cap, tmask;
};

// One level: nb grids of side n (node index = grid * n^3 + (z * n + y) * n + x),
// children in the previous level's grids of side 2n; or (rows = 1, the voxel
// builder) a list of count rows, node index i's eight child words at src[8 i].
struct GpuLevel {
    const uint32_t *src;   // child ids, or leaf codes (codes = 1: the child id is leaf_id[code])
    int codes;
    int log2n;
    uint32_t count;        // nb * n^3, or the rows
    int h;
    int rows = 0;
};

constexpr int kCounters = 64;

// Block-wide count, then one atomic per block on one of kCounters addresses.
__device__ inline void count_nodes(const GpuStore &S, bool nz)
{
    __shared__ uint32_t block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    const uint64_t b = __ballot(nz);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&block_count, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && block_count)
        atomicAdd(S.tree_nodes + 16 * (blockIdx.x % kCounters), (unsigned long long)block_count);
}

__device__ inline uint32_t alloc_node(const GpuStore &S, const uint32_t c[8], int h)
{
    const uint32_t id = atomicAdd(S.next, 1u);
    if (id >= S.cap) {
        atomicOr(S.overflow, 1u);
        return 0;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(S.nodes + (size_t)id * 8);
    dst[0] = make_uint4(c[0], c[1], c[2], c[3]);
    dst[1] = make_uint4(c[4], c[5], c[6], c[7]);
    S.level[id] = (uint8_t)h;
    return id;
}

__device__ inline bool gather(const GpuStore &S, const GpuLevel &L, uint32_t idx, uint32_t c[8])
{
    if (L.rows) {   // child words as they are: a leaf-level row holds voxel ids, all 32 bits
        const uint4 *row = reinterpret_cast<const uint4 *>(L.src + (size_t)idx * 8);
        const uint4 a = row[0], b = row[1];
        c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
        return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0;
    }
    const uint32_t n = 1u << L.log2n, m = 2u * n;
    const uint32_t g = idx >> (3 * L.log2n), r = idx & ((1u << (3 * L.log2n)) - 1u);
    const uint32_t x = r & (n - 1u), y = (r >> L.log2n) & (n - 1u), z = r >> (2 * L.log2n);
    const size_t base = (size_t)g * m * m * m;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t cx = 2u * x + (k & 1), cy = 2u * y + ((k >> 1) & 1), cz = 2u * z + ((k >> 2) & 1);
        uint32_t v = L.src[base + ((size_t)cz * m + cy) * m + cx];
        if (L.codes && v) v = S.leaf_id[v];
        c[k] = v;
        any |= v != 0;
    }
    return any;
}

__global__ __launch_bounds__(256) void k_intern_codes(GpuStore S, const uint32_t *__restrict__ codes, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t code = i < count ? codes[i] : 0u;   // counted by k_brick_codes (info[7])
    if (!code) return;
    // A plain (cached) load: a stale 0 only sends the thread to the CAS, which
    // sees the truth; most codes were interned by an earlier batch.
    if (S.leaf_id[code] != 0 || atomicCAS(&S.leaf_id[code], 0u, kCand) != 0u) return;
    uint32_t c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = (code >> (3 * k)) & 7u;
    __hip_atomic_store(&S.leaf_id[code], alloc_node(S, c, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Probe the table for node idx of level L (children c, not all empty): the
// node's rep value.  The claimant of an empty slot allocates the id and
// returns it (slot[idx] = its slot); everyone else returns what the slot of an
// equal node holds, kCand | the claimant's index or a finished id.  Only table
// values carry the kCand flag: child words are compared, never tested for it.
__device__ inline uint32_t probe_node(const GpuStore &S, const GpuLevel &L, uint32_t idx, const uint32_t c[8],
                                      uint32_t *__restrict__ slot)
{
    uint32_t i = (uint32_t)node_hash(c, L.h) & S.tmask;
    for (uint32_t probe = 0; probe <= S.tmask; ++probe, i = (i + 1u) & S.tmask) {
        uint32_t v = S.table[i];   // a stale 0 is corrected by the CAS; claims and ids are never stale
        if (v == 0) {
            v = atomicCAS(&S.table[i], 0u, kCand | idx);
            if (v == 0) {
                slot[idx] = i;
                return alloc_node(S, c, L.h);
            }
        }
        bool same = true;
        if (v & kCand) {
            uint32_t d[8];
            gather(S, L, v & ~kCand, d);
#pragma unroll
            for (int k = 0; k < 8; ++k) same &= d[k] == c[k];
        } else {
            const uint4 *rec = reinterpret_cast<const uint4 *>(S.nodes + (size_t)v * 8);
            const uint4 a = rec[0], b = rec[1];
            same = S.level[v] == (uint8_t)L.h && a.x == c[0] && a.y == c[1] && a.z == c[2] && a.w == c[3] &&
                   b.x == c[4] && b.y == c[5] && b.z == c[6] && b.w == c[7];
        }
        if (same) return v;
    }
    atomicOr(S.overflow, 2u);
    return 0;
}

__global__ __launch_bounds__(256) void k_intern(GpuStore S, GpuLevel L, uint32_t *__restrict__ rep,
                                                uint32_t *__restrict__ slot)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c[8];
    const bool any = idx < L.count && gather(S, L, idx, c);
    count_nodes(S, any);
    if (idx >= L.count) return;
    slot[idx] = kNoSlot;
    rep[idx] = any ? probe_node(S, L, idx, c, slot) : 0u;
}

// The voxel builder's rows (GpuLevel.rows; none is empty).  A solid region is
// millions of equal rows in a row, all bound for one table slot: the lanes of
// a wavefront whose row equals its first lane's leave the probe to that lane
// and take its rep value through the registers, so one slot sees a wavefront's
// worth fewer compare-and-swaps while the claim is still invisible to others.
// kEmptyRows (the voxel editor's rows): a row of zeros is no node, its rep
// value is 0 and it never probes or claims a table slot.
template <bool kEmptyRows>
__global__ __launch_bounds__(256) void k_intern_rows(GpuStore S, GpuLevel L, uint32_t *__restrict__ rep,
                                                     uint32_t *__restrict__ slot)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < L.count;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool any = live && gather(S, L, idx, c);
    // lane 0 of a wavefront is live whenever any of its lanes is (idx ascends)
    bool follows = live && (threadIdx.x & 63u) != 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) follows &= __shfl(c[k], 0) == c[k];
    uint32_t r = 0;
    if (live) slot[idx] = kNoSlot;
    if (live && !follows && (!kEmptyRows || any)) r = probe_node(S, L, idx, c, slot);
    const uint32_t lead = __shfl(r, 0);   // an id or kCand | index (or 0), all final for an equal row
    if (live) rep[idx] = follows ? lead : r;
}

// dst[dst_index ? dst_index[idx] : idx] = the node's id.
__global__ __launch_bounds__(256) void k_settle(GpuStore S, uint32_t count, const uint32_t *__restrict__ rep,
                                                const uint32_t *__restrict__ slot, uint32_t *__restrict__ dst,
                                                const uint32_t *__restrict__ dst_index)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count) return;
    uint32_t r = rep[idx];
    if (r & kCand) r = rep[r & ~kCand];
    dst[dst_index ? dst_index[idx] : idx] = r;
    const uint32_t s = slot[idx];
    if (s != kNoSlot) S.table[s] = r;
}

// A store of cap ids in scope G, cleared and with id 0 the zero node: the
// table is the next power of two at or above 2 cap, the tree-node counters
// are always there, the leaf-code map only for a builder that interns codes.
int gpu_store_create(GpuScope &G, uint32_t cap, bool leaf_map, GpuStore &S)
{
    uint64_t tsize = 1;
    while (tsize < 2 * (uint64_t)cap) tsize <<= 1;
    const size_t head_bytes = 256 + 128 * kCounters, leaf_bytes = (size_t)4 << 24;
    S = GpuStore{};
    S.cap = cap;
    S.tmask = (uint32_t)(tsize - 1);
    if (!G.alloc(&S.nodes, (size_t)cap * 32) || !G.alloc(&S.level, cap) || !G.alloc(&S.next, head_bytes) ||
        !G.alloc(&S.table, (size_t)tsize * 4) || (leaf_map && !G.alloc(&S.leaf_id, leaf_bytes)))
        return OCH_E_NOMEM;
    S.overflow = S.next + 1;
    S.tree_nodes = reinterpret_cast<unsigned long long *>(S.next + 64);
    static const uint32_t one = 1;
    GPU_TRY(hipMemsetAsync(S.next, 0, head_bytes, G.st));
    GPU_TRY(hipMemcpyAsync(S.next, &one, 4, hipMemcpyHostToDevice, G.st));
    GPU_TRY(hipMemsetAsync(S.table, 0, (size_t)tsize * 4, G.st));
    if (leaf_map) GPU_TRY(hipMemsetAsync(S.leaf_id, 0, leaf_bytes, G.st));
    GPU_TRY(hipMemsetAsync(S.nodes, 0, 32, G.st));
    return OCH_OK;
}

// After the last dispatch on the store: synchronises st (the caller's own
// read-backs queued before this call are complete with it) and gives the ids
// in use, or the status of what the overflow word recorded.
int gpu_store_used(const GpuStore &S, hipStream_t st, uint32_t *used)
{
    uint32_t head[2] = {0, 0};
    GPU_TRY(hipMemcpyAsync(head, S.next, 8, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipStreamSynchronize(st));
    if (head[1] & 4u) return och::report(OCH_E_HIP, "GPU voxel builder: a row outside its level");
    if (head[1]) return OCH_E_CAPACITY;
    *used = std::min(head[0], S.cap);
    return OCH_OK;
}

// Breadth-first renumbering on the device, one BFS level at a time (ids of
// one height are reachable at one depth only: the height is part of every
// node's key).  The frontier is order[off, off + f), in BFS order; its
// children, in (parent, slot) order, are the candidates q = 8 i + k, and a
// child's first candidate (k_bfs_first, atomicMin) places it (k_bfs_place,
// after an exclusive scan of k_bfs_mark's flags) -- the host renumbering's
// first-occurrence order.
__global__ __launch_bounds__(256) void k_bfs_first(const uint32_t *__restrict__ store, const uint32_t *__restrict__ front,
                                                   uint32_t f, uint32_t *__restrict__ first)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 8u * f) return;
    const uint32_t c = store[(size_t)front[q >> 3] * 8 + (q & 7u)];
    // first[] only decreases: a cached value at or below q (stale ones are
    // only larger) makes the atomic unnecessary -- shared children (solid
    // stone) are named by millions of slots, and one address's atomics serialise
    if (c && q < first[c]) atomicMin(&first[c], q);
}

__global__ __launch_bounds__(256) void k_bfs_mark(const uint32_t *__restrict__ store, const uint32_t *__restrict__ front,
                                                  uint32_t f, const uint32_t *__restrict__ first, uint32_t *__restrict__ mark)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 8u * f) return;
    const uint32_t c = store[(size_t)front[q >> 3] * 8 + (q & 7u)];
    mark[q] = (c && first[c] == q) ? 1u : 0u;
}

// order[next + pos[q]] = child, newid[child] = base + next + pos[q]
__global__ __launch_bounds__(256) void k_bfs_place(const uint32_t *__restrict__ store, const uint32_t *__restrict__ front,
                                                   uint32_t f, const uint32_t *__restrict__ mark,
                                                   const uint32_t *__restrict__ pos, uint32_t *__restrict__ order,
                                                   uint32_t next, uint32_t *__restrict__ newid, uint32_t base)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 8u * f || !mark[q]) return;
    const uint32_t c = store[(size_t)front[q >> 3] * 8 + (q & 7u)];
    order[next + pos[q]] = c;
    newid[c] = base + next + pos[q];
}

__global__ __launch_bounds__(256) void k_bfs_output(const uint32_t *__restrict__ store, const uint8_t *__restrict__ level,
                                                    const uint32_t *__restrict__ order, const uint32_t *__restrict__ newid,
                                                    uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 8u * n) return;
    const uint32_t v = order[q >> 3];
    const uint32_t c = store[(size_t)v * 8 + (q & 7u)];
    out[q] = (level[v] == 0 || !c) ? c : newid[c];
}

// The renumbered pool where renumber_gpu left it on the device (the scope's
// memory), for a caller that goes on there: ids lo .. lo + level_counts[l] - 1
// are the nodes at depth l, lo = 1 + the counts before it.
struct DevicePool {
    const uint32_t *nodes = nullptr;   // n_out x 8
    std::vector<uint32_t> level_counts;
};

// The store's nodes reachable from root (!= 0), renumbered breadth-first and
// 1-based on the device (k_bfs_*), with buffers of the build's scope.
// *out: malloc'd n_out x 8 words, as renumber(); out = null leaves the pool on
// the device only (dev).
int renumber_gpu(const GpuStore &S, uint32_t used, uint32_t root, int depth, GpuScope &G, uint32_t **out, uint32_t *n_out,
                 bool trace, DevicePool *dev = nullptr)
{
    const auto t_bfs = std::chrono::steady_clock::now();
    const hipStream_t st = G.st;
    // first / newid / order over the ids, mark / pos over one level's candidates
    uint32_t *d_first, *d_newid, *d_order, *d_mark, *d_pos, *d_out;
    const size_t max_cand = (size_t)used * 8;
    if (!G.alloc(&d_first, (size_t)used * 4) || !G.alloc(&d_newid, (size_t)used * 4) ||
        !G.alloc(&d_order, (size_t)used * 4) || !G.alloc(&d_mark, max_cand * 4) || !G.alloc(&d_pos, max_cand * 4) ||
        !G.alloc(&d_out, max_cand * 4))
        return OCH_E_NOMEM;
    size_t scan_bytes = 0;
    GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_mark, d_pos, (int)max_cand, st));
    void *d_scan = nullptr;
    if (!G.alloc(&d_scan, scan_bytes)) return OCH_E_NOMEM;
    const uint32_t base = 1;
    GPU_TRY(hipMemsetAsync(d_first, 0xFF, (size_t)used * 4, st));
    GPU_TRY(hipMemcpyAsync(d_order, &root, 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(d_newid + root, &base, 4, hipMemcpyHostToDevice, st));
    uint32_t off = 0, f = 1;
    for (int l = 1; l < depth && f; ++l) {
        const uint32_t nc = 8 * f, next = off + f;
        if (dev) dev->level_counts.push_back(f);
        hipLaunchKernelGGL(k_bfs_first, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_first);
        hipLaunchKernelGGL(k_bfs_mark, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_first, d_mark);
        GPU_TRY(hipGetLastError());
        GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_mark, d_pos, (int)nc, st));
        hipLaunchKernelGGL(k_bfs_place, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_mark, d_pos, d_order,
                           next, d_newid, base);
        GPU_TRY(hipGetLastError());
        uint32_t tail[2];
        GPU_TRY(hipMemcpyAsync(&tail[0], d_pos + nc - 1, 4, hipMemcpyDeviceToHost, st));
        GPU_TRY(hipMemcpyAsync(&tail[1], d_mark + nc - 1, 4, hipMemcpyDeviceToHost, st));
        GPU_TRY(hipStreamSynchronize(st));
        off = next;
        f = tail[0] + tail[1];
    }
    const uint32_t n = off + f;
    if (dev) {
        dev->level_counts.push_back(f);
        dev->nodes = d_out;
    }
    hipLaunchKernelGGL(k_bfs_output, blocks((size_t)n * 8), dim3(256), 0, st, S.nodes, S.level, d_order, d_newid, n, d_out);
    GPU_TRY(hipGetLastError());
    *n_out = n;
    if (!out) return OCH_OK;
    uint32_t *nodes = static_cast<uint32_t *>(std::malloc((size_t)n * 32));
    if (!nodes) return OCH_E_NOMEM;
    if (hipMemcpyAsync(nodes, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        std::free(nodes);
        return OCH_E_HIP;
    }
    *out = nodes;
    if (trace)
        std::fprintf(stderr, "[och_build] gpu renumbering %.3f s\n",
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bfs).count());
    return OCH_OK;
}

}  // namespace
