// och_builder.cpp -- parallel bottom-up builder of the demo terrain DAG.
//
// The reference builds its tree by recursive create_volume + per-voxel
// h_octree::set edits (ORT/test_och_h_octree.cpp:651-695, :767-787;
// ORT/och_h_octree.h:110-237): single-threaded, ~100 s at depth 10.  Because
// the final content is a pure per-voxel function (och_terrain.h), the same
// canonical DAG (identical subtrees shared, empty subtrees 0) is built here
// brick by brick on all host threads: each 32^3 brick is voxelised, reduced
// bottom-up and hash-consed into one lock-free table; the levels above the
// bricks follow; finally the pool is renumbered breadth-first so the top of
// the DAG is contiguous at the front of the pool.
//
// Unlike the reference's table, a node belongs to exactly one level here
// (the level is part of the key): the reference may share one slot between a
// leaf-level node and an interior node whose child indices happen to spell
// the same 8 words -- harmless for tracing, impossible to renumber.
//
// use_gpu: the voxel function -- simplex noise for every voxel below the
// surface, 2 * 10^10 evaluations at depth 12 -- runs on the GPU instead
// (k_brick_codes): one workgroup per 32^3 brick writes the brick's 4096
// leaf-level nodes as 24-bit codes (3 bits per child voxel), its voxel
// histogram and whether all its leaves are equal.  A DAG is then hash-consed
// on the GPU too (build_dag_gpu, below) and only renumbered on the host; an
// expanded tree's nodes are allocated by host threads from the codes, batch
// after batch, while the GPU computes the next batch.  Same pool either way.
//
// och_build_voxels ("voxel builder", below) builds the same canonical DAG from
// a caller's voxels -- a record list or a dense grid -- through Morton keys and
// a sort, with the same table, kernels and renumbering.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "och_internal.h"
#include "och_terrain.h"

namespace {

using och_terrain::Tables;

const Tables kTables = {OCH_PERM_TABLE, OCH_GRAD_TABLE};

int default_threads()
{
    if (const char *e = std::getenv("OMP_NUM_THREADS")) {
        const int v = std::atoi(e);
        if (v > 0) return std::min(v, 256);
    }
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) return std::max(1, std::min(CPU_COUNT(&set), 256));
    return std::max(1u, std::min(std::thread::hardware_concurrency(), 256u));
}

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

__host__ __device__ inline uint64_t mix64(uint64_t h)
{
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

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

    // A leaf-level node given as its code (3 bits per child, child k at bits 3k).
    uint32_t intern_code(uint32_t code)
    {
        uint32_t c[8];
        for (int k = 0; k < 8; ++k) c[k] = (code >> (3 * k)) & 7u;
        if (!dedup) return alloc(c, 0);
        std::atomic<uint32_t> &slot = leaf_ids[code];
        uint32_t id = slot.load(std::memory_order_acquire);
        if (id) return id;
        const uint32_t mine = alloc(c, 0);
        if (!mine) return 0;
        if (slot.compare_exchange_strong(id, mine, std::memory_order_acq_rel)) return mine;
        return id;
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
            if (small) {
                std::atomic<uint32_t> &slot = leaf_ids[code];
                uint32_t id = slot.load(std::memory_order_acquire);
                if (id) return id;
                const uint32_t mine = alloc(c, h);
                if (!mine) return 0;
                if (slot.compare_exchange_strong(id, mine, std::memory_order_acq_rel)) return mine;
                return id;
            }
        }
        uint64_t w[4];
        std::memcpy(w, c, 32);
        uint64_t hs = mix64((uint64_t)h * 0x9E3779B97F4A7C15ull ^ w[0]);
        hs = mix64(hs ^ w[1]);
        hs = mix64(hs ^ w[2]);
        hs = mix64(hs ^ w[3]);
        uint64_t i = hs & table_mask;
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

struct Terrain {
    int depth = 0, dim = 0;
    bool tunnels = true;
    std::vector<int32_t> heights;
    std::vector<uint8_t> tops;
    std::vector<int32_t> brick_hmax;   // max column height per brick column
};

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

struct BrickStats {
    uint64_t hist[8] = {0};
    uint64_t tree_nodes = 0;
};

// Reduce a brick's leaf-level ids (n^3, n = S/2, (z*n+y)*n+x) to its subtree
// root: levels h = 1 .. s_log2 - 1, in place.
uint32_t reduce_brick(NodeStore &ns, int s_log2, std::vector<uint32_t> &ids, BrickStats &st)
{
    int n = (1 << s_log2) / 2;
    for (int h = 1; h < s_log2; ++h) {
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
                        ++st.tree_nodes;
                    }
                    ids[((size_t)z * m + y) * m + x] = id;   // safe: writes trail reads
                }
        n = m;
    }
    return ids[0];
}

// Voxelise one brick of side S at (bx, by, bz) (brick units) and reduce it to
// its subtree root.  vox: S^3 scratch, ids: (S/2)^3 scratch.
uint32_t build_brick(const Terrain &tr, NodeStore &ns, int s_log2, int bx, int by, int bz, std::vector<uint8_t> &vox,
                     std::vector<uint32_t> &ids, BrickStats &st)
{
    const int S = 1 << s_log2;
    const int x0 = bx * S, y0 = by * S, z0 = bz * S;
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            const size_t col = (size_t)(y0 + y) * tr.dim + (x0 + x);
            const int h = tr.heights[col], top = tr.tops[col];
            uint8_t *v = &vox[((size_t)y * S + x) * S];   // z fastest
            for (int z = 0; z < S; ++z) {
                const uint32_t val = och_terrain::voxel_value(kTables, x0 + x, y0 + y, z0 + z, h, top, tr.tunnels);
                v[z] = (uint8_t)val;
                st.hist[val & 7]++;
            }
        }
    // h = 0: children are voxels, child index c = x | y << 1 | z << 2
    const int n = S / 2;
    for (int z = 0; z < n; ++z)
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                uint32_t c[8];
                bool any = false;
                for (int k = 0; k < 8; ++k) {
                    const int vx = 2 * x + (k & 1), vy = 2 * y + ((k >> 1) & 1), vz = 2 * z + ((k >> 2) & 1);
                    c[k] = vox[((size_t)vy * S + vx) * S + vz];
                    any |= c[k] != 0;
                }
                uint32_t id = 0;
                if (any) {
                    id = ns.intern(c, 0);
                    ++st.tree_nodes;
                }
                ids[((size_t)z * n + y) * n + x] = id;
            }
    return reduce_brick(ns, s_log2, ids, st);
}

// ------------------------------------------------------------ GPU voxelisation

constexpr int kBrickLog2 = 5, kBrick = 32, kLeaves = 4096;   // 32^3 voxels, 16^3 leaf-level nodes
constexpr uint32_t kMixed = 0xFFFFFFFFu;

__constant__ och_terrain::Tables c_tables = {OCH_PERM_TABLE, OCH_GRAD_TABLE};

// One workgroup per brick (bricks[i] = bx | by << 10 | bz << 20): the 4096
// leaf codes, (z * 16 + y) * 16 + x order; info[i] = {the common code when
// every leaf is equal, else kMixed; voxel counts of ids 0..5; non-empty leaf codes}.
__global__ __launch_bounds__(256) void k_brick_codes(const int32_t *__restrict__ heights, const uint8_t *__restrict__ tops,
                                                     int dim, int tunnels, const uint32_t *__restrict__ bricks,
                                                     uint32_t *__restrict__ codes, uint32_t *__restrict__ info)
{
    __shared__ och_terrain::Tables T;
    __shared__ uint32_t hist[8], firsts[256];
    __shared__ uint32_t leaves;   // non-empty leaf-level nodes of the brick
    __shared__ int mixed;
    for (int i = threadIdx.x; i < (int)sizeof(T); i += blockDim.x)
        reinterpret_cast<uint8_t *>(&T)[i] = reinterpret_cast<const uint8_t *>(&c_tables)[i];
    if (threadIdx.x < 8) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) mixed = 0, leaves = 0;
    __syncthreads();
    const uint32_t b = bricks[blockIdx.x];
    const int x0 = (int)(b & 1023u) * kBrick, y0 = (int)((b >> 10) & 1023u) * kBrick, z0 = (int)(b >> 20) * kBrick;
    uint32_t cnt[5] = {0, 0, 0, 0, 0}, other = 0;
    uint32_t first = 0, nonempty = 0;
    bool same = true;
    for (int leaf = threadIdx.x; leaf < kLeaves; leaf += blockDim.x) {
        const int lx = leaf & 15, ly = (leaf >> 4) & 15, lz = leaf >> 8;
        uint32_t code = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int x = x0 + 2 * lx + (k & 1), y = y0 + 2 * ly + ((k >> 1) & 1), z = z0 + 2 * lz + ((k >> 2) & 1);
            const size_t col = (size_t)y * dim + x;
            const uint32_t v = och_terrain::voxel_value(T, x, y, z, heights[col], tops[col], tunnels != 0);
            code |= (v & 7u) << (3 * k);
            if (v < 5) ++cnt[v];
            else ++other;
        }
        codes[(size_t)blockIdx.x * kLeaves + leaf] = code;
        nonempty += code != 0;
        if (leaf == (int)threadIdx.x) first = code;
        same &= code == first;
    }
    for (int v = 0; v < 5; ++v)
        if (cnt[v]) atomicAdd(&hist[v], cnt[v]);
    if (other) atomicAdd(&hist[5], other);        // ids above 4 do not occur in this terrain
    if (nonempty) atomicAdd(&leaves, nonempty);
    firsts[threadIdx.x] = first;
    if (!same) mixed = 1;
    __syncthreads();
    if (firsts[threadIdx.x] != firsts[0]) mixed = 1;
    __syncthreads();
    if (threadIdx.x == 0) info[(size_t)blockIdx.x * 8] = mixed ? kMixed : firsts[0];
    if (threadIdx.x < 6) info[(size_t)blockIdx.x * 8 + 1 + threadIdx.x] = hist[threadIdx.x];
    if (threadIdx.x == 6) info[(size_t)blockIdx.x * 8 + 7] = leaves;
}

#define BUILD_HIP(expr)                       \
    do {                                      \
        if ((expr) != hipSuccess) return false; \
    } while (0)

// Voxelise `work` on the current GPU in batches and hash-cons the codes on
// `threads` host threads, overlapping batch k + 1 on the GPU with batch k on
// the host.  Returns false when no GPU could run the voxel kernel; the caller
// then fails the build with OCH_E_NODEV (no host fallback).
bool build_bricks_gpu(const Terrain &tr, NodeStore &ns, int threads, const std::vector<uint32_t> &work, int G,
                      std::vector<uint32_t> &brick_root, std::vector<BrickStats> &stats, double *gpu_seconds)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return false;
    (void)hipGetLastError();        // a stale error of an earlier HIP call (another library's) is not this build's
    const size_t n_work = work.size();
    const size_t B = 4096;                        // bricks per batch: 64 MiB of codes
    int32_t *d_heights = nullptr;
    uint8_t *d_tops = nullptr;
    uint32_t *d_bricks[2] = {nullptr, nullptr}, *d_codes[2] = {nullptr, nullptr}, *d_info[2] = {nullptr, nullptr};
    uint32_t *h_codes[2] = {nullptr, nullptr}, *h_info[2] = {nullptr, nullptr}, *h_bricks[2] = {nullptr, nullptr};
    hipStream_t st[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    auto cleanup = [&] {
        for (int k = 0; k < 2; ++k) {
            if (st[k]) (void)hipStreamSynchronize(st[k]);
            if (d_bricks[k]) (void)hipFree(d_bricks[k]);
            if (d_codes[k]) (void)hipFree(d_codes[k]);
            if (d_info[k]) (void)hipFree(d_info[k]);
            if (h_codes[k]) (void)hipHostFree(h_codes[k]);
            if (h_info[k]) (void)hipHostFree(h_info[k]);
            if (h_bricks[k]) (void)hipHostFree(h_bricks[k]);
            if (done[k]) (void)hipEventDestroy(done[k]);
            if (st[k]) (void)hipStreamDestroy(st[k]);
        }
        if (d_heights) (void)hipFree(d_heights);
        if (d_tops) (void)hipFree(d_tops);
    };
    auto run = [&]() -> bool {
        const size_t cols = (size_t)tr.dim * tr.dim;
        BUILD_HIP(hipMalloc(&d_heights, cols * 4));
        BUILD_HIP(hipMalloc(&d_tops, cols));
        BUILD_HIP(hipMemcpy(d_heights, tr.heights.data(), cols * 4, hipMemcpyHostToDevice));
        BUILD_HIP(hipMemcpy(d_tops, tr.tops.data(), cols, hipMemcpyHostToDevice));
        for (int k = 0; k < 2; ++k) {
            BUILD_HIP(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
            BUILD_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
            BUILD_HIP(hipMalloc(&d_bricks[k], B * 4));
            BUILD_HIP(hipMalloc(&d_codes[k], B * kLeaves * 4));
            BUILD_HIP(hipMalloc(&d_info[k], B * 8 * 4));
            BUILD_HIP(hipHostMalloc(&h_codes[k], B * kLeaves * 4, hipHostMallocDefault));
            BUILD_HIP(hipHostMalloc(&h_info[k], B * 8 * 4, hipHostMallocDefault));
            BUILD_HIP(hipHostMalloc(&h_bricks[k], B * 4, hipHostMallocDefault));
        }
        const size_t n_batches = (n_work + B - 1) / B;
        auto launch = [&](size_t batch) -> bool {
            const int k = (int)(batch & 1);
            const size_t lo = batch * B, n = std::min(B, n_work - lo);
            for (size_t i = 0; i < n; ++i) {
                const uint32_t w = work[lo + i];
                const uint32_t bx = w % G, by = (w / G) % G, bz = w / (G * G);
                h_bricks[k][i] = bx | by << 10 | bz << 20;
            }
            BUILD_HIP(hipMemcpyAsync(d_bricks[k], h_bricks[k], n * 4, hipMemcpyHostToDevice, st[k]));
            hipLaunchKernelGGL(k_brick_codes, dim3((unsigned)n), dim3(256), 0, st[k], d_heights, d_tops, tr.dim,
                               tr.tunnels ? 1 : 0, d_bricks[k], d_codes[k], d_info[k]);
            BUILD_HIP(hipGetLastError());
            BUILD_HIP(hipMemcpyAsync(h_codes[k], d_codes[k], n * kLeaves * 4, hipMemcpyDeviceToHost, st[k]));
            BUILD_HIP(hipMemcpyAsync(h_info[k], d_info[k], n * 8 * 4, hipMemcpyDeviceToHost, st[k]));
            BUILD_HIP(hipEventRecord(done[k], st[k]));
            return true;
        };
        // Bricks whose 4096 leaves are one repeated code reduce to the same root.
        std::mutex memo_mu;
        std::unordered_map<uint32_t, std::pair<uint32_t, uint64_t>> memo;   // code -> (root, tree nodes)
        std::vector<std::vector<uint32_t>> ids(threads, std::vector<uint32_t>(kLeaves));
        const auto t0 = std::chrono::steady_clock::now();
        if (n_batches && !launch(0)) return false;
        double wait_s = 0.0, host_s = 0.0;
        size_t mixed = 0;
        for (size_t batch = 0; batch < n_batches; ++batch) {
            const int k = (int)(batch & 1);
            const auto w0 = std::chrono::steady_clock::now();
            BUILD_HIP(hipEventSynchronize(done[k]));
            const auto w1 = std::chrono::steady_clock::now();
            wait_s += std::chrono::duration<double>(w1 - w0).count();
            // the other buffer is free: its batch was consumed in the previous round
            if (batch + 1 < n_batches && !launch(batch + 1)) return false;
            const size_t lo = batch * B, n = std::min(B, n_work - lo);
            const uint32_t *codes = h_codes[k], *info = h_info[k];
            parallel_for(threads, n, [&](uint64_t i, int t) {
                BrickStats &bs = stats[t];
                const uint32_t *inf = info + i * 8;
                for (int v = 0; v < 6; ++v) bs.hist[v] += inf[1 + v];
                // an expanded tree (dedup = 0) shares nothing: every brick reduced on its own
                const uint32_t uni = ns.dedup ? inf[0] : kMixed;
                uint32_t root = 0;
                if (uni != kMixed) {
                    {
                        std::lock_guard<std::mutex> g(memo_mu);
                        auto it = memo.find(uni);
                        if (it != memo.end()) {
                            bs.tree_nodes += it->second.second;
                            brick_root[work[lo + i]] = it->second.first;
                            return;
                        }
                    }
                    BrickStats one;
                    std::vector<uint32_t> &id = ids[t];
                    const uint32_t leaf = uni ? ns.intern_code(uni) : 0;
                    std::fill(id.begin(), id.end(), leaf);
                    one.tree_nodes = uni ? (uint64_t)kLeaves : 0;
                    root = reduce_brick(ns, kBrickLog2, id, one);
                    bs.tree_nodes += one.tree_nodes;
                    std::lock_guard<std::mutex> g(memo_mu);
                    memo.emplace(uni, std::make_pair(root, one.tree_nodes));
                } else {
                    std::vector<uint32_t> &id = ids[t];
                    const uint32_t *c = codes + i * kLeaves;
                    uint32_t last_code = 0, last_id = 0;
                    for (int l = 0; l < kLeaves; ++l) {
                        const uint32_t code = c[l];
                        if (code != last_code || !ns.dedup) {
                            last_code = code;
                            last_id = code ? ns.intern_code(code) : 0;
                        }
                        id[l] = last_id;
                        bs.tree_nodes += code != 0;
                    }
                    root = reduce_brick(ns, kBrickLog2, id, bs);
                }
                brick_root[work[lo + i]] = root;
            });
            for (size_t i = 0; i < n; ++i) mixed += h_info[k][i * 8] == kMixed;
            host_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w1).count();
        }
        if (std::getenv("OCH_BUILD_TRACE"))
            std::fprintf(stderr, "[och_build] bricks: %zu (%zu mixed), %zu batches, waited %.3f s, host %.3f s\n", n_work,
                         mixed, (size_t)n_batches, wait_s, host_s);
        if (gpu_seconds) *gpu_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return true;
    };
    const bool ok = run();
    cleanup();
    return ok;
}

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
    uint32_t *overflow;              // 1: capacity exhausted, 2: table exhausted
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

__device__ inline uint32_t node_slot(const uint32_t c[8], int h, uint32_t mask)
{
    uint64_t hs = mix64((uint64_t)h * 0x9E3779B97F4A7C15ull ^ ((uint64_t)c[1] << 32 | c[0]));
    hs = mix64(hs ^ ((uint64_t)c[3] << 32 | c[2]));
    hs = mix64(hs ^ ((uint64_t)c[5] << 32 | c[4]));
    hs = mix64(hs ^ ((uint64_t)c[7] << 32 | c[6]));
    return (uint32_t)hs & mask;
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
    uint32_t i = node_slot(c, L.h, S.tmask);
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
__global__ __launch_bounds__(256) void k_intern_rows(GpuStore S, GpuLevel L, uint32_t *__restrict__ rep,
                                                     uint32_t *__restrict__ slot)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < L.count;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) gather(S, L, idx, c);
    // lane 0 of a wavefront is live whenever any of its lanes is (idx ascends)
    bool follows = live && (threadIdx.x & 63u) != 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) follows &= __shfl(c[k], 0) == c[k];
    uint32_t r = 0;
    if (live) slot[idx] = kNoSlot;
    if (live && !follows) r = probe_node(S, L, idx, c, slot);
    const uint32_t lead = __shfl(r, 0);   // an id or kCand | index, both final for an equal row
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

#define DAG_HIP(expr)                          \
    do {                                       \
        if ((expr) != hipSuccess) return OCH_E_HIP; \
    } while (0)

using DeviceAlloc = std::function<bool(void **, size_t)>;   // hipMalloc into the caller's list of buffers

dim3 blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// The store's nodes reachable from root (!= 0), renumbered breadth-first and
// 1-based on the device (k_bfs_*).  *out: malloc'd n_out x 8 words, as renumber().
int renumber_gpu(const GpuStore &S, uint32_t used, uint32_t root, int depth, hipStream_t st, const DeviceAlloc &dalloc,
                 uint32_t **out, uint32_t *n_out, bool trace)
{
    const auto t_bfs = std::chrono::steady_clock::now();
    // first / newid / order over the ids, mark / pos over one level's candidates
    uint32_t *d_first, *d_newid, *d_order, *d_mark, *d_pos, *d_out;
    const size_t max_cand = (size_t)used * 8;
    if (!dalloc((void **)&d_first, (size_t)used * 4) || !dalloc((void **)&d_newid, (size_t)used * 4) ||
        !dalloc((void **)&d_order, (size_t)used * 4) || !dalloc((void **)&d_mark, max_cand * 4) ||
        !dalloc((void **)&d_pos, max_cand * 4) || !dalloc((void **)&d_out, max_cand * 4))
        return OCH_E_NOMEM;
    size_t scan_bytes = 0;
    DAG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_mark, d_pos, (int)max_cand, st));
    void *d_scan = nullptr;
    if (!dalloc(&d_scan, std::max<size_t>(scan_bytes, 4))) return OCH_E_NOMEM;
    const uint32_t base = 1;
    DAG_HIP(hipMemsetAsync(d_first, 0xFF, (size_t)used * 4, st));
    DAG_HIP(hipMemcpyAsync(d_order, &root, 4, hipMemcpyHostToDevice, st));
    DAG_HIP(hipMemcpyAsync(d_newid + root, &base, 4, hipMemcpyHostToDevice, st));
    uint32_t off = 0, f = 1;
    for (int l = 1; l < depth && f; ++l) {
        const uint32_t nc = 8 * f, next = off + f;
        hipLaunchKernelGGL(k_bfs_first, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_first);
        hipLaunchKernelGGL(k_bfs_mark, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_first, d_mark);
        DAG_HIP(hipGetLastError());
        DAG_HIP(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_mark, d_pos, (int)nc, st));
        hipLaunchKernelGGL(k_bfs_place, blocks(nc), dim3(256), 0, st, S.nodes, d_order + off, f, d_mark, d_pos, d_order,
                           next, d_newid, base);
        DAG_HIP(hipGetLastError());
        uint32_t tail[2];
        DAG_HIP(hipMemcpyAsync(&tail[0], d_pos + nc - 1, 4, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipMemcpyAsync(&tail[1], d_mark + nc - 1, 4, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipStreamSynchronize(st));
        off = next;
        f = tail[0] + tail[1];
    }
    const uint32_t n = off + f;
    hipLaunchKernelGGL(k_bfs_output, blocks((size_t)n * 8), dim3(256), 0, st, S.nodes, S.level, d_order, d_newid, n, d_out);
    DAG_HIP(hipGetLastError());
    uint32_t *nodes = static_cast<uint32_t *>(std::malloc((size_t)n * 32));
    if (!nodes) return OCH_E_NOMEM;
    if (hipMemcpyAsync(nodes, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        std::free(nodes);
        return OCH_E_HIP;
    }
    *out = nodes;
    *n_out = n;
    if (trace)
        std::fprintf(stderr, "[och_build] gpu renumbering %.3f s\n",
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bfs).count());
    return OCH_OK;
}

// The whole DAG on the current GPU: bricks voxelised (k_brick_codes) and
// interned batch by batch, then the levels above the bricks, then renumbered
// breadth-first (1-based).  *out: malloc'd n_out x 8 words, as renumber().
// Returns a status.
int build_dag_gpu(const Terrain &tr, uint32_t cap, const std::vector<uint32_t> &work, int G, uint32_t **out,
                  uint32_t *n_out, uint32_t &root, BrickStats &total, bool trace)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OCH_E_NODEV;
    (void)hipGetLastError();        // a stale error of an earlier HIP call (another library's) is not this build's
    const size_t n_work = work.size();
    const size_t B = 8192;                                    // bricks per batch
    const size_t cols = (size_t)tr.dim * tr.dim, grid_cells = (size_t)G * G * G;
    uint32_t tsize = 1;
    while (tsize < 2 * cap) tsize <<= 1;
    const size_t rep_cap = std::max(B * 512, grid_cells / 8);
    std::vector<void *> bufs;
    hipStream_t st = nullptr;
    auto dalloc = [&](void **p, size_t bytes) {
        if (hipMalloc(p, bytes) != hipSuccess) return false;
        bufs.push_back(*p);
        return true;
    };
    int status = OCH_OK;
    auto run = [&]() -> int {
        int32_t *d_heights;
        uint8_t *d_tops;
        uint32_t *d_enc, *d_work, *d_codes, *d_info, *d_rep, *d_slot, *d_a, *d_b, *d_grid[2];
        GpuStore S{};
        S.cap = cap;
        S.tmask = tsize - 1;
        bool ok = dalloc((void **)&d_heights, cols * 4) && dalloc((void **)&d_tops, cols) &&
                  dalloc((void **)&d_enc, std::max<size_t>(n_work, 1) * 4) &&
                  dalloc((void **)&d_work, std::max<size_t>(n_work, 1) * 4) && dalloc((void **)&d_codes, B * kLeaves * 4) &&
                  dalloc((void **)&d_info, std::max<size_t>(n_work, 1) * 32) && dalloc((void **)&d_rep, rep_cap * 4) &&
                  dalloc((void **)&d_slot, rep_cap * 4) && dalloc((void **)&d_a, B * 512 * 4) &&
                  dalloc((void **)&d_b, B * 64 * 4) && dalloc((void **)&d_grid[0], grid_cells * 4) &&
                  dalloc((void **)&d_grid[1], grid_cells * 4) && dalloc((void **)&S.nodes, (size_t)cap * 32) &&
                  dalloc((void **)&S.level, cap) && dalloc((void **)&S.next, 256 + 128 * kCounters) &&
                  dalloc((void **)&S.table, (size_t)tsize * 4) && dalloc((void **)&S.leaf_id, (size_t)4 << 24);
        if (!ok) return OCH_E_NOMEM;
        S.overflow = S.next + 1;
        S.tree_nodes = reinterpret_cast<unsigned long long *>(S.next + 64);
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return OCH_E_HIP;
        std::vector<uint32_t> enc(n_work);
        for (size_t i = 0; i < n_work; ++i) {
            const uint32_t w = work[i];
            enc[i] = (w % G) | ((w / G) % G) << 10 | (w / (G * G)) << 20;
        }
        const uint32_t one = 1;
        DAG_HIP(hipMemcpyAsync(d_heights, tr.heights.data(), cols * 4, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemcpyAsync(d_tops, tr.tops.data(), cols, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemcpyAsync(d_enc, enc.data(), n_work * 4, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemcpyAsync(d_work, work.data(), n_work * 4, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemsetAsync(S.next, 0, 256 + 128 * kCounters, st));
        DAG_HIP(hipMemcpyAsync(S.next, &one, 4, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemsetAsync(S.table, 0, (size_t)tsize * 4, st));
        DAG_HIP(hipMemsetAsync(S.leaf_id, 0, (size_t)4 << 24, st));
        DAG_HIP(hipMemsetAsync(S.nodes, 0, 32, st));
        DAG_HIP(hipMemsetAsync(d_grid[0], 0, grid_cells * 4, st));
        auto level_pass = [&](const GpuLevel &L, uint32_t *dst, const uint32_t *dst_index) -> bool {
            if (L.count == 0) return true;
            hipLaunchKernelGGL(k_intern, blocks(L.count), dim3(256), 0, st, S, L, d_rep, d_slot);
            hipLaunchKernelGGL(k_settle, blocks(L.count), dim3(256), 0, st, S, L.count, d_rep, d_slot, dst, dst_index);
            return hipGetLastError() == hipSuccess;
        };
        for (size_t lo = 0; lo < n_work; lo += B) {
            const uint32_t n = (uint32_t)std::min(B, n_work - lo);
            hipLaunchKernelGGL(k_brick_codes, dim3(n), dim3(256), 0, st, d_heights, d_tops, tr.dim, tr.tunnels ? 1 : 0,
                               d_enc + lo, d_codes, d_info + lo * 8);
            hipLaunchKernelGGL(k_intern_codes, blocks((size_t)n * kLeaves), dim3(256), 0, st, S, d_codes,
                               n * (uint32_t)kLeaves);
            DAG_HIP(hipGetLastError());
            // brick levels 1..4: 8^3, 4^3, 2^3, 1 node per brick; the roots land in the grid
            if (!level_pass({d_codes, 1, 3, n * 512u, 1}, d_a, nullptr) ||
                !level_pass({d_a, 0, 2, n * 64u, 2}, d_b, nullptr) || !level_pass({d_b, 0, 1, n * 8u, 3}, d_a, nullptr) ||
                !level_pass({d_a, 0, 0, n, 4}, d_grid[0], d_work + lo))
                return OCH_E_HIP;
        }
        // levels above the bricks, one grid of side G / 2, G / 4, ... 1
        int cur = 0, log2n = 0;
        while ((1 << (log2n + 1)) < G) ++log2n;   // G = 2^(log2n + 1)
        for (int h = kBrickLog2; h < tr.depth; ++h, --log2n) {
            if (!level_pass({d_grid[cur], 0, log2n, 1u << (3 * log2n), h}, d_grid[cur ^ 1], nullptr)) return OCH_E_HIP;
            cur ^= 1;
        }
        uint32_t head[4] = {0, 0, 0, 0};
        std::vector<unsigned long long> counts((size_t)16 * kCounters);
        DAG_HIP(hipMemcpyAsync(head, S.next, 16, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipMemcpyAsync(counts.data(), S.tree_nodes, counts.size() * 8, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipMemcpyAsync(&root, d_grid[cur], 4, hipMemcpyDeviceToHost, st));
        std::vector<uint32_t> info(n_work * 8);
        DAG_HIP(hipMemcpyAsync(info.data(), d_info, n_work * 32, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipStreamSynchronize(st));
        if (head[1]) return OCH_E_CAPACITY;
        const uint32_t used = std::min(head[0], cap);
        total.tree_nodes = 0;
        for (int k = 0; k < kCounters; ++k) total.tree_nodes += counts[(size_t)16 * k];
        for (size_t i = 0; i < n_work; ++i) {
            for (int v = 0; v < 6; ++v) total.hist[v] += info[i * 8 + 1 + v];
            total.tree_nodes += info[i * 8 + 7];
        }
        if (!root) {   // empty world: one zero node
            *n_out = 1;
            *out = static_cast<uint32_t *>(std::calloc(8, 4));
            return *out ? OCH_OK : OCH_E_NOMEM;
        }
        const int rs = renumber_gpu(S, used, root, tr.depth, st, dalloc, out, n_out, trace);
        if (rs == OCH_OK && trace) std::fprintf(stderr, "[och_build] gpu dag: %zu bricks, %u ids\n", n_work, used);
        return rs;
    };
    status = run();
    if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    for (void *p : bufs) (void)hipFree(p);
    return status;
}

// Breadth-first renumbering of a node store (ids 1 .. used - 1, records of 8
// child words, level[id] = height above the voxels): level by level from the
// root, children in slot order; 1-based (h_octree, slot 0 never used) or
// 0-based octree.  *out: malloc'd n_out x 8 words (one zero node when empty).
int renumber(const uint32_t *store, const uint8_t *level, uint32_t used, uint32_t root, int depth, int base,
             uint32_t **out, uint32_t *n_out)
{
    std::vector<uint32_t> newid(used, 0);
    std::vector<uint32_t> order;
    if (root) {
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
    }
    *n_out = (uint32_t)std::max<size_t>(order.size(), 1);
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

// ------------------------------------------------------------ voxel builder
//
// A DAG from the caller's voxels (och_build_voxels): a list of (x, y, z, id)
// records that act as successive h_octree::set calls, or a dense grid of ids.
// Every voxel gets a Morton key, three bits per level with the leaf level's
// child index x | y << 1 | z << 2 in the low bits, so key >> 3 (h + 1) names
// its ancestor at height h and a sorted list of unique keys holds every node's
// children side by side.  Host and GPU run the same steps:
//   keys      -- one key per record, value = the record's index; a record
//                outside the tree gets bit 3 depth, sorts last and is dropped.
//                A grid's cell i *is* key i: sorted and unique as it stands.
//   sort      -- stable, so equal keys keep record order.
//   last wins -- an entry survives iff it is the last of its key and its id is
//                not 0; the survivors are counted per id here.
//   counts    -- neighbours i - 1, i of the unique list first differ in child
//                index t = (highest differing bit) / 3: entry i opens a new
//                node at the heights below t.  One pass bins t; the suffix
//                sums are the node counts of all levels, which size every
//                buffer and launch before the level loop starts.
//   levels    -- h = 0 .. depth - 1: entries with equal key >> 3 form one row
//                of eight child words (voxel ids at h = 0, all 32 bits; node
//                ids above), rows are interned into (level, 8 words) -> id and
//                the ids become the next level's child words.
//   renumber  -- breadth-first, as the terrain builder.
// On the GPU each step is its own dispatch: rows, keys and node records are
// read only by later dispatches than the one that wrote them, and within a
// dispatch workgroups meet only in the atomics (k_intern's rule, above).

constexpr int kMaxVoxelDepth = 21;   // 3 * 21 key bits + the out-of-range bit = 64
constexpr int kBins = 32;            // level bins per counter row (>= kMaxVoxelDepth + 1)

struct VoxelStats {
    uint64_t solid = 0, hist[8] = {0}, tree_nodes = 0;
};

__host__ __device__ inline uint64_t spread3(uint64_t x)   // bit i of 21 -> bit 3 i
{
    x &= 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__host__ __device__ inline uint32_t compact3(uint64_t x)   // bit 3 i -> bit i
{
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10C30C30C30C30C3ull;
    x = (x ^ (x >> 4)) & 0x100F00F00F00F00Full;
    x = (x ^ (x >> 8)) & 0x1F0000FF0000FFull;
    x = (x ^ (x >> 16)) & 0x1F00000000FFFFull;
    x = (x ^ (x >> 32)) & 0x1FFFFFull;
    return (uint32_t)x;
}

__host__ __device__ inline uint64_t voxel_key(uint32_t x, uint32_t y, uint32_t z, int depth)
{
    if ((x | y | z) >> depth) return 1ull << (3 * depth);   // outside the tree
    return spread3(x) | spread3(y) << 1 | spread3(z) << 2;
}

// The heights below which `key` opens new nodes after its predecessor `prev`
// in the unique list (first = no predecessor: a new node at every height).
__host__ __device__ inline int level_bin(bool first, uint64_t prev, uint64_t key, int depth)
{
    return first ? depth : (63 - __builtin_clzll(prev ^ key)) / 3;
}

// counts[h], h < depth, from the bins; returns their sum (the expanded tree's nodes).
uint64_t level_counts(const uint64_t *bins, int depth, uint64_t *counts)
{
    uint64_t above = 0, sum = 0;
    for (int h = depth - 1; h >= 0; --h) {
        above += bins[h + 1];
        counts[h] = above;
        sum += above;
    }
    return sum;
}

// Ids to reserve: the caller's, or the exact bound (one per tree node, + id 0).
// Ids and row indices share a word with the kCand flag: below 2^31 both.
uint32_t voxel_capacity(uint32_t wanted, uint64_t tree_nodes)
{
    const uint64_t bound = std::min<uint64_t>(tree_nodes + 1, kCand);
    return (uint32_t)(wanted ? std::min<uint64_t>(wanted, bound) : bound);
}

// Block-wide count of the kept voxels per id 1..7, then one atomic per id and
// block on one of kCounters rows (128 B apart), as count_nodes.
__device__ inline void count_ids(bool keep, uint32_t id, unsigned long long *counters)
{
    __shared__ uint32_t hist[8];
    if (threadIdx.x < 8) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t k = 1; k < 8; ++k) {
        const uint64_t b = __ballot(keep && id == k);
        if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&hist[k], (uint32_t)__popcll(b));
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < 8 && hist[threadIdx.x])
        atomicAdd(counters + 16 * (blockIdx.x % kCounters) + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_vox_keys(const uint32_t *__restrict__ recs, uint32_t n, int depth,
                                                  uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *r = recs + (size_t)i * 4;
    keys[i] = voxel_key(r[0], r[1], r[2], depth);
    vals[i] = i;
}

// Last wins, over the sorted list: flags[i] = entry i is kept, ids[i] = its id.
__global__ __launch_bounds__(256) void k_vox_last(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                  const uint32_t *__restrict__ recs, uint32_t n, int depth,
                                                  uint32_t *__restrict__ flags, uint32_t *__restrict__ ids,
                                                  unsigned long long *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t id = 0;
    if (i < n) {
        const uint64_t key = keys[i];
        if (!(key >> (3 * depth)) && (i + 1 == n || keys[i + 1] != key)) id = recs[(size_t)vals[i] * 4 + 3];
        flags[i] = id != 0;
        ids[i] = id;
    }
    count_ids(id != 0, id, counters);
}

// A grid's cells in key order (n = dim^3 <= 2^30): thread i is key i.
template <class T>
__global__ __launch_bounds__(256) void k_vox_cells(const T *__restrict__ grid, uint32_t n, int depth,
                                                   uint32_t *__restrict__ flags, uint32_t *__restrict__ ids,
                                                   unsigned long long *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t id = 0;
    if (i < n) {
        const size_t x = compact3(i), y = compact3(i >> 1), z = compact3(i >> 2);
        id = grid[(z << depth | y) << depth | x];
        flags[i] = id != 0;
        ids[i] = id;
    }
    count_ids(id != 0, id, counters);
}

// The kept entries, packed: pos = the inclusive sum of flags; keys = null for a grid.
__global__ __launch_bounds__(256) void k_vox_compact(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flags,
                                                     const uint32_t *__restrict__ pos, const uint32_t *__restrict__ ids,
                                                     uint32_t n, uint64_t *__restrict__ ukeys, uint32_t *__restrict__ words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const uint32_t p = pos[i] - 1u;
    ukeys[p] = keys ? keys[i] : (uint64_t)i;
    words[p] = ids[i];
}

// Level bins of the unique list: an LDS histogram per block, then one atomic
// per bin and block on one of kCounters rows of kBins.
__global__ __launch_bounds__(256) void k_vox_levels(const uint64_t *__restrict__ ukeys, uint32_t m, int depth,
                                                    uint32_t *__restrict__ bins)
{
    __shared__ uint32_t hist[kBins];
    if (threadIdx.x < kBins) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) {
        const int t = level_bin(i == 0, i ? ukeys[i - 1] : 0, ukeys[i], depth);
        if (t) atomicAdd(&hist[t], 1u);   // t = 0: another voxel of the same leaf-level node
    }
    __syncthreads();
    if (threadIdx.x < kBins && hist[threadIdx.x])
        atomicAdd(bins + kBins * (blockIdx.x % kCounters) + threadIdx.x, hist[threadIdx.x]);
}

// flags[i] = entry i is the first child of its parent.
__global__ __launch_bounds__(256) void k_vox_heads(const uint64_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = i == 0 || (keys[i] >> 3) != (keys[i - 1] >> 3);
}

// Entry i's child word into its parent's (pre-zeroed) row, node = pos[i] - 1
// (pos = the inclusive sum of the head flags); every head stores the parent key.
__global__ __launch_bounds__(256) void k_vox_rows(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ words,
                                                  uint32_t n, const uint32_t *__restrict__ flags,
                                                  const uint32_t *__restrict__ pos, uint32_t n_rows,
                                                  uint32_t *__restrict__ rows, uint64_t *__restrict__ parents,
                                                  uint32_t *__restrict__ overflow)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = pos[i] - 1u;
    if (node >= n_rows) {   // the level counts size the rows: never, unless they are wrong
        atomicOr(overflow, 4u);
        return;
    }
    const uint64_t key = keys[i];
    rows[(size_t)node * 8 + (key & 7u)] = words[i];
    if (flags[i]) parents[node] = key >> 3;
}

int build_voxels_gpu(const och_voxel_params &P, uint32_t **out, uint32_t *n_out, uint32_t &root, VoxelStats &vs, bool trace)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OCH_E_NODEV;
    (void)hipGetLastError();        // a stale error of an earlier HIP call (another library's) is not this build's
    const int depth = P.depth;
    const bool list = P.kind == OCH_VOXELS_LIST;
    const uint32_t n = list ? (uint32_t)P.n : 1u << (3 * depth);
    const size_t in_bytes = list ? (size_t)n * 16 : (size_t)n * (P.kind == OCH_VOXELS_GRID_U8 ? 1 : 4);
    auto empty = [&] {   // no voxels: one zero node
        root = 0;
        *n_out = 1;
        *out = static_cast<uint32_t *>(std::calloc(8, 4));
        return *out ? OCH_OK : OCH_E_NOMEM;
    };
    if (n == 0) return empty();
    std::vector<void *> bufs;
    hipStream_t st = nullptr;
    auto dalloc = [&](void **p, size_t bytes) {
        if (hipMalloc(p, std::max<size_t>(bytes, 4)) != hipSuccess) return false;
        bufs.push_back(*p);
        return true;
    };
    auto run = [&]() -> int {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return OCH_E_HIP;
        auto t_last = std::chrono::steady_clock::now();
        auto phase = [&](const char *name) -> bool {   // OCH_BUILD_TRACE only: a synchronise per phase
            if (!trace) return true;
            if (hipStreamSynchronize(st) != hipSuccess) return false;
            const auto now = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[och_build] voxels gpu %-10s %8.4f s\n", name,
                         std::chrono::duration<double>(now - t_last).count());
            t_last = now;
            return true;
        };
        const void *d_in = P.data;
        if (!P.on_device) {
            void *up;
            if (!dalloc(&up, in_bytes)) return OCH_E_NOMEM;
            DAG_HIP(hipMemcpyAsync(up, P.data, in_bytes, hipMemcpyHostToDevice, st));
            d_in = up;
        }
        uint64_t *d_keys[2] = {nullptr, nullptr};
        uint32_t *d_words[2] = {nullptr, nullptr}, *d_flags, *d_pos, *d_ids, *d_bins;
        unsigned long long *d_counters;
        const size_t bins_bytes = (size_t)kCounters * kBins * 4, counters_bytes = (size_t)kCounters * 128;
        if (!dalloc((void **)&d_flags, (size_t)n * 4) || !dalloc((void **)&d_pos, (size_t)n * 4) ||
            !dalloc((void **)&d_ids, (size_t)n * 4) || !dalloc((void **)&d_bins, bins_bytes) ||
            !dalloc((void **)&d_counters, counters_bytes))
            return OCH_E_NOMEM;
        if (list && (!dalloc((void **)&d_keys[0], (size_t)n * 8) || !dalloc((void **)&d_keys[1], (size_t)n * 8) ||
                     !dalloc((void **)&d_words[0], (size_t)n * 4) || !dalloc((void **)&d_words[1], (size_t)n * 4)))
            return OCH_E_NOMEM;
        const int key_bits = std::min(64, 3 * depth + 1);
        size_t sort_bytes = 0, scan_bytes = 0;
        if (list)
            DAG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_keys[0], d_keys[1], d_words[0], d_words[1],
                                                       (int)n, 0, key_bits, st));
        DAG_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, d_flags, d_pos, (int)n, st));
        const size_t temp_bytes = std::max(sort_bytes, scan_bytes);
        void *d_temp;
        if (!dalloc(&d_temp, temp_bytes)) return OCH_E_NOMEM;
        DAG_HIP(hipMemsetAsync(d_bins, 0, bins_bytes, st));
        DAG_HIP(hipMemsetAsync(d_counters, 0, counters_bytes, st));
        if (!phase("upload")) return OCH_E_HIP;
        const uint64_t *d_sorted = nullptr;
        if (list) {
            const uint32_t *recs = static_cast<const uint32_t *>(d_in);
            hipLaunchKernelGGL(k_vox_keys, blocks(n), dim3(256), 0, st, recs, n, depth, d_keys[0], d_words[0]);
            DAG_HIP(hipGetLastError());
            size_t tb = temp_bytes;
            DAG_HIP(hipcub::DeviceRadixSort::SortPairs(d_temp, tb, d_keys[0], d_keys[1], d_words[0], d_words[1], (int)n, 0,
                                                       key_bits, st));
            if (!phase("sort")) return OCH_E_HIP;
            hipLaunchKernelGGL(k_vox_last, blocks(n), dim3(256), 0, st, d_keys[1], d_words[1], recs, n, depth, d_flags,
                               d_ids, d_counters);
            d_sorted = d_keys[1];
        } else if (P.kind == OCH_VOXELS_GRID_U8) {
            hipLaunchKernelGGL(k_vox_cells<uint8_t>, blocks(n), dim3(256), 0, st, static_cast<const uint8_t *>(d_in), n,
                               depth, d_flags, d_ids, d_counters);
        } else {
            hipLaunchKernelGGL(k_vox_cells<uint32_t>, blocks(n), dim3(256), 0, st, static_cast<const uint32_t *>(d_in), n,
                               depth, d_flags, d_ids, d_counters);
        }
        DAG_HIP(hipGetLastError());
        size_t tb = temp_bytes;
        DAG_HIP(hipcub::DeviceScan::InclusiveSum(d_temp, tb, d_flags, d_pos, (int)n, st));
        uint32_t m = 0;
        DAG_HIP(hipMemcpyAsync(&m, d_pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipStreamSynchronize(st));
        if (m == 0) return empty();
        // a list packs into the sort's input buffers (free by now) and the levels
        // alternate with its output buffers; a grid's are sized by its voxels
        if (!list && (!dalloc((void **)&d_keys[0], (size_t)m * 8) || !dalloc((void **)&d_keys[1], (size_t)m * 8) ||
                      !dalloc((void **)&d_words[0], (size_t)m * 4) || !dalloc((void **)&d_words[1], (size_t)m * 4)))
            return OCH_E_NOMEM;
        hipLaunchKernelGGL(k_vox_compact, blocks(n), dim3(256), 0, st, d_sorted, d_flags, d_pos, d_ids, n, d_keys[0],
                           d_words[0]);
        hipLaunchKernelGGL(k_vox_levels, blocks(m), dim3(256), 0, st, d_keys[0], m, depth, d_bins);
        DAG_HIP(hipGetLastError());
        std::vector<uint32_t> h_bins((size_t)kCounters * kBins);
        std::vector<unsigned long long> h_counters((size_t)kCounters * 16);
        DAG_HIP(hipMemcpyAsync(h_bins.data(), d_bins, bins_bytes, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipMemcpyAsync(h_counters.data(), d_counters, counters_bytes, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipStreamSynchronize(st));
        if (!phase("last wins")) return OCH_E_HIP;
        uint64_t bins[kBins] = {0}, counts[kMaxVoxelDepth] = {0};
        for (int r = 0; r < kCounters; ++r) {
            for (int t = 0; t < kBins; ++t) bins[t] += h_bins[(size_t)r * kBins + t];
            for (int k = 1; k < 8; ++k) vs.hist[k] += h_counters[(size_t)r * 16 + k];
        }
        vs.solid = m;
        vs.tree_nodes = level_counts(bins, depth, counts);
        if (counts[0] > m || counts[depth - 1] != 1) return och::report(OCH_E_HIP, "GPU voxel builder: inconsistent level counts");
        const uint32_t rows_max = (uint32_t)counts[0];   // counts only shrink towards the root
        GpuStore S{};
        S.cap = voxel_capacity(P.capacity, vs.tree_nodes);
        uint64_t tsize = 1;
        while (tsize < 2 * (uint64_t)S.cap) tsize <<= 1;
        S.tmask = (uint32_t)(tsize - 1);
        uint32_t *d_rows, *d_rep, *d_slot;
        if (!dalloc((void **)&d_rows, (size_t)rows_max * 32) || !dalloc((void **)&d_rep, (size_t)rows_max * 4) ||
            !dalloc((void **)&d_slot, (size_t)rows_max * 4) || !dalloc((void **)&S.nodes, (size_t)S.cap * 32) ||
            !dalloc((void **)&S.level, S.cap) || !dalloc((void **)&S.next, 256) ||
            !dalloc((void **)&S.table, (size_t)tsize * 4))
            return OCH_E_NOMEM;
        S.overflow = S.next + 1;
        const uint32_t one = 1;
        DAG_HIP(hipMemsetAsync(S.next, 0, 256, st));
        DAG_HIP(hipMemcpyAsync(S.next, &one, 4, hipMemcpyHostToDevice, st));
        DAG_HIP(hipMemsetAsync(S.table, 0, (size_t)tsize * 4, st));
        DAG_HIP(hipMemsetAsync(S.nodes, 0, 32, st));
        int cur = 0;
        uint32_t n_in = m;
        for (int h = 0; h < depth; ++h) {
            const uint32_t n_rows = (uint32_t)counts[h];
            hipLaunchKernelGGL(k_vox_heads, blocks(n_in), dim3(256), 0, st, d_keys[cur], n_in, d_flags);
            DAG_HIP(hipGetLastError());
            tb = temp_bytes;
            DAG_HIP(hipcub::DeviceScan::InclusiveSum(d_temp, tb, d_flags, d_pos, (int)n_in, st));
            DAG_HIP(hipMemsetAsync(d_rows, 0, (size_t)n_rows * 32, st));
            hipLaunchKernelGGL(k_vox_rows, blocks(n_in), dim3(256), 0, st, d_keys[cur], d_words[cur], n_in, d_flags, d_pos,
                               n_rows, d_rows, d_keys[cur ^ 1], S.overflow);
            GpuLevel L{d_rows, 0, 0, n_rows, h, 1};
            hipLaunchKernelGGL(k_intern_rows, blocks(n_rows), dim3(256), 0, st, S, L, d_rep, d_slot);
            hipLaunchKernelGGL(k_settle, blocks(n_rows), dim3(256), 0, st, S, n_rows, d_rep, d_slot, d_words[cur ^ 1], nullptr);
            DAG_HIP(hipGetLastError());
            cur ^= 1;
            n_in = n_rows;
        }
        uint32_t head[2] = {0, 0};
        DAG_HIP(hipMemcpyAsync(head, S.next, 8, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipMemcpyAsync(&root, d_words[cur], 4, hipMemcpyDeviceToHost, st));
        DAG_HIP(hipStreamSynchronize(st));
        if (!phase("levels")) return OCH_E_HIP;
        if (head[1] & 4u) return och::report(OCH_E_HIP, "GPU voxel builder: a row outside its level");
        if (head[1] || !root) return OCH_E_CAPACITY;
        const uint32_t used = std::min(head[0], S.cap);
        const int rs = renumber_gpu(S, used, root, depth, st, dalloc, out, n_out, trace);
        if (rs == OCH_OK && trace)
            std::fprintf(stderr, "[och_build] voxels gpu: %u entries, %u voxels, %u ids of %u\n", n, m, used - 1, S.cap - 1);
        return rs;
    };
    const int status = run();
    if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    for (void *p : bufs) (void)hipFree(p);
    return status;
}

// Stable sort of (key, record) pairs by key: sorted chunks on the threads, then merged pairwise.
void sort_pairs_host(std::vector<std::pair<uint64_t, uint32_t>> &v, int threads)
{
    auto less = [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; };
    size_t parts = 1;
    while ((int)(parts * 2) <= threads && v.size() / (parts * 2) >= 65536) parts *= 2;
    auto edge = [&](size_t k) { return v.size() * k / parts; };
    parallel_for((int)parts, parts, [&](uint64_t k, int) { std::stable_sort(v.begin() + edge(k), v.begin() + edge(k + 1), less); });
    for (size_t w = 1; w < parts; w *= 2)
        parallel_for((int)(parts / (2 * w)), parts / (2 * w), [&](uint64_t k, int) {
            std::inplace_merge(v.begin() + edge(2 * w * k), v.begin() + edge(2 * w * k + w), v.begin() + edge(2 * w * (k + 1)), less);
        });
}

int build_voxels_host(const och_voxel_params &P, int threads, uint32_t **out, uint32_t *n_out, uint32_t &root,
                      VoxelStats &vs, const std::function<void(const char *)> &phase)
{
    const int depth = P.depth;
    std::vector<uint64_t> keys;    // unique, ascending
    std::vector<uint32_t> words;   // the ids, then each level's node ids
    if (P.kind == OCH_VOXELS_LIST) {
        const uint32_t *recs = static_cast<const uint32_t *>(P.data);
        const size_t n = (size_t)P.n;
        std::vector<std::pair<uint64_t, uint32_t>> kv(n);
        const size_t chunk = 1 << 16;
        parallel_for(threads, (n + chunk - 1) / chunk, [&](uint64_t c, int) {
            for (size_t i = c * chunk; i < std::min(n, (c + 1) * chunk); ++i)
                kv[i] = {voxel_key(recs[i * 4], recs[i * 4 + 1], recs[i * 4 + 2], depth), (uint32_t)i};
        });
        sort_pairs_host(kv, threads);
        phase("sort");
        for (size_t i = 0; i < n; ++i) {
            const uint64_t key = kv[i].first;
            if (key >> (3 * depth)) break;   // the records outside the tree, sorted last
            if (i + 1 < n && kv[i + 1].first == key) continue;
            const uint32_t id = recs[(size_t)kv[i].second * 4 + 3];
            if (!id) continue;
            keys.push_back(key);
            words.push_back(id);
        }
    } else {
        // key ranges in order, one at a time per thread, joined in order
        const size_t n = (size_t)1 << (3 * depth), parts = (size_t)std::min<uint64_t>(n, 256);
        const uint8_t *g8 = static_cast<const uint8_t *>(P.data);
        const uint32_t *g32 = static_cast<const uint32_t *>(P.data);
        std::vector<std::vector<uint64_t>> part_keys(parts);
        std::vector<std::vector<uint32_t>> part_words(parts);
        parallel_for(threads, parts, [&](uint64_t p, int) {
            for (size_t i = n / parts * p; i < n / parts * (p + 1); ++i) {
                const size_t x = compact3(i), y = compact3(i >> 1), z = compact3(i >> 2);
                const size_t cell = (z << depth | y) << depth | x;
                const uint32_t id = P.kind == OCH_VOXELS_GRID_U8 ? g8[cell] : g32[cell];
                if (!id) continue;
                part_keys[p].push_back(i);
                part_words[p].push_back(id);
            }
        });
        for (size_t p = 0; p < parts; ++p) {
            keys.insert(keys.end(), part_keys[p].begin(), part_keys[p].end());
            words.insert(words.end(), part_words[p].begin(), part_words[p].end());
        }
        phase("cells");
    }
    const size_t m = keys.size();
    vs.solid = m;
    uint64_t bins[kBins] = {0}, counts[kMaxVoxelDepth] = {0};
    for (size_t i = 0; i < m; ++i) {
        if (words[i] < 8) ++vs.hist[words[i]];
        ++bins[level_bin(i == 0, i ? keys[i - 1] : 0, keys[i], depth)];
    }
    vs.tree_nodes = level_counts(bins, depth, counts);
    phase("last wins");
    if (m == 0) {
        root = 0;
        return renumber(nullptr, nullptr, 0, 0, depth, 1, out, n_out);
    }
    NodeStore ns;
    if (!ns.init(voxel_capacity(P.capacity, vs.tree_nodes), true)) {
        ns.release();
        return OCH_E_NOMEM;
    }
    std::vector<uint64_t> pkeys;
    std::vector<uint32_t> pwords, heads;
    for (int h = 0; h < depth; ++h) {
        const size_t n_in = keys.size(), n_rows = (size_t)counts[h];
        heads.clear();
        for (size_t i = 0; i < n_in; ++i)
            if (i == 0 || (keys[i] >> 3) != (keys[i - 1] >> 3)) heads.push_back((uint32_t)i);
        if (heads.size() != n_rows) {   // the level counts and the grouping are two views of one list
            ns.release();
            return OCH_E_INVALID;
        }
        pkeys.resize(n_rows);
        pwords.resize(n_rows);
        const size_t chunk = 4096;
        parallel_for(threads, (n_rows + chunk - 1) / chunk, [&](uint64_t c, int) {
            for (size_t r = c * chunk; r < std::min(n_rows, (c + 1) * chunk); ++r) {
                uint32_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                const size_t end = r + 1 < n_rows ? heads[r + 1] : n_in;
                for (size_t i = heads[r]; i < end; ++i) row[keys[i] & 7u] = words[i];
                pkeys[r] = keys[heads[r]] >> 3;
                pwords[r] = ns.intern(row, h);
            }
        });
        keys.swap(pkeys);
        words.swap(pwords);
    }
    phase("levels");
    root = words[0];
    if (ns.full.load() || !root) {
        ns.release();
        return OCH_E_CAPACITY;
    }
    const int rs = renumber(ns.nodes, ns.level, std::min(ns.next.load(), ns.cap), root, depth, 1, out, n_out);
    ns.release();
    return rs;
}

}  // namespace

extern "C" {

OCH_API void och_host_pool_free(och_host_pool *p)
{
    if (!p) return;
    std::free(p->nodes);
    p->nodes = nullptr;
    p->n_nodes = 0;
}

OCH_API int och_build_terrain(const och_terrain_params *params, och_host_pool *out)
{
    if (!params || !out) return OCH_E_INVALID;
    const int depth = params->depth;
    if (depth < 1 || depth > 12) return OCH_E_INVALID;
    if (!params->dedup && depth > 10) return OCH_E_INVALID;   // expanded tree would exceed 1 GB
    const auto t_start = std::chrono::steady_clock::now();
    // OCH_BUILD_TRACE=1: phase times on stderr
    const bool trace = std::getenv("OCH_BUILD_TRACE") != nullptr;
    auto phase = [&, t_last = t_start](const char *name) mutable {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[och_build] %-10s %8.3f s\n", name, std::chrono::duration<double>(now - t_last).count());
        t_last = now;
    };
    std::memset(out, 0, sizeof *out);
    const int threads = params->threads > 0 ? params->threads : default_threads();

    Terrain tr;
    tr.depth = depth;
    tr.dim = 1 << depth;
    tr.tunnels = params->tunnels != 0;
    const int dim = tr.dim;
    tr.heights.resize((size_t)dim * dim);
    tr.tops.resize((size_t)dim * dim);
    parallel_for(threads, (uint64_t)dim, [&](uint64_t y, int) {
        for (int x = 0; x < dim; ++x)
            tr.heights[y * dim + x] = och_terrain::column_height(kTables, x, (int)y, dim);
    });
    // Column tops: one rand() per column, y outer, x inner (ORT/test_och_h_octree.cpp:776-780).
    if (params->rand_kind == 1) {
        och_terrain::MsvcRand r;
        for (size_t i = 0; i < tr.tops.size(); ++i) tr.tops[i] = (uint8_t)(2 + (r.next() > 0x7FFF / 2));
    } else {
        och_terrain::GlibcRand r;
        r.seed(1);
        for (size_t i = 0; i < tr.tops.size(); ++i) tr.tops[i] = (uint8_t)(2 + (r.next() > 0x7FFFFFFF / 2));
    }

    phase("columns");
    const int s_log2 = std::min(depth, 5);
    const int S = 1 << s_log2, G = dim / S;
    tr.brick_hmax.assign((size_t)G * G, -1);
    for (int by = 0; by < G; ++by)
        for (int bx = 0; bx < G; ++bx) {
            int hm = -1;
            for (int y = by * S; y < (by + 1) * S; ++y)
                for (int x = bx * S; x < (bx + 1) * S; ++x) hm = std::max(hm, tr.heights[(size_t)y * dim + x]);
            tr.brick_hmax[(size_t)by * G + bx] = hm;
        }

    // DAG capacity: 3x the unique nodes of the default terrain (19 318 / 334 025 /
    // 4 980 409 at depth 8 / 10 / 12); the hash table is twice the capacity
    const uint32_t cap = params->dedup ? (depth <= 8 ? (1u << 20) : depth <= 10 ? (1u << 23) : (1u << 24))
                                       : (uint32_t)std::min<uint64_t>(1ull << 28, 48ull << (2 * depth));
    phase("init");
    // Bricks that reach below the highest surface of their columns.
    std::vector<uint32_t> work;
    for (int bz = 0; bz < G; ++bz)
        for (int by = 0; by < G; ++by)
            for (int bx = 0; bx < G; ++bx)
                if (bz * S <= tr.brick_hmax[(size_t)by * G + bx]) work.push_back(((uint32_t)bz * G + by) * G + bx);
    const int base = params->dedup ? 1 : 0;
    BrickStats total;
    uint32_t root = 0, n_out = 0;
    uint32_t *nodes = nullptr;
    if (params->use_gpu && params->dedup && s_log2 == kBrickLog2) {
        // the whole DAG on the GPU, renumbering included
        const int st = build_dag_gpu(tr, cap, work, G, &nodes, &n_out, root, total, trace);
        if (st != OCH_OK)
            return och::report(st, st == OCH_E_NODEV    ? "use_gpu: no HIP device"
                                   : st == OCH_E_CAPACITY ? "GPU builder: node capacity exhausted"
                                   : st == OCH_E_NOMEM    ? "GPU builder: device allocation failed"
                                                          : "GPU builder: HIP error");
        phase("gpu dag");
    } else {
        NodeStore ns;
        if (!ns.init(cap, params->dedup != 0)) {
            ns.release();
            return OCH_E_NOMEM;
        }
        std::vector<uint32_t> brick_root((size_t)G * G * G, 0);
        std::vector<BrickStats> stats(threads);
        double gpu_s = 0.0;
        if (params->use_gpu && s_log2 == kBrickLog2) {
            // an expanded tree: voxels from the GPU, one node per tree node on the host
            if (!build_bricks_gpu(tr, ns, threads, work, G, brick_root, stats, &gpu_s)) {
                ns.release();
                return och::report(OCH_E_NODEV, "use_gpu: no HIP device could run the voxel kernel");
            }
        } else {
            std::vector<std::vector<uint8_t>> vox(threads, std::vector<uint8_t>((size_t)S * S * S));
            std::vector<std::vector<uint32_t>> ids(threads, std::vector<uint32_t>((size_t)S * S * S / 8));
            parallel_for(threads, work.size(), [&](uint64_t i, int t) {
                const uint32_t b = work[i];
                const int bx = b % G, by = (b / G) % G, bz = b / (G * G);
                brick_root[b] = build_brick(tr, ns, s_log2, bx, by, bz, vox[t], ids[t], stats[t]);
            });
        }
        phase("bricks");
        for (auto &s : stats) {
            for (int k = 0; k < 8; ++k) total.hist[k] += s.hist[k];
            total.tree_nodes += s.tree_nodes;
        }
        // Levels above the bricks.
        {
            std::vector<uint32_t> cur = brick_root, nxt;
            int n = G;
            for (int h = s_log2; h < depth; ++h) {
                const int m = n / 2;
                nxt.assign((size_t)m * m * m, 0);
                for (int z = 0; z < m; ++z)
                    for (int y = 0; y < m; ++y)
                        for (int x = 0; x < m; ++x) {
                            uint32_t c[8];
                            bool any = false;
                            for (int k = 0; k < 8; ++k) {
                                const int cx = 2 * x + (k & 1), cy = 2 * y + ((k >> 1) & 1), cz = 2 * z + ((k >> 2) & 1);
                                c[k] = cur[((size_t)cz * n + cy) * n + cx];
                                any |= c[k] != 0;
                            }
                            if (any) {
                                nxt[((size_t)z * m + y) * m + x] = ns.intern(c, h);
                                ++total.tree_nodes;
                            }
                        }
                cur.swap(nxt);
                n = m;
            }
            root = cur[0];
        }
        phase("upper");
        if (ns.full.load()) {
            ns.release();
            return OCH_E_CAPACITY;
        }
        const int rs = renumber(ns.nodes, ns.level, std::min(ns.next.load(), ns.cap), root, depth, base, &nodes, &n_out);
        ns.release();
        if (rs != OCH_OK) return rs;
    }
    phase("renumber");

    out->nodes = nodes;
    out->n_nodes = n_out;
    out->root = root ? (uint32_t)base : 0;
    out->depth = depth;
    out->index_base = base;
    out->tree_nodes = total.tree_nodes;
    for (int k = 0; k < 8; ++k) out->voxel_hist[k] = total.hist[k];
    out->solid_voxels = 0;
    for (int k = 1; k < 8; ++k) out->solid_voxels += total.hist[k];
    out->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return OCH_OK;
}

OCH_API int och_build_voxels(const och_voxel_params *params, och_host_pool *out)
{
    if (!params || !out) return och::report(OCH_E_INVALID, "och_build_voxels: null argument");
    const och_voxel_params &P = *params;
    if (P.depth < 1 || P.depth > kMaxVoxelDepth)
        return och::report(OCH_E_INVALID, "och_build_voxels: depth must be 1..21 (a Morton key of 3 * depth bits and the "
                                          "out-of-range bit fill 64 bits)");
    if (P.kind != OCH_VOXELS_LIST && P.kind != OCH_VOXELS_GRID_U8 && P.kind != OCH_VOXELS_GRID_U32)
        return och::report(OCH_E_INVALID, "och_build_voxels: unknown kind");
    if (P.kind == OCH_VOXELS_LIST && P.n >= (1ull << 31))
        return och::report(OCH_E_INVALID, "och_build_voxels: a list holds fewer than 2^31 records");
    if (P.kind != OCH_VOXELS_LIST && P.depth > (P.kind == OCH_VOXELS_GRID_U8 ? 10 : 9))
        return och::report(OCH_E_INVALID, "och_build_voxels: a dense grid is limited to depth 10 (u8) / 9 (u32); pass a list");
    if (!P.data && (P.kind != OCH_VOXELS_LIST || P.n))
        return och::report(OCH_E_INVALID, "och_build_voxels: data is null");
    if (P.on_device && !P.use_gpu)
        return och::report(OCH_E_INVALID, "och_build_voxels: device data needs use_gpu = 1");
    const auto t_start = std::chrono::steady_clock::now();
    const bool trace = std::getenv("OCH_BUILD_TRACE") != nullptr;
    auto phase = [&, t_last = t_start](const char *name) mutable {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[och_build] voxels %-10s %8.4f s\n", name, std::chrono::duration<double>(now - t_last).count());
        t_last = now;
    };
    std::memset(out, 0, sizeof *out);
    VoxelStats vs;
    uint32_t root = 0, n_out = 0;
    uint32_t *nodes = nullptr;
    const int st = P.use_gpu ? build_voxels_gpu(P, &nodes, &n_out, root, vs, trace)
                             : build_voxels_host(P, P.threads > 0 ? P.threads : default_threads(), &nodes, &n_out, root, vs, phase);
    if (st != OCH_OK)
        return och::report(st, st == OCH_E_NODEV      ? "use_gpu: no HIP device"
                               : st == OCH_E_CAPACITY ? "voxel builder: node capacity exhausted"
                               : st == OCH_E_NOMEM    ? "voxel builder: allocation failed"
                                                      : "voxel builder: HIP error");
    phase(P.use_gpu ? "gpu, whole" : "renumber");
    out->nodes = nodes;
    out->n_nodes = n_out;
    out->root = root ? 1 : 0;
    out->depth = P.depth;
    out->index_base = 1;
    out->tree_nodes = vs.tree_nodes;
    for (int k = 1; k < 8; ++k) out->voxel_hist[k] = vs.hist[k];
    out->solid_voxels = vs.solid;
    out->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return OCH_OK;
}

}  // extern "C"
