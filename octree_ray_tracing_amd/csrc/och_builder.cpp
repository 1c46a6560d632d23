// och_builder.cpp -- the builders' C-ABI entries (och_build_terrain,
// och_build_voxels, och_edit_voxels, och_host_pool_free, och_world_*) and the terrain
// builder: the demo terrain's canonical DAG, built bottom-up in parallel.  The
// DAG stores, their kernels and the renumbering are och_dag.h's; the voxel
// builder, which builds the same DAG from a caller's voxels, is
// och_voxel_build.h; the batch editor, which applies a list of edits to an
// existing pool, is och_voxel_edit.h; the resident world, which keeps that
// editor's store on the device between strokes, is och_world.h, with what all
// three world headers share (the state record, the box convention, the entry
// wrapper, the staging and read-back steps); what reads that world back on the
// device (at, a box to a grid, the exact box) is och_world_read.h; snapshots
// of that world, checkout and the diff of two roots are och_world_history.h;
// its box- and ball-shaped strokes (fill, clear, restore) are och_world_region.h,
// those conditional on the old voxel (paint, fill-under, replace) och_world_paint.h.
// One translation unit: the headers are included here and nowhere else.
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
// use_gpu: the voxel function -- simplex noise for every voxel below the
// surface, 2 * 10^10 evaluations at depth 12 -- runs on the GPU instead
// (k_brick_codes): one workgroup per 32^3 brick writes the brick's 4096
// leaf-level nodes as 24-bit codes (3 bits per child voxel), its voxel
// histogram and whether all its leaves are equal.  A DAG is then hash-consed
// and renumbered on the GPU too (build_dag_gpu, below); an
// expanded tree's nodes are allocated by host threads from the codes, batch
// after batch, while the GPU computes the next batch.  Same pool either way.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <mutex>
#include <unordered_map>

#include "och_dag.h"
#include "och_terrain.h"
#include "och_voxel_build.h"
#include "och_voxel_edit.h"
#include "och_world.h"
#include "och_world_read.h"
#include "och_world_history.h"
#include "och_world_region.h"
#include "och_world_paint.h"

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

struct Terrain {
    int depth = 0, dim = 0;
    bool tunnels = true;
    std::vector<int32_t> heights;
    std::vector<uint8_t> tops;
    std::vector<int32_t> brick_hmax;   // max column height per brick column
};

// Voxelise one brick of side S at (bx, by, bz) (brick units) and reduce it to
// its subtree root.  vox: S^3 scratch, ids: (S/2)^3 scratch.
uint32_t build_brick(const Terrain &tr, NodeStore &ns, int s_log2, int bx, int by, int bz, std::vector<uint8_t> &vox,
                     std::vector<uint32_t> &ids, BuildStats &st)
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
    return reduce_grid(ns, 1, s_log2, ids, st.tree_nodes);
}

// ------------------------------------------------------------ GPU voxelisation

constexpr int kBrickLog2 = 5, kBrick = 32, kLeaves = 4096;   // 32^3 voxels, 16^3 leaf-level nodes
constexpr uint32_t kMixed = 0xFFFFFFFFu;

__constant__ och_terrain::Tables c_tables = {OCH_PERM_TABLE, OCH_GRAD_TABLE};

// Brick w of a grid of side G, (bz * G + by) * G + bx, as k_brick_codes reads it.
inline uint32_t brick_code(uint32_t w, uint32_t G) { return (w % G) | ((w / G) % G) << 10 | (w / (G * G)) << 20; }

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

// Voxelise `work` on the current GPU in batches and hash-cons the codes on
// `threads` host threads, overlapping batch k + 1 on the GPU with batch k on
// the host.  Any status but OCH_OK: no GPU could run the voxel kernel; the
// caller then fails the build with OCH_E_NODEV (no host fallback).  Two
// streams, two events and pinned host buffers, so not a GpuScope.
int build_bricks_gpu(const Terrain &tr, NodeStore &ns, int threads, const std::vector<uint32_t> &work, int G,
                     std::vector<uint32_t> &brick_root, std::vector<BuildStats> &stats, double *gpu_seconds)
{
    if (!gpu_present()) return OCH_E_NODEV;
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
    auto run = [&]() -> int {
        const size_t cols = (size_t)tr.dim * tr.dim;
        GPU_TRY(hipMalloc(&d_heights, cols * 4));
        GPU_TRY(hipMalloc(&d_tops, cols));
        GPU_TRY(hipMemcpy(d_heights, tr.heights.data(), cols * 4, hipMemcpyHostToDevice));
        GPU_TRY(hipMemcpy(d_tops, tr.tops.data(), cols, hipMemcpyHostToDevice));
        for (int k = 0; k < 2; ++k) {
            GPU_TRY(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
            GPU_TRY(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
            GPU_TRY(hipMalloc(&d_bricks[k], B * 4));
            GPU_TRY(hipMalloc(&d_codes[k], B * kLeaves * 4));
            GPU_TRY(hipMalloc(&d_info[k], B * 8 * 4));
            GPU_TRY(hipHostMalloc(&h_codes[k], B * kLeaves * 4, hipHostMallocDefault));
            GPU_TRY(hipHostMalloc(&h_info[k], B * 8 * 4, hipHostMallocDefault));
            GPU_TRY(hipHostMalloc(&h_bricks[k], B * 4, hipHostMallocDefault));
        }
        const size_t n_batches = (n_work + B - 1) / B;
        auto launch = [&](size_t batch) -> int {
            const int k = (int)(batch & 1);
            const size_t lo = batch * B, n = std::min(B, n_work - lo);
            for (size_t i = 0; i < n; ++i) h_bricks[k][i] = brick_code(work[lo + i], G);
            GPU_TRY(hipMemcpyAsync(d_bricks[k], h_bricks[k], n * 4, hipMemcpyHostToDevice, st[k]));
            hipLaunchKernelGGL(k_brick_codes, dim3((unsigned)n), dim3(256), 0, st[k], d_heights, d_tops, tr.dim,
                               tr.tunnels ? 1 : 0, d_bricks[k], d_codes[k], d_info[k]);
            GPU_TRY(hipGetLastError());
            GPU_TRY(hipMemcpyAsync(h_codes[k], d_codes[k], n * kLeaves * 4, hipMemcpyDeviceToHost, st[k]));
            GPU_TRY(hipMemcpyAsync(h_info[k], d_info[k], n * 8 * 4, hipMemcpyDeviceToHost, st[k]));
            GPU_TRY(hipEventRecord(done[k], st[k]));
            return OCH_OK;
        };
        // Bricks whose 4096 leaves are one repeated code reduce to the same root.
        std::mutex memo_mu;
        std::unordered_map<uint32_t, std::pair<uint32_t, uint64_t>> memo;   // code -> (root, tree nodes)
        std::vector<std::vector<uint32_t>> ids(threads, std::vector<uint32_t>(kLeaves));
        const auto t0 = std::chrono::steady_clock::now();
        if (n_batches && launch(0) != OCH_OK) return OCH_E_HIP;
        double wait_s = 0.0, host_s = 0.0;
        size_t mixed = 0;
        for (size_t batch = 0; batch < n_batches; ++batch) {
            const int k = (int)(batch & 1);
            const auto w0 = std::chrono::steady_clock::now();
            GPU_TRY(hipEventSynchronize(done[k]));
            const auto w1 = std::chrono::steady_clock::now();
            wait_s += std::chrono::duration<double>(w1 - w0).count();
            // the other buffer is free: its batch was consumed in the previous round
            if (batch + 1 < n_batches && launch(batch + 1) != OCH_OK) return OCH_E_HIP;
            const size_t lo = batch * B, n = std::min(B, n_work - lo);
            const uint32_t *codes = h_codes[k], *info = h_info[k];
            parallel_for(threads, n, [&](uint64_t i, int t) {
                BuildStats &bs = stats[t];
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
                    BuildStats one;
                    std::vector<uint32_t> &id = ids[t];
                    const uint32_t leaf = uni ? ns.intern_code(uni) : 0;
                    std::fill(id.begin(), id.end(), leaf);
                    one.tree_nodes = uni ? (uint64_t)kLeaves : 0;
                    root = reduce_grid(ns, 1, kBrickLog2, id, one.tree_nodes);
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
                    root = reduce_grid(ns, 1, kBrickLog2, id, bs.tree_nodes);
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
        return OCH_OK;
    };
    const int status = run();
    cleanup();
    return status;
}

// The whole DAG on the current GPU: bricks voxelised (k_brick_codes) and
// interned batch by batch, then the levels above the bricks, then renumbered
// breadth-first (1-based).  *out: malloc'd n_out x 8 words, as renumber().
// Returns a status.
int build_dag_gpu(const Terrain &tr, uint32_t cap, const std::vector<uint32_t> &work, int G, uint32_t **out,
                  uint32_t *n_out, uint32_t &root, BuildStats &total, bool trace)
{
    GpuScope scope;
    if (const int os = scope.open()) return os;
    const hipStream_t st = scope.st;
    const size_t n_work = work.size();
    const size_t B = 8192;                                    // bricks per batch
    const size_t cols = (size_t)tr.dim * tr.dim, grid_cells = (size_t)G * G * G;
    const size_t rep_cap = std::max(B * 512, grid_cells / 8);
    int32_t *d_heights;
    uint8_t *d_tops;
    uint32_t *d_enc, *d_work, *d_codes, *d_info, *d_rep, *d_slot, *d_a, *d_b, *d_grid[2];
    if (!scope.alloc(&d_heights, cols * 4) || !scope.alloc(&d_tops, cols) || !scope.alloc(&d_enc, n_work * 4) ||
        !scope.alloc(&d_work, n_work * 4) || !scope.alloc(&d_codes, B * kLeaves * 4) || !scope.alloc(&d_info, n_work * 32) ||
        !scope.alloc(&d_rep, rep_cap * 4) || !scope.alloc(&d_slot, rep_cap * 4) || !scope.alloc(&d_a, B * 512 * 4) ||
        !scope.alloc(&d_b, B * 64 * 4) || !scope.alloc(&d_grid[0], grid_cells * 4) || !scope.alloc(&d_grid[1], grid_cells * 4))
        return OCH_E_NOMEM;
    GpuStore S;
    if (const int cs = gpu_store_create(scope, cap, true, S)) return cs;
    std::vector<uint32_t> enc(n_work);
    for (size_t i = 0; i < n_work; ++i) enc[i] = brick_code(work[i], G);
    GPU_TRY(hipMemcpyAsync(d_heights, tr.heights.data(), cols * 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(d_tops, tr.tops.data(), cols, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(d_enc, enc.data(), n_work * 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(d_work, work.data(), n_work * 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemsetAsync(d_grid[0], 0, grid_cells * 4, st));
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
        hipLaunchKernelGGL(k_intern_codes, blocks((size_t)n * kLeaves), dim3(256), 0, st, S, d_codes, n * (uint32_t)kLeaves);
        GPU_TRY(hipGetLastError());
        // brick levels 1..4: 8^3, 4^3, 2^3, 1 node per brick; the roots land in the grid
        if (!level_pass({d_codes, 1, 3, n * 512u, 1}, d_a, nullptr) || !level_pass({d_a, 0, 2, n * 64u, 2}, d_b, nullptr) ||
            !level_pass({d_b, 0, 1, n * 8u, 3}, d_a, nullptr) || !level_pass({d_a, 0, 0, n, 4}, d_grid[0], d_work + lo))
            return OCH_E_HIP;
    }
    // levels above the bricks, one grid of side G / 2, G / 4, ... 1
    int cur = 0, log2n = 0;
    while ((1 << (log2n + 1)) < G) ++log2n;   // G = 2^(log2n + 1)
    for (int h = kBrickLog2; h < tr.depth; ++h, --log2n) {
        if (!level_pass({d_grid[cur], 0, log2n, 1u << (3 * log2n), h}, d_grid[cur ^ 1], nullptr)) return OCH_E_HIP;
        cur ^= 1;
    }
    std::vector<unsigned long long> counts((size_t)16 * kCounters);
    GPU_TRY(hipMemcpyAsync(counts.data(), S.tree_nodes, counts.size() * 8, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipMemcpyAsync(&root, d_grid[cur], 4, hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> info(n_work * 8);
    GPU_TRY(hipMemcpyAsync(info.data(), d_info, n_work * 32, hipMemcpyDeviceToHost, st));
    uint32_t used = 0;
    if (const int us = gpu_store_used(S, st, &used)) return us;
    total.tree_nodes = 0;
    for (int k = 0; k < kCounters; ++k) total.tree_nodes += counts[(size_t)16 * k];
    for (size_t i = 0; i < n_work; ++i) {
        for (int v = 0; v < 6; ++v) total.hist[v] += info[i * 8 + 1 + v];
        total.tree_nodes += info[i * 8 + 7];
    }
    if (!root) return empty_pool(out, n_out, root);
    const int rs = renumber_gpu(S, used, root, tr.depth, scope, out, n_out, trace);
    if (rs == OCH_OK && trace) std::fprintf(stderr, "[och_build] gpu dag: %zu bricks, %u ids\n", n_work, used);
    return rs;
}

}  // namespace

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
    PhaseTimer phase{"", 3};
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
    BuildStats total;
    uint32_t root = 0, n_out = 0;
    uint32_t *nodes = nullptr;
    if (params->use_gpu && params->dedup && s_log2 == kBrickLog2) {
        // the whole DAG on the GPU, renumbering included
        const int st = build_dag_gpu(tr, cap, work, G, &nodes, &n_out, root, total, phase.on);
        if (st != OCH_OK) return report_build(st, "GPU builder", "device allocation failed");
        phase("gpu dag");
    } else {
        NodeStore ns;
        if (!ns.init(cap, params->dedup != 0)) {
            ns.release();
            return OCH_E_NOMEM;
        }
        std::vector<uint32_t> brick_root((size_t)G * G * G, 0);
        std::vector<BuildStats> stats(threads);
        double gpu_s = 0.0;
        if (params->use_gpu && s_log2 == kBrickLog2) {
            // an expanded tree: voxels from the GPU, one node per tree node on the host
            if (build_bricks_gpu(tr, ns, threads, work, G, brick_root, stats, &gpu_s) != OCH_OK) {
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
        // Levels above the bricks: the grid of brick roots, side G = 2^(depth - s_log2).
        root = reduce_grid(ns, s_log2, depth, brick_root, total.tree_nodes);
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
    for (int k = 1; k < 8; ++k) total.solid += total.hist[k];
    return finish_pool(out, nodes, n_out, root, base, depth, total, t_start);
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
    PhaseTimer phase{"voxels ", 4};
    std::memset(out, 0, sizeof *out);
    BuildStats vs;
    uint32_t root = 0, n_out = 0;
    uint32_t *nodes = nullptr;
    const int st = P.use_gpu ? build_voxels_gpu(P, &nodes, &n_out, root, vs)
                             : build_voxels_host(P, P.threads > 0 ? P.threads : default_threads(), &nodes, &n_out, root, vs, phase);
    if (st != OCH_OK) return report_build(st, "voxel builder", "allocation failed");
    phase(P.use_gpu ? "gpu, whole" : "renumber");
    return finish_pool(out, nodes, n_out, root, 1, P.depth, vs, t_start);
}

OCH_API int och_edit_voxels(const och_edit_params *params, och_host_pool *out)
{
    if (!params || !out) return och::report(OCH_E_INVALID, "och_edit_voxels: null argument");
    const och_edit_params &P = *params;
    if (P.depth < 1 || P.depth > kMaxVoxelDepth)
        return och::report(OCH_E_INVALID, "och_edit_voxels: depth must be 1..21 (a Morton key of 3 * depth bits and the "
                                          "out-of-range bit fill 64 bits)");
    if (P.n >= (1ull << 31)) return och::report(OCH_E_INVALID, "och_edit_voxels: a list holds fewer than 2^31 records");
    if (P.on_device && !P.use_gpu) return och::report(OCH_E_INVALID, "och_edit_voxels: device records need use_gpu = 1");
    if (!P.nodes && P.n_nodes) return och::report(OCH_E_INVALID, "och_edit_voxels: nodes is null");
    if (!P.records && P.n) return och::report(OCH_E_INVALID, "och_edit_voxels: records is null");
    if (P.root > P.n_nodes) return och::report(OCH_E_INVALID, "och_edit_voxels: root lies past the pool's end");
    const auto t_start = std::chrono::steady_clock::now();
    PhaseTimer phase{P.use_gpu ? "edit gpu " : "edit host ", 4};
    // *out is written only by finish_pool: a refused edit leaves it as it was
    BuildStats vs;
    uint32_t root = 0, n_out = 0;
    uint32_t *nodes = nullptr;
    const int st = P.use_gpu ? edit_voxels_gpu(P, &nodes, &n_out, root, vs)
                             : edit_voxels_host(P, P.threads > 0 ? P.threads : default_threads(), &nodes, &n_out, root, phase);
    if (st == OCH_E_INVALID) return st;   // reported where it was found
    if (st != OCH_OK) return report_build(st, "voxel editor", "allocation failed");
    phase(P.use_gpu ? "gpu, whole" : "renumber");
    if (!P.use_gpu) {
        pool_stats(nodes, n_out, root, P.depth, vs);
        phase("statistics");
    }
    return finish_pool(out, nodes, n_out, root, 1, P.depth, vs, t_start);
}
