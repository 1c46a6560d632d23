// och_voxel_build.h -- the voxel builder (och_build_voxels): the canonical DAG
// of och_dag.h from the caller's voxels, on the host (build_voxels_host) or on
// the GPU (build_voxels_gpu, the k_vox_* kernels).  Included by och_builder.cpp
// only, after och_dag.h, whose stores, kernels and renumbering it uses.
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
// dispatch workgroups meet only in the atomics (k_intern's rule, och_dag.h).
#pragma once
#include "och_dag.h"

namespace {

constexpr int kMaxVoxelDepth = 21;   // 3 * 21 key bits + the out-of-range bit = 64
constexpr int kBins = 32;            // level bins per counter row (>= kMaxVoxelDepth + 1)

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

int build_voxels_gpu(const och_voxel_params &P, uint32_t **out, uint32_t *n_out, uint32_t &root, BuildStats &vs)
{
    GpuScope G;
    if (const int os = G.open()) return os;
    const hipStream_t st = G.st;
    const int depth = P.depth;
    const bool list = P.kind == OCH_VOXELS_LIST;
    const uint32_t n = list ? (uint32_t)P.n : 1u << (3 * depth);
    const size_t in_bytes = list ? (size_t)n * 16 : (size_t)n * (P.kind == OCH_VOXELS_GRID_U8 ? 1 : 4);
    if (n == 0) return empty_pool(out, n_out, root);
    PhaseTimer phase{"voxels gpu ", 4, st};
    const void *d_in = P.data;
    if (!P.on_device) {
        void *up;
        if (!G.alloc(&up, in_bytes)) return OCH_E_NOMEM;
        GPU_TRY(hipMemcpyAsync(up, P.data, in_bytes, hipMemcpyHostToDevice, st));
        d_in = up;
    }
    uint64_t *d_keys[2] = {nullptr, nullptr};
    uint32_t *d_words[2] = {nullptr, nullptr}, *d_flags, *d_pos, *d_ids, *d_bins;
    unsigned long long *d_counters;
    const size_t bins_bytes = (size_t)kCounters * kBins * 4, counters_bytes = (size_t)kCounters * 128;
    if (!G.alloc(&d_flags, (size_t)n * 4) || !G.alloc(&d_pos, (size_t)n * 4) || !G.alloc(&d_ids, (size_t)n * 4) ||
        !G.alloc(&d_bins, bins_bytes) || !G.alloc(&d_counters, counters_bytes))
        return OCH_E_NOMEM;
    if (list && (!G.alloc(&d_keys[0], (size_t)n * 8) || !G.alloc(&d_keys[1], (size_t)n * 8) ||
                 !G.alloc(&d_words[0], (size_t)n * 4) || !G.alloc(&d_words[1], (size_t)n * 4)))
        return OCH_E_NOMEM;
    const int key_bits = std::min(64, 3 * depth + 1);
    size_t sort_bytes = 0, scan_bytes = 0;
    if (list)
        GPU_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_keys[0], d_keys[1], d_words[0], d_words[1], (int)n,
                                                   0, key_bits, st));
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, d_flags, d_pos, (int)n, st));
    const size_t temp_bytes = std::max(sort_bytes, scan_bytes);
    void *d_temp;
    if (!G.alloc(&d_temp, temp_bytes)) return OCH_E_NOMEM;
    GPU_TRY(hipMemsetAsync(d_bins, 0, bins_bytes, st));
    GPU_TRY(hipMemsetAsync(d_counters, 0, counters_bytes, st));
    if (!phase("upload")) return OCH_E_HIP;
    const uint64_t *d_sorted = nullptr;
    if (list) {
        const uint32_t *recs = static_cast<const uint32_t *>(d_in);
        hipLaunchKernelGGL(k_vox_keys, blocks(n), dim3(256), 0, st, recs, n, depth, d_keys[0], d_words[0]);
        GPU_TRY(hipGetLastError());
        size_t tb = temp_bytes;
        GPU_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp, tb, d_keys[0], d_keys[1], d_words[0], d_words[1], (int)n, 0,
                                                   key_bits, st));
        if (!phase("sort")) return OCH_E_HIP;
        hipLaunchKernelGGL(k_vox_last, blocks(n), dim3(256), 0, st, d_keys[1], d_words[1], recs, n, depth, d_flags, d_ids,
                           d_counters);
        d_sorted = d_keys[1];
    } else if (P.kind == OCH_VOXELS_GRID_U8) {
        hipLaunchKernelGGL(k_vox_cells<uint8_t>, blocks(n), dim3(256), 0, st, static_cast<const uint8_t *>(d_in), n, depth,
                           d_flags, d_ids, d_counters);
    } else {
        hipLaunchKernelGGL(k_vox_cells<uint32_t>, blocks(n), dim3(256), 0, st, static_cast<const uint32_t *>(d_in), n, depth,
                           d_flags, d_ids, d_counters);
    }
    GPU_TRY(hipGetLastError());
    size_t tb = temp_bytes;
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(d_temp, tb, d_flags, d_pos, (int)n, st));
    uint32_t m = 0;
    GPU_TRY(hipMemcpyAsync(&m, d_pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipStreamSynchronize(st));
    if (m == 0) return empty_pool(out, n_out, root);
    // a list packs into the sort's input buffers (free by now) and the levels
    // alternate with its output buffers; a grid's are sized by its voxels
    if (!list && (!G.alloc(&d_keys[0], (size_t)m * 8) || !G.alloc(&d_keys[1], (size_t)m * 8) ||
                  !G.alloc(&d_words[0], (size_t)m * 4) || !G.alloc(&d_words[1], (size_t)m * 4)))
        return OCH_E_NOMEM;
    hipLaunchKernelGGL(k_vox_compact, blocks(n), dim3(256), 0, st, d_sorted, d_flags, d_pos, d_ids, n, d_keys[0], d_words[0]);
    hipLaunchKernelGGL(k_vox_levels, blocks(m), dim3(256), 0, st, d_keys[0], m, depth, d_bins);
    GPU_TRY(hipGetLastError());
    std::vector<uint32_t> h_bins((size_t)kCounters * kBins);
    std::vector<unsigned long long> h_counters((size_t)kCounters * 16);
    GPU_TRY(hipMemcpyAsync(h_bins.data(), d_bins, bins_bytes, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipMemcpyAsync(h_counters.data(), d_counters, counters_bytes, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipStreamSynchronize(st));
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
    uint32_t *d_rows, *d_rep, *d_slot;
    if (!G.alloc(&d_rows, (size_t)rows_max * 32) || !G.alloc(&d_rep, (size_t)rows_max * 4) ||
        !G.alloc(&d_slot, (size_t)rows_max * 4))
        return OCH_E_NOMEM;
    GpuStore S;
    if (const int cs = gpu_store_create(G, voxel_capacity(P.capacity, vs.tree_nodes), false, S)) return cs;
    int cur = 0;
    uint32_t n_in = m;
    for (int h = 0; h < depth; ++h) {
        const uint32_t n_rows = (uint32_t)counts[h];
        hipLaunchKernelGGL(k_vox_heads, blocks(n_in), dim3(256), 0, st, d_keys[cur], n_in, d_flags);
        GPU_TRY(hipGetLastError());
        tb = temp_bytes;
        GPU_TRY(hipcub::DeviceScan::InclusiveSum(d_temp, tb, d_flags, d_pos, (int)n_in, st));
        GPU_TRY(hipMemsetAsync(d_rows, 0, (size_t)n_rows * 32, st));
        hipLaunchKernelGGL(k_vox_rows, blocks(n_in), dim3(256), 0, st, d_keys[cur], d_words[cur], n_in, d_flags, d_pos, n_rows,
                           d_rows, d_keys[cur ^ 1], S.overflow);
        GpuLevel L{d_rows, 0, 0, n_rows, h, 1};
        hipLaunchKernelGGL(k_intern_rows<false>, blocks(n_rows), dim3(256), 0, st, S, L, d_rep, d_slot);
        hipLaunchKernelGGL(k_settle, blocks(n_rows), dim3(256), 0, st, S, n_rows, d_rep, d_slot, d_words[cur ^ 1], nullptr);
        GPU_TRY(hipGetLastError());
        cur ^= 1;
        n_in = n_rows;
    }
    uint32_t used = 0;
    GPU_TRY(hipMemcpyAsync(&root, d_words[cur], 4, hipMemcpyDeviceToHost, st));
    const int us = gpu_store_used(S, st, &used);
    if (!phase("levels")) return OCH_E_HIP;
    if (us != OCH_OK) return us;
    if (!root) return OCH_E_CAPACITY;
    const int rs = renumber_gpu(S, used, root, depth, G, out, n_out, phase.on);
    if (rs == OCH_OK && phase.on)
        std::fprintf(stderr, "[och_build] voxels gpu: %u entries, %u voxels, %u ids of %u\n", n, m, used - 1, S.cap - 1);
    return rs;
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
                      BuildStats &vs, PhaseTimer &phase)
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
    if (m == 0) return empty_pool(out, n_out, root);
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
