// och_voxel_edit.h -- the batch editor (och_edit_voxels): the canonical DAG of
// an existing pool's voxels after a list of set() records, on the host
// (edit_voxels_host) or on the GPU (edit_voxels_gpu, the k_edit_* kernels).
// Included by och_builder.cpp only, after och_voxel_build.h, whose keys, sort,
// level counts and row-per-parent level loop it uses over och_dag.h's stores.
// och_world.h, included after this file, runs the GPU path's steps over a store
// that stays on the device between calls.
//
// The voxel builder's rows start from zeros; an edit's rows start from the old
// tree.  Host and GPU run the same steps:
//   reach     -- breadth-first from the caller's root, one pass per depth:
//                each depth's distinct nodes.  Every child word of an interior
//                node is compared with n_nodes before it is used as an index;
//                a word past the end, or a node met at two depths (a cycle is
//                one), refuses the pool.  Nothing unreachable is read.
//   records   -- keys, stable sort and last-wins as the builder, but a kept
//                id 0 stays in the list: it is a removal, not nothing.  The
//                level counts of these unique keys size the level loop and,
//                with the reachable nodes, the store.
//   adopt     -- bottom-up, one depth at a time: a node's row is its eight
//                words, interior words mapped old id -> store id; the row is
//                interned and its id becomes map[old id].  A row of zeros (an
//                all-zero node, or one whose children all mapped to 0) is no
//                node: id 0.  Duplicates of the caller's pool meet here.
//   levels    -- h = 0 .. depth - 1: a row is the old node on the path of its
//                parent key (walked down the store from the adopted root;
//                zeros where the path leaves the old tree) overlaid with its
//                entries' words, zeros included.  An empty row gets id 0 and
//                never probes the table; ids, zeros included, are the next
//                level's child words, so an emptied node empties its parents.
//   renumber  -- breadth-first from the top row's id (0: the empty pool); what
//                the old tree no longer shares with the new one drops out here.
//   statistics -- over the renumbered pool, top-down, one depth at a time:
//                paths[node] = the root paths that reach it; their sum is the
//                expanded tree's nodes, and a leaf-level word counts paths
//                voxels (pool_stats, pool_stats_gpu).
// On the GPU each step is its own dispatch and k_intern's rule (och_dag.h)
// holds: rows, keys, map[] and node records are read only by later dispatches
// than the one that wrote them; within a dispatch workgroups meet only in the
// atomics (the table, the id counter, reach's placed[] claims and its append,
// the statistics' paths[] of the next depth).
#pragma once
#include "och_voxel_build.h"

namespace {

// The expanded tree's nodes and the voxel counts of a renumbered (breadth-
// first, 1-based, root 1) pool: levels are contiguous and a level's children
// follow it, so one pass in id order sees every node after all its parents.
void pool_stats(const uint32_t *nodes, uint32_t n, uint32_t root, int depth, BuildStats &vs)
{
    if (!root) return;
    std::vector<uint64_t> paths((size_t)n + 1, 0);
    paths[1] = 1;
    uint32_t lo = 1, hi = 2;
    for (int l = 0; l < depth; ++l) {
        uint32_t next_hi = hi;
        for (uint32_t id = lo; id < hi; ++id) {
            const uint64_t p = paths[id];
            const uint32_t *c = nodes + (size_t)(id - 1) * 8;
            vs.tree_nodes += p;
            for (int k = 0; k < 8; ++k) {
                if (!c[k]) continue;
                if (l == depth - 1) {
                    vs.solid += p;
                    if (c[k] < 8) vs.hist[c[k]] += p;
                } else {
                    paths[c[k]] += p;
                    next_hi = std::max(next_hi, c[k] + 1);
                }
            }
        }
        lo = hi;
        hi = next_hi;
    }
}

// Child index under the node at height H on the way to the node of key pk at height h < H.
__host__ __device__ inline uint32_t path_child(uint64_t pk, int H, int h) { return (uint32_t)(pk >> (3 * (H - 1 - h))) & 7u; }

const char *kBadChild = "och_edit_voxels: an interior node's child word lies past the pool's end";
const char *kTwoHeights = "och_edit_voxels: a node is reachable at two heights (or the pool has a cycle)";

// ------------------------------------------------------------ GPU kernels

// One depth of the reach: candidate q = 8 i + k is child k of front[i].  A
// child's first claim of placed[] (tag = its depth + 1) appends it to next[];
// head[0] = the appended, head[1] |= 1 a word past the end, 2 a node at two depths.
__global__ __launch_bounds__(256) void k_edit_reach(const uint32_t *__restrict__ pool, uint32_t n_nodes,
                                                    const uint32_t *__restrict__ front, uint32_t f, uint32_t tag,
                                                    uint32_t *__restrict__ placed, uint32_t *__restrict__ next,
                                                    uint32_t *__restrict__ head)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    bool won = false;
    if (q < (size_t)f * 8) {
        c = pool[(size_t)(front[q >> 3] - 1u) * 8 + (q & 7u)];
        if (c > n_nodes) {   // checked before any use as an index
            atomicOr(head + 1, 1u);
            c = 0;
        }
        if (c) {
            uint32_t p = placed[c];   // 0 -> tag once: a cached non-zero is final, a stale 0 meets the CAS
            if (!p) {
                p = atomicCAS(&placed[c], 0u, tag);
                won = p == 0;
            }
            if (!won && p != tag) atomicOr(head + 1, 2u);
        }
    }
    // one append per wavefront
    const uint64_t b = __ballot(won);
    if (!b) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = __ffsll((unsigned long long)b) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(head, (uint32_t)__popcll(b));
    base = __shfl(base, leader);
    if (won) next[base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = c;
}

// The rows of one depth's nodes: word q = 8 i + k of list[i], interior words through map[].
__global__ __launch_bounds__(256) void k_edit_adopt_rows(const uint32_t *__restrict__ pool, uint32_t n_nodes,
                                                         const uint32_t *__restrict__ list, uint32_t count, int interior,
                                                         const uint32_t *__restrict__ map, uint32_t *__restrict__ rows)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)count * 8) return;
    uint32_t w = pool[(size_t)(list[q >> 3] - 1u) * 8 + (q & 7u)];
    if (interior && w) w = w <= n_nodes ? map[w] : 0u;   // the reach refused a word past the end already
    rows[q] = w;
}

// Last wins, zeros kept: flags[i] = entry i is the last of a key inside the tree, ids[i] = its id.
__global__ __launch_bounds__(256) void k_edit_last(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   const uint32_t *__restrict__ recs, uint32_t n, int depth,
                                                   uint32_t *__restrict__ flags, uint32_t *__restrict__ ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const bool keep = !(key >> (3 * depth)) && (i + 1 == n || keys[i + 1] != key);
    flags[i] = keep;
    ids[i] = keep ? recs[(size_t)vals[i] * 4 + 3] : 0u;
}

// The row of every head entry i (node = pos[i] - 1, parent key pk): the old
// node at pk, reached from *old_root down the store, with the words of the
// entries of pk (at most eight, side by side from i) laid over it.
__global__ __launch_bounds__(256) void k_edit_rows(GpuStore S, const uint32_t *__restrict__ old_root,
                                                   const uint64_t *__restrict__ keys, const uint32_t *__restrict__ words,
                                                   uint32_t n, const uint32_t *__restrict__ flags,
                                                   const uint32_t *__restrict__ pos, uint32_t n_rows, int depth, int h,
                                                   uint32_t *__restrict__ rows, uint64_t *__restrict__ parents)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const uint32_t node = pos[i] - 1u;
    if (node >= n_rows) {   // the level counts size the rows: never, unless they are wrong
        atomicOr(S.overflow, 4u);
        return;
    }
    const uint64_t pk = keys[i] >> 3;
    uint32_t cur = *old_root;
    for (int H = depth - 1; H > h && cur; --H) cur = S.nodes[(size_t)cur * 8 + path_child(pk, H, h)];
    const uint4 *rec = reinterpret_cast<const uint4 *>(S.nodes + (size_t)cur * 8);   // id 0 is the zero node
    const uint4 a = rec[0], b = rec[1];
    uint32_t c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    for (uint32_t j = i; j < n && j < i + 8u && (keys[j] >> 3) == pk; ++j) {
        const uint32_t at = (uint32_t)keys[j] & 7u, w = words[j];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) c[k] = at == k ? w : c[k];
    }
    uint4 *row = reinterpret_cast<uint4 *>(rows + (size_t)node * 8);
    row[0] = make_uint4(c[0], c[1], c[2], c[3]);
    row[1] = make_uint4(c[4], c[5], c[6], c[7]);
    parents[node] = pk;
}

// The sum of v over a wavefront, in every lane.
__device__ inline unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One depth of the statistics: word q = 8 i + k of node lo + i of the renumbered
// pool.  paths[] of this depth is complete (an earlier dispatch's atomics); an
// interior word adds it to its child's, a leaf-level word counts as that many
// voxels.  counters: kCounters rows of 16, [0] = tree nodes, [1..7] = voxels
// per id, [8] = voxels of any id.  A shared child (solid stone) is named by
// millions of words, and one address's atomics serialise: the words of a
// wavefront that name one child add up in registers and go out as one atomic,
// child after child until none is pending (at most 64 rounds of a few
// instructions); the counters take one sum per wavefront in the same way.
__global__ __launch_bounds__(256) void k_edit_paths(const uint32_t *__restrict__ pool, uint32_t lo, uint32_t count, int leaf,
                                                    unsigned long long *__restrict__ paths,
                                                    unsigned long long *__restrict__ counters)
{
    __shared__ unsigned long long acc[9];
    if (threadIdx.x < 9) acc[threadIdx.x] = 0;
    __syncthreads();
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long p = 0;
    uint32_t c = 0;
    bool first_word = false;
    if (q < (size_t)count * 8) {
        const uint32_t id = lo + (uint32_t)(q >> 3);
        first_word = (q & 7u) == 0;
        p = paths[id];
        c = pool[(size_t)(id - 1u) * 8 + (q & 7u)];
    }
    unsigned long long sums[9] = {wave_sum(first_word ? p : 0ull), 0, 0, 0, 0, 0, 0, 0, 0};
    if (leaf) {   // the same in every lane
        sums[8] = wave_sum(c ? p : 0ull);
#pragma unroll
        for (uint32_t id = 1; id < 8; ++id) sums[id] = wave_sum(c == id ? p : 0ull);
    } else {
        bool pending = c != 0;
        for (uint64_t todo = __ballot(pending); todo; todo = __ballot(pending)) {
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const uint32_t child = __shfl(c, lead);
            const bool mine = pending && c == child;
            const unsigned long long sum = wave_sum(mine ? p : 0ull);
            if ((int)lane == lead) atomicAdd(&paths[child], sum);
            pending = pending && !mine;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (sums[k]) atomicAdd(&acc[k], sums[k]);
    }
    __syncthreads();
    if (threadIdx.x < 9 && acc[threadIdx.x])
        atomicAdd(counters + 16 * (blockIdx.x % kCounters) + threadIdx.x, acc[threadIdx.x]);
}

// pool_stats on the device, over the pool renumber_gpu left there (n nodes).
int pool_stats_gpu(GpuScope &G, const DevicePool &dev, uint32_t n, int depth, BuildStats &vs)
{
    const hipStream_t st = G.st;
    unsigned long long *d_paths, *d_counters;
    const size_t counters_bytes = (size_t)kCounters * 128;
    if (!G.alloc(&d_paths, ((size_t)n + 1) * 8) || !G.alloc(&d_counters, counters_bytes)) return OCH_E_NOMEM;
    const unsigned long long one = 1;
    GPU_TRY(hipMemsetAsync(d_paths, 0, ((size_t)n + 1) * 8, st));
    GPU_TRY(hipMemsetAsync(d_counters, 0, counters_bytes, st));
    GPU_TRY(hipMemcpyAsync(d_paths + 1, &one, 8, hipMemcpyHostToDevice, st));
    uint32_t lo = 1;
    for (size_t l = 0; l < dev.level_counts.size(); ++l) {
        const uint32_t cnt = dev.level_counts[l];
        if (!cnt || lo + (uint64_t)cnt > (uint64_t)n + 1) break;   // the levels partition ids 1 .. n
        hipLaunchKernelGGL(k_edit_paths, blocks((size_t)cnt * 8), dim3(256), 0, st, dev.nodes, lo, cnt,
                           (int)l == depth - 1 ? 1 : 0, d_paths, d_counters);
        GPU_TRY(hipGetLastError());
        lo += cnt;
    }
    std::vector<unsigned long long> h((size_t)kCounters * 16);
    GPU_TRY(hipMemcpyAsync(h.data(), d_counters, counters_bytes, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < kCounters; ++r) {
        vs.tree_nodes += h[(size_t)r * 16];
        for (int k = 1; k < 8; ++k) vs.hist[k] += h[(size_t)r * 16 + k];
        vs.solid += h[(size_t)r * 16 + 8];
    }
    return OCH_OK;
}

// ------------------------------------------------------------ GPU path
//
// In the steps och_edit_voxels (edit_voxels_gpu) and a resident world
// (och_world.h) share: upload + reach + adopt bring a caller's pool into a
// store, records + levels apply one list of records to a store.

// A caller's pool on the device: its nodes, each depth's distinct nodes
// (d_order[lv_off[l], + lv_cnt[l]), each id placed once: <= n_nodes in all)
// and, after edit_adopt, d_map[old id] = store id.
struct EditReach {
    uint32_t *d_pool = nullptr, *d_placed = nullptr, *d_map = nullptr, *d_order = nullptr, *d_head = nullptr;
    uint32_t n_nodes = 0, root = 0;
    uint32_t lv_off[kMaxVoxelDepth + 1] = {0}, lv_cnt[kMaxVoxelDepth + 1] = {0};
    uint64_t reach = 0;   // the distinct reachable nodes

    uint32_t widest() const { return *std::max_element(lv_cnt, lv_cnt + kMaxVoxelDepth + 1); }
};

// The work buffers of the records phase (n_cap records) and of a level loop (rows_cap rows).
struct EditWork {
    uint64_t *keys[2] = {nullptr, nullptr};
    uint32_t *words[2] = {nullptr, nullptr}, *flags = nullptr, *pos = nullptr, *ids = nullptr, *bins = nullptr;
    void *temp = nullptr;
    size_t temp_bytes = 0;
    uint32_t n_cap = 0;
    uint32_t *rows = nullptr, *rep = nullptr, *slot = nullptr;
    uint32_t rows_cap = 0;
};

// The reach's and the adoption's arrays for a pool of n_nodes, nothing placed
// yet.  `upload`: the caller's host pool, which gets its device copy here;
// nullptr: R.d_pool is set already (a world's store).  The pool's allocation
// comes first and its copy between the allocations and the clears: the order
// och_edit_voxels always had (every hipMalloc ahead of the large pageable copy).
int edit_reach_arrays(GpuScope &G, EditReach &R, uint32_t n_nodes, uint32_t root, const uint32_t *upload)
{
    const hipStream_t st = G.st;
    R.n_nodes = n_nodes;
    R.root = root;
    if ((upload && !G.alloc(&R.d_pool, (size_t)n_nodes * 32)) || !G.alloc(&R.d_placed, ((size_t)n_nodes + 1) * 4) ||
        !G.alloc(&R.d_map, ((size_t)n_nodes + 1) * 4) || !G.alloc(&R.d_order, (size_t)n_nodes * 4) || !G.alloc(&R.d_head, 8))
        return OCH_E_NOMEM;
    if (upload && n_nodes) GPU_TRY(hipMemcpyAsync(R.d_pool, upload, (size_t)n_nodes * 32, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemsetAsync(R.d_placed, 0, ((size_t)n_nodes + 1) * 4, st));
    GPU_TRY(hipMemsetAsync(R.d_map, 0, 4, st));   // map[0]: the adopted root of a world without voxels
    GPU_TRY(hipMemsetAsync(R.d_head, 0, 8, st));
    return OCH_OK;
}

int edit_upload(GpuScope &G, EditReach &R, const uint32_t *nodes, uint32_t n_nodes, uint32_t root)
{
    static const uint32_t none[8] = {0};   // a pool of no nodes still names one to upload from
    return edit_reach_arrays(G, R, n_nodes, root, nodes ? nodes : none);
}

// The reach below depth 0, whose R.lv_cnt[0] distinct nodes stand in d_order with placed[] = 1.
int edit_reach_levels(hipStream_t st, EditReach &R, int depth)
{
    for (int l = 0; l + 1 < depth && R.lv_cnt[l]; ++l) {
        uint32_t head[2] = {0, 0};
        R.lv_off[l + 1] = R.lv_off[l] + R.lv_cnt[l];
        hipLaunchKernelGGL(k_edit_reach, blocks((size_t)R.lv_cnt[l] * 8), dim3(256), 0, st, R.d_pool, R.n_nodes,
                           R.d_order + R.lv_off[l], R.lv_cnt[l], (uint32_t)l + 2u, R.d_placed, R.d_order + R.lv_off[l + 1],
                           R.d_head);
        GPU_TRY(hipGetLastError());
        GPU_TRY(hipMemcpyAsync(head, R.d_head, 8, hipMemcpyDeviceToHost, st));
        GPU_TRY(hipMemsetAsync(R.d_head, 0, 4, st));
        GPU_TRY(hipStreamSynchronize(st));
        if (head[1]) return och::report(OCH_E_INVALID, head[1] & 1u ? kBadChild : kTwoHeights);
        R.lv_cnt[l + 1] = head[0];
    }
    for (int l = 0; l < depth; ++l) R.reach += R.lv_cnt[l];
    return OCH_OK;
}

int edit_reach(hipStream_t st, EditReach &R, int depth)
{
    if (!R.root) return OCH_OK;
    const uint32_t first_tag = 1;
    GPU_TRY(hipMemcpyAsync(R.d_order, &R.root, 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(R.d_placed + R.root, &first_tag, 4, hipMemcpyHostToDevice, st));
    R.lv_cnt[0] = 1;
    return edit_reach_levels(st, R, depth);
}

// Adopt, leaf level first: map[old id] = store id; W holds rows for the widest depth.
int edit_adopt(hipStream_t st, const EditReach &R, const GpuStore &S, const EditWork &W, int depth)
{
    for (int l = depth - 1; l >= 0; --l) {
        const uint32_t cnt = R.lv_cnt[l];
        if (!cnt) continue;
        const int h = depth - 1 - l;
        hipLaunchKernelGGL(k_edit_adopt_rows, blocks((size_t)cnt * 8), dim3(256), 0, st, R.d_pool, R.n_nodes,
                           R.d_order + R.lv_off[l], cnt, h > 0 ? 1 : 0, R.d_map, W.rows);
        GpuLevel L{W.rows, 0, 0, cnt, h, 1};
        hipLaunchKernelGGL(k_intern_rows<true>, blocks(cnt), dim3(256), 0, st, S, L, W.rep, W.slot);
        hipLaunchKernelGGL(k_settle, blocks(cnt), dim3(256), 0, st, S, cnt, W.rep, W.slot, R.d_map, R.d_order + R.lv_off[l]);
        GPU_TRY(hipGetLastError());
    }
    return OCH_OK;
}

// What the sort and the scans of n records need as temporary storage.
int edit_temp_bytes(uint32_t n, int depth, hipStream_t st, size_t *bytes)
{
    uint64_t *k = nullptr;
    uint32_t *w = nullptr;
    size_t sort_bytes = 0, scan_bytes = 0;
    GPU_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k, k, w, w, (int)n, 0, std::min(64, 3 * depth + 1), st));
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, w, w, (int)n, st));
    *bytes = std::max(sort_bytes, scan_bytes);
    return OCH_OK;
}

int edit_work_records(GpuScope &G, EditWork &W, uint32_t n, int depth)
{
    if (const int ts = edit_temp_bytes(n, depth, G.st, &W.temp_bytes)) return ts;
    if (!G.alloc(&W.flags, (size_t)n * 4) || !G.alloc(&W.pos, (size_t)n * 4) || !G.alloc(&W.ids, (size_t)n * 4) ||
        !G.alloc(&W.bins, (size_t)kCounters * kBins * 4) || !G.alloc(&W.keys[0], (size_t)n * 8) ||
        !G.alloc(&W.keys[1], (size_t)n * 8) || !G.alloc(&W.words[0], (size_t)n * 4) || !G.alloc(&W.words[1], (size_t)n * 4) ||
        !G.alloc(&W.temp, W.temp_bytes))
        return OCH_E_NOMEM;
    W.n_cap = n;
    return OCH_OK;
}

int edit_work_rows(GpuScope &G, EditWork &W, uint32_t rows)
{
    if (!G.alloc(&W.rows, (size_t)rows * 32) || !G.alloc(&W.rep, (size_t)rows * 4) || !G.alloc(&W.slot, (size_t)rows * 4))
        return OCH_E_NOMEM;
    W.rows_cap = rows;
    return OCH_OK;
}

// records: the unique in-range keys of recs[n] (device memory, 0 < n <= W.n_cap),
// zeros kept, packed into W.keys[0] / W.words[0]; m = how many, counts[h] = the
// rows of level h (all 0 when m is), rows_total their sum.
int edit_records(hipStream_t st, const EditWork &W, const uint32_t *recs, uint32_t n, int depth, PhaseTimer &phase,
                 uint32_t &m, uint64_t *counts, uint64_t &rows_total)
{
    const size_t bins_bytes = (size_t)kCounters * kBins * 4;
    const int key_bits = std::min(64, 3 * depth + 1);
    GPU_TRY(hipMemsetAsync(W.bins, 0, bins_bytes, st));
    hipLaunchKernelGGL(k_vox_keys, blocks(n), dim3(256), 0, st, recs, n, depth, W.keys[0], W.words[0]);
    GPU_TRY(hipGetLastError());
    size_t tb = W.temp_bytes;
    GPU_TRY(hipcub::DeviceRadixSort::SortPairs(W.temp, tb, W.keys[0], W.keys[1], W.words[0], W.words[1], (int)n, 0, key_bits,
                                               st));
    if (!phase("sort")) return OCH_E_HIP;
    hipLaunchKernelGGL(k_edit_last, blocks(n), dim3(256), 0, st, W.keys[1], W.words[1], recs, n, depth, W.flags, W.ids);
    GPU_TRY(hipGetLastError());
    tb = W.temp_bytes;
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(W.temp, tb, W.flags, W.pos, (int)n, st));
    GPU_TRY(hipMemcpyAsync(&m, W.pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
    GPU_TRY(hipStreamSynchronize(st));
    if (m) {
        hipLaunchKernelGGL(k_vox_compact, blocks(n), dim3(256), 0, st, W.keys[1], W.flags, W.pos, W.ids, n, W.keys[0],
                           W.words[0]);
        hipLaunchKernelGGL(k_vox_levels, blocks(m), dim3(256), 0, st, W.keys[0], m, depth, W.bins);
        GPU_TRY(hipGetLastError());
        std::vector<uint32_t> h_bins((size_t)kCounters * kBins);
        GPU_TRY(hipMemcpyAsync(h_bins.data(), W.bins, bins_bytes, hipMemcpyDeviceToHost, st));
        GPU_TRY(hipStreamSynchronize(st));
        uint64_t bins[kBins] = {0};
        for (int r = 0; r < kCounters; ++r)
            for (int t = 0; t < kBins; ++t) bins[t] += h_bins[(size_t)r * kBins + t];
        rows_total = level_counts(bins, depth, counts);
        if (counts[0] > m || counts[depth - 1] != 1)
            return och::report(OCH_E_HIP, "GPU voxel editor: inconsistent level counts");
    }
    if (!phase("last wins")) return OCH_E_HIP;
    return OCH_OK;
}

// levels: the m keys edit_records left in W, level by level over the store S
// from *d_old_root (device memory); *d_root names the device word that holds
// the new root (d_old_root itself when m is 0).  W.rows_cap >= counts[0].
int edit_levels(hipStream_t st, const EditWork &W, const GpuStore &S, const uint32_t *d_old_root, uint32_t m,
                const uint64_t *counts, int depth, const uint32_t **d_root)
{
    int cur = 0;
    uint32_t n_in = m;
    for (int h = 0; h < depth && m; ++h) {
        const uint32_t n_rows = (uint32_t)counts[h];
        hipLaunchKernelGGL(k_vox_heads, blocks(n_in), dim3(256), 0, st, W.keys[cur], n_in, W.flags);
        GPU_TRY(hipGetLastError());
        size_t tb = W.temp_bytes;
        GPU_TRY(hipcub::DeviceScan::InclusiveSum(W.temp, tb, W.flags, W.pos, (int)n_in, st));
        hipLaunchKernelGGL(k_edit_rows, blocks(n_in), dim3(256), 0, st, S, d_old_root, W.keys[cur], W.words[cur], n_in, W.flags,
                           W.pos, n_rows, depth, h, W.rows, W.keys[cur ^ 1]);
        GpuLevel L{W.rows, 0, 0, n_rows, h, 1};
        hipLaunchKernelGGL(k_intern_rows<true>, blocks(n_rows), dim3(256), 0, st, S, L, W.rep, W.slot);
        hipLaunchKernelGGL(k_settle, blocks(n_rows), dim3(256), 0, st, S, n_rows, W.rep, W.slot, W.words[cur ^ 1], nullptr);
        GPU_TRY(hipGetLastError());
        cur ^= 1;
        n_in = n_rows;
    }
    *d_root = m ? W.words[cur] : d_old_root;
    return OCH_OK;
}

int edit_voxels_gpu(const och_edit_params &P, uint32_t **out, uint32_t *n_out, uint32_t &root, BuildStats &vs)
{
    GpuScope G;
    if (const int os = G.open()) return os;
    const hipStream_t st = G.st;
    const int depth = P.depth;
    const uint32_t n = (uint32_t)P.n;
    PhaseTimer phase{"edit gpu ", 4, st};
    EditReach R;
    if (const int us = edit_upload(G, R, P.nodes, P.n_nodes, P.root)) return us;
    const void *d_in = P.records;
    if (n && !P.on_device) {
        void *up;
        if (!G.alloc(&up, (size_t)n * 16)) return OCH_E_NOMEM;
        GPU_TRY(hipMemcpyAsync(up, P.records, (size_t)n * 16, hipMemcpyHostToDevice, st));
        d_in = up;
    }
    if (!phase("upload")) return OCH_E_HIP;
    if (const int rs = edit_reach(st, R, depth)) return rs;
    if (!phase("reach")) return OCH_E_HIP;

    EditWork W;
    uint32_t m = 0;
    uint64_t counts[kMaxVoxelDepth] = {0}, rows_total = 0;
    if (n) {
        if (const int ws = edit_work_records(G, W, n, depth)) return ws;
        if (const int es = edit_records(st, W, static_cast<const uint32_t *>(d_in), n, depth, phase, m, counts, rows_total))
            return es;
    }
    // counts only shrink towards the root
    if (const int ws = edit_work_rows(G, W, std::max((uint32_t)counts[0], R.widest()))) return ws;
    GpuStore S;
    if (const int cs = gpu_store_create(G, voxel_capacity(P.capacity, R.reach + rows_total), false, S)) return cs;
    if (const int as = edit_adopt(st, R, S, W, depth)) return as;
    if (!phase("adopt")) return OCH_E_HIP;

    const uint32_t *d_root = nullptr;
    if (const int ls = edit_levels(st, W, S, R.d_map + P.root, m, counts, depth, &d_root)) return ls;
    uint32_t used = 0;
    GPU_TRY(hipMemcpyAsync(&root, d_root, 4, hipMemcpyDeviceToHost, st));
    const int us = gpu_store_used(S, st, &used);
    if (!phase("levels")) return OCH_E_HIP;
    if (us != OCH_OK) return us;
    if (!root) return empty_pool(out, n_out, root);
    DevicePool dev;
    if (const int rs = renumber_gpu(S, used, root, depth, G, out, n_out, phase.on, &dev)) return rs;
    if (!phase("renumber")) return OCH_E_HIP;
    if (const int ss = pool_stats_gpu(G, dev, *n_out, depth, vs)) {
        std::free(*out);
        *out = nullptr;
        return ss;
    }
    if (!phase("statistics")) return OCH_E_HIP;
    if (phase.on)
        std::fprintf(stderr, "[och_build] edit gpu: %llu old nodes, %u records, %u keys, %u ids of %u\n",
                     (unsigned long long)R.reach, n, m, used - 1, S.cap - 1);
    return OCH_OK;
}

// ------------------------------------------------------------ host path

int edit_voxels_host(const och_edit_params &P, int threads, uint32_t **out, uint32_t *n_out, uint32_t &root,
                     PhaseTimer &phase)
{
    const int depth = P.depth;
    const uint32_t n_nodes = P.n_nodes;
    auto old_node = [&](uint32_t id) { return P.nodes + (size_t)(id - 1) * 8; };

    // reach
    std::vector<std::vector<uint32_t>> lv(depth);
    uint64_t reach = 0;
    if (P.root) {
        std::vector<uint8_t> placed((size_t)n_nodes + 1, 0);   // depth + 1
        lv[0].push_back(P.root);
        placed[P.root] = 1;
        for (int l = 0; l + 1 < depth; ++l)
            for (uint32_t v : lv[l])
                for (int k = 0; k < 8; ++k) {
                    const uint32_t c = old_node(v)[k];
                    if (!c) continue;
                    if (c > n_nodes) return och::report(OCH_E_INVALID, kBadChild);
                    if (!placed[c]) {
                        placed[c] = (uint8_t)(l + 2);
                        lv[l + 1].push_back(c);
                    } else if (placed[c] != l + 2) {
                        return och::report(OCH_E_INVALID, kTwoHeights);
                    }
                }
        for (int l = 0; l < depth; ++l) reach += lv[l].size();
    }
    phase("reach");

    // records
    std::vector<uint64_t> keys;    // unique, ascending
    std::vector<uint32_t> words;   // the ids, zeros kept, then each level's node ids
    {
        const uint32_t *recs = static_cast<const uint32_t *>(P.records);
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
            keys.push_back(key);
            words.push_back(recs[(size_t)kv[i].second * 4 + 3]);
        }
    }
    const size_t m = keys.size();
    uint64_t bins[kBins] = {0}, counts[kMaxVoxelDepth] = {0};
    for (size_t i = 0; i < m; ++i) ++bins[level_bin(i == 0, i ? keys[i - 1] : 0, keys[i], depth)];
    const uint64_t rows_total = m ? level_counts(bins, depth, counts) : 0;
    phase("last wins");

    NodeStore ns;
    if (!ns.init(voxel_capacity(P.capacity, reach + rows_total), true)) {
        ns.release();
        return OCH_E_NOMEM;
    }
    const size_t chunk = 4096;

    // adopt, leaf level first
    std::vector<uint32_t> map(P.root ? (size_t)n_nodes + 1 : 1, 0);
    for (int l = depth - 1; l >= 0; --l) {
        const std::vector<uint32_t> &list = lv[l];
        const int h = depth - 1 - l;
        parallel_for(threads, (list.size() + chunk - 1) / chunk, [&](uint64_t c, int) {
            for (size_t i = c * chunk; i < std::min(list.size(), (c + 1) * chunk); ++i) {
                uint32_t row[8], any = 0;
                for (int k = 0; k < 8; ++k) {
                    const uint32_t w = old_node(list[i])[k];
                    row[k] = h > 0 && w ? map[w] : w;
                    any |= row[k];
                }
                map[list[i]] = any ? ns.intern(row, h) : 0;
            }
        });
    }
    const uint32_t old_root = map[P.root];
    phase("adopt");

    std::vector<uint64_t> pkeys;
    std::vector<uint32_t> pwords, heads;
    for (int h = 0; h < depth && m; ++h) {
        const size_t n_in = keys.size(), n_rows = (size_t)counts[h];
        heads.clear();
        for (size_t i = 0; i < n_in; ++i)
            if (i == 0 || (keys[i] >> 3) != (keys[i - 1] >> 3)) heads.push_back((uint32_t)i);
        if (heads.size() != n_rows) {   // the level counts and the grouping are two views of one list
            ns.release();
            return och::report(OCH_E_INVALID, "och_edit_voxels: inconsistent level counts");
        }
        pkeys.resize(n_rows);
        pwords.resize(n_rows);
        parallel_for(threads, (n_rows + chunk - 1) / chunk, [&](uint64_t c, int) {
            for (size_t r = c * chunk; r < std::min(n_rows, (c + 1) * chunk); ++r) {
                const uint64_t pk = keys[heads[r]] >> 3;
                uint32_t at = old_root;
                for (int H = depth - 1; H > h && at; --H) at = ns.nodes[(size_t)at * 8 + path_child(pk, H, h)];
                uint32_t row[8], any = 0;
                std::memcpy(row, ns.nodes + (size_t)at * 8, 32);   // id 0 is the zero node
                const size_t end = r + 1 < n_rows ? heads[r + 1] : n_in;
                for (size_t i = heads[r]; i < end; ++i) row[keys[i] & 7u] = words[i];
                for (int k = 0; k < 8; ++k) any |= row[k];
                pkeys[r] = pk;
                pwords[r] = any ? ns.intern(row, h) : 0;
            }
        });
        keys.swap(pkeys);
        words.swap(pwords);
    }
    phase("levels");
    root = m ? words[0] : old_root;
    if (ns.full.load()) {
        ns.release();
        return OCH_E_CAPACITY;
    }
    const int rs = renumber(ns.nodes, ns.level, std::min(ns.next.load(), ns.cap), root, depth, 1, out, n_out);
    ns.release();
    return rs;
}

}  // namespace
