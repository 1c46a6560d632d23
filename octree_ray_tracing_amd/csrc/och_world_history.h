// och_world_history.h -- a resident world's earlier roots (och_world_snapshot,
// _checkout, _release, _snapshots) and the diff of two of them on its GPU
// (och_world_diff).  Included by och_builder.cpp only, after och_world_read.h.
//
// Snapshots.  The store is append-only (och_world.h): no row an earlier root
// reaches ever changes, so an earlier state of the world is its root.  A
// snapshot is a handle to a copy of the world's state (och_world::now: root,
// child mask, the box at the call), host state only; a checkout assigns the
// copy back and launches nothing (the next
// stroke, which starts from the root word in the store's head, uploads it
// first: 8 bytes, only after a checkout).  used, strokes, generation and the
// store stay as they are, so strokes after a checkout branch off and the state
// left behind stays reachable through its own snapshot.  The flush copies the ids [published, used) whatever the root
// is, which covers every id any snapshot reaches, and the ids it writes are
// reached by no root that pool has published: it still waits for no kernel.
//
// Compaction keeps what the current root or any live snapshot reaches
// (world_compact_history): the store itself is the 1-based pool of an
// EditReach (d_pool = nodes + 8, n_nodes = used - 1), depth 0 of the reach is
// seeded with the distinct non-zero roots, edit_adopt interns the reached rows
// into a fresh store and every root is read back through d_map.  Ids inside a
// store are claim-ordered and mean nothing outside it, so nothing is renumbered
// canonically.  A world without live snapshots compacts as before (och_world.h).
//
// The diff.  Rows are interned per height and no all-zero row exists, so inside
// one generation two ids at one height are equal exactly when their subtrees
// hold the same voxels.  A walk from two roots at once therefore drops every
// position whose two ids are equal: the frontier of a level is the pairs
// (id under from, id under to, key of the position) whose ids differ, and its
// cost follows the change, not the world.  Per level, top down:
//   k_diff_count -- one thread per (pair, child word): eight neighbouring lanes
//                   read the two 32-byte rows (id 0 is the zero row); a
//                   candidate survives when its two words differ; the pair's
//                   survivors are a byte of the wavefront's ballot.  At height
//                   0 the words are voxel ids and the survivors' box is
//                   reduced per wavefront (box_reduce, as k_world_box).
//   scan         -- hipcub's inclusive sum of the pairs' counts, 64-bit.
//   read-back    -- the level's total (8 bytes, one synchronise): the next
//                   frontier's size, or n at height 0, where it is compared
//                   with the caller's capacity before a record is written.
//   k_diff_emit  -- the same loads and ballot; survivor j of the level (the
//                   scan's base of its pair + the survivors below it in the
//                   ballot's byte) becomes pair j of the next frontier, or
//                   record j.  Child digits ascend inside a pair and pairs are
//                   in Morton order, so every frontier and the records are in
//                   ascending Morton order without an atomic.
// Visibility is och_world_read.h's: every row is an earlier dispatch's and
// never changes; the frontier, counts and positions are read by later
// dispatches than the ones that wrote them; inside a dispatch nothing meets
// but the box's atomics and what the scan library does.
//
// Buffers.  Frontiers (two), counts, positions, the box and the scan's
// temporary storage are one device buffer kept in the world, for a power of
// two of pairs a level.  A level that outgrows it ends the walk, the buffer is
// replaced by a larger one and the walk starts over from the roots: a steady-
// state diff calls neither hipMalloc nor hipFree.
//
// Out of scope: snapshots across och_world_destroy or their serialisation; a
// diff between two worlds or two generations; at / read_box of a snapshot
// (check it out: O(1)); asynchronous diffs; replicated worlds themselves (the
// diff is their primitive); frame groups and the sharded paths.
#pragma once
#include "och_world_read.h"

namespace {

// The two words of candidate q = 8 i + k (child k of pair i), 0 past the
// frontier.  An interior word at or above cap reads as empty (k_world_at).
__device__ inline void diff_words(const GpuStore &S, const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb, uint32_t f,
                                  int interior, size_t q, uint32_t &wa, uint32_t &wb)
{
    wa = wb = 0;
    if (q >= (size_t)f * 8) return;
    const size_t i = q >> 3, k = q & 7u;
    wa = S.nodes[(size_t)fa[i] * 8 + k];
    wb = S.nodes[(size_t)fb[i] * 8 + k];
    if (interior) {
        wa = wa < S.cap ? wa : 0u;
        wb = wb < S.cap ? wb : 0u;
    }
}

// cnt[i] = the child words of pair i that differ.  Leaf level (interior = 0):
// the box of the differing voxels too (box: kNoBox before).
__global__ __launch_bounds__(256) void k_diff_count(GpuStore S, const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb,
                                                    const uint64_t *__restrict__ keys, uint32_t f, int interior,
                                                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ box)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t wa, wb;
    diff_words(S, fa, fb, f, interior, q, wa, wb);
    const bool differ = wa != wb;
    const uint64_t b = __ballot(differ);
    const uint32_t lane = threadIdx.x & 63u;
    if (q < (size_t)f * 8 && (lane & 7u) == 0) cnt[q >> 3] = (uint32_t)__popcll((b >> lane) & 0xFFull);
    if (interior || !b) return;   // the same in every lane
    box_reduce(differ, [&] { return keys[q >> 3] << 3 | (q & 7u); }, true, box);
}

// Survivor j of the level: pos[] is the inclusive sum of k_diff_count's cnt[].
// Interior: pair j of the next frontier.  Leaf level: record j, (x, y, z, the id
// under `to`), 4 x uint32.
__global__ __launch_bounds__(256) void k_diff_emit(GpuStore S, const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb,
                                                   const uint64_t *__restrict__ keys, uint32_t f, int interior,
                                                   const uint64_t *__restrict__ pos, uint32_t *__restrict__ next_a,
                                                   uint32_t *__restrict__ next_b, uint64_t *__restrict__ next_keys,
                                                   uint32_t *__restrict__ records)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t wa, wb;
    diff_words(S, fa, fb, f, interior, q, wa, wb);
    const bool differ = wa != wb;
    const uint64_t b = __ballot(differ);
    if (!differ) return;
    const uint32_t lane = threadIdx.x & 63u, k = (uint32_t)(q & 7u);
    const size_t i = q >> 3;
    const uint64_t below = (b >> (lane & 56u)) & ((1ull << k) - 1ull);
    const uint64_t j = (i ? pos[i - 1] : 0ull) + (uint64_t)__popcll(below);
    const uint64_t key = keys[i] << 3 | k;
    if (interior) {
        next_a[j] = wa;
        next_b[j] = wb;
        next_keys[j] = key;
    } else {
        uint32_t *r = records + j * 4;
        r[0] = compact3(key);
        r[1] = compact3(key >> 1);
        r[2] = compact3(key >> 2);
        r[3] = wb;
    }
}

// placed[seeds[i]] = 1: the reach's depth 0 holds every seed (distinct ids).
__global__ __launch_bounds__(256) void k_history_seed(const uint32_t *__restrict__ seeds, uint32_t n, uint32_t *__restrict__ placed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) placed[seeds[i]] = 1u;
}

// out[i] = map[seeds[i]]
__global__ __launch_bounds__(256) void k_history_gather(const uint32_t *__restrict__ map, const uint32_t *__restrict__ seeds,
                                                        uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = map[seeds[i]];
}

struct DiffWiden {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
using DiffCounts = hipcub::TransformInputIterator<uint64_t, DiffWiden, const uint32_t *>;

// The world's diff buffer (och_world.d_diff) for diff_cap pairs a level, carved.
struct DiffWork {
    uint64_t *keys[2], *pos;
    uint32_t *fa[2], *fb[2], *cnt, *box;
    void *temp;
};

constexpr size_t kDiffFixed = 256;   // the box's words, and the temporary storage's alignment

DiffWork diff_carve(const och_world &w)
{
    const size_t c = w.diff_cap;
    uint8_t *p = w.d_diff.d;
    DiffWork D{};
    D.box = reinterpret_cast<uint32_t *>(p);
    p += kDiffFixed;
    for (int s = 0; s < 2; ++s, p += c * 8) D.keys[s] = reinterpret_cast<uint64_t *>(p);
    D.pos = reinterpret_cast<uint64_t *>(p);
    p += c * 8;
    for (int s = 0; s < 2; ++s, p += c * 4) D.fa[s] = reinterpret_cast<uint32_t *>(p);
    for (int s = 0; s < 2; ++s, p += c * 4) D.fb[s] = reinterpret_cast<uint32_t *>(p);
    D.cnt = reinterpret_cast<uint32_t *>(p);
    p += c * 4;
    D.temp = p;   // c is a multiple of 64: 256-byte aligned like the buffer
    return D;
}

// Buffers for frontiers of f pairs (f < 2^31): kept while they suffice, else replaced by larger ones.
int diff_reserve(och_world &w, uint64_t f)
{
    if (f <= w.diff_cap) return OCH_OK;
    uint64_t cap = 1024;
    while (cap < f) cap <<= 1;
    size_t temp = 0;
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, temp, DiffCounts(nullptr, DiffWiden()), static_cast<uint64_t *>(nullptr),
                                             (int)std::min<uint64_t>(cap, 0x7FFFFFFFull), w.st));
    w.diff_cap = 0;
    if (w.d_diff.reserve(kDiffFixed + (size_t)cap * 44 + temp) != hipSuccess) return OCH_E_NOMEM;
    w.diff_cap = (uint32_t)cap;
    w.diff_temp_bytes = temp;
    return OCH_OK;
}

const char *kDiffTooMany = "och_world_diff: a level's frontier, or the differing voxels, number 2^31 or more";

// One walk from the two roots (different ids).  *grow != 0 on return: a level
// of that many pairs outgrew the buffers, nothing was written and the caller
// reserves and walks again.  Otherwise *out is complete before the capacity is
// looked at.
int diff_walk(och_world &w, uint32_t ra, uint32_t rb, void *records, uint64_t capacity, bool on_device, och_diff_stats *out,
              uint64_t *grow)
{
    const hipStream_t st = w.st;
    const DiffWork D = diff_carve(w);
    const uint64_t zero_key = 0;
    GPU_TRY(hipMemcpyAsync(D.fa[0], &ra, 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(D.fb[0], &rb, 4, hipMemcpyHostToDevice, st));
    GPU_TRY(hipMemcpyAsync(D.keys[0], &zero_key, 8, hipMemcpyHostToDevice, st));
    och_diff_stats ds{};
    uint32_t f = 1;
    int cur = 0;
    for (int h = w.depth - 1; h >= 0 && f; --h) {
        const int interior = h > 0 ? 1 : 0;
        uint32_t box[6] = {0};
        uint64_t total = 0;
        ds.pairs += f;
        if (!interior) GPU_TRY(hipMemcpyAsync(D.box, kNoBox, sizeof kNoBox, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_diff_count, blocks((size_t)f * 8), dim3(256), 0, st, w.S, D.fa[cur], D.fb[cur], D.keys[cur], f, interior,
                           D.cnt, D.box);
        GPU_TRY(hipGetLastError());
        size_t tb = w.diff_temp_bytes;
        GPU_TRY(hipcub::DeviceScan::InclusiveSum(D.temp, tb, DiffCounts(D.cnt, DiffWiden()), D.pos, (int)f, st));
        if (const int rs = world_read_back(w, {{&total, D.pos + (f - 1), 8}, {box, D.box, interior ? 0 : sizeof box}})) return rs;
        if (total >= (1ull << 31)) return och::report(OCH_E_INVALID, kDiffTooMany);
        if (interior) {
            if (total > w.diff_cap) {
                *grow = total;
                return OCH_OK;
            }
            if (total) {
                hipLaunchKernelGGL(k_diff_emit, blocks((size_t)f * 8), dim3(256), 0, st, w.S, D.fa[cur], D.fb[cur], D.keys[cur], f, 1,
                                   D.pos, D.fa[cur ^ 1], D.fb[cur ^ 1], D.keys[cur ^ 1], nullptr);
                GPU_TRY(hipGetLastError());
            }
            cur ^= 1;
            f = (uint32_t)total;
            continue;
        }
        ds.n = total;
        const WorldBox changed = box_decode(box);   // no voxel, all 0, exactly when total is 0
        std::memcpy(ds.box_lo, changed.lo, sizeof ds.box_lo);
        std::memcpy(ds.box_hi, changed.hi, sizeof ds.box_hi);
        *out = ds;
        if (!records || !total) return OCH_OK;
        if (total > capacity)
            return och::fail(OCH_E_CAPACITY, "och_world_diff: %llu records, the buffer holds %llu", (unsigned long long)total,
                             (unsigned long long)capacity);
        uint32_t *d_records = static_cast<uint32_t *>(world_stage(w, records, (size_t)total * 16, on_device));
        if (!d_records) return OCH_E_NOMEM;
        hipLaunchKernelGGL(k_diff_emit, blocks((size_t)f * 8), dim3(256), 0, st, w.S, D.fa[cur], D.fb[cur], D.keys[cur], f, 0, D.pos,
                           nullptr, nullptr, nullptr, d_records);
        GPU_TRY(hipGetLastError());
        return world_read_back(w, {{records, d_records, on_device ? 0 : (size_t)total * 16}});
    }
    *out = ds;   // a level without survivors: only words at or above cap differed
    return OCH_OK;
}

int world_diff(och_world &w, uint32_t ra, uint32_t rb, void *records, uint64_t capacity, bool on_device, och_diff_stats *out)
{
    PhaseTimer phase = world_phase(w);
    if (ra == rb) {   // equal ids: equal content
        *out = och_diff_stats{};
        return OCH_OK;
    }
    for (uint64_t want = 1;;) {
        if (const int rs = diff_reserve(w, want)) return rs;
        uint64_t grow = 0;
        if (const int ws = diff_walk(w, ra, rb, records, capacity, on_device, out, &grow)) return ws;
        if (!grow) break;
        want = grow;
    }
    phase("diff");
    return OCH_OK;
}

// A handle's snapshot; OCH_WORLD_CURRENT: the world's current state.
int world_snapshot_of(const och_world &w, uint64_t handle, const char *who, WorldSnapshot *s)
{
    if (handle == OCH_WORLD_CURRENT) {
        *s = w.now;
        return OCH_OK;
    }
    const auto it = w.snapshots.find(handle);
    if (it == w.snapshots.end())
        return och::fail(OCH_E_INVALID, "%s: snapshot %llu is unknown or released", who, (unsigned long long)handle);
    *s = it->second;
    return OCH_OK;
}

int world_compact_history(och_world &w)
{
    const hipStream_t st = w.st;
    PhaseTimer phase = world_phase(w);
    std::vector<uint32_t> seeds;
    if (w.now.root) seeds.push_back(w.now.root);
    for (const auto &s : w.snapshots)
        if (s.second.root) seeds.push_back(s.second.root);
    std::sort(seeds.begin(), seeds.end());
    seeds.erase(std::unique(seeds.begin(), seeds.end()), seeds.end());
    for (uint32_t s : seeds)
        if (s >= w.used) return och::report(OCH_E_INVALID, "och_world_compact: a snapshot's root lies outside the store");
    const uint32_t n_seeds = (uint32_t)seeds.size(), n = w.used - 1;
    GpuScope T(st);
    EditReach R;
    R.d_pool = w.S.nodes + 8;   // id's row at d_pool[(id - 1) * 8]
    uint32_t *d_new = nullptr;
    if (const int as = edit_reach_arrays(T, R, n, w.now.root, nullptr)) return as;
    if (!T.alloc(&d_new, (size_t)n_seeds * 4)) return OCH_E_NOMEM;
    if (n_seeds) {
        GPU_TRY(hipMemcpyAsync(R.d_order, seeds.data(), (size_t)n_seeds * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_history_seed, blocks(n_seeds), dim3(256), 0, st, R.d_order, n_seeds, R.d_placed);
        GPU_TRY(hipGetLastError());
        R.lv_cnt[0] = n_seeds;
        if (const int rs = edit_reach_levels(st, R, w.depth)) return rs;
    }
    if (!phase("reach")) return OCH_E_HIP;
    std::unique_ptr<GpuScope> scope;
    GpuStore S;
    WorldHead H;
    if (const int as = world_adopt(w, T, R, w.S.cap, scope, S, &H)) return as;
    std::vector<uint32_t> moved(n_seeds);
    if (n_seeds) {
        hipLaunchKernelGGL(k_history_gather, blocks(n_seeds), dim3(256), 0, st, R.d_map, R.d_order, n_seeds, d_new);
        GPU_TRY(hipGetLastError());
        if (const int rs = world_read_back(w, {{moved.data(), d_new, (size_t)n_seeds * 4}})) return rs;
    }
    if (!phase("adopt")) return OCH_E_HIP;
    auto new_id = [&](uint32_t old) {
        return old ? moved[(size_t)(std::lower_bound(seeds.begin(), seeds.end(), old) - seeds.begin())] : 0u;
    };
    for (uint32_t s : seeds)
        if (!new_id(s)) return och::report(OCH_E_HIP, "och_world_compact: a root was lost in the adoption");
    if (phase.on) std::fprintf(stderr, "[och_build] world: compacted %u ids to %u, %u roots kept\n", w.used, H.used, n_seeds);
    // nothing of the world has changed so far: a failure above leaves the old store and every handle in place
    for (auto &s : w.snapshots) s.second.root = new_id(s.second.root);   // the child masks are content: unchanged
    world_install(w, scope, S, H);
    return OCH_OK;
}

}  // namespace

OCH_API int och_world_snapshot(och_world *w, uint64_t *snapshot)
{
    if (!snapshot) return och::report(OCH_E_INVALID, "och_world_snapshot: snapshot is NULL");
    if (const int us = world_usable(w, "och_world_snapshot")) return us;
    if (w->snapshots.size() >= OCH_WORLD_MAX_SNAPSHOTS)
        return och::fail(OCH_E_CAPACITY, "och_world_snapshot: %d snapshots are live; release one", OCH_WORLD_MAX_SNAPSHOTS);
    WorldSnapshot s;
    (void)world_snapshot_of(*w, OCH_WORLD_CURRENT, "och_world_snapshot", &s);
    const uint64_t handle = w->next_snapshot++;
    w->snapshots.emplace(handle, s);
    *snapshot = handle;
    return OCH_OK;
}

OCH_API int och_world_checkout(och_world *w, uint64_t snapshot)
{
    if (const int us = world_usable(w, "och_world_checkout")) return us;
    WorldSnapshot s;
    if (const int ss = world_snapshot_of(*w, snapshot, "och_world_checkout", &s)) return ss;
    w->head_stale = w->head_stale || s.root != w->now.root;   // the next stroke uploads the root it starts from
    w->now = s;
    return OCH_OK;
}

OCH_API int och_world_release(och_world *w, uint64_t snapshot)
{
    if (const int us = world_usable(w, "och_world_release")) return us;
    if (snapshot == OCH_WORLD_CURRENT)
        return och::report(OCH_E_INVALID, "och_world_release: OCH_WORLD_CURRENT is not a snapshot");
    if (!w->snapshots.erase(snapshot))
        return och::fail(OCH_E_INVALID, "och_world_release: snapshot %llu is unknown or released", (unsigned long long)snapshot);
    return OCH_OK;
}

OCH_API int och_world_snapshots(const och_world *w, uint64_t *ids, uint32_t capacity, uint32_t *count)
{
    if (!count) return och::report(OCH_E_INVALID, "och_world_snapshots: count is NULL");
    if (!ids && capacity) return och::report(OCH_E_INVALID, "och_world_snapshots: ids is NULL");
    if (const int us = world_usable(w, "och_world_snapshots")) return us;
    uint32_t i = 0;
    for (const auto &s : w->snapshots) {
        if (i >= capacity) break;
        ids[i++] = s.first;
    }
    *count = (uint32_t)w->snapshots.size();
    return OCH_OK;
}

OCH_API int och_world_diff(och_world *w, uint64_t from, uint64_t to, void *records, uint64_t capacity, int on_device,
                           och_diff_stats *stats)
{
    if (!stats) return och::report(OCH_E_INVALID, "och_world_diff: stats is NULL");
    return world_call(w, "och_world_diff", "och_world_diff", kStays, kOwnTexts, [&] {
        WorldSnapshot a, b;
        if (const int ss = world_snapshot_of(*w, from, "och_world_diff", &a)) return ss;
        if (const int ss = world_snapshot_of(*w, to, "och_world_diff", &b)) return ss;
        return world_diff(*w, a.root, b.root, records, capacity, on_device != 0, stats);
    });
}
