// och_world_region.h -- strokes of a resident world whose shape is a box
// (och_world_fill_box, och_world_restore_box) or a ball (och_world_fill_sphere,
// och_world_restore_sphere), at a cost that follows the shape's surface.
// Included by och_builder.cpp only, after och_world_history.h.  The text below
// speaks of the box; a ball is the same walk with another classifier (the end).
//
// A box is a union of maximal aligned cubes.  A cube of side 2^h that lies
// wholly inside the box is one child word at height h: 0 for a clear, the id
// of the uniform subtree of that height for a fill, the word the snapshot's
// root holds at that position for a restore.  Only the cells that straddle the
// box's faces get new rows.  A stroke is two passes over the levels:
//
// The walk, top down, reads the store and interns nothing.  A frontier entry
// is a cell of height H that straddles the box: its Morton key and, for a
// restore, its ids under the current and the snapshot's root.  Per level:
//   k_region_count -- one thread per (cell, child): the child cube's corners
//                     against the clipped box, integer compares.  Outside:
//                     nothing.  Inside: a cube, an entry (child key, word) of
//                     height H - 1.  Straddling: a cell of the next frontier.
//                     The cell's cubes and cells are two bytes of the
//                     wavefront's two ballots, counted into one 64-bit word
//                     (cubes high, cells low: both stay below 2^31).
//   scan           -- hipcub's inclusive sum of those words.
//   k_region_emit  -- the same classification; survivor j of either kind (the
//                     scan's base of its cell + the survivors below it in the
//                     ballot's byte) becomes cube j of height H - 1 or cell j
//                     of the next frontier.  Child digits ascend inside a cell
//                     and cells are in Morton order, so each height's cubes and
//                     each frontier are in ascending Morton order, no sort.
// A fill never prunes and never reads a row: every count is a closed form of
// the box (och::box_cube_counts), known before the first launch, so its walk
// runs without a read-back.  A restore prunes as the diff does (within one
// store, equal ids at one height hold equal voxels): a straddling child whose
// two words are equal is no cell, an inside child whose two words are equal is
// no cube; the level's two totals come back in one 8-byte read.
//
// The levels, bottom up, are edit_levels' loop (och_voxel_edit.h) with entries
// injected at every height, not only at height 0.  At level h the entries are
// the cubes of height h merged with the ids carried up from level h - 1 (the
// rebuilt cells of height h).  Both lists are Morton-sorted and their keys are
// disjoint (a cube lies inside the box, a cell straddles it), so they are
// merged as two lists, k_region_merge: every entry finds its rank in the other
// list by binary search and its place is the sum; no radix sort, no temporary
// storage, and a level without cubes skips the merge.  Then k_vox_heads, the
// scan, k_edit_rows, k_intern_rows<true> and k_settle, unchanged.  The rows of
// level h are the cells of height h + 1 that have an entry: for a fill all of
// them (a closed form again), for a restore the scan's total, read back (4
// bytes a level), since a cell whose ids differ may differ only outside the box.
// The uniform subtrees of a fill are U_0 = id, U_h = the row of eight U_(h-1):
// that row is one extra row of level h - 1's batch (k_region_uniform), so U_h
// exists a dispatch before level h's merge reads it.  k_intern's rule
// (och_dag.h) holds throughout: rows, keys and ids are read only by later
// dispatches than the ones that wrote them.
//
// Capacity is checked after the walk and before the first intern (och_world.h
// says why): used + cells + T ids, cells the walk's frontiers summed, T the
// uniform subtrees of a fill.  For a fill both are closed forms and the check
// comes before any launch.  Buffers: one device buffer kept in the world.  A
// fill sizes it by the box's closed forms.  A restore's cubes and cells are
// subsets of the fill's and usually far fewer (a box of 2^60 voxels over two
// states that differ in three is a handful of cells), so its buffer starts
// small and a level that outgrows it ends the walk, the buffer is replaced by
// a larger one and the walk starts over from the roots, as the diff's does.
// A height of 2^31 entries or more is refused; a restore also refuses a
// frontier of 2^28 cells or more, whose children's counts share a 64-bit word.
//
// The walk is generic over the shape: region_class(shape, key, h) is all that
// k_region_count and k_region_emit ask of it, and a restore is
// world_restore_region<Shape>.  A ball (RegionBall, och_ball.h) is classified in
// integers per axis, exactly.  It has no closed forms, and its fill never
// prunes, so a fill's walk keeps its counts on the device (region_walk_dev):
// each level's kernels read their frontier's size from the totals the level
// above left (RegionTotals), their grids and the scan's length are a host-side
// upper bound (ball_plan), and one read-back after the last level brings every
// level's totals for the capacity check, the rows and the stats: a fill stroke
// synchronises twice, for these and for the head.  Nothing rests on the bound:
// the host holds each level's real frontier against what was launched, top
// down, and walks again with more where one was cut short.
//
// A third mode of the walk (kWalkPaint) serves the strokes conditional on the
// old voxel, och_world_paint.h: one root, and a child the predicate cannot
// touch is dropped.
//
// Out of scope: shapes other than boxes and balls; copying a box to another
// place; replicated worlds.
#pragma once
#include "och_world_history.h"

namespace {

struct RegionBox {
    int32_t lo[3], hi[3];   // clipped to the tree, hi exclusive
};

// A level's frontier: f cells, their keys and (restore) ids under the two roots.
struct RegionFront {
    uint64_t *keys;
    uint32_t *fa, *fb;
    uint32_t f;
};

// The cube of side 2^h with Morton key `key` at height h against the box: 0 outside, 1 straddling, 2 inside.
__device__ inline int region_class(const RegionBox &B, uint64_t key, int h)
{
    bool inside = true, outside = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int32_t c = (int32_t)(compact3(key >> a) << h), e = c + ((int32_t)1 << h);
        inside = inside && B.lo[a] <= c && e <= B.hi[a];
        outside = outside || c >= B.hi[a] || e <= B.lo[a];
    }
    return outside ? 0 : inside ? 2 : 1;
}

// A ball (och_ball.h): the classifier is all a shape needs.
using RegionBall = och::Ball;

__device__ inline int region_class(const RegionBall &B, uint64_t key, int h)
{
    const int32_t c[3] = {(int32_t)(compact3(key) << h), (int32_t)(compact3(key >> 1) << h), (int32_t)(compact3(key >> 2) << h)};
    return och::ball_class(B, c, h);
}

// What a walk reads of the store: nothing (a fill), each child's words under
// two roots, equal ones dropped (a restore), or its word under one root, a
// child that is not open dropped (a paint: RegionPaint).
constexpr int kWalkFill = 0, kWalkRestore = 1, kWalkPaint = 2;

// A shape with a predicate on the old voxel, pred(v) = (v == match) != when:
// the shape's classifier, and which children a paint's walk keeps.
template <class Shape>
struct RegionPaint {
    Shape shape;
    uint32_t when, match;
};

template <class Shape>
__device__ inline int region_class(const RegionPaint<Shape> &B, uint64_t key, int h)
{
    return region_class(B.shape, key, h);
}

__host__ __device__ inline bool paint_pred(uint32_t when, uint32_t match, uint32_t v) { return (v == match) != (when != 0); }

// A child of height H - 1 whose word is w is open when the stroke can touch
// it: a node always, an empty cube or a voxel iff pred(w).
template <class Shape>
__device__ inline bool region_open(const Shape &, int, uint32_t)
{
    return true;
}

template <class Shape>
__device__ inline bool region_open(const RegionPaint<Shape> &B, int H, uint32_t w)
{
    return (H > 1 && w) || paint_pred(B.when, B.match, w);
}

// Candidate q = 8 i + k, child k of cell i of the frontier at height H: its
// key, whether it is a cube or a cell of the next frontier, and (restore) its
// two words, (paint) its word in wa.  An interior word at or above cap reads
// as empty (k_world_at).
template <int kMode, class Shape>
__device__ inline void region_child(const GpuStore &S, const Shape &B, const RegionFront &F, int H, size_t q, uint64_t &key,
                                    uint32_t &wa, uint32_t &wb, bool &cube, bool &cell)
{
    cube = cell = false;
    wa = wb = 0;
    key = 0;
    if (q >= (size_t)F.f * 8) return;
    const size_t i = q >> 3, k = q & 7u;
    key = F.keys[i] << 3 | k;
    const int c = region_class(B, key, H - 1);
    if (!c) return;
    if (kMode == kWalkRestore) {
        wa = S.nodes[(size_t)F.fa[i] * 8 + k];   // id 0 is the zero row
        wb = S.nodes[(size_t)F.fb[i] * 8 + k];
        if (H > 1) {
            wa = wa < S.cap ? wa : 0u;
            wb = wb < S.cap ? wb : 0u;
        }
        if (wa == wb) return;
    }
    if (kMode == kWalkPaint) {
        wa = S.nodes[(size_t)F.fa[i] * 8 + k];
        if (H > 1) wa = wa < S.cap ? wa : 0u;
        if (!region_open(B, H, wa)) return;
    }
    cube = c == 2;
    cell = c == 1;
}

// cnt[i] = cell i's cubes << 32 | its cells of the next frontier.
template <int kMode, class Shape>
__device__ inline void region_count(const GpuStore &S, const Shape &B, const RegionFront &F, int H, uint64_t *__restrict__ cnt)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key;
    uint32_t wa, wb;
    bool cube, cell;
    region_child<kMode>(S, B, F, H, q, key, wa, wb, cube, cell);
    const uint64_t bc = __ballot(cube), bf = __ballot(cell);
    const uint32_t lane = threadIdx.x & 63u;
    if (q < (size_t)F.f * 8 && (lane & 7u) == 0)
        cnt[q >> 3] = (uint64_t)__popcll((bc >> lane) & 0xFFull) << 32 | (uint64_t)__popcll((bf >> lane) & 0xFFull);
}

template <int kMode, class Shape>
__global__ __launch_bounds__(256) void k_region_count(GpuStore S, Shape B, RegionFront F, int H, uint64_t *__restrict__ cnt)
{
    region_count<kMode>(S, B, F, H, cnt);
}

// Survivor j of either kind: pos[] is the inclusive sum of k_region_count's
// cnt[].  A cube: entry j of height H - 1 (cubes, and for a restore its word
// under the snapshot, for a paint its word).  A cell: cell j of the next
// frontier.  n_cubes and N.f are what the buffers hold; the counts never
// exceed them.
template <int kMode, class Shape>
__device__ inline void region_emit(const GpuStore &S, const Shape &B, const RegionFront &F, int H, const uint64_t *__restrict__ pos,
                                   uint64_t *__restrict__ cubes, uint32_t *__restrict__ cube_words, uint32_t n_cubes,
                                   const RegionFront &N)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key;
    uint32_t wa, wb;
    bool cube, cell;
    region_child<kMode>(S, B, F, H, q, key, wa, wb, cube, cell);
    const uint64_t bc = __ballot(cube), bf = __ballot(cell);
    if (!cube && !cell) return;
    const uint32_t lane = threadIdx.x & 63u, k = (uint32_t)(q & 7u);
    const size_t i = q >> 3;
    const uint64_t base = i ? pos[i - 1] : 0ull, lower = (1ull << k) - 1ull;
    if (cube) {
        const uint32_t j = (uint32_t)(base >> 32) + (uint32_t)__popcll((bc >> (lane & 56u)) & lower);
        if (j >= n_cubes) return;
        cubes[j] = key;
        if (kMode) cube_words[j] = kMode == kWalkPaint ? wa : wb;
    } else {
        const uint32_t j = (uint32_t)base + (uint32_t)__popcll((bf >> (lane & 56u)) & lower);
        if (j >= N.f) return;
        N.keys[j] = key;
        if (kMode) N.fa[j] = wa;
        if (kMode == kWalkRestore) N.fb[j] = wb;
    }
}

template <int kMode, class Shape>
__global__ __launch_bounds__(256) void k_region_emit(GpuStore S, Shape B, RegionFront F, int H, const uint64_t *__restrict__ pos,
                                                     uint64_t *__restrict__ cubes, uint32_t *__restrict__ cube_words,
                                                     uint32_t n_cubes, RegionFront N)
{
    region_emit<kMode>(S, B, F, H, pos, cubes, cube_words, n_cubes, N);
}

// A fill's walk with its counts on the device: what the walk of a shape
// without closed forms knows of its levels.  tot[h] = the cubes of height h
// << 32 | the cells of height h (the frontier of level h), first[h] = the
// cubes of the greater heights, where height h's start in the cubes' buffer.
// Level H's kernels read tot[H] and first[H - 1], which level H + 1's emit (or
// the seed) wrote a dispatch earlier, and write tot[H - 1] and first[H - 2].
struct RegionTotals {
    uint64_t tot[22], first[22];
};

// k_region_count for `F.f` cells launched, a host-side bound: the real
// frontier is tot[H]'s cells, the cells beyond it count zero.  A frontier
// above the bound is cut to it: the level's totals are then too small, which
// the host sees in tot[H] itself.
template <class Shape>
__global__ __launch_bounds__(256) void k_region_count_dev(GpuStore S, Shape B, RegionFront F, int H,
                                                          const RegionTotals *__restrict__ T, uint64_t *__restrict__ cnt)
{
    const uint32_t bound = F.f;
    F.f = (uint32_t)min((uint64_t)bound, T->tot[H] & 0xFFFFFFFFull);
    region_count<kWalkFill>(S, B, F, H, cnt);
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)F.f * 8 && q < (size_t)bound * 8 && (q & 7u) == 0) cnt[q >> 3] = 0;
}

// k_region_emit likewise; pos[] has `F.f` entries, the last one the level's
// totals, which one thread files for the level below.  The cubes go to
// first[H - 1] of the buffer's n_cubes, and no further.
template <class Shape>
__global__ __launch_bounds__(256) void k_region_emit_dev(GpuStore S, Shape B, RegionFront F, int H, const uint64_t *__restrict__ pos,
                                                         RegionTotals *__restrict__ T, uint64_t *__restrict__ cubes,
                                                         uint64_t n_cubes, RegionFront N)
{
    const uint32_t bound = F.f;
    const uint64_t first = T->first[H - 1];
    F.f = (uint32_t)min((uint64_t)bound, T->tot[H] & 0xFFFFFFFFull);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t total = pos[bound - 1];
        T->tot[H - 1] = total;
        if (H >= 2) T->first[H - 2] = first + (total >> 32);
    }
    const uint64_t room = first < n_cubes ? n_cubes - first : 0;
    region_emit<kWalkFill>(S, B, F, H, pos, cubes + min(first, n_cubes), nullptr, (uint32_t)min(room, (uint64_t)0xFFFFFFFFull), N);
}

// The first frontier: the root cell, key 0, with its two ids; T: a walk with
// device counts starts from one cell of height `depth` and no cube.
__global__ __launch_bounds__(64) void k_region_seed(RegionFront F, uint32_t ra, uint32_t rb, bool restore, RegionTotals *T, int depth)
{
    if (blockIdx.x || threadIdx.x) return;
    F.keys[0] = 0;
    if (restore) {
        F.fa[0] = ra;
        F.fb[0] = rb;
    }
    if (T) {
        T->tot[depth] = 1;
        T->first[depth - 1] = 0;
    }
}

// Two Morton-sorted lists with disjoint keys into one: the ids carried up (ka,
// wa; na) and the level's cubes (kb; nb), whose words are wb[], or without wb
// the uniform word: *uni, or `id` without uni.  Entry j's place is j + its
// rank in the other list.
__global__ __launch_bounds__(256) void k_region_merge(const uint64_t *__restrict__ ka, const uint32_t *__restrict__ wa, uint32_t na,
                                                      const uint64_t *__restrict__ kb, const uint32_t *__restrict__ wb, uint32_t nb,
                                                      const uint32_t *__restrict__ uni, uint32_t id, uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na + nb) return;
    const bool carried = i < na;
    const uint32_t j = carried ? i : i - na;
    const uint64_t key = carried ? ka[j] : kb[j];
    const uint64_t *other = carried ? kb : ka;
    uint32_t lo = 0, hi = carried ? nb : na;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (other[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    keys[j + lo] = key;
    words[j + lo] = carried ? wa[j] : wb ? wb[j] : uni ? *uni : id;
}

// One row of eight equal words: *uni, or `id` without uni.
__global__ __launch_bounds__(64) void k_region_uniform(uint32_t *__restrict__ row, const uint32_t *__restrict__ uni, uint32_t id)
{
    if (blockIdx.x == 0 && threadIdx.x < 8) row[threadIdx.x] = uni ? *uni : id;
}

// The world's region buffer (och_world.d_region), carved for one stroke:
// cubes for n_cubes entries, frontiers, counts and the scan for n_front cells.
struct RegionWork {
    uint64_t *cubes = nullptr;       // every height's cubes, height h's from RegionPlan.first[h]
    uint32_t *cube_words = nullptr;  // restore: their words under the snapshot
    uint64_t n_cubes = 0;
    RegionFront front[2] = {};       // .f: what each holds, n_front
    uint64_t *cnt = nullptr, *pos = nullptr;
    RegionTotals *totals = nullptr;  // a walk with device counts: its levels' totals
    void *temp = nullptr;
    size_t temp_bytes = 0;
};

const char *kRegionTooMany = "och_world: a height of the box holds 2^31 cubes or cells or more";
constexpr uint64_t kRegionLimit = 1ull << 31;
constexpr uint64_t kRegionFrontLimit = 1ull << 28;   // a restore's frontier: its children stay below 2^31

int region_reserve(och_world &w, uint64_t n_cubes, uint64_t n_front, bool restore, RegionWork &R)
{
    n_cubes = std::max<uint64_t>(n_cubes, 1);
    n_front = std::max<uint64_t>(n_front, 1);
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, R.temp_bytes, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                             (int)n_front, w.st));
    size_t bytes = 0;
    auto place = [&](size_t n) {   // 256-byte aligned, like the buffer
        const size_t at = bytes;
        bytes += (n + 255) & ~(size_t)255;
        return at;
    };
    const size_t at_cubes = place(n_cubes * 8), at_words = place(restore ? n_cubes * 4 : 0);
    size_t at_keys[2], at_fa[2], at_fb[2];
    for (int s = 0; s < 2; ++s) {
        at_keys[s] = place(n_front * 8);
        at_fa[s] = place(restore ? n_front * 4 : 0);
        at_fb[s] = place(restore ? n_front * 4 : 0);
    }
    const size_t at_cnt = place(n_front * 8), at_pos = place(n_front * 8), at_totals = place(sizeof(RegionTotals)),
                 at_temp = place(R.temp_bytes);
    if (w.d_region.reserve(bytes) != hipSuccess) return OCH_E_NOMEM;
    uint8_t *p = w.d_region.d;
    R.cubes = reinterpret_cast<uint64_t *>(p + at_cubes);
    R.cube_words = restore ? reinterpret_cast<uint32_t *>(p + at_words) : nullptr;
    R.n_cubes = n_cubes;
    for (int s = 0; s < 2; ++s)
        R.front[s] = RegionFront{reinterpret_cast<uint64_t *>(p + at_keys[s]), restore ? reinterpret_cast<uint32_t *>(p + at_fa[s]) : nullptr,
                                 restore ? reinterpret_cast<uint32_t *>(p + at_fb[s]) : nullptr, (uint32_t)n_front};
    R.cnt = reinterpret_cast<uint64_t *>(p + at_cnt);
    R.pos = reinterpret_cast<uint64_t *>(p + at_pos);
    R.totals = reinterpret_cast<RegionTotals *>(p + at_totals);
    R.temp = p + at_temp;
    return OCH_OK;
}

// What a stroke injects and rebuilds, by height: for a fill the box's closed
// forms, for a restore what the walk (cubes, cells) and the levels (rows) found.
struct RegionPlan {
    uint64_t cubes[22] = {0};   // entries injected at height h, at first[h] of the cubes' buffer
    uint64_t first[22] = {0};   // in the walk's order: the greatest height first
    uint64_t cells[22] = {0};   // the frontier at height H
    uint64_t rows[22] = {0};    // rows of level h: the rebuilt cells of height h + 1
    uint64_t front = 0;         // the frontiers, summed
};

// The walk from the root cell down.  Fill: P is complete before the call and
// nothing is read back.  Restore (ra != rb) and paint (ra, the one root): P is
// filled in as the levels' totals come back; grow_cubes / grow_front != 0 on
// return: a level outgrew the buffers, the caller reserves that much and walks
// again.
template <int kMode, class Shape>
int region_walk(och_world &w, const Shape &B, const RegionWork &R, uint32_t ra, uint32_t rb, RegionPlan &P, uint64_t *grow_cubes,
                uint64_t *grow_front)
{
    const hipStream_t st = w.st;
    hipLaunchKernelGGL(k_region_seed, dim3(1), dim3(64), 0, st, R.front[0], ra, rb, kMode != kWalkFill, static_cast<RegionTotals *>(nullptr), 0);
    GPU_TRY(hipGetLastError());
    uint32_t f = 1;
    uint64_t at = 0;   // the cubes emitted so far
    int cur = 0;
    if (kMode) P = RegionPlan{};
    for (int H = w.depth; H >= 1 && f; --H) {
        RegionFront F = R.front[cur], N = R.front[cur ^ 1];
        const uint32_t held = N.f;
        F.f = f;
        if (kMode) {
            P.cells[H] = f;
            P.front += f;
        }
        hipLaunchKernelGGL((k_region_count<kMode, Shape>), blocks((size_t)f * 8), dim3(256), 0, st, w.S, B, F, H, R.cnt);
        GPU_TRY(hipGetLastError());
        size_t tb = R.temp_bytes;
        GPU_TRY(hipcub::DeviceScan::InclusiveSum(R.temp, tb, R.cnt, R.pos, (int)f, st));
        if (kMode) {
            uint64_t total = 0;
            if (const int rs = world_read_back(w, {{&total, R.pos + (f - 1), 8}})) return rs;
            P.cubes[H - 1] = total >> 32;
            P.cells[H - 1] = total & 0xFFFFFFFFull;
            P.first[H - 1] = at;
            if (at + P.cubes[H - 1] >= kRegionLimit || P.cells[H - 1] >= kRegionFrontLimit)
                return och::report(OCH_E_INVALID, kMode == kWalkRestore
                                                      ? "och_world: a height of the restore holds 2^31 differing cubes, or 2^28 differing cells, or more"
                                                      : "och_world: a height of the paint holds 2^31 open cubes, or 2^28 open cells, or more");
            if (at + P.cubes[H - 1] > R.n_cubes || P.cells[H - 1] > held) {
                *grow_cubes = at + P.cubes[H - 1];
                *grow_front = P.cells[H - 1];
                return OCH_OK;
            }
        }
        const uint64_t n_cubes = P.cubes[H - 1], n_cells = P.cells[H - 1];
        N.f = (uint32_t)n_cells;
        if (n_cubes || n_cells) {
            hipLaunchKernelGGL((k_region_emit<kMode, Shape>), blocks((size_t)f * 8), dim3(256), 0, st, w.S, B, F, H, R.pos,
                               R.cubes + P.first[H - 1], kMode ? R.cube_words + P.first[H - 1] : nullptr, (uint32_t)n_cubes, N);
            GPU_TRY(hipGetLastError());
        }
        at += n_cubes;
        cur ^= 1;
        f = (uint32_t)n_cells;
    }
    return OCH_OK;
}

// A fill's walk for a shape without closed forms, its counts on the device and
// no read-back per level.  bound[H] >= 1 cells are launched and scanned at
// level H (at most what R's frontiers hold); each level's kernels read their
// real frontier from the totals the level above left (k_region_count_dev).
// One read-back after the last level brings every level's totals.  Then, top
// down, each level's real frontier against what was launched and the cubes
// against the buffer: a level's totals are right whenever all levels above it
// ran whole.  P is complete on return, or *grow_front / *grow_cubes name what
// the first level that was cut short needs (its height in *grow_at) and the
// caller walks again with more.
template <class Shape>
int region_walk_dev(och_world &w, const Shape &B, const RegionWork &R, const uint64_t bound[22], RegionPlan &P, uint64_t *grow_cubes,
                    uint64_t *grow_front, int *grow_at)
{
    const hipStream_t st = w.st;
    hipLaunchKernelGGL(k_region_seed, dim3(1), dim3(64), 0, st, R.front[0], 0u, 0u, false, R.totals, w.depth);
    GPU_TRY(hipGetLastError());
    int cur = 0;
    for (int H = w.depth; H >= 1; --H) {
        RegionFront F = R.front[cur];
        const RegionFront N = R.front[cur ^ 1];
        F.f = (uint32_t)bound[H];
        hipLaunchKernelGGL(k_region_count_dev<Shape>, blocks((size_t)F.f * 8), dim3(256), 0, st, w.S, B, F, H, R.totals, R.cnt);
        GPU_TRY(hipGetLastError());
        size_t tb = R.temp_bytes;
        GPU_TRY(hipcub::DeviceScan::InclusiveSum(R.temp, tb, R.cnt, R.pos, (int)F.f, st));
        hipLaunchKernelGGL(k_region_emit_dev<Shape>, blocks((size_t)F.f * 8), dim3(256), 0, st, w.S, B, F, H, R.pos, R.totals, R.cubes,
                           R.n_cubes, N);
        GPU_TRY(hipGetLastError());
        cur ^= 1;
    }
    RegionTotals T;
    if (const int rs = world_read_back(w, {{&T, R.totals, sizeof T}})) return rs;
    P = RegionPlan{};
    P.cells[w.depth] = 1;
    P.front = 1;
    uint64_t at = 0;
    for (int h = w.depth - 1; h >= 0; --h) {
        P.cubes[h] = T.tot[h] >> 32;
        P.cells[h] = T.tot[h] & 0xFFFFFFFFull;
        P.first[h] = at;
        if (at + P.cubes[h] >= kRegionLimit || P.cells[h] >= kRegionFrontLimit)
            return och::report(OCH_E_INVALID, "och_world: a height of the ball holds 2^31 cubes, or 2^28 cells, or more");
        if (at + P.cubes[h] > R.n_cubes || (h >= 1 && P.cells[h] > bound[h])) {
            *grow_cubes = at + P.cubes[h];
            *grow_front = P.cells[h];
            *grow_at = h;
            return OCH_OK;
        }
        at += P.cubes[h];
        P.front += P.cells[h];
        P.rows[h] = P.cells[h + 1];   // a straddling cell holds a voxel of the ball: it always has an entry
    }
    return OCH_OK;
}

// The levels: P.cubes[h] entries of R injected at height h (their words: R's,
// or the uniform word of `id`), T > 0: the uniform subtrees up to height T are
// made on the way.  read_rows (restore): P.rows[h] is the scan's total, read
// back; otherwise it is given.  *d_root: the device word that holds the new
// root, nullptr when no level had an entry.  w.W holds the widest level + 1.
int region_levels(och_world &w, const RegionWork &R, RegionPlan &P, uint32_t id, int T, bool read_rows, const uint32_t **d_root)
{
    const hipStream_t st = w.st;
    const EditWork &W = w.W;
    const int depth = w.depth;
    int c = 1;                       // the buffer of the carried ids
    uint32_t na = 0;                 // how many: the rows of the level below
    const uint32_t *uni = nullptr;   // the uniform word of this height, from the level below
    *d_root = nullptr;
    for (int h = 0; h < depth; ++h) {
        const uint32_t nb = (uint32_t)P.cubes[h], n_in = na + nb, extra = h < T ? 1u : 0u;
        if (!n_in && !extra) {
            uni = nullptr;
            continue;
        }
        int src = c;
        if (nb) {
            src = c ^ 1;
            hipLaunchKernelGGL(k_region_merge, blocks(n_in), dim3(256), 0, st, W.keys[c], W.words[c], na, R.cubes + P.first[h],
                               R.cube_words ? R.cube_words + P.first[h] : nullptr, nb, uni, id, W.keys[src], W.words[src]);
            GPU_TRY(hipGetLastError());
        }
        const int dst = src ^ 1;
        uint32_t n_rows = 0;
        if (n_in) {
            hipLaunchKernelGGL(k_vox_heads, blocks(n_in), dim3(256), 0, st, W.keys[src], n_in, W.flags);
            GPU_TRY(hipGetLastError());
            size_t tb = W.temp_bytes;
            GPU_TRY(hipcub::DeviceScan::InclusiveSum(W.temp, tb, W.flags, W.pos, (int)n_in, st));
            if (read_rows) {
                uint32_t total = 0;
                if (const int rs = world_read_back(w, {{&total, W.pos + (n_in - 1), 4}})) return rs;
                P.rows[h] = std::min(total, n_in);
            }
            n_rows = (uint32_t)P.rows[h];
            hipLaunchKernelGGL(k_edit_rows, blocks(n_in), dim3(256), 0, st, w.S, w.head() + kHeadRoot, W.keys[src], W.words[src], n_in,
                               W.flags, W.pos, n_rows, depth, h, W.rows, W.keys[dst]);
            GPU_TRY(hipGetLastError());
        }
        if (extra) hipLaunchKernelGGL(k_region_uniform, dim3(1), dim3(64), 0, st, W.rows + (size_t)n_rows * 8, uni, id);
        const uint32_t n = n_rows + extra;
        GpuLevel L{W.rows, 0, 0, n, h, 1};
        hipLaunchKernelGGL(k_intern_rows<true>, blocks(n), dim3(256), 0, st, w.S, L, W.rep, W.slot);
        hipLaunchKernelGGL(k_settle, blocks(n), dim3(256), 0, st, w.S, n, W.rep, W.slot, W.words[dst], nullptr);
        GPU_TRY(hipGetLastError());
        uni = extra ? W.words[dst] + n_rows : nullptr;
        c = dst;
        na = n_rows;
        if (h == depth - 1) *d_root = n_rows ? W.words[dst] : uni;   // the top row, or the tree's uniform subtree
    }
    return OCH_OK;
}

// The stroke's end, shared: the new root into the head, the head read back, the world's state.
int region_finish(och_world &w, const uint32_t *d_root, och_region_stats &rs)
{
    if (d_root) {
        hipLaunchKernelGGL(k_world_root, dim3(1), dim3(64), 0, w.st, w.S, d_root, w.head());
        GPU_TRY(hipGetLastError());
    }
    WorldHead H;
    if (const int hs = world_read_head(w, w.S, &H)) return hs;
    rs.new_ids = H.used - w.used;
    w.used = H.used;
    w.now.root = H.root;
    w.now.root_mask = H.mask;
    return OCH_OK;
}

// A checkout left the head's root word behind the host's: the stroke starts from the head.
int region_head(och_world &w)
{
    if (!w.head_stale) return OCH_OK;
    w.head_up[0] = w.now.root;
    w.head_up[1] = w.now.root_mask;
    GPU_TRY(hipMemcpyAsync(w.head() + kHeadRoot, w.head_up, sizeof w.head_up, hipMemcpyHostToDevice, w.st));
    w.head_stale = false;
    return OCH_OK;
}

// A new root that the host alone knows (a box over the whole tree): as a checkout.
void region_set_root(och_world &w, uint32_t root, uint32_t mask)
{
    w.head_stale = w.head_stale || root != w.now.root;
    w.now.root = root;
    w.now.root_mask = mask;
}

WorldBox region_world_box(const och::BoxCubes &C)
{
    WorldBox b;
    b.any = C.any;
    std::memcpy(b.lo, C.lo, sizeof b.lo);
    std::memcpy(b.hi, C.hi, sizeof b.hi);
    return b;
}

och_region_stats region_stats(const och::BoxCubes &C)
{
    och_region_stats rs{};
    std::memcpy(rs.lo, C.lo, sizeof rs.lo);
    std::memcpy(rs.hi, C.hi, sizeof rs.hi);
    return rs;
}

void region_trace(const och_world &w, const PhaseTimer &phase, const char *what, const och_region_stats &rs)
{
    if (phase.on)
        std::fprintf(stderr, "[och_build] world: %s, %llu cubes, %llu cells, %llu new ids, %u of %u used\n", what,
                     (unsigned long long)rs.cubes, (unsigned long long)rs.cells, (unsigned long long)rs.new_ids, w.used, w.S.cap);
}

int world_fill_box(och_world &w, const int32_t lo[3], const int32_t hi[3], uint32_t id, och_region_stats *out)
{
    PhaseTimer phase = world_phase(w);
    const och::BoxCubes C = och::box_cube_counts(lo, hi, w.depth);
    och_region_stats rs = region_stats(C);
    if (!C.any) {   // nothing of the box inside the tree
        ++w.strokes;
        if (out) *out = rs;
        return OCH_OK;
    }
    const int T = id ? C.top : 0;
    uint64_t widest = 1, widest_front = 1;
    for (int h = 0; h <= w.depth; ++h) {
        if (C.cubes[h] + C.cells[h] >= kRegionLimit) return och::report(OCH_E_INVALID, kRegionTooMany);
        widest = std::max(widest, C.cubes[h] + C.cells[h]);
        widest_front = std::max(widest_front, C.cells[h]);
    }
    // before anything is interned or launched: closed forms of the box alone
    if ((uint64_t)w.used + C.n_cells + (uint64_t)T > w.S.cap) return report_build(OCH_E_CAPACITY, "och_world", "");
    rs.cubes = C.n_cubes;
    rs.cells = C.n_cells;
    if (C.top == w.depth && !id) {   // the whole tree, cleared
        region_set_root(w, 0, 0);
    } else {
        RegionPlan P;   // in the walk's order: the greatest height's cubes first
        for (int h = w.depth - 1; h >= 0; --h) {
            P.cubes[h] = C.cubes[h];
            P.cells[h] = C.cells[h];
            P.rows[h] = C.cells[h + 1];
            P.first[h] = h + 1 < w.depth ? P.first[h + 1] + P.cubes[h + 1] : 0;
        }
        RegionWork R;
        if (const int rr = region_reserve(w, C.n_cubes, widest_front, false, R)) return rr;
        if (const int ws = world_reserve(w, (uint32_t)widest + 1)) return ws;
        if (const int hs = region_head(w)) return hs;
        const RegionBox B{{C.lo[0], C.lo[1], C.lo[2]}, {C.hi[0], C.hi[1], C.hi[2]}};
        if (C.top < w.depth)
            if (const int ws = region_walk<kWalkFill, RegionBox>(w, B, R, 0, 0, P, nullptr, nullptr)) return ws;
        if (!phase("walk")) return OCH_E_HIP;
        const uint32_t *d_root = nullptr;
        if (const int ls = region_levels(w, R, P, id, T, false, &d_root)) return ls;
        if (const int fs = region_finish(w, d_root, rs)) return fs;
        if (!phase("levels")) return OCH_E_HIP;
    }
    if (id) box_union(w.now.box, region_world_box(C));
    ++w.strokes;
    region_trace(w, phase, id ? "fill" : "clear", rs);
    if (out) *out = rs;
    return OCH_OK;
}

// What a restore needs of its shape besides the classifier: the shape's
// clipped axis box (any: something of the shape lies inside the tree), whether
// it covers the whole tree, and the first sizes of the walk's buffers.
struct RegionClip {
    WorldBox box;
    bool whole = false;
    uint64_t want_cubes = 1, want_front = 1;
};

template <class Shape>
int world_restore_region(och_world &w, uint64_t snapshot, const char *who, const Shape &B, const RegionClip &C, och_region_stats rs,
                         och_region_stats *out)
{
    PhaseTimer phase = world_phase(w);
    WorldSnapshot s;
    if (const int ss = world_snapshot_of(w, snapshot, who, &s)) return ss;
    const auto done = [&] {
        ++w.strokes;
        region_trace(w, phase, "restore", rs);
        if (out) *out = rs;
        return OCH_OK;
    };
    if (!C.box.any || s.root == w.now.root) return done();   // equal ids: equal content
    WorldBox grown = C.box;   // the clipped box inside the snapshot's
    for (int a = 0; a < 3; ++a) {
        grown.lo[a] = std::max(grown.lo[a], s.box.lo[a]);
        grown.hi[a] = std::min(grown.hi[a], s.box.hi[a]);
        grown.any = grown.any && s.box.any && grown.lo[a] < grown.hi[a];
    }
    if (C.whole) {   // the whole tree
        region_set_root(w, s.root, s.root_mask);
        rs.cubes = 1;
        box_union(w.now.box, grown);
        return done();
    }
    RegionWork R;
    RegionPlan P;
    // the buffers start at what a fill of the shape would take where that is small (a restore's cubes
    // and cells are subsets of the fill's) and grow with what the walk finds: a level that outgrows
    // them ends the walk, which starts over from the roots
    uint64_t want_cubes = C.want_cubes, want_front = C.want_front;
    for (;;) {
        if (const int rr = region_reserve(w, want_cubes, want_front, true, R)) return rr;
        uint64_t grow_cubes = 0, grow_front = 0;
        if (const int ws = region_walk<kWalkRestore, Shape>(w, B, R, w.now.root, s.root, P, &grow_cubes, &grow_front)) return ws;
        if (!grow_cubes && !grow_front) break;
        if (grow_cubes > want_cubes) want_cubes = std::max(grow_cubes, 2 * want_cubes);
        if (grow_front > want_front) want_front = std::max(grow_front, 2 * want_front);
    }
    if (!phase("walk")) return OCH_E_HIP;
    uint64_t widest = 1;
    for (int h = 0; h < w.depth; ++h) {
        rs.cubes += P.cubes[h];
        widest = std::max(widest, P.cubes[h] + P.cells[h]);
    }
    if (!rs.cubes) return done();   // the two states differ outside the box only
    if (widest >= kRegionLimit) return och::report(OCH_E_INVALID, kRegionTooMany);
    if (const int ws = world_reserve(w, (uint32_t)widest + 1)) return ws;
    // before anything is interned: a rebuilt row is a cell the walk expanded
    if ((uint64_t)w.used + P.front > w.S.cap) return report_build(OCH_E_CAPACITY, "och_world", "");
    if (const int hs = region_head(w)) return hs;
    const uint32_t *d_root = nullptr;
    if (const int ls = region_levels(w, R, P, 0, 0, true, &d_root)) return ls;
    if (const int fs = region_finish(w, d_root, rs)) return fs;
    if (!phase("levels")) return OCH_E_HIP;
    for (int h = 0; h < w.depth; ++h) rs.cells += P.rows[h];
    box_union(w.now.box, grown);
    return done();
}

constexpr uint64_t kRestoreCubes = 1u << 16, kRestoreFront = 1u << 14;   // a restore's first buffers, at most

RegionClip region_clip(const och::BoxCubes &C, int depth)
{
    RegionClip clip;
    clip.box = region_world_box(C);
    clip.whole = C.top == depth;
    clip.want_cubes = std::min<uint64_t>(C.n_cubes, kRestoreCubes);
    for (int h = 0; h <= depth; ++h) clip.want_front = std::max(clip.want_front, std::min<uint64_t>(C.cells[h], kRestoreFront));
    return clip;
}

int world_restore_box(och_world &w, uint64_t snapshot, const int32_t lo[3], const int32_t hi[3], och_region_stats *out)
{
    const och::BoxCubes C = och::box_cube_counts(lo, hi, w.depth);
    const RegionBox B{{C.lo[0], C.lo[1], C.lo[2]}, {C.hi[0], C.hi[1], C.hi[2]}};
    return world_restore_region(w, snapshot, "och_world_restore_box", B, region_clip(C, w.depth), region_stats(C), out);
}

// A ball against a tree of `depth`, on the host: its clipped axis box, what the
// root cell is to it, and upper bounds of what its walk finds.  A straddling
// cell of side s meets the sphere's surface, so it lies in the shell of radii
// r -+ s sqrt 3 around the centre: cells[H] <= the shell's volume / s^3, and
// at most the cells of height H that the axis box touches, and at most eight
// times the level above.  The cubes of a ball number about 4 pi r^2: `cubes`
// is an estimate with room, not a bound, and at most 7 per straddling cell.
// Nothing rests on either: region_walk_dev checks every level against them.
struct BallPlan {
    WorldBox box;
    int root = 0;                // region_class of the root cell: 0 outside, 1 straddling, 2 inside
    uint64_t cells[22] = {0};    // 1 <= cells[H], H = 1 .. depth
    uint64_t cubes = 1;
};

BallPlan ball_plan(const int32_t c2[3], uint32_t diameter, int depth)
{
    BallPlan b;
    b.box.any = och::ball_axis_box(c2, diameter, depth, b.box.lo, b.box.hi);
    if (!b.box.any) return b;
    const int32_t origin[3] = {0, 0, 0};
    b.root = och::ball_class(och::make_ball(c2, diameter), origin, depth);
    const double r = 0.5 * diameter, pi = 3.14159265358979323846;
    uint64_t sum = 0;
    b.cells[depth] = 1;
    for (int H = depth - 1; H >= 1; --H) {
        const double s = (double)((uint64_t)1 << H), out = r + s * 1.7320508075688773, in = std::max(0.0, r - s * 1.7320508075688773);
        const double shell = 4.0 / 3.0 * pi * (out * out * out - in * in * in) / (s * s * s) * 1.001 + 8.0;
        uint64_t touch = 1;
        for (int a = 0; a < 3; ++a) touch *= (uint64_t)(((b.box.hi[a] - 1) >> H) - (b.box.lo[a] >> H) + 1);
        b.cells[H] = std::max<uint64_t>(1, std::min({touch, 8 * b.cells[H + 1], shell < 1e18 ? (uint64_t)shell : ~(uint64_t)0}));
    }
    for (int H = 1; H <= depth; ++H) sum += 7 * b.cells[H];
    const double area = 1.25 * pi * (double)diameter * (double)diameter + 64.0;
    b.cubes = std::min<uint64_t>(sum, area < 1e18 ? (uint64_t)area : ~(uint64_t)0);
    return b;
}

RegionClip region_clip(const BallPlan &C, int depth)
{
    RegionClip clip;
    clip.box = C.box;
    clip.box.any = C.box.any && C.root != 0;
    clip.whole = C.root == 2;
    clip.want_cubes = std::min(C.cubes, kRestoreCubes);
    for (int H = 1; H <= depth; ++H) clip.want_front = std::max(clip.want_front, std::min(C.cells[H], kRestoreFront));
    return clip;
}

och_region_stats region_stats(const WorldBox &b)
{
    och_region_stats rs{};
    std::memcpy(rs.lo, b.lo, sizeof rs.lo);
    std::memcpy(rs.hi, b.hi, sizeof rs.hi);
    return rs;
}

// A fill's first buffers and launched frontiers, at most: the bounds are loose (a ball clipped by the
// tree, a shell several cells thick), a walk interns nothing and costs little beside the levels, and
// a stroke that needs more walks again with it.
constexpr uint64_t kFillCubes = 1u << 17, kFillFront = 1u << 15;

int world_fill_sphere(och_world &w, const int32_t c2[3], uint32_t diameter, uint32_t id, och_region_stats *out)
{
    PhaseTimer phase = world_phase(w);
    if (const char *range = och::ball_range_error(c2, diameter)) return och::fail(OCH_E_INVALID, "och_world_fill_sphere: %s", range);
    const BallPlan C = ball_plan(c2, diameter, w.depth);
    och_region_stats rs = region_stats(C.box);
    if (!C.box.any || C.root == 0) {   // no voxel of the ball inside the tree
        ++w.strokes;
        if (out) *out = rs;
        return OCH_OK;
    }
    const RegionBall B = och::make_ball(c2, diameter);
    RegionWork R;
    RegionPlan P;
    int T = 0;
    if (C.root == 2) {   // the whole tree: one cube of height depth, no cell
        T = id ? w.depth : 0;
        rs.cubes = 1;
    } else {
        uint64_t want_cubes = std::min(C.cubes, kFillCubes), cap_front = kFillFront, slack = 1;
        for (;;) {
            uint64_t bound[22] = {0}, n_front = 1;
            for (int H = 1; H <= w.depth; ++H) {
                bound[H] = std::min(C.cells[H] * slack, cap_front);
                n_front = std::max(n_front, bound[H]);
            }
            if (const int rr = region_reserve(w, want_cubes, n_front, false, R)) return rr;
            uint64_t grow_cubes = 0, grow_front = 0;
            int grow_at = 0;
            if (const int ws = region_walk_dev(w, B, R, bound, P, &grow_cubes, &grow_front, &grow_at)) return ws;
            if (!grow_cubes && !grow_front) break;
            // a frontier grows about fourfold a level down to height 1; the cubes, once short, get the whole estimate
            if (grow_at >= 1 && grow_front > bound[grow_at]) {
                while (C.cells[grow_at] * slack < grow_front) slack *= 2;   // the bound itself fell short: nothing rests on it
                cap_front = std::min(kRegionFrontLimit, std::max(2 * cap_front, grow_front << (2 * std::min(grow_at - 1, 8))));
            }
            if (grow_cubes > want_cubes) want_cubes = std::max({grow_cubes, 2 * want_cubes, std::min(C.cubes, kRegionLimit)});
        }
        for (int h = 0; h < w.depth; ++h) {
            rs.cubes += P.cubes[h];
            if (P.cubes[h]) T = id ? h : 0;
        }
        rs.cells = P.front;
    }
    if (!phase("walk")) return OCH_E_HIP;
    // after the walk, before anything is interned: the ball and the depth alone decide
    if ((uint64_t)w.used + rs.cells + (uint64_t)T > w.S.cap) return report_build(OCH_E_CAPACITY, "och_world", "");
    if (C.root == 2 && !id) {   // the whole tree, cleared
        region_set_root(w, 0, 0);
    } else {
        uint64_t widest = 1;
        for (int h = 0; h < w.depth; ++h) widest = std::max(widest, P.cubes[h] + P.cells[h]);
        if (widest >= kRegionLimit) return och::report(OCH_E_INVALID, kRegionTooMany);
        if (const int ws = world_reserve(w, (uint32_t)widest + 1)) return ws;
        if (const int hs = region_head(w)) return hs;
        const uint32_t *d_root = nullptr;
        if (const int ls = region_levels(w, R, P, id, T, false, &d_root)) return ls;
        if (const int fs = region_finish(w, d_root, rs)) return fs;
        if (!phase("levels")) return OCH_E_HIP;
    }
    if (id) box_union(w.now.box, C.box);
    ++w.strokes;
    region_trace(w, phase, id ? "fill sphere" : "clear sphere", rs);
    if (out) *out = rs;
    return OCH_OK;
}

int world_restore_sphere(och_world &w, uint64_t snapshot, const int32_t c2[3], uint32_t diameter, och_region_stats *out)
{
    if (const char *range = och::ball_range_error(c2, diameter)) return och::fail(OCH_E_INVALID, "och_world_restore_sphere: %s", range);
    const BallPlan C = ball_plan(c2, diameter, w.depth);
    return world_restore_region(w, snapshot, "och_world_restore_sphere", och::make_ball(c2, diameter), region_clip(C, w.depth),
                                region_stats(C.box), out);
}

}  // namespace

OCH_API int och_world_fill_box(och_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t id, och_region_stats *stats)
{
    if (!lo || !hi) return och::report(OCH_E_INVALID, "och_world_fill_box: lo or hi is NULL");
    return world_call(w, "och_world_fill_box", "och_world", kBreaks, kOwnTexts, [&] { return world_fill_box(*w, lo, hi, id, stats); });
}

OCH_API int och_world_restore_box(och_world *w, uint64_t snapshot, const int32_t lo[3], const int32_t hi[3],
                                  och_region_stats *stats)
{
    if (!lo || !hi) return och::report(OCH_E_INVALID, "och_world_restore_box: lo or hi is NULL");
    return world_call(w, "och_world_restore_box", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_restore_box(*w, snapshot, lo, hi, stats); });
}

OCH_API int och_world_fill_sphere(och_world *w, const int32_t centre2[3], uint32_t diameter, uint32_t id, och_region_stats *stats)
{
    if (!centre2) return och::report(OCH_E_INVALID, "och_world_fill_sphere: centre2 is NULL");
    return world_call(w, "och_world_fill_sphere", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_fill_sphere(*w, centre2, diameter, id, stats); });
}

OCH_API int och_world_restore_sphere(och_world *w, uint64_t snapshot, const int32_t centre2[3], uint32_t diameter,
                                     och_region_stats *stats)
{
    if (!centre2) return och::report(OCH_E_INVALID, "och_world_restore_sphere: centre2 is NULL");
    return world_call(w, "och_world_restore_sphere", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_restore_sphere(*w, snapshot, centre2, diameter, stats); });
}
