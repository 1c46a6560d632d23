// och_world_paint.h -- strokes of a resident world that are conditional on
// the old voxel (och_world_paint_box, och_world_paint_sphere): inside the shape
// every voxel v becomes pred(v) ? id : v, pred(v) = (v == match) != when.
// Paint (the solid voxels), fill-under (the empty ones), replace, erase or
// keep one material.  Included by och_builder.cpp only, after
// och_world_region.h, whose walk, levels and finish it runs.
//
// A cube of side 2^h inside the shape is one child word, as for a fill.  Its
// new word is a function of the subtree its old word names, and in a DAG that
// function is evaluated once per distinct node, not once per position: the
// stroke costs the shape's surface plus the distinct nodes under it.  Heights
// are counted as the header does: a voxel is height 0, a node of height h >= 1
// has eight children of height h - 1 (the store keeps it with level h - 1).
// Three phases, each dispatch reading only what earlier ones wrote (k_intern's
// rule, och_dag.h):
//
// The walk, top down, is a restore's with one root (region_walk<kWalkPaint>):
// a frontier entry is a straddling open cell's key and id.  A child the
// predicate cannot touch (an empty cube or a voxel with !pred(word)) is
// dropped, an open child inside the shape is a cube (key, old word), an open
// child that straddles is a cell of the next frontier.
//
// The map.  M_h sends a node of height h to the node of the same subtree with
// every voxel through pred.  Down, from the greatest height with a cube: the
// candidates of height h are the cubes' words of that height and the children
// of N_(h+1); a radix sort of the 32-bit ids, head flags, a scan and a compact
// make N_h, the sorted distinct non-zero ones (4 bytes read back a height).
// Nothing is sized, cleared or launched by the store's capacity or the shape's
// volume, and there is no atomic.  Up, from height 1: k_paint_rows writes the
// mapped row of every node of N_h, one thread per (node, child) -- a voxel
// through pred, an empty child U_(h-1) where pred(0) and id != 0, a node
// M_(h-1)[its rank in N_(h-1)], found by binary search -- then
// k_intern_rows<true> and k_settle, unchanged, leave the ids as M_h.  A row
// that maps to zeros is word 0 and never probes the table.  U_h, the uniform
// subtree of id, is one extra row of height h's batch (k_region_uniform), so
// it exists a dispatch before anything reads it.  k_paint_lookup then turns
// every cube's old word into its new one: M_h[old], U_h for an empty cube,
// pred for a voxel.
//
// The levels are region_levels with those words and read_rows (a straddling
// open cell may have no cube beneath it), then region_finish.  A cube whose
// word did not change is harmless: its rows are found in the store.
//
// Capacity, after the walk and the map's way down and before the first intern:
// used + cells + nodes + T, one id a rebuilt cell, one a mapped node, one a
// uniform subtree.  The map's buffer (och_world.d_paint) starts small; a height
// that outgrows it ends the way down, which starts over with more.
#pragma once
#include "och_world_region.h"

namespace {

// The candidates of height h: the children of the `above` nodes of N_(h+1)
// (an interior word at or above cap reads as empty), then the words of the
// n_cubes cubes of height h.
__global__ __launch_bounds__(256) void k_paint_candidates(GpuStore S, const uint32_t *__restrict__ nodes_above, uint32_t above,
                                                          const uint32_t *__restrict__ cube_words, uint32_t n_cubes,
                                                          uint32_t *__restrict__ cand)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n_children = (size_t)above * 8;
    if (q >= n_children + n_cubes) return;
    uint32_t c;
    if (q < n_children) {
        c = S.nodes[(size_t)nodes_above[q >> 3] * 8 + (q & 7u)];
        c = c < S.cap ? c : 0u;
    } else {
        c = cube_words[q - n_children];
    }
    cand[q] = c;
}

// flags[i] = sorted[i] is the first of a non-zero id.
__global__ __launch_bounds__(256) void k_paint_heads(const uint32_t *__restrict__ sorted, uint32_t n, uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = sorted[i];
    flags[i] = v != 0 && (i == 0 || sorted[i - 1] != v);
}

// nodes[pos[i] - 1] = sorted[i] for every head: the distinct ids, ascending; `room` of them at most.
__global__ __launch_bounds__(256) void k_paint_compact(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ flags,
                                                       const uint32_t *__restrict__ pos, uint32_t n, uint32_t room,
                                                       uint32_t *__restrict__ nodes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const uint32_t p = pos[i] - 1u;
    if (p < room) nodes[p] = sorted[i];
}

// The rank of id in the ascending list[n] that holds it (n >= 1).
__device__ inline uint32_t paint_rank(const uint32_t *__restrict__ list, uint32_t n, uint32_t id)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return min(lo, n - 1u);
}

// What a stroke writes: pred(v) ? id : v, and whether an empty position turns solid.
struct PaintRule {
    uint32_t when, match, id;
    __host__ __device__ bool pred(uint32_t v) const { return paint_pred(when, match, v); }
    __host__ __device__ bool grows() const { return pred(0) && id != 0; }
};

// The mapped rows of the n nodes of N_h: thread q = 8 i + k is child k of
// nodes[i], eight nodes a wavefront, a row's 32 bytes one coalesced read.  At
// height 1 the voxel through pred; above, an empty child becomes U_(h-1)
// (*uni; without uni: id, the uniform voxel) where the rule grows, and a node
// becomes mapped_below[its rank in nodes_below[n_below]].
__global__ __launch_bounds__(256) void k_paint_rows(GpuStore S, const uint32_t *__restrict__ nodes, uint32_t n, int h,
                                                    const uint32_t *__restrict__ nodes_below, const uint32_t *__restrict__ mapped_below,
                                                    uint32_t n_below, const uint32_t *__restrict__ uni, PaintRule rule,
                                                    uint32_t *__restrict__ rows)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)n * 8) return;
    uint32_t c = S.nodes[(size_t)nodes[q >> 3] * 8 + (q & 7u)];
    if (h == 1) {
        c = rule.pred(c) ? rule.id : c;
    } else {
        c = c < S.cap ? c : 0u;
        if (!c)
            c = rule.grows() ? (uni ? *uni : rule.id) : 0u;
        else
            c = n_below ? mapped_below[paint_rank(nodes_below, n_below, c)] : 0u;
    }
    rows[q] = c;
}

// The n cubes of height h, their old words turned into the new ones in place.
__global__ __launch_bounds__(256) void k_paint_lookup(uint32_t *__restrict__ words, uint32_t n, int h, const uint32_t *__restrict__ nodes,
                                                      const uint32_t *__restrict__ mapped, uint32_t n_nodes,
                                                      const uint32_t *__restrict__ uni, PaintRule rule)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t old = words[j];
    uint32_t now;
    if (h == 0)
        now = rule.pred(old) ? rule.id : old;
    else if (!old)
        now = rule.grows() && uni ? *uni : 0u;
    else
        now = n_nodes ? mapped[paint_rank(nodes, n_nodes, old)] : 0u;
    words[j] = now;
}

// The one cube of a shape that covers the tree: key 0 at height depth, its word the root.
__global__ __launch_bounds__(64) void k_paint_whole(uint64_t *__restrict__ cubes, uint32_t *__restrict__ cube_words, uint32_t root)
{
    if (blockIdx.x || threadIdx.x) return;
    cubes[0] = 0;
    cube_words[0] = root;
}

// The map's buffer (och_world.d_paint), carved for one stroke: the nodes of
// every height and what they map to, side by side (height h's from
// PaintPlan.off[h], one word more than its nodes: U_h), and the candidates'
// sort, flags and scan.
struct PaintWork {
    uint32_t *nodes = nullptr, *mapped = nullptr;
    uint64_t n_nodes = 0;
    uint32_t *cand[2] = {nullptr, nullptr}, *flags = nullptr, *pos = nullptr;
    uint64_t n_cand = 0;
    void *temp = nullptr;
    size_t temp_bytes = 0;
};

struct PaintPlan {
    uint64_t count[23] = {0};   // |N_h|
    uint64_t off[23] = {0};
    uint64_t nodes = 0;         // summed
    uint64_t widest = 0;
};

int paint_reserve(och_world &w, uint64_t n_nodes, uint64_t n_cand, PaintWork &M)
{
    uint32_t *k = nullptr;
    size_t sort_bytes = 0, scan_bytes = 0;
    GPU_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, k, k, (int)n_cand, 0, 32, w.st));
    GPU_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, k, k, (int)n_cand, w.st));
    M.temp_bytes = std::max(sort_bytes, scan_bytes);
    size_t bytes = 0;
    auto place = [&](size_t n) {   // 256-byte aligned, like the buffer
        const size_t at = bytes;
        bytes += (n + 255) & ~(size_t)255;
        return at;
    };
    const size_t at_nodes = place(n_nodes * 4), at_mapped = place(n_nodes * 4), at_c0 = place(n_cand * 4), at_c1 = place(n_cand * 4),
                 at_flags = place(n_cand * 4), at_pos = place(n_cand * 4), at_temp = place(M.temp_bytes);
    if (w.d_paint.reserve(bytes) != hipSuccess) return OCH_E_NOMEM;
    uint8_t *p = w.d_paint.d;
    M.nodes = reinterpret_cast<uint32_t *>(p + at_nodes);
    M.mapped = reinterpret_cast<uint32_t *>(p + at_mapped);
    M.n_nodes = n_nodes;
    M.cand[0] = reinterpret_cast<uint32_t *>(p + at_c0);
    M.cand[1] = reinterpret_cast<uint32_t *>(p + at_c1);
    M.flags = reinterpret_cast<uint32_t *>(p + at_flags);
    M.pos = reinterpret_cast<uint32_t *>(p + at_pos);
    M.n_cand = n_cand;
    M.temp = p + at_temp;
    return OCH_OK;
}

// The map's way down from height `top`: N_h for every height, in M.nodes at
// Q.off[h].  *grow_nodes / *grow_cand != 0 on return: a height outgrew the
// buffer, the caller reserves that much and starts over.
int paint_down(och_world &w, const RegionWork &R, const RegionPlan &P, int top, const PaintWork &M, PaintPlan &Q, uint64_t *grow_nodes,
               uint64_t *grow_cand)
{
    const hipStream_t st = w.st;
    int id_bits = 1;
    while (id_bits < 32 && ((uint64_t)1 << id_bits) < w.S.cap) ++id_bits;
    Q = PaintPlan{};
    uint64_t at = 0, above = 0, above_at = 0;
    for (int h = top; h >= 1; --h) {
        const uint64_t n_cand = above * 8 + P.cubes[h];
        if (n_cand >= kRegionLimit) return och::report(OCH_E_INVALID, "och_world: a height of the paint holds 2^31 candidates or more");
        if (n_cand > M.n_cand || at + 1 > M.n_nodes) {
            *grow_cand = std::max<uint64_t>(n_cand, 1);
            *grow_nodes = at + 1;
            return OCH_OK;
        }
        Q.off[h] = at;
        uint32_t total = 0;
        if (n_cand) {
            hipLaunchKernelGGL(k_paint_candidates, blocks(n_cand), dim3(256), 0, st, w.S, M.nodes + above_at, (uint32_t)above,
                               R.cube_words + P.first[h], (uint32_t)P.cubes[h], M.cand[0]);
            GPU_TRY(hipGetLastError());
            size_t tb = M.temp_bytes;
            GPU_TRY(hipcub::DeviceRadixSort::SortKeys(M.temp, tb, M.cand[0], M.cand[1], (int)n_cand, 0, id_bits, st));
            hipLaunchKernelGGL(k_paint_heads, blocks(n_cand), dim3(256), 0, st, M.cand[1], (uint32_t)n_cand, M.flags);
            GPU_TRY(hipGetLastError());
            tb = M.temp_bytes;
            GPU_TRY(hipcub::DeviceScan::InclusiveSum(M.temp, tb, M.flags, M.pos, (int)n_cand, st));
            if (const int rs = world_read_back(w, {{&total, M.pos + (n_cand - 1), 4}})) return rs;
            total = (uint32_t)std::min<uint64_t>(total, n_cand);
            if (at + total + 1 > M.n_nodes) {
                *grow_nodes = at + total + 1;
                return OCH_OK;
            }
            if (total) {
                hipLaunchKernelGGL(k_paint_compact, blocks(n_cand), dim3(256), 0, st, M.cand[1], M.flags, M.pos, (uint32_t)n_cand, total,
                                   M.nodes + at);
                GPU_TRY(hipGetLastError());
            }
        }
        Q.count[h] = total;
        Q.nodes += total;
        Q.widest = std::max<uint64_t>(Q.widest, total);
        above = total;
        above_at = at;
        at += (uint64_t)total + 1;
    }
    return OCH_OK;
}

// The map's way up: M_h for every height from 1 to top and, where the rule
// grows, U_h, then every cube's new word in place of its old one.
int paint_up(och_world &w, const RegionWork &R, const RegionPlan &P, int top, int T, const PaintWork &M, const PaintPlan &Q,
             const PaintRule &rule)
{
    const hipStream_t st = w.st;
    const EditWork &W = w.W;
    const uint32_t *uni = nullptr;   // U_(h-1); U_0 is the id itself
    for (int h = 1; h <= top; ++h) {
        const uint32_t n = (uint32_t)Q.count[h], extra = h <= T ? 1u : 0u;
        if (!n && !extra) continue;
        if (n) {
            hipLaunchKernelGGL(k_paint_rows, blocks((size_t)n * 8), dim3(256), 0, st, w.S, M.nodes + Q.off[h], n, h,
                               h > 1 ? M.nodes + Q.off[h - 1] : nullptr, h > 1 ? M.mapped + Q.off[h - 1] : nullptr,
                               h > 1 ? (uint32_t)Q.count[h - 1] : 0u, uni, rule, W.rows);
            GPU_TRY(hipGetLastError());
        }
        if (extra) hipLaunchKernelGGL(k_region_uniform, dim3(1), dim3(64), 0, st, W.rows + (size_t)n * 8, uni, rule.id);
        const uint32_t rows = n + extra;
        GpuLevel L{W.rows, 0, 0, rows, h - 1, 1};
        hipLaunchKernelGGL(k_intern_rows<true>, blocks(rows), dim3(256), 0, st, w.S, L, W.rep, W.slot);
        hipLaunchKernelGGL(k_settle, blocks(rows), dim3(256), 0, st, w.S, rows, W.rep, W.slot, M.mapped + Q.off[h], nullptr);
        GPU_TRY(hipGetLastError());
        uni = extra ? M.mapped + Q.off[h] + n : nullptr;
    }
    for (int h = 0; h <= top; ++h) {
        const uint32_t n = (uint32_t)P.cubes[h];
        if (!n) continue;
        const uint32_t *u = h >= 1 && h <= T ? M.mapped + Q.off[h] + Q.count[h] : nullptr;
        hipLaunchKernelGGL(k_paint_lookup, blocks(n), dim3(256), 0, st, R.cube_words + P.first[h], n, h, h ? M.nodes + Q.off[h] : nullptr,
                           h ? M.mapped + Q.off[h] : nullptr, h ? (uint32_t)Q.count[h] : 0u, u, rule);
        GPU_TRY(hipGetLastError());
    }
    return OCH_OK;
}

constexpr uint64_t kPaintNodes = 1u << 16, kPaintCand = 1u << 17;   // the map's first buffer

template <class Shape>
int world_paint_region(och_world &w, const Shape &shape, const RegionClip &C, const PaintRule &rule, och_paint_stats ps,
                       och_paint_stats *out)
{
    PhaseTimer phase = world_phase(w);
    const auto done = [&] {
        ++w.strokes;
        if (phase.on)
            std::fprintf(stderr, "[och_build] world: paint, %llu cubes, %llu cells, %llu nodes, %llu new ids, %u of %u used\n",
                         (unsigned long long)ps.cubes, (unsigned long long)ps.cells, (unsigned long long)ps.nodes,
                         (unsigned long long)ps.new_ids, w.used, w.S.cap);
        if (out) *out = ps;
        return OCH_OK;
    };
    const uint32_t root = w.now.root;
    // nothing of the shape inside the tree, or a root cell the predicate cannot touch
    if (!C.box.any || !(root || rule.pred(0))) return done();
    const int depth = w.depth;
    RegionWork R;
    RegionPlan P;
    if (C.whole) {   // one cube of height depth, no cell
        if (const int rr = region_reserve(w, 1, 1, true, R)) return rr;
        hipLaunchKernelGGL(k_paint_whole, dim3(1), dim3(64), 0, w.st, R.cubes, R.cube_words, root);
        GPU_TRY(hipGetLastError());
        P.cubes[depth] = 1;
    } else {
        const RegionPaint<Shape> B{shape, rule.when, rule.match};
        uint64_t want_cubes = C.want_cubes, want_front = C.want_front;
        for (;;) {
            if (const int rr = region_reserve(w, want_cubes, want_front, true, R)) return rr;
            uint64_t grow_cubes = 0, grow_front = 0;
            if (const int ws = region_walk<kWalkPaint, RegionPaint<Shape>>(w, B, R, root, 0, P, &grow_cubes, &grow_front)) return ws;
            if (!grow_cubes && !grow_front) break;
            if (grow_cubes > want_cubes) want_cubes = std::max(grow_cubes, 2 * want_cubes);
            if (grow_front > want_front) want_front = std::max(grow_front, 2 * want_front);
        }
        ps.cells = P.front;
    }
    if (!phase("walk")) return OCH_E_HIP;
    int top = 0;
    uint64_t widest = 1;
    for (int h = 0; h <= depth; ++h) {
        ps.cubes += P.cubes[h];
        if (P.cubes[h]) top = h;
        widest = std::max(widest, P.cubes[h] + P.cells[h]);
    }
    if (!ps.cubes) return done();   // no open cube inside the shape: nothing changes
    if (widest >= kRegionLimit) return och::report(OCH_E_INVALID, kRegionTooMany);
    const int T = rule.grows() ? top : 0;
    PaintWork M;
    PaintPlan Q;
    uint64_t want_nodes = kPaintNodes, want_cand = kPaintCand;
    for (int h = 1; h <= top; ++h) want_cand = std::max(want_cand, P.cubes[h]);
    for (;;) {
        if (const int rr = paint_reserve(w, want_nodes, want_cand, M)) return rr;
        uint64_t grow_nodes = 0, grow_cand = 0;
        if (const int ds = paint_down(w, R, P, top, M, Q, &grow_nodes, &grow_cand)) return ds;
        if (!grow_nodes && !grow_cand) break;
        if (grow_nodes > want_nodes) want_nodes = std::max(grow_nodes, 2 * want_nodes);
        if (grow_cand > want_cand) want_cand = std::max(grow_cand, 2 * want_cand);
    }
    ps.nodes = Q.nodes;
    if (!phase("map down")) return OCH_E_HIP;
    // after the walk and the way down, before anything is interned: content, shape and predicate alone decide
    if ((uint64_t)w.used + ps.cells + ps.nodes + (uint64_t)T > w.S.cap) return report_build(OCH_E_CAPACITY, "och_world", "");
    if (const int ws = world_reserve(w, (uint32_t)std::max(widest, Q.widest + 1) + 1)) return ws;
    if (const int hs = region_head(w)) return hs;
    if (const int us = paint_up(w, R, P, top, T, M, Q, rule)) return us;
    if (!phase("map up")) return OCH_E_HIP;
    const uint32_t *d_root = R.cube_words;   // a shape over the whole tree: its one cube's new word
    if (!C.whole)
        if (const int ls = region_levels(w, R, P, 0, 0, true, &d_root)) return ls;
    och_region_stats rs{};
    if (const int fs = region_finish(w, d_root, rs)) return fs;
    ps.new_ids = rs.new_ids;
    if (!phase("levels")) return OCH_E_HIP;
    if (rule.grows()) box_union(w.now.box, C.box);
    return done();
}

och_paint_stats paint_stats(const WorldBox &b)
{
    och_paint_stats ps{};
    std::memcpy(ps.lo, b.lo, sizeof ps.lo);
    std::memcpy(ps.hi, b.hi, sizeof ps.hi);
    return ps;
}

const char *kPaintWhen = "when is OCH_WHEN_IS (0) or OCH_WHEN_IS_NOT (1)";

int world_paint_box(och_world &w, const int32_t lo[3], const int32_t hi[3], int when, uint32_t match, uint32_t id, och_paint_stats *out)
{
    const och::BoxCubes C = och::box_cube_counts(lo, hi, w.depth);
    const RegionClip clip = region_clip(C, w.depth);
    const RegionBox B{{C.lo[0], C.lo[1], C.lo[2]}, {C.hi[0], C.hi[1], C.hi[2]}};
    return world_paint_region(w, B, clip, PaintRule{(uint32_t)when, match, id}, paint_stats(clip.box), out);
}

int world_paint_sphere(och_world &w, const int32_t c2[3], uint32_t diameter, int when, uint32_t match, uint32_t id, och_paint_stats *out)
{
    if (const char *range = och::ball_range_error(c2, diameter)) return och::fail(OCH_E_INVALID, "och_world_paint_sphere: %s", range);
    const BallPlan C = ball_plan(c2, diameter, w.depth);
    return world_paint_region(w, och::make_ball(c2, diameter), region_clip(C, w.depth), PaintRule{(uint32_t)when, match, id},
                              paint_stats(C.box), out);
}

}  // namespace

OCH_API int och_world_paint_box(och_world *w, const int32_t lo[3], const int32_t hi[3], int when, uint32_t match, uint32_t id,
                                och_paint_stats *stats)
{
    if (!lo || !hi) return och::report(OCH_E_INVALID, "och_world_paint_box: lo or hi is NULL");
    if (when != OCH_WHEN_IS && when != OCH_WHEN_IS_NOT) return och::fail(OCH_E_INVALID, "och_world_paint_box: %s", kPaintWhen);
    return world_call(w, "och_world_paint_box", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_paint_box(*w, lo, hi, when, match, id, stats); });
}

OCH_API int och_world_paint_sphere(och_world *w, const int32_t centre2[3], uint32_t diameter, int when, uint32_t match, uint32_t id,
                                   och_paint_stats *stats)
{
    if (!centre2) return och::report(OCH_E_INVALID, "och_world_paint_sphere: centre2 is NULL");
    if (when != OCH_WHEN_IS && when != OCH_WHEN_IS_NOT) return och::fail(OCH_E_INVALID, "och_world_paint_sphere: %s", kPaintWhen);
    return world_call(w, "och_world_paint_sphere", "och_world", kBreaks, kOwnTexts,
                      [&] { return world_paint_sphere(*w, centre2, diameter, when, match, id, stats); });
}
