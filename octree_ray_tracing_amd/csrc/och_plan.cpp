// och_plan.cpp -- launch planning (och_plan.h): the launch order of a frame's
// workgroups from their measured costs, its split form, and the chunk costs of a
// row deal.  och_api.cpp runs the planning renders and uploads what these return.
// The pure planners: vectors and integers in and out, no HIP call, no pool; external
// linkage, so that a host program can call them (tests/test_plan_host.py pins them).
#include "och_plan.h"

#include <algorithm>
#include <utility>

namespace och {
namespace plan {

// The stable costliest-first permutation of the workgroups.
std::vector<uint32_t> by_cost(const std::vector<uint32_t> &costs)
{
    std::vector<uint32_t> order(costs.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return costs[a] > costs[b]; });
    return order;
}

// The launch order from the costliest-first list (OCH_OPT_PLAN): 0 = all
// workgroups costliest first; P in 1..99 = the costliest P % first, then the
// rest in natural order (the tails a frame ends on start early, while the bulk
// keeps the raster order's mix of sky and terrain tiles); 100 = alternate the
// costliest and the cheapest left.  Default 10: with frames in flight, every
// frame starting all its costly tiles at once cost 3.5 % over long runs
// (profiles/r03/ab/plan_*).
void shape(std::vector<uint32_t> &order, int mode)
{
    const size_t n = order.size();
    if (mode <= 0 || n < 2) return;
    std::vector<uint32_t> out;
    out.reserve(n);
    if (mode >= 100) {
        for (size_t i = 0, j = n - 1; i <= j && j < n; ++i, --j) {
            out.push_back(order[i]);
            if (j != i) out.push_back(order[j]);
            if (j == 0) break;
        }
    } else {
        const size_t head = n * (size_t)mode / 100;
        std::vector<uint8_t> taken(n, 0);
        for (size_t i = 0; i < head; ++i) {
            out.push_back(order[i]);
            taken[order[i]] = 1;
        }
        for (uint32_t b = 0; b < n; ++b)
            if (!taken[b]) out.push_back(b);
    }
    order.swap(out);
}

// Grouped per XCD (OCH_OPT_TILE_ORDER = 3): workgroup slot i runs on XCD
// i % 8, so deal 64x64-pixel supertiles over the XCDs (each XCD's L2 then
// holds the nodes of its own neighbouring tiles) and keep the costliest-
// first order within each XCD's list.  Workgroup b starts at tile b * (block / 64).
std::vector<uint32_t> group_by_xcd(const std::vector<uint32_t> &order, uint32_t tiles_x, uint32_t tiles_y, uint32_t block)
{
    const uint32_t stx = (tiles_x + 7) / 8, sty = (tiles_y + 7) / 8;
    std::vector<std::vector<uint32_t>> lists(8);
    for (uint32_t b : order) {
        const uint32_t tile = b * (block / 64), view = tile / (tiles_x * tiles_y), t = tile % (tiles_x * tiles_y);
        const uint32_t super = (view * sty + (t / tiles_x) / 8) * stx + (t % tiles_x) / 8;
        lists[super % 8].push_back(b);
    }
    std::vector<uint32_t> grouped;
    grouped.reserve(order.size());
    std::vector<size_t> at(8, 0);
    while (grouped.size() < order.size())
        for (uint32_t x = 0; x < 8 && grouped.size() < order.size(); ++x) {
            uint32_t from = x;
            if (at[x] == lists[x].size())       // this XCD's list ran dry: the fullest other list
                for (uint32_t y = 0; y < 8; ++y)
                    if (lists[y].size() - at[y] > lists[from].size() - at[from]) from = y;
            grouped.push_back(lists[from][at[from]++]);
        }
    return grouped;
}

// A split tile's rays longer than this % of its longest walk over
// OCH_OPT_SPLIT_SEGS lanes; the others take one lane and walk whole
// (tools/split_model.c: 30 % keeps the critical path of splitting every ray
// and adds almost no work).
constexpr int kSplitRayPct = 30;

// The split form of a primary plan (OCH_OPT_SPLIT).  The tiles
// whose planning cost reaches opt_split % of the costliest one's are split:
// one counting render gives every pixel's walked PUSHes, a tile's rays longer
// than kSplitRayPct % of its longest get opt_split_segs lanes each (segment
// lanes), the others one, and its rays are packed, costliest first, into
// waves of 64 lanes with every lane of a ray in one wave (their records merge
// through that wave's LDS).  Rows of d_split_tasks: the tile, then 64 lane
// tasks (pixel | seg << 6 | log2(S) << 10, ~0 idle).  The order: the split
// waves (1 << 31 | row), then the plan's other workgroups in its order.
// Block 64 only (workgroup = tile), packed layout, tiles < 2^24, and a split
// level above the leaves; otherwise no split plan.

// One tile's waves, 64 lane tasks each, from its pixels' PUSHes (-1: outside the frame).
std::vector<uint32_t> pack_split_tile(const int cnt[64], int S)
{
    const int log2s = __builtin_ctz((unsigned)S), mx = std::max(0, *std::max_element(cnt, cnt + 64));
    auto long_ray = [&](int l) { return cnt[l] * 100 > kSplitRayPct * mx; };
    std::vector<std::pair<int, int>> rays;                  // (estimated lane cost, pixel)
    for (int l = 0; l < 64; ++l)
        if (cnt[l] >= 0) rays.push_back({long_ray(l) ? cnt[l] / S : cnt[l], l});
    std::stable_sort(rays.begin(), rays.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<uint32_t> waves, used;                      // 64 words per wave, idle at first; lanes taken
    for (const auto &r : rays) {
        const uint32_t l = (uint32_t)r.second, lanes = long_ray(r.second) ? (uint32_t)S : 1u;
        size_t w = 0;
        while (w < used.size() && used[w] + lanes > 64) ++w;
        if (w == used.size()) {
            used.push_back(0);
            waves.resize(waves.size() + 64, ~0u);
        }
        for (uint32_t s = 0; s < lanes; ++s)
            waves[w * 64 + used[w]++] = l | s << 6 | (uint32_t)(lanes > 1 ? log2s : 0) << 10;
    }
    return waves;
}

// The heavy tiles (pct % of the costliest, at most max(1, n / 16): a bound on the
// planner's work), their waves, and the split order; push: slices of rows x W.
Split split_order(const std::vector<uint16_t> &push, int W, int rows, const std::vector<uint32_t> &by_cost,
                  const std::vector<uint32_t> &order, const std::vector<uint32_t> &c, int pct, int S)
{
    Split sp;
    const uint32_t n = (uint32_t)order.size();
    if (pct <= 0 || n == 0) return sp;
    const double thr = (double)c[by_cost[0]] * pct / 100.0;
    const uint32_t cap = std::max(1u, n / 16);
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, per_view = tiles_x * (uint32_t)((rows + 7) / 8);
    std::vector<uint8_t> heavy(n, 0);
    for (uint32_t k = 0; k < n && k < cap && (double)c[by_cost[k]] >= thr; ++k, ++sp.tiles) {
        const uint32_t t = by_cost[k];
        heavy[t] = 1;
        const uint32_t view = t / per_view, tt = t % per_view, ty = tt / tiles_x, tx = tt % tiles_x;
        int cnt[64];
        for (int l = 0; l < 64; ++l) {
            const uint32_t col = tx * 8 + (uint32_t)(l % 8), srow = ty * 8 + (uint32_t)(l / 8);
            cnt[l] = col < (uint32_t)W && srow < (uint32_t)rows ? push[((size_t)view * rows + srow) * W + col] : -1;
        }
        const std::vector<uint32_t> waves = pack_split_tile(cnt, S);
        for (size_t w = 0; w < waves.size(); w += 64) {
            sp.order.push_back(0x80000000u | (uint32_t)(sp.tasks.size() / 65));
            sp.tasks.push_back(t);
            sp.tasks.insert(sp.tasks.end(), waves.begin() + w, waves.begin() + w + 64);
        }
    }
    sp.extra = (uint32_t)sp.order.size() - sp.tiles;
    for (uint32_t b : order)
        if (!heavy[b]) sp.order.push_back(b);
    return sp;
}

// A workgroup's time spread over its per_block tiles (natural 8x8-tile order), a
// tile's over its 8 rows, summed per chunk of row_chunk rows (och_gpu_chunk_costs).
std::vector<float> spread_chunk_costs(const std::vector<uint32_t> &c, int n_views, int W, int H, uint32_t per_block,
                                      int row_chunk)
{
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, tiles_y = (uint32_t)(H + 7) / 8;
    const uint32_t tiles = (uint32_t)n_views * tiles_x * tiles_y;
    std::vector<double> acc((H + row_chunk - 1) / row_chunk, 0.0);
    for (uint32_t b = 0; b < c.size(); ++b)
        for (uint32_t t = b * per_block; t < std::min(tiles, (b + 1) * per_block); ++t) {
            const uint32_t ty = (t % (tiles_x * tiles_y)) / tiles_x;
            const int r0 = (int)ty * 8, r1 = std::min(H, r0 + 8);
            for (int r = r0; r < r1; ++r) acc[r / row_chunk] += (double)c[b] / per_block / (r1 - r0);
        }
    return std::vector<float>(acc.begin(), acc.end());
}

}  // namespace plan
}  // namespace och
