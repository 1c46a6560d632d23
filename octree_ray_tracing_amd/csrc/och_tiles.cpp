// och_tiles.cpp -- the host side of a camera launch's tile table (och_tiles.h):
// which 8x8 pixel tile of which view each wave of the launch walks, where its
// rows lie in the frame and in the shard's slice, and whether the whole tile is
// inside the frame.  All of it follows from the frame's geometry and the launch
// order, so it is worked out here once per geometry, not by every wave of every
// frame.  Host only, no HIP.
#include "och_tiles.h"

#include <algorithm>

#include "../../include/och_gpu.h"

namespace och {
namespace plan {
namespace {

// Workgroups are dealt round-robin over the 8 XCDs (blocks b, b + 8, ... share
// one XCD and its L2).  Remap so each XCD receives runs of `group`
// consecutive logical blocks -- one supertile of neighbouring rays, which walk
// the same DAG nodes -- instead of every eighth block.  A bijection on the
// grid; placement only changes speed, never results.
uint32_t xcd_block(uint32_t b, uint32_t nb, uint32_t group)
{
    if (group == 0) return b;
    const uint32_t span = 8u * group, full = nb - nb % span;
    if (b >= full) return b;
    const uint32_t x = b & 7u, s = b >> 3;
    return ((s / group) * 8u + x) * group + s % group;
}

// The descriptor of logical wave `wave` of the frame: view after view, 8x8
// tile after tile, row-major or in supertiles of 8x8 tiles.
uint64_t tile_entry(const TileGeometry &g, uint32_t wave, uint32_t tiles_x, uint32_t supertiles_x, uint32_t per_view)
{
    const uint32_t view = wave / per_view, tile = wave % per_view;
    if (view >= (uint32_t)g.n_views) return kTileEmpty;
    uint32_t tx, ty;
    if (g.supertiles) {
        const uint32_t st = tile >> 6, sub = tile & 63u, sy = st / supertiles_x;
        tx = (st - sy * supertiles_x) * 8u + (sub & 7u);
        ty = sy * 8u + (sub >> 3);
    } else {
        ty = tile / tiles_x;
        tx = tile - ty * tiles_x;
    }
    const int col0 = (int)(tx * 8u), srow0 = (int)(ty * 8u);
    if (col0 >= g.width || srow0 >= g.slice_rows) return kTileEmpty;
    // global row of a slice row: its local chunk's global chunk, dealt or round-robin
    auto global_row = [&](int srow) {
        const int chunk = srow / g.row_chunk, within = srow - chunk * g.row_chunk;
        const int gc = g.chunk_map ? g.chunk_map[chunk] : chunk * g.n_shards + g.shard;
        return gc < 0 ? g.height : std::min(g.height, gc * g.row_chunk + within);
    };
    const int last = std::min(srow0 + 7, g.slice_rows - 1);
    const int row0 = global_row(srow0);
    bool affine = true, any = false, all = col0 + 7 < g.width && srow0 + 7 < g.slice_rows;
    for (int s = srow0; s <= last; ++s) {
        const int r = global_row(s);
        // past the frame's last row only "no pixel" matters, and row0 + k says that too
        affine = affine && (r == row0 + (s - srow0) || (r >= g.height && row0 + (s - srow0) >= g.height));
        any = any || r < g.height;
        all = all && r < g.height;
    }
    if (!any) return kTileEmpty;
    uint32_t w0 = (uint32_t)col0 | view << 16, w1 = (uint32_t)srow0 << 16;
    if (affine) {
        w1 |= (uint32_t)row0;                   // row0 < height <= kTileMaxExtent
        if (all) w0 |= kTileInside;
    } else {
        w0 |= kTileRows;
    }
    return (uint64_t)w1 << 32 | w0;
}

}  // namespace

int tile_table(const TileGeometry &g, const uint32_t *order, uint32_t order_n, const uint32_t *split_tasks,
               uint32_t split_tasks_n, std::vector<uint64_t> &table, uint32_t &grid, const char **why)
{
    const char *unused;
    if (!why) why = &unused;
    *why = "";
    table.clear();
    grid = 0;
    if (g.width <= 0 || g.height <= 0 || g.n_views < 1 || g.n_views > OCH_MAX_VIEWS || g.row_chunk <= 0 ||
        g.n_shards <= 0 || g.shard < 0 || g.shard >= g.n_shards || g.slice_rows <= 0 || g.block < 64 || g.block % 64)
        return *why = "bad geometry", OCH_E_INVALID;
    if (g.width > kTileMaxExtent || g.height > kTileMaxExtent || g.slice_rows > kTileMaxExtent)
        return *why = "more than 65535 columns, rows or slice rows", OCH_E_INVALID;
    const uint32_t tiles_x = (uint32_t)(g.width + 7) / 8, tiles_y = (uint32_t)(g.slice_rows + 7) / 8;
    const uint32_t supertiles_x = (tiles_x + 7) / 8;
    const uint64_t per_view64 =
        g.supertiles ? (uint64_t)supertiles_x * ((tiles_y + 7) / 8) * 64u : (uint64_t)tiles_x * tiles_y;
    if (per_view64 * (uint64_t)g.n_views >= (1u << 25)) return *why = "more than 2^25 tiles", OCH_E_INVALID;
    const uint32_t per_view = (uint32_t)per_view64, waves = per_view * (uint32_t)g.n_views;
    const uint32_t wpb = (uint32_t)g.block / 64u, blocks = (waves + wpb - 1) / wpb;
    // blocks per 64x64-pixel supertile, the unit one XCD receives
    const uint32_t xcd_group = g.supertiles && !order && 64u >= wpb ? 64u / wpb : 0u;
    const uint32_t n_launch = order ? order_n : blocks;
    if (order && order_n < blocks) return *why = "an order shorter than the grid", OCH_E_INVALID;
    if (order && order_n >= (1u << 25)) return *why = "an order of more than 2^25 workgroups", OCH_E_INVALID;
    uint32_t n_split = 0;
    if (order)
        for (uint32_t b = 0; b < order_n; ++b) n_split += order[b] >> 31;
    if (n_split && (wpb != 1 || !split_tasks)) return *why = "split waves need block 64 and their tasks", OCH_E_INVALID;
    table.reserve((size_t)n_launch * wpb + n_split);
    table.resize((size_t)n_launch * wpb);
    for (uint32_t b = 0; b < n_launch; ++b) {
        const uint32_t blk = order ? order[b] : xcd_block(b, blocks, xcd_group);
        if (blk >> 31) {                        // a split wave: its task row, and its tile's descriptor behind the launch
            const uint32_t row = blk & 0x7FFFFFFFu;
            if ((uint64_t)row * 65u + 65u > split_tasks_n) return table.clear(), *why = "a task row out of range", OCH_E_INVALID;
            const uint32_t tile = split_tasks[(size_t)row * 65u];
            if (tile >= waves) return table.clear(), *why = "a split tile out of range", OCH_E_INVALID;
            table[b] = (uint64_t)table.size() << 32 | (kTileSplit | row);
            table.push_back(tile_entry(g, tile, tiles_x, supertiles_x, per_view));
            continue;
        }
        if (blk >= blocks) return table.clear(), *why = "an order entry outside the grid", OCH_E_INVALID;
        for (uint32_t w = 0; w < wpb; ++w) {
            const uint32_t wave = blk * wpb + w;
            table[(size_t)b * wpb + w] = wave < waves ? tile_entry(g, wave, tiles_x, supertiles_x, per_view) : kTileEmpty;
        }
    }
    grid = n_launch;
    return OCH_OK;
}

}  // namespace plan
}  // namespace och
