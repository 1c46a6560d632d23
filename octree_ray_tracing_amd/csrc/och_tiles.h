// och_tiles.h -- the tile table of a camera launch: what the render kernels
// (och_kernels.hip CameraSource) read in place of per-wave tile arithmetic, and
// the host function that makes it (och_tiles.cpp).  Host and device; needs no
// HIP header, so the builder also compiles into a stand-alone program
// (tests/test_tile_table_host.py).  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <vector>

namespace och {

// A tile descriptor: one 8-byte entry per wave of a camera launch, in launch
// order.  Word 0 (the low word): the tile's first column in bits 0..15, the
// view in bits 16..19, flags above; word 1: frame row of the tile's first row
// in bits 0..15, its slice row in bits 16..31.  Frames of more than 65 535
// columns, rows or slice rows do not fit (plan::tile_table refuses them).
constexpr uint32_t kTileRows = 1u << 28;    // rows straddle row chunks: lanes map their own rows
constexpr uint32_t kTileInside = 1u << 29;  // all 64 pixels lie in the frame: no per-lane bounds tests
constexpr uint32_t kTileEmpty = 1u << 30;   // no pixel of the frame (padding wave)
// A split wave (bit 31, split plans): word 0 = kTileSplit | task row, word 1 =
// the table entry, behind the launch's own, that holds the heavy tile's descriptor.
constexpr uint32_t kTileSplit = 1u << 31;
constexpr int kTileMaxExtent = 65535;

namespace plan {

// What a tile table depends on: the frame's geometry and the launch order.
struct TileGeometry {
    int width, height, n_views, row_chunk, shard, n_shards, slice_rows;
    int block;                  // threads per workgroup of the launch (a multiple of 64)
    int supertiles;             // tiles enumerated in 64x64-pixel supertiles, grouped per XCD (tile_order 1)
    const int32_t *chunk_map;   // host copy of this shard's row deal (slice_rows / row_chunk entries), or null
};

// The launch's table.  order (optional): the workgroup permutation, entries
// with bit 31 set split waves whose task rows are in split_tasks (65 words
// each: the tile, then the lane tasks).  Returns 0, or OCH_E_INVALID with *why
// naming the reason when the geometry does not fit a descriptor or an order
// entry names a workgroup outside the grid.  grid receives the launch's
// workgroups, table its entries: grid * block / 64, then the split tiles'.
int tile_table(const TileGeometry &g, const uint32_t *order, uint32_t order_n, const uint32_t *split_tasks,
               uint32_t split_tasks_n, std::vector<uint64_t> &table, uint32_t &grid, const char **why);

}  // namespace plan
}  // namespace och
