// och_plan.h -- the pure launch planners (och_plan.cpp, each described at its
// definition): vectors and integers in and out, no HIP call, no pool.  Host
// only and without a HIP header, so they also compile into a stand-alone program
// (tests/test_plan_host.py pins them).  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <vector>

namespace och {
namespace plan {

std::vector<uint32_t> by_cost(const std::vector<uint32_t> &costs);
void shape(std::vector<uint32_t> &order, int mode);
std::vector<uint32_t> group_by_xcd(const std::vector<uint32_t> &order, uint32_t tiles_x, uint32_t tiles_y, uint32_t block);
std::vector<uint32_t> pack_split_tile(const int cnt[64], int S);

struct Split {
    std::vector<uint32_t> order, tasks;
    uint32_t tiles = 0, extra = 0;      // heavy tiles; waves - heavy tiles
};

Split split_order(const std::vector<uint16_t> &push, int W, int rows, const std::vector<uint32_t> &by_cost,
                  const std::vector<uint32_t> &order, const std::vector<uint32_t> &c, int pct, int S);
std::vector<float> spread_chunk_costs(const std::vector<uint32_t> &c, int n_views, int W, int H, uint32_t per_block,
                                      int row_chunk);

}  // namespace plan
}  // namespace och
