// och_ball.h -- a ball of voxels against the aligned cubes of a tree, in
// integers, for the host (och_sphere_cubes, och_pool.cpp) and the device (the
// region strokes, och_world_region.h) alike.
//
// Half-voxel units: voxel (x, y, z) has its centre at (2x+1, 2y+1, 2z+1), the
// ball is twice its centre, c2 (so it may sit on a voxel's centre, face, edge
// or corner), and its diameter d in voxels.  The voxel is in the ball iff the
// three squared offsets sum to at most d^2.  With |c2| <= 2^24, d <= 2^24 and
// coordinates below 2^21 an offset stays below 2^24.4 and fits an int32; the
// sum of three squares stays below 2^51: uint64_t is exact.
//
// The cube [c, c + 2^h)^3: its voxel centres are a product set and the squared
// distance is a sum over the axes, so its nearest and its farthest centre are
// found per axis.  With a = 2c+1-c2 and b = 2(c+2^h)-1-c2 (a <= b, both of the
// parity of c2 + 1) the farthest offset is max(|a|, |b|); the nearest is a for
// a > 0, -b for b < 0, and between them the least offset of that parity: 0
// for an odd c2, 1 for an even one (no voxel centre has an even half-coordinate).
#pragma once
#include <cstdint>

#ifndef OCH_HD
#ifdef __HIPCC__
#define OCH_HD __host__ __device__ __forceinline__
#else
#define OCH_HD inline
#endif
#endif

namespace och {

constexpr int32_t kBallRange = 1 << 24;   // |c2[a]| and the diameter at most

struct Ball {
    int32_t c2[3];   // twice the centre
    uint64_t d2;     // the diameter squared
};

OCH_HD Ball make_ball(const int32_t c2[3], uint32_t diameter)
{
    return Ball{{c2[0], c2[1], c2[2]}, (uint64_t)diameter * diameter};
}

// What och_sphere_cubes and the sphere strokes refuse alike; nullptr: in range.
inline const char *ball_range_error(const int32_t c2[3], uint32_t diameter)
{
    for (int a = 0; a < 3; ++a)
        if (c2[a] < -kBallRange || c2[a] > kBallRange) return "a component of centre2 outside -2^24 .. 2^24";
    return diameter > (uint32_t)kBallRange ? "a diameter above 2^24" : nullptr;
}

// The cube of side 2^h at corner c against the ball: 0 outside, 1 straddling
// (it holds a voxel inside and a voxel outside), 2 inside.  Height 0 never straddles.
OCH_HD int ball_class(const Ball &B, const int32_t c[3], int h)
{
    uint64_t far2 = 0, near2 = 0;
    for (int a = 0; a < 3; ++a) {
        const int32_t lo = 2 * c[a] + 1 - B.c2[a], hi = 2 * (c[a] + ((int32_t)1 << h)) - 1 - B.c2[a];
        const uint32_t alo = (uint32_t)(lo < 0 ? -lo : lo), ahi = (uint32_t)(hi < 0 ? -hi : hi);
        const uint32_t far = alo > ahi ? alo : ahi;
        const uint32_t near = lo > 0 ? alo : hi < 0 ? ahi : (B.c2[a] & 1) ? 0u : 1u;
        far2 += (uint64_t)far * far;   // 32 x 32 -> 64 bits, one multiply-add
        near2 += (uint64_t)near * near;
    }
    return near2 > B.d2 ? 0 : far2 <= B.d2 ? 2 : 1;
}

// The ball's axis box clipped to a tree of `depth`: lo = ceil((c2 - d - 1) / 2),
// hi = floor((c2 + d - 1) / 2) + 1, a loose superset of its voxels.  False, lo
// and hi all 0, where nothing is left.
inline bool ball_axis_box(const int32_t c2[3], uint32_t diameter, int depth, int32_t lo[3], int32_t hi[3])
{
    const int64_t dim = (int64_t)1 << depth;
    bool any = true;
    for (int a = 0; a < 3; ++a) {
        const int64_t l = ((int64_t)c2[a] - (int64_t)diameter) >> 1;              // ceil((n - 1) / 2) = floor(n / 2)
        const int64_t h = (((int64_t)c2[a] + (int64_t)diameter - 1) >> 1) + 1;
        lo[a] = (int32_t)(l < 0 ? 0 : l > dim ? dim : l);
        hi[a] = (int32_t)(h < 0 ? 0 : h > dim ? dim : h);
        any = any && lo[a] < hi[a];
    }
    if (!any)
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
    return any;
}

}  // namespace och
