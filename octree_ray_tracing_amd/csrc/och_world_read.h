// och_world_read.h -- reading a resident world back on its GPU (och_world_at,
// och_world_read_box, och_world_tighten).  Included by och_builder.cpp only,
// after och_world.h, whose och_world it reads:
//   at       -- one lane per coordinate walks from the current root (k_world_at).
//   read_box -- the grid is zeroed, then per aligned 4x4x4 brick that meets
//               the box and the tree a wavefront walks to the brick's height-1
//               node as one and each lane does its own last two loads
//               (k_world_read).  och_pool_read_box (och_pool.cpp) is the host
//               counterpart and gives the same bytes.
//   tighten  -- every id's local box, the box of the voxels below it relative
//               to the node, one dispatch per height (k_world_lbox); the root's
//               is the world's exact box.
//
// Visibility.  Every row read here was written by an earlier dispatch of the
// world's stream (a stroke ends before the call starts: one thread at a time
// per world), and a row never changes once written (och_world.h, append-only).
// So the queries take the root by value and need no lock, no wait and nothing
// inside a dispatch; k_world_lbox reads local boxes of an earlier dispatch (a
// lower height) or an earlier call only.
//
// Local boxes stay.  An id's content never changes, so neither does its local
// box: the array is allocated once for `capacity` ids (16 bytes each: 256 MiB
// at capacity 2^24) at the first tighten, filled for [1, used) then and for
// the ids handed out since on every later call.  och_world_compact renumbers:
// the array then belongs to another generation and the next tighten starts over.
//
// Out of scope: queries on an och_gpu_pool; asynchronous queries on a caller's
// stream; run-length or sparse output; shrinking the box inside a stroke.  An
// older root is read by checking its snapshot out first (och_world_history.h).
#pragma once
#include "och_world.h"

namespace {

constexpr int kHeadFlag = 24;   // the head's word for k_world_read's u8 overflow (the largest id met above 255)

__device__ inline uint32_t child_digit(uint32_t x, uint32_t y, uint32_t z, int l)
{
    return ((x >> l) & 1u) | ((y >> l) & 1u) << 1 | ((z >> l) & 1u) << 2;
}

// ids[i] = the voxel at coords[3 i ..] under root, 0 outside [0, dim): depth
// dependent loads per lane.  An interior word at or above cap (never written
// by this library) reads as empty rather than out of bounds.
__global__ __launch_bounds__(256) void k_world_at(GpuStore S, uint32_t root, int depth, const int32_t *__restrict__ coords,
                                                  uint32_t n, uint32_t *__restrict__ ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = (uint32_t)coords[(size_t)i * 3], y = (uint32_t)coords[(size_t)i * 3 + 1],
                   z = (uint32_t)coords[(size_t)i * 3 + 2];
    const uint32_t dim = 1u << depth;
    uint32_t w = 0;
    if (root && x < dim && y < dim && z < dim) {   // a negative coordinate is a large unsigned one
        w = root;
        for (int l = depth - 1; l >= 0; --l) {
            w = S.nodes[(size_t)w * 8 + child_digit(x, y, z, l)];
            if (l == 0 || !w) break;
            if (w >= S.cap) {
                w = 0;
                break;
            }
        }
    }
    ids[i] = w;
}

// The box of a read, clipped to the tree, and its bricks.
struct ReadBox {
    int32_t lo[3];        // the caller's lo: the grid's origin
    uint32_t clo[3], chi[3];   // the box inside [0, dim): cells outside stay 0
    uint32_t b0[3], nb[3];     // the first brick per axis (in bricks) and how many
    uint32_t bricks;
    uint64_t nx, ny;      // the grid's extents in x and y
    int u8;
};

// Brick `wave` of the clipped box, by one wavefront.  The brick is wave-uniform,
// so the walk down to its height-1 node is too (depth - 2 loads a wavefront);
// an empty word on the way ends the brick.  Lane t is cell (t & 3, t >> 2 & 3,
// t >> 4) of the brick and does the last two loads (one at depth 1, where the
// root is the leaf-level node).  Zero cells are not stored: the grid was
// zeroed.  u8: an id above 255 is not stored, the flag takes the largest one.
__device__ inline void read_brick(const GpuStore &S, uint32_t root, int depth, const ReadBox &B, uint32_t wave,
                                  void *__restrict__ grid, uint32_t *__restrict__ flag)
{
    const uint32_t bx = wave % B.nb[0], by = wave / B.nb[0] % B.nb[1], bz = wave / B.nb[0] / B.nb[1];
    const uint32_t X = (B.b0[0] + bx) * 4u, Y = (B.b0[1] + by) * 4u, Z = (B.b0[2] + bz) * 4u;
    uint32_t cur = root;
    for (int l = depth - 1; l >= 2; --l) {
        cur = S.nodes[(size_t)cur * 8 + child_digit(X, Y, Z, l)];
        if (!cur || cur >= S.cap) return;
    }
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t x = X + (t & 3u), y = Y + ((t >> 2) & 3u), z = Z + (t >> 4);
    if (x < B.clo[0] || x >= B.chi[0] || y < B.clo[1] || y >= B.chi[1] || z < B.clo[2] || z >= B.chi[2]) return;
    uint32_t w = cur;
    for (int l = depth > 1 ? 1 : 0; l >= 0; --l) {
        w = S.nodes[(size_t)w * 8 + child_digit(x, y, z, l)];
        if (l == 0 || !w) break;
        if (w >= S.cap) return;
    }
    if (!w) return;
    const size_t at = ((size_t)((int64_t)z - B.lo[2]) * B.ny + (size_t)((int64_t)y - B.lo[1])) * B.nx + (size_t)((int64_t)x - B.lo[0]);
    if (!B.u8)
        static_cast<uint32_t *>(grid)[at] = w;
    else if (w <= 255u)
        static_cast<uint8_t *>(grid)[at] = (uint8_t)w;
    else
        atomicMax(flag, w);
}

// A launch is at most kReadMaxBlocks workgroups of four wavefronts, far more
// than the device holds at once: a wavefront takes the bricks wave, wave +
// stride, ... of the clipped box (stride = the launch's wavefronts), so any
// box below 2^32 bricks is one launch whose thread count stays below 2^32.
constexpr uint32_t kReadMaxBlocks = 1u << 16;

__global__ __launch_bounds__(256) void k_world_read(GpuStore S, uint32_t root, int depth, ReadBox B, void *__restrict__ grid,
                                                    uint32_t *__restrict__ flag)
{
    const uint32_t stride = gridDim.x * 4u;
    uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    while (wave < B.bricks) {
        read_brick(S, root, depth, B, wave, grid, flag);
        if (B.bricks - wave <= stride) break;   // wave + stride may pass 2^32
        wave += stride;
    }
}

// A local box: x | y << 21 | z << 42 of the least and of the greatest voxel
// (inclusive, so 21 bits hold depth 21); no voxel: lo all ones, hi 0.
constexpr unsigned long long kNoLbox = ~0ull;

// The local boxes of the ids [first, used) at height h: a leaf-level node's
// from its non-zero words, any other node's the union of its children's, each
// shifted by its octant times 2^h.  The children's are an earlier dispatch's
// (height h - 1) or an earlier call's.
__global__ __launch_bounds__(256) void k_world_lbox(GpuStore S, uint32_t first, uint32_t used, int h, ulonglong2 *__restrict__ lbox)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= used - first) return;
    const uint32_t id = first + i;
    if (S.level[id] != (uint8_t)h) return;
    const uint4 *rec = reinterpret_cast<const uint4 *>(S.nodes + (size_t)id * 8);
    const uint4 a = rec[0], b = rec[1];
    const uint32_t c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!c[k]) continue;
        unsigned long long clo = 0, chi = 0;   // leaf level: the voxel itself
        if (h > 0) {
            if (c[k] >= used) continue;
            const ulonglong2 cb = lbox[c[k]];
            if (cb.x == kNoLbox) continue;
            clo = cb.x;
            chi = cb.y;
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const uint32_t off = ((uint32_t)(k >> ax) & 1u) << h;
            lo[ax] = min(lo[ax], off + (uint32_t)((clo >> (21 * ax)) & 0x1FFFFFu));
            hi[ax] = max(hi[ax], off + (uint32_t)((chi >> (21 * ax)) & 0x1FFFFFu));
        }
    }
    ulonglong2 out;
    out.x = kNoLbox;
    out.y = 0;
    if (lo[0] != 0xFFFFFFFFu) {
        out.x = (unsigned long long)lo[0] | (unsigned long long)lo[1] << 21 | (unsigned long long)lo[2] << 42;
        out.y = (unsigned long long)hi[0] | (unsigned long long)hi[1] << 21 | (unsigned long long)hi[2] << 42;
    }
    lbox[id] = out;
}

// The root's local box into the head as k_world_box leaves a stroke's (a device
// box, kNoBox without a voxel), for the head's one read-back.
__global__ __launch_bounds__(64) void k_world_lbox_root(const ulonglong2 *__restrict__ lbox, uint32_t root, uint32_t *__restrict__ head)
{
    if (blockIdx.x || threadIdx.x) return;
    ulonglong2 rb;
    rb.x = kNoLbox;
    rb.y = 0;
    if (root) rb = lbox[root];
    for (int ax = 0; ax < 3; ++ax) {
        head[kHeadBox + ax] = rb.x == kNoLbox ? kNoBox[0] : (uint32_t)((rb.x >> (21 * ax)) & 0x1FFFFFu);
        head[kHeadBox + 3 + ax] = rb.x == kNoLbox ? kNoBox[3] : (uint32_t)((rb.y >> (21 * ax)) & 0x1FFFFFu);
    }
}

int world_at(och_world &w, const int32_t *coords, uint32_t n, uint32_t *ids, bool on_device)
{
    const hipStream_t st = w.st;
    PhaseTimer phase = world_phase(w);
    // host arrays: the ids' n words of the staging buffer, then the coordinates' 3 n
    uint32_t *d_ids = static_cast<uint32_t *>(world_stage(w, ids, (size_t)n * 16, on_device));
    if (!d_ids) return OCH_E_NOMEM;
    const int32_t *d_coords = coords;
    if (!on_device) {
        d_coords = reinterpret_cast<const int32_t *>(d_ids + n);
        GPU_TRY(hipMemcpyAsync(d_ids + n, coords, (size_t)n * 12, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_world_at, blocks(n), dim3(256), 0, st, w.S, w.now.root, w.depth, d_coords, n, d_ids);
    GPU_TRY(hipGetLastError());
    if (const int rs = world_read_back(w, {{ids, d_ids, on_device ? 0 : (size_t)n * 4}})) return rs;
    phase("at");
    return OCH_OK;
}

// The box is checked (och::read_box_cells) and not empty: `cells` of it.
int world_read_box(och_world &w, const int32_t lo[3], const int32_t hi[3], int kind, void *grid, uint64_t cells, bool on_device)
{
    const hipStream_t st = w.st;
    PhaseTimer phase = world_phase(w);
    const size_t bytes = (size_t)cells * (kind == OCH_VOXELS_GRID_U8 ? 1 : 4);
    void *d_grid = world_stage(w, grid, bytes, on_device);
    if (!d_grid) return OCH_E_NOMEM;
    ReadBox B{};
    const int64_t dim = (int64_t)1 << w.depth;
    bool meets = w.now.root != 0;
    uint64_t bricks = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t clo = std::max<int64_t>(lo[a], 0), chi = std::min<int64_t>(hi[a], dim);
        if (clo >= chi) {
            meets = false;
            break;
        }
        B.lo[a] = lo[a];
        B.clo[a] = (uint32_t)clo;
        B.chi[a] = (uint32_t)chi;
        B.b0[a] = (uint32_t)(clo >> 2);
        B.nb[a] = (uint32_t)((chi + 3) >> 2) - B.b0[a];
        bricks *= B.nb[a];   // three factors of at most 2^19 each
    }
    if (meets && bricks > 0xFFFFFFFCull) return och::report(OCH_E_INVALID, "och_world_read_box: a box of 2^32 bricks (2^38 cells) or more");
    B.bricks = (uint32_t)bricks;
    B.nx = (uint64_t)((int64_t)hi[0] - lo[0]);
    B.ny = (uint64_t)((int64_t)hi[1] - lo[1]);
    B.u8 = kind == OCH_VOXELS_GRID_U8;
    uint32_t *flag = w.head() + kHeadFlag;
    GPU_TRY(hipMemsetAsync(flag, 0, 4, st));
    GPU_TRY(hipMemsetAsync(d_grid, 0, bytes, st));
    if (meets) {
        hipLaunchKernelGGL(k_world_read, dim3(std::min((B.bricks + 3u) / 4u, kReadMaxBlocks)), dim3(256), 0, st, w.S, w.now.root, w.depth, B, d_grid, flag);
        GPU_TRY(hipGetLastError());
    }
    uint32_t over = 0;
    if (const int rs = world_read_back(w, {{&over, flag, 4}, {grid, d_grid, on_device ? 0 : bytes}})) return rs;
    phase("read_box");
    if (over) return och::fail(OCH_E_INVALID, "och_world_read_box: voxel id %u does not fit a u8 grid", over);
    return OCH_OK;
}

int world_tighten(och_world &w)
{
    const hipStream_t st = w.st;
    PhaseTimer phase = world_phase(w);
    if (w.d_lbox.n < w.S.cap) {
        w.boxed = 1;
        if (w.d_lbox.reserve(w.S.cap) != hipSuccess) return OCH_E_NOMEM;
        if (!phase("lbox alloc")) return OCH_E_HIP;
    }
    if (w.lbox_generation != w.generation) w.boxed = 1;   // a compaction renumbered the ids
    w.lbox_generation = w.generation;
    const uint32_t first = std::min(w.boxed, w.used);
    if (w.used > first)
        for (int h = 0; h < w.depth; ++h) {
            hipLaunchKernelGGL(k_world_lbox, blocks(w.used - first), dim3(256), 0, st, w.S, first, w.used, h, w.d_lbox.d);
            GPU_TRY(hipGetLastError());
        }
    hipLaunchKernelGGL(k_world_lbox_root, dim3(1), dim3(64), 0, st, w.d_lbox.d, w.now.root, w.head());
    GPU_TRY(hipGetLastError());
    WorldHead H;
    if (const int hs = world_read_head(w, w.S, &H)) return hs;
    if (!phase("tighten")) return OCH_E_HIP;
    if (phase.on) std::fprintf(stderr, "[och_build] world: local boxes of ids [%u, %u)\n", first, w.used);
    w.boxed = w.used;
    w.now.box = box_decode(H.box);
    return OCH_OK;
}

}  // namespace

OCH_API int och_world_at(och_world *w, const int32_t *coords, uint64_t n, uint32_t *ids, int on_device)
{
    if (n >= (1ull << 31)) return och::report(OCH_E_INVALID, "och_world_at: a call takes fewer than 2^31 coordinates");
    if ((!coords || !ids) && n) return och::report(OCH_E_INVALID, "och_world_at: coords or ids is null");
    if (!n) return world_usable(w, "och_world_at");
    return world_call(w, "och_world_at", "och_world_at", kStays, kOwnTexts,
                      [&] { return world_at(*w, coords, (uint32_t)n, ids, on_device != 0); });
}

OCH_API int och_world_read_box(och_world *w, const int32_t lo[3], const int32_t hi[3], int kind, void *grid, size_t capacity_bytes,
                               int on_device)
{
    uint64_t cells = 0;
    if (const int cs = och::read_box_cells("och_world_read_box", lo, hi, kind, grid, capacity_bytes, &cells)) return cs;
    if (!cells) return world_usable(w, "och_world_read_box");
    return world_call(w, "och_world_read_box", "och_world_read_box", kStays, kOwnTexts,
                      [&] { return world_read_box(*w, lo, hi, kind, grid, cells, on_device != 0); });
}

OCH_API int och_world_tighten(och_world *w)
{
    return world_call(w, "och_world_tighten", "och_world", kBreaks, kOwnTexts, [&] { return world_tighten(*w); });
}
