// och_host.h -- the host layer's shared plumbing (och_pool.cpp, och_api.cpp,
// och_rcp.cpp, och_group.cpp, och_comm.cpp, och_editor.cpp and och_builder.cpp's
// och_world.h): the error text, the device guard,
// the device-memory owner and the internal entry points these files call in each
// other.  Host only, not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "och_ball.h"
#include "och_internal.h"

typedef struct ncclComm *ncclComm_t;    // as <rccl/rccl.h> declares it

namespace och {

// Record the formatted text as och_last_error's (this thread's) and return
// status (och_pool.cpp, beside the text; och::report is its one-string form).
int fail(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define OCH_HIP(expr)                                                                             \
    do {                                                                                          \
        const hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return och::fail(OCH_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Keep the caller's current device (torch sets one per rank) across calls.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && dev != prev) ok = hipSetDevice(dev) == hipSuccess;
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// A device buffer that only grows.  A reallocation that fails leaves it empty,
// so the pointer never names freed memory.
template <class T>
struct DevBuf {
    T *d = nullptr;
    size_t n = 0;                   // elements allocated
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)release(); }
    hipError_t release()
    {
        n = 0;
        return d ? hipFree(std::exchange(d, nullptr)) : hipSuccess;
    }
    void swap(DevBuf &o) { std::swap(d, o.d); std::swap(n, o.n); }
    hipError_t reserve(size_t want)
    {
        if (want <= n) return hipSuccess;
        hipError_t e = release();
        if (e == hipSuccess) e = hipMalloc(&d, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    hipError_t upload(const std::vector<T> &v)
    {
        const hipError_t e = reserve(v.size());
        return e != hipSuccess ? e : hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// A resident world's pools (och_pool.cpp for och_world.h's och_world_pool_create
// and och_world_flush; they stand here, not beside the editor's hooks in
// och_internal.h, because that header is part of the identity of the kernel
// source that the committed profiles are keyed by).
// pool_create_for_world: a 1-based pool of `capacity` slots on `device` (current),
// miss t = +INF, both layouts allocated (the packed one, numbered like the slots,
// only for capacity <= 2^24), no content, root 0, no host mirror, marked with the
// world's id.  pool_world: that id, 0 for any other pool -- och_gpu_pool_update
// and och_editor_flush refuse a marked pool.  pool_world_view: the buffers the
// flush's copy and pack kernel write and where the pool keeps what the last
// flush published; OCH_E_INVALID unless the pool was made from `world`.
struct WorldPoolView {
    uint32_t *raw, *packed;   // n_nodes x 8 words each; packed = null: raw only
    uint32_t n_nodes;
    uint64_t *generation;     // the world generation of the published ids
    uint32_t *published;      // ids [0, *published) are on the pool
};
int pool_create_for_world(int device, int depth, uint32_t capacity, uint64_t world, och_gpu_pool **out);
uint64_t pool_world(const och_gpu_pool *pool);
int pool_world_view(och_gpu_pool *pool, uint64_t world, WorldPoolView *view);

// What och_pool_read_box and och_world_read_box (och_world_read.h) refuse
// alike before anything is written (och_pool.cpp): a NULL lo, hi or grid,
// another kind than the two grids, hi[a] < lo[a], a volume times the cell size
// above capacity_bytes.  *cells: the box's volume, 0 for an empty box.
int read_box_cells(const char *who, const int32_t lo[3], const int32_t hi[3], int kind, const void *grid,
                   size_t capacity_bytes, uint64_t *cells);

// The maximal aligned cubes of the box lo <= (x, y, z) < hi clipped to a tree
// of `depth`, counted (och_pool.cpp, for och_box_cubes and the region strokes
// of och_world_region.h).  Per axis at height H, touch = ceil(hi / 2^H) -
// floor(lo / 2^H) cells meet the box and in = max(0, floor(hi / 2^H) -
// ceil(lo / 2^H)) lie inside it: cells[H] = prod touch - prod in straddle it,
// cubes[h] = prod in(h) - 8 prod in(h + 1) are inside while their parent is not.
struct BoxCubes {
    bool any = false;                             // something of the box lies inside the tree
    int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // the clipped box; all 0 without one
    uint64_t cubes[22] = {0}, cells[22] = {0};    // by height, 0 .. depth
    uint64_t n_cubes = 0, n_cells = 0;
    int top = -1;                                 // the greatest height with a cube
};
BoxCubes box_cube_counts(const int32_t lo[3], const int32_t hi[3], int depth);

// The same of a ball (och_ball.h) for och_sphere_cubes: there are no closed
// forms, the counts come from the top-down walk itself, whose cost follows the
// ball's surface.  any, lo, hi: the ball's clipped axis box, a loose superset
// (n_cubes may be 0 with any set).  keys and heights, both or neither: every
// cube, ascending height then ascending Morton key, written only while
// n_cubes <= capacity (the counts are complete either way).
BoxCubes ball_cube_walk(const int32_t c2[3], uint32_t diameter, int depth, uint64_t *keys, uint8_t *heights, uint64_t capacity);

// n_views views of one positive width and height (och_api.cpp).
int check_views(const och_camera *cams, int n_views);

// och_gpu_render_sharded_steps_dev's window (och_api.cpp), for the frame group
// too: per frame render this rank's slices, exchange, shade, all on the
// frame's stream.  codes: the slices travel as 1-byte colour codes and the
// shade needs the pool's code table; otherwise as RGBA8 words (slices and
// gathered then hold 4 bytes a pixel) and the frames are only unsharded.
// light (optional, refused together with bounce): lit frames -- with codes the
// slices travel as 2-byte lit codes (och_gpu_render_lit_codes_views_dev) and
// the shade is och_gpu_shade_lit_unshard_views_dev, otherwise as lit RGBA8
// words.  It is checked, like the buffers, before the first frame is queued.
int sharded_steps(och_gpu_pool *pool, och_comm *comm, const och_camera *cams, int n_views, int n_steps,
                  void *const *streams, uint8_t *const *slices, uint8_t *const *gathered, uint32_t *const *frames,
                  int n_buffers, void *const *start_events, void *const *stop_events, int row_chunk, int bounce,
                  int exchange, bool codes, const och_light *light = nullptr);

// An och_comm around an RCCL communicator the caller made (och_comm.cpp).
och_comm *comm_adopt(ncclComm_t comm, int n_ranks, int rank, int device);
// The communicator's handle, leaving null behind: of the threads that ask, one
// gets it and with it the duty to abort or destroy it; the och_comm then
// reports itself destroyed.
ncclComm_t comm_take(och_comm *comm);

}  // namespace och
