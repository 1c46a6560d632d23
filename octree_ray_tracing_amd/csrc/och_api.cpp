// och_api.cpp -- the C ABI's launches (include/och_gpu.h): per-launch timing,
// the plan and tile table a camera launch takes, the trace, batch, render,
// supersampled, lit and code entries with their argument checks, the planning
// renders (och_gpu_plan_*, och_gpu_chunk_costs), the row deal, the unshard and
// shade entries and the frame loops, single and sharded.  The pool itself, its
// settings and the error text are och_pool.cpp; the planners' arithmetic is
// och_plan.cpp, the tile table's och_tiles.cpp, the RCPPS table's och_rcp.cpp.
#include <algorithm>

#include "och_plan.h"
#include "och_pool.h"

using och::check_ready;
using och::check_views;
using och::DevBuf;
using och::DeviceGuard;
using och::ensure_scratch;
using och::fail;
using och::LaunchPlan;
using och::SplitPlan;
using och::TileTable;

int och::check_views(const och_camera *cams, int n_views)
{
    for (int v = 0; v < n_views; ++v)
        if (cams[v].width != cams[0].width || cams[v].height != cams[0].height || cams[v].width <= 0 || cams[v].height <= 0)
            return fail(OCH_E_INVALID, "views must share one positive width and height");
    return OCH_OK;
}

namespace {

int tiled_args(const och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs, uint32_t n,
               uint32_t width)
{
    if (!p || (n && (!origin || !dirs))) return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (width == 0) return fail(OCH_E_INVALID, "width must be positive");
    const uint64_t rows = ((uint64_t)n + width - 1) / width;
    if ((uint64_t)((width + 7) / 8) * ((rows + 7) / 8) * 64 >= (1ull << 32))
        return fail(OCH_E_INVALID, "batch of %u rays %u wide too large", n, width);
    return check_ready(p);
}

// The key of a tiled batch's launch plan: the geometry and the block size.
void batch_key(const och_gpu_pool *p, uint32_t n, uint32_t width, int64_t key[9])
{
    const int64_t k[9] = {n, width, p->opt_block, 0, 0, 0, 0, 0, 0};
    std::memcpy(key, k, sizeof k);
}

// The key of a frame's launch plan: the geometry, the sharding, the block
// size, config 5's compaction and the row deal the frame was made for.
void frame_key(const och_gpu_pool *p, const och::DevFrame &f, bool bounce, int64_t key[9])
{
    const int64_t k[9] = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards, p->opt_block,
                          bounce ? p->opt_bounce_compact : 0, f.chunk_map ? (int64_t)p->deal_serial : 0};
    std::memcpy(key, k, sizeof k);
}

// The frame of n_views checked views (check_views) as the kernels take it,
// with this shard's slice height and, under a row deal, its chunk map.
och::DevFrame make_frame(const och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *out, uint8_t *codes,
                         int row_chunk, int shard, int n_shards)
{
    och::DevFrame f;
    for (int v = 0; v < n_views; ++v) f.cams[v] = cams[v];
    f.n_views = n_views;
    f.palette = p->d_palette.d;
    f.n_voxels = p->n_voxels;
    f.out = out;
    f.codes = codes;
    f.row_chunk = row_chunk;
    f.shard = shard;
    f.n_shards = n_shards;
    f.slice_rows = p->slice_rows(cams[0].height, row_chunk, n_shards);
    const bool dealt = p->deal_for(cams[0].height, row_chunk, n_shards);
    f.chunk_map = dealt ? p->d_chunk_map.d + (size_t)shard * p->deal_max : nullptr;
    return f;
}

// Per-launch timing of the traversal kernel (OCH_OPT_TIMING).  1 (default):
// the dispatch itself records the pool's events (hipExtLaunchKernel, no
// packets of its own); 2: hipEventRecord before and after the launch (two
// marker packets, each with a system-scope release: ~10 us of idle GPU
// between two launches of a stream); 0: none.  Events handed
// over by och_gpu_set_launch_events take the place of the pool's for one launch.
och::Schedule timed_schedule(och_gpu_pool *p, int &st)
{
    och::Schedule sc = p->schedule();
    st = OCH_OK;
    if (p->next_ev_start || p->next_ev_stop) {
        sc.ev_start = p->next_ev_start;
        sc.ev_stop = p->next_ev_stop;
        p->next_ev_start = p->next_ev_stop = nullptr;
    } else if (p->opt_timing == 1) {
        sc.ev_start = p->ev_start;
        sc.ev_stop = p->ev_stop;
    } else if (p->opt_timing == 2 && hipEventRecord(p->ev_start, p->stream()) != hipSuccess) {
        st = fail(OCH_E_HIP, "hipEventRecord: %s", hipGetErrorString(hipGetLastError()));
    }
    return sc;
}

// After the launch: och_gpu_last_kernel_ms reads the pool's events only if
// this launch recorded them (n = 0 launches nothing).
int timed_done(och_gpu_pool *p, const och::Schedule &sc, bool launched)
{
    if (sc.ev_start == p->ev_start && sc.ev_start) {
        p->timed = launched;
    } else if (!sc.ev_start && !sc.ev_stop && p->opt_timing == 2) {
        OCH_HIP(hipEventRecord(p->ev_stop, p->stream()));
        p->timed = true;
    } else {
        p->timed = false;
    }
    return OCH_OK;
}

// A frame loop points the pool at each frame's stream and hands each launch its events; when
// it ends, also after a failure, the pool's own stream is back and no event waits for a launch.
struct FrameLoopScope {
    och_gpu_pool *const p;
    const bool had_ext = p->use_ext;
    const hipStream_t prev = p->ext_stream;
    ~FrameLoopScope()
    {
        p->next_ev_start = p->next_ev_stop = nullptr;
        p->ext_stream = prev;
        p->use_ext = had_ext;
    }
    void frame(void *stream, void *const *start_events, void *const *stop_events, int k)
    {
        p->ext_stream = static_cast<hipStream_t>(stream);
        p->use_ext = true;
        if (start_events) {
            p->next_ev_start = static_cast<hipEvent_t>(start_events[k]);
            p->next_ev_stop = static_cast<hipEvent_t>(stop_events[k]);
        }
    }
};

// The launch order of frame f under OCH_OPT_TILE_ORDER 2 / 3: the pool's plan
// (och_gpu_plan_views) when it was made for this geometry, else none (natural
// order).  split: the launch can run the plan's split form (the grid kernel);
// without it the order stays an unsplit permutation of the frame's grid.
void use_plan(const och_gpu_pool *p, const och::DevFrame &f, bool bounce, bool split, och::Schedule &sc)
{
    const LaunchPlan &plan = p->plans[bounce ? 1 : 0];
    if (p->opt_tile_order < 2 || !plan.order.d) return;
    int64_t key[9];
    frame_key(p, f, bounce, key);
    if (!plan.matches(key)) return;
    sc.order = p->opt_tile_order == 3 ? plan.order_xcd.d : plan.order.d;
    sc.order_n = plan.blocks;
    // the plan's split form, while the options it was made with hold
    const SplitPlan &sp = p->split;
    if (split && !bounce && p->opt_tile_order == 2 && sp.n && p->dev().packed && p->opt_split == sp.params[0] &&
        p->opt_split_segs == sp.params[1] && p->opt_split_level == sp.params[2]) {
        sc.order = sp.order.d;
        sc.order_n = sp.n;
        sc.split_extra = sp.extra;
        sc.split_tasks = sp.tasks.d;
        sc.split_level = (uint32_t)p->opt_split_level;
    }
}

// The tile table of frame f's launch under sc (after use_plan): the pool's
// table of this geometry, block size and launch order, made and uploaded when
// the pool holds none.  Nothing in it depends on the cameras.  bounce: the
// config-5 kernel's launch (its own block size).
int use_tiles(och_gpu_pool *p, const och::DevFrame &f, bool bounce, och::Schedule &sc)
{
    const int block = bounce ? std::max(och::kBounceBlock, sc.block) : sc.block;
    const LaunchPlan &plan = p->plans[bounce ? 1 : 0];
    // the launch order: the split plan's, the plan's (whole, or grouped per XCD), or none
    const std::vector<uint32_t> *order = nullptr, *tasks = nullptr;
    int mode = sc.tile_order == 1 ? 1 : 0;
    if (sc.split_tasks) {
        order = &p->split.h_order;
        tasks = &p->split.h_tasks;
        mode = 4;
    } else if (sc.order) {
        mode = p->opt_tile_order == 3 ? 3 : 2;
        order = mode == 3 ? &plan.h_order_xcd : &plan.h_order;
    }
    const int64_t key[12] = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards,
                             f.slice_rows, block, mode, f.chunk_map ? (int64_t)p->deal_serial : 0,
                             order ? (int64_t)plan.serial : 0, bounce ? 1 : 0};
    TileTable *t = nullptr, *oldest = &p->tile_tables[0];
    for (TileTable &c : p->tile_tables) {
        if (c.used && std::memcmp(c.key, key, sizeof key) == 0) t = &c;
        if (c.used < oldest->used) oldest = &c;
    }
    if (!t) {
        och::plan::TileGeometry g = {f.cams[0].width, f.cams[0].height, f.n_views, f.row_chunk, f.shard, f.n_shards,
                                     f.slice_rows, block, mode == 1 ? 1 : 0, nullptr};
        if (f.chunk_map) g.chunk_map = p->h_chunk_map.data() + (size_t)f.shard * p->deal_max;
        std::vector<uint64_t> table;
        uint32_t grid = 0;
        // a plan of another grid (stale, or for another block size) is not this launch's: natural order
        const uint32_t blocks = (uint32_t)(((uint64_t)f.n_views * ((f.cams[0].width + 7) / 8) * ((f.slice_rows + 7) / 8) * 64 +
                                            block - 1) / block);
        if (order && mode != 4 && order->size() != blocks) order = nullptr;
        const char *why = "";
        if (int st = och::plan::tile_table(g, order ? order->data() : nullptr, order ? (uint32_t)order->size() : 0u,
                                           tasks ? tasks->data() : nullptr, tasks ? (uint32_t)tasks->size() : 0u, table,
                                           grid, &why))
            return fail(st, "tile table of a %d x %d frame, %d views: %s", g.width, g.height, g.n_views, why);
        t = oldest;
        if (t->used) {                          // launches in flight on other streams may read the table it replaces
            t->used = 0;
            if (int ds = och::pool_drain(p)) return ds;
        }
        OCH_HIP(t->d.upload(table));
        t->n = (uint32_t)table.size();
        t->grid = grid;
        t->block = (uint32_t)block;
        std::memcpy(t->key, key, sizeof key);
    }
    t->used = ++p->tile_clock;
    sc.tiles = t->d.d;
    sc.tiles_n = t->n;
    sc.tiles_grid = t->grid;
    sc.tiles_block = t->block;
    return OCH_OK;
}

// A planning render: launch(sc) in natural order, sc.cost naming n_words words preset to
// 0xFFFFFFFF that every launched workgroup overwrites with its duration; c receives them.
// frame: the camera frame the launch renders (bounce: by the config-5 kernel), for its tile table.
template <class Launch>
int cost_render(och_gpu_pool *p, uint32_t *cost, uint32_t n_words, std::vector<uint32_t> &c, Launch launch,
                const och::DevFrame *frame = nullptr, bool bounce = false)
{
    och::Schedule sc = p->schedule();
    sc.tile_order = 0;
    sc.cost = cost;
    if (frame)
        if (int ts = use_tiles(p, *frame, bounce, sc)) return ts;
    OCH_HIP(hipMemsetAsync(cost, 0xFF, (size_t)n_words * 4, p->stream()));
    OCH_HIP(launch(sc));
    c.resize(n_words);
    OCH_HIP(hipMemcpyAsync(c.data(), cost, (size_t)n_words * 4, hipMemcpyDeviceToHost, p->stream()));
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

// One camera launch of frame f: the schedule with the launch's timing, the plan of
// this geometry (split: its split form too), the tile table, the launch, the timing's
// end.  CAMERA_LAUNCH's launch expression takes the schedule as `sc`; a failure names it.
template <class Launch>
int camera_launch(och_gpu_pool *p, const och::DevFrame &f, bool bounce, bool split, const char *what, Launch launch)
{
    int ts;
    och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    use_plan(p, f, bounce, split, sc);
    if (int us = use_tiles(p, f, bounce, sc)) return us;
    const hipError_t e = launch(sc);
    if (e != hipSuccess) return fail(OCH_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return timed_done(p, sc, true);
}
#define CAMERA_LAUNCH(p, f, bounce, split, call) \
    camera_launch(p, f, bounce, split, #call, [&](const och::Schedule &sc) { return call; })

// A host form: render(scratch) into the pool's scratch (pixels words and `spare`
// bytes), then the pixels to the caller's rgba, complete on return.
template <class Render>
int to_host(och_gpu_pool *p, size_t pixels, size_t spare, uint32_t *rgba, Render render)
{
    DeviceGuard g(p->device);
    int st = ensure_scratch(p, pixels * 4 + spare);
    if (st != OCH_OK) return st;
    st = render(reinterpret_cast<uint32_t *>(p->scratch.d));
    if (st != OCH_OK) return st;
    OCH_HIP(hipMemcpyAsync(rgba, p->scratch.d, pixels * 4, hipMemcpyDeviceToHost, p->stream()));
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

}  // namespace

OCH_API int och_gpu_occupancy(const och_gpu_pool *p, int kind, int *blocks_per_cu)
{
    if (!p || !blocks_per_cu) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    OCH_HIP(och::occupancy_blocks_per_cu(kind, p->opt_block, p->depth, blocks_per_cu));
    return OCH_OK;
}

OCH_API int och_gpu_synchronize(och_gpu_pool *p)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    DeviceGuard g(p->device);
    OCH_HIP(hipStreamSynchronize(p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_last_kernel_ms(och_gpu_pool *p, float *ms)
{
    if (!p || !ms) return fail(OCH_E_INVALID, "pool/ms is NULL");
    if (!p->timed)
        return fail(OCH_E_INVALID, "the last launch on this pool was not timed (none yet, n = 0, OCH_OPT_TIMING 0, "
                                   "or the caller's events)");
    DeviceGuard g(p->device);
    OCH_HIP(hipEventSynchronize(p->ev_stop));
    OCH_HIP(hipEventElapsedTime(ms, p->ev_start, p->ev_stop));
    return OCH_OK;
}

OCH_API int och_gpu_trace_batch_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                    uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time,
                                    uint32_t *push_count)
{
    OCH_ENTRY();
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    int ts;
    const och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    OCH_HIP(och::launch_trace_batch(p->dev(), origin, origin_stride, dirs, n, hit_dir, hit_voxel,
                                    reinterpret_cast<uint32_t *>(hit_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_trace_bounce_batch_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                           uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time,
                                           int32_t *bounce_dir, uint32_t *bounce_voxel, float *bounce_time,
                                           uint32_t *push_count)
{
    OCH_ENTRY();
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time || !bounce_dir || !bounce_voxel ||
                     !bounce_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    int ts;
    const och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    OCH_HIP(och::launch_trace_bounce_batch(p->dev(), origin, origin_stride, dirs, n, hit_dir, hit_voxel,
                                           reinterpret_cast<uint32_t *>(hit_time), bounce_dir, bounce_voxel,
                                           reinterpret_cast<uint32_t *>(bounce_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_trace_batch_tiled_dev(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                          uint32_t n, uint32_t width, int32_t *hit_dir, uint32_t *hit_voxel,
                                          float *hit_time, uint32_t *push_count)
{
    OCH_ENTRY();
    if (int st = tiled_args(p, origin, origin_stride, dirs, n, width)) return st;
    if (n && (!hit_dir || !hit_voxel || !hit_time)) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    int ts;
    och::Schedule sc = timed_schedule(p, ts);
    if (ts) return ts;
    if (p->opt_tile_order >= 2 && p->plans[2].order.d) {
        int64_t key[9];
        batch_key(p, n, width, key);
        if (p->plans[2].matches(key)) {
            sc.order = p->plans[2].order.d;
            sc.order_n = p->plans[2].blocks;
        }
    }
    OCH_HIP(och::launch_trace_batch_tiled(p->dev(), origin, origin_stride, dirs, n, width, hit_dir, hit_voxel,
                                          reinterpret_cast<uint32_t *>(hit_time), push_count, sc, p->stream()));
    return timed_done(p, sc, n > 0);
}

OCH_API int och_gpu_plan_batch_tiled(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                     uint32_t n, uint32_t width)
{
    OCH_ENTRY();
    if (int st = tiled_args(p, origin, origin_stride, dirs, n, width)) return st;
    if (n == 0) return OCH_OK;
    DeviceGuard g(p->device);
    const uint32_t tiles = ((width + 7) / 8) * (uint32_t)(((n + width - 1) / width + 7) / 8);
    const uint32_t max_blocks = (uint32_t)(((uint64_t)tiles * 64 + p->opt_block - 1) / p->opt_block);
    const size_t out_bytes = (((size_t)n * 4 + 255) & ~(size_t)255);
    int st = ensure_scratch(p, 3 * out_bytes + (size_t)max_blocks * 4);
    if (st != OCH_OK) return st;
    char *base = p->scratch.d;
    std::vector<uint32_t> c;
    st = cost_render(p, reinterpret_cast<uint32_t *>(base + 3 * out_bytes), max_blocks, c, [&](const och::Schedule &sc) {
        return och::launch_trace_batch_tiled(p->dev(), origin, origin_stride, dirs, n, width,
                                             reinterpret_cast<int32_t *>(base), reinterpret_cast<uint32_t *>(base + out_bytes),
                                             reinterpret_cast<uint32_t *>(base + 2 * out_bytes), nullptr, sc, p->stream());
    });
    if (st != OCH_OK) return st;
    const std::vector<uint32_t> order = och::plan::by_cost(c);
    LaunchPlan &plan = p->plans[2];
    plan.invalidate();                        // no plan until the new one is in place (a failure below leaves none)
    if (int ds = och::pool_drain(p)) return ds;   // launches in flight on other streams may read the old order
    OCH_HIP(plan.order.upload(order));
    batch_key(p, n, width, plan.key);
    plan.blocks = max_blocks;
    return OCH_OK;
}

namespace {

// Host rays in, host records out, synchronous: the rays staged in the pool's
// scratch, traced by the array kernel (width 0) or as a `width`-wide image of
// 8x8 tiles (och_gpu_trace_batch_tiled_dev), the records copied back.
int host_batch(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs, uint32_t n, uint32_t width,
               int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time)
{
    if (!p || (n && (!origin || !dirs || !hit_dir || !hit_voxel || !hit_time)))
        return fail(OCH_E_INVALID, "NULL argument");
    if (origin_stride != 0 && origin_stride != 3) return fail(OCH_E_INVALID, "origin_stride must be 0 or 3");
    if (n == 0) return OCH_OK;
    DeviceGuard g(p->device);
    const size_t n_orig = origin_stride ? (size_t)n * 3 : 3;
    const size_t b_orig = (n_orig * 4 + 255) & ~(size_t)255;
    const size_t b_dirs = ((size_t)n * 12 + 255) & ~(size_t)255;
    const size_t b_out = ((size_t)n * 4 + 255) & ~(size_t)255;
    int st = ensure_scratch(p, b_orig + b_dirs + 3 * b_out);
    if (st != OCH_OK) return st;
    char *base = p->scratch.d;
    float *d_orig = reinterpret_cast<float *>(base);
    float *d_dirs = reinterpret_cast<float *>(base + b_orig);
    int32_t *d_dir = reinterpret_cast<int32_t *>(base + b_orig + b_dirs);
    uint32_t *d_vox = reinterpret_cast<uint32_t *>(base + b_orig + b_dirs + b_out);
    float *d_t = reinterpret_cast<float *>(base + b_orig + b_dirs + 2 * b_out);
    hipStream_t s = p->stream();
    OCH_HIP(hipMemcpyAsync(d_orig, origin, n_orig * 4, hipMemcpyHostToDevice, s));
    OCH_HIP(hipMemcpyAsync(d_dirs, dirs, (size_t)n * 12, hipMemcpyHostToDevice, s));
    st = width ? och_gpu_trace_batch_tiled_dev(p, d_orig, origin_stride, d_dirs, n, width, d_dir, d_vox, d_t, nullptr)
               : och_gpu_trace_batch_dev(p, d_orig, origin_stride, d_dirs, n, d_dir, d_vox, d_t, nullptr);
    if (st != OCH_OK) return st;
    OCH_HIP(hipMemcpyAsync(hit_dir, d_dir, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipMemcpyAsync(hit_voxel, d_vox, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipMemcpyAsync(hit_time, d_t, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OCH_HIP(hipStreamSynchronize(s));
    return OCH_OK;
}

}  // namespace

OCH_API int och_gpu_trace_batch(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                uint32_t n, int32_t *hit_dir, uint32_t *hit_voxel, float *hit_time)
{
    OCH_ENTRY();
    return host_batch(p, origin, origin_stride, dirs, n, 0, hit_dir, hit_voxel, hit_time);
}

OCH_API int och_gpu_trace_batch_image(och_gpu_pool *p, const float *origin, int origin_stride, const float *dirs,
                                      uint32_t n, uint32_t width, int32_t *hit_dir, uint32_t *hit_voxel,
                                      float *hit_time)
{
    OCH_ENTRY();
    if (width == 0) return fail(OCH_E_INVALID, "width must be positive");
    return host_batch(p, origin, origin_stride, dirs, n, width, hit_dir, hit_voxel, hit_time);
}

OCH_API int och_gpu_trace(och_gpu_pool *p, float ox, float oy, float oz, float dx, float dy, float dz,
                          int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time)
{
    OCH_ENTRY();
    if (!hit_direction || !hit_voxel || !hit_time) return fail(OCH_E_INVALID, "NULL output");
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    return och_gpu_trace_batch(p, o, 0, d, 1, hit_direction, hit_voxel, hit_time);
}

OCH_API int och_camera_setup(float px, float py, float pz, float yaw, float pitch, float fov, int width, int height,
                             och_camera *cam)
{
    if (!cam || width <= 0 || height <= 0) return fail(OCH_E_INVALID, "bad camera arguments");
    // ORT/test_och_h_octree.cpp:89-115, evaluated in float exactly as written.
    cam->pos[0] = px;
    cam->pos[1] = py;
    cam->pos[2] = pz;
    cam->aspect = (float)width / (float)height;
    cam->view_x = 2.0F / (float)width;
    cam->view_y = 2.0F / (float)height;
    cam->fov_factor = 1 / tanf(fov / 2);
    const float sin_a = 0, cos_a = 1;
    const float sin_b = sinf(yaw), cos_b = cosf(yaw);
    const float sin_c = sinf(pitch), cos_c = cosf(pitch);
    cam->rot[0] = cos_a * cos_b;
    cam->rot[1] = cos_a * sin_b * sin_c - sin_a * cos_c;
    cam->rot[2] = cos_a * sin_b * cos_c + sin_a * sin_c;
    cam->rot[3] = sin_a * cos_b;
    cam->rot[4] = sin_a * sin_b * sin_c + cos_a * cos_c;
    cam->rot[5] = sin_a * sin_b * cos_c - cos_a * sin_c;
    cam->rot[6] = -sin_b;
    cam->rot[7] = cos_b * sin_c;
    cam->rot[8] = cos_b * cos_c;
    cam->width = width;
    cam->height = height;
    return OCH_OK;
}

OCH_API int och_gpu_raygen_dev(och_gpu_pool *p, const och_camera *cam, float *dirs)
{
    OCH_ENTRY();
    if (!p || !cam || !dirs) return fail(OCH_E_INVALID, "NULL argument");
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_raygen(*cam, dirs, p->stream()));
    return OCH_OK;
}

OCH_API int och_shard_rows(int height, int row_chunk, int n_shards)
{
    if (height <= 0 || row_chunk <= 0 || n_shards <= 0) return 0;
    const int chunks = (height + row_chunk - 1) / row_chunk;
    return ((chunks + n_shards - 1) / n_shards) * row_chunk;
}

namespace {

// `what` (code frames of some kind) needs the code table of a palette small enough for 1-byte codes.
static int needs_code_palette(const och_gpu_pool *p, const char *what)
{
    if (p->n_voxels > OCH_CODE_MAX_VOXELS || !p->d_code_table.d)
        return fail(OCH_E_INVALID, "%s need a palette (och_gpu_set_palette) of at most %d voxel ids", what,
                    OCH_CODE_MAX_VOXELS);
    return OCH_OK;
}

// The shape of a sharded frame: the views, the sharding triple, one size, a token per pixel.
static int frame_args(const och_camera *cams, int n_views, int row_chunk, int shard, int n_shards)
{
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (row_chunk <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards)
        return fail(OCH_E_INVALID, "bad sharding (%d, %d, %d)", row_chunk, shard, n_shards);
    if (int vs = och::check_views(cams, n_views)) return vs;
    if ((uint64_t)cams[0].width * cams[0].height * n_views >= (1ull << 32)) return fail(OCH_E_INVALID, "frame too large");
    return OCH_OK;
}

// A frame loop's arguments: the window, its events, a frame per buffer.
static int loop_args(int n_steps, int n_buffers, void *const *start_events, void *const *stop_events, uint32_t *const *frames)
{
    if (n_steps < 0 || n_buffers < 1) return fail(OCH_E_INVALID, "n_steps %d / n_buffers %d", n_steps, n_buffers);
    if ((start_events == nullptr) != (stop_events == nullptr))
        return fail(OCH_E_INVALID, "start_events and stop_events: both or neither");
    for (int b = 0; b < n_buffers; ++b)
        if (!frames[b]) return fail(OCH_E_INVALID, "frames[%d] is NULL", b);
    return OCH_OK;
}

// What the three unshard entries refuse (table: the entry shades through the code table).
static int unshard_args(const och_gpu_pool *p, const void *gathered, const uint32_t *frames, int width, int height,
                        int row_chunk, int n_shards, int n_views, bool table)
{
    if (!p || !gathered || !frames || width <= 0 || height <= 0 || row_chunk <= 0 || n_shards <= 0 || n_views < 1)
        return fail(OCH_E_INVALID, "bad unshard arguments");
    if (table && !p->d_code_table.d)
        return fail(OCH_E_INVALID, "no code table: set a palette of at most %d voxel ids", OCH_CODE_MAX_VOXELS);
    return OCH_OK;
}

// The host forms' refusal before the staging buffer is sized; the device form checks again.
static int host_capacity(size_t capacity_pixels, int width, int height, size_t &pixels)
{
    pixels = (size_t)width * (size_t)height;
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "rgba holds %zu pixels, %d x %d need %zu", capacity_pixels, width, height, pixels);
    return OCH_OK;
}

int render_views(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices, int row_chunk, int shard,
                 int n_shards, bool bounce, uint8_t *code_slices = nullptr)
{
    if (!p || !cams || (!rgba_slices && !code_slices)) return fail(OCH_E_INVALID, "NULL argument");
    if (int cs = code_slices ? needs_code_palette(p, "indexed-colour frames") : OCH_OK) return cs;
    if (int fs = frame_args(cams, n_views, row_chunk, shard, n_shards)) return fs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    const och::DevFrame f = make_frame(p, cams, n_views, rgba_slices, code_slices, row_chunk, shard, n_shards);
    if (code_slices) return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render_codes(p->dev(), f, sc, bounce, p->stream()));
    if (bounce) return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render_bounce(p->dev(), f, sc, p->stream()));
    return CAMERA_LAUNCH(p, f, bounce, true, och::launch_render(p->dev(), f, sc, p->stream()));
}

// What the four supersampled entries refuse of s, the views and the sample grid
// (the host forms pass their one camera).
static int ssaa_args(const och_camera *cams, int n_views, int s)
{
    if (s != 2 && s != 4 && s != 8) return fail(OCH_E_INVALID, "samples per axis %d: must be 2, 4 or 8", s);
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (int vs = och::check_views(cams, n_views)) return vs;
    if (cams[0].width % s || cams[0].height % s)
        return fail(OCH_E_INVALID, "sample grid %d x %d is not a multiple of %d", cams[0].width, cams[0].height, s);
    return OCH_OK;
}

// och_gpu_render_ssaa_views_dev (light null) and och_gpu_render_lit_ssaa_views_dev behind
// their NULL and light checks.  Every refusal comes before anything is written or launched.
static int render_ssaa_views(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light, int s,
                             uint32_t *rgba, size_t capacity_pixels)
{
    if (int as = ssaa_args(cams, n_views, s)) return as;
    const int Ws = cams[0].width, Hs = cams[0].height;
    if ((uint64_t)Ws * Hs * n_views >= (1ull << 32)) return fail(OCH_E_INVALID, "frame too large");
    const size_t pixels = (size_t)n_views * (Ws / s) * (Hs / s);
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "rgba holds %zu pixels, %d views of %d x %d need %zu", capacity_pixels, n_views, Ws / s,
                    Hs / s, pixels);
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // the sample grid as the 1-sample render's whole frame: its plan, never the split form
    const och::DevFrame f = make_frame(p, cams, n_views, rgba, nullptr, Hs, 0, 1);
    if (light)
        return CAMERA_LAUNCH(p, f, false, false,
                             och::launch_render_lit_ssaa(p->dev(), f, sc, *light, s == 2 ? 1 : s == 4 ? 2 : 3, p->stream()));
    return CAMERA_LAUNCH(p, f, false, false, och::launch_render_ssaa(p->dev(), f, sc, s == 2 ? 1 : s == 4 ? 2 : 3, p->stream()));
}

// The primary plan's split form (och::plan::split_order has the whole story):
// the counting render, the split order and task rows, their upload.
int plan_split(och_gpu_pool *p, const och::DevFrame &f, const std::vector<uint32_t> &by_cost,
               const std::vector<uint32_t> &order, const std::vector<uint32_t> &c)
{
    SplitPlan &sp = p->split;
    sp.invalidate();
    const uint32_t n = (uint32_t)order.size();
    if (p->opt_split <= 0 || p->opt_block != 64 || !p->dev().packed || p->opt_split_level >= p->depth || n == 0 ||
        n >= (1u << 24))
        return OCH_OK;
    // every pixel's walked PUSHes (one counting render of the planned frame)
    std::vector<uint16_t> push((size_t)f.n_views * f.slice_rows * f.cams[0].width);
    DevBuf<uint16_t> d_push;
    OCH_HIP(d_push.reserve(push.size()));
    och::Schedule sc = p->schedule();
    sc.tile_order = 0;
    if (int us = use_tiles(p, f, false, sc)) return us;
    // The counting render writes only the frame's pixels: rows past the height in
    // the last chunk and padding chunks keep the cleared 0, a ray without a PUSH,
    // so the plan does not depend on what the allocation held.
    hipError_t e = hipMemsetAsync(d_push.d, 0, push.size() * 2, p->stream());
    if (e == hipSuccess) e = och::launch_render_push(p->dev(), f, sc, d_push.d, p->stream());
    if (e == hipSuccess) e = hipMemcpyAsync(push.data(), d_push.d, push.size() * 2, hipMemcpyDeviceToHost, p->stream());
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream());
    (void)d_push.release();
    if (e != hipSuccess) return fail(OCH_E_HIP, "split plan: counting render: %s", hipGetErrorString(e));
    const och::plan::Split s = och::plan::split_order(push, f.cams[0].width, f.slice_rows, by_cost, order, c, p->opt_split,
                                                      p->opt_split_segs);
    if (s.tiles == 0) return OCH_OK;
    OCH_HIP(sp.order.upload(s.order));
    OCH_HIP(sp.tasks.upload(s.tasks));
    sp.h_order = s.order;
    sp.h_tasks = s.tasks;
    sp.n = (uint32_t)s.order.size();
    sp.extra = s.extra;
    sp.tiles = s.tiles;
    sp.params[0] = p->opt_split;
    sp.params[1] = p->opt_split_segs;
    sp.params[2] = p->opt_split_level;
    return OCH_OK;
}

}  // namespace

OCH_API int och_gpu_plan_views(och_gpu_pool *p, const och_camera *cams, int n_views, int row_chunk, int shard,
                               int n_shards)
{
    OCH_ENTRY();
    if (!p || !cams) return fail(OCH_E_INVALID, "NULL argument");
    if (n_views < 1 || n_views > OCH_MAX_VIEWS || row_chunk <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards)
        return fail(OCH_E_INVALID, "bad plan arguments");
    if (int vs = check_views(cams, n_views)) return vs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // One planning render per kernel (primary grid, config-5 bounce) into
    // scratch in natural order, timing every workgroup.
    const int W = cams[0].width, rows = p->slice_rows(cams[0].height, row_chunk, n_shards);
    const uint32_t tiles_x = (uint32_t)(W + 7) / 8, tiles_y = (uint32_t)(rows + 7) / 8;
    const size_t frame_bytes = (size_t)n_views * rows * W * 4;
    const uint32_t max_blocks = (uint32_t)((size_t)n_views * tiles_y * tiles_x) + 1024;
    int st = ensure_scratch(p, frame_bytes + (size_t)max_blocks * 4);
    if (st != OCH_OK) return st;
    uint32_t *cost = reinterpret_cast<uint32_t *>(p->scratch.d + frame_bytes);
    const och::DevFrame f = make_frame(p, cams, n_views, reinterpret_cast<uint32_t *>(p->scratch.d), nullptr, row_chunk,
                                       shard, n_shards);
    for (int which = 0; which < 2; ++which) {
        LaunchPlan &plan = p->plans[which];
        std::vector<uint32_t> c;
        st = cost_render(p, cost, max_blocks, c, [&](const och::Schedule &sc) {
            return which ? och::launch_render_bounce(p->dev(), f, sc, p->stream())
                         : och::launch_render(p->dev(), f, sc, p->stream());
        }, &f, which != 0);
        if (st != OCH_OK) return st;
        c.resize(std::find(c.begin(), c.end(), 0xFFFFFFFFu) - c.begin());   // launched blocks wrote a cost
        if (c.empty()) {
            plan.invalidate();                   // no plan: later launches run in natural order
            return fail(OCH_E_INVALID, "planning render wrote no workgroup costs (kernel without cost output?)");
        }
        const std::vector<uint32_t> by_cost = och::plan::by_cost(c);
        std::vector<uint32_t> order = by_cost;
        och::plan::shape(order, p->opt_plan);
        const uint32_t block = (uint32_t)(which ? std::max(och::kBounceBlock, p->opt_block) : p->opt_block);
        const std::vector<uint32_t> grouped = och::plan::group_by_xcd(order, tiles_x, tiles_y, block);
        plan.invalidate();                    // no plan until the new one is in place (a failure below leaves none)
        if (int ds = och::pool_drain(p)) return ds;   // launches in flight on other streams may read the old order
        OCH_HIP(plan.order.upload(order));
        OCH_HIP(plan.order_xcd.upload(grouped));
        plan.h_order = order;
        plan.h_order_xcd = grouped;
        plan.serial = ++p->plan_serial;
        if (which == 0)
            if (int ss = plan_split(p, f, by_cost, order, c)) return ss;
        frame_key(p, f, which != 0, plan.key);
        plan.blocks = (uint32_t)order.size();
    }
    return OCH_OK;
}

OCH_API int och_gpu_set_row_deal(och_gpu_pool *p, int height, int row_chunk, int n_shards, const int32_t *chunk_shard)
{
    if (!p) return fail(OCH_E_INVALID, "pool is NULL");
    if (!chunk_shard && !p->deal_n) return OCH_OK;                      // round-robin already
    if (chunk_shard && p->deal_for(height, row_chunk, n_shards) && row_chunk > 0 &&
        std::equal(p->deal_table.begin(), p->deal_table.end(), chunk_shard))
        return OCH_OK;                                                  // this deal already (plans stay valid)
    // Validate the new deal and build its tables on the host first: a bad
    // call leaves the pool's current deal in place.
    std::vector<int32_t> map, owner;
    int n_chunks = 0, max_chunks = 1;
    if (chunk_shard) {
        if (height <= 0 || row_chunk <= 0 || n_shards <= 0 || n_shards > 32767)
            return fail(OCH_E_INVALID, "bad row deal geometry (%d, %d, %d)", height, row_chunk, n_shards);
        n_chunks = (height + row_chunk - 1) / row_chunk;
        std::vector<std::vector<int32_t>> mine(n_shards);
        for (int c = 0; c < n_chunks; ++c) {
            if (chunk_shard[c] < 0 || chunk_shard[c] >= n_shards)
                return fail(OCH_E_INVALID, "chunk %d dealt to shard %d of %d", c, chunk_shard[c], n_shards);
            mine[chunk_shard[c]].push_back(c);
        }
        for (const auto &m : mine) max_chunks = std::max(max_chunks, (int)m.size());
        if (max_chunks > 65535) return fail(OCH_E_INVALID, "more than 65535 chunks for one shard");
        map.assign((size_t)n_shards * max_chunks, -1);
        owner.assign(n_chunks, 0);
        for (int sh = 0; sh < n_shards; ++sh)
            for (size_t l = 0; l < mine[sh].size(); ++l) {
                map[(size_t)sh * max_chunks + l] = mine[sh][l];
                owner[mine[sh][l]] = (sh << 16) | (int32_t)l;
            }
    }
    DeviceGuard g(p->device);
    DevBuf<int32_t> d_map, d_own;             // the new tables; after the swap below, the old ones (freed on return)
    if (chunk_shard) {
        hipError_t e = d_map.upload(map);
        if (e == hipSuccess) e = d_own.upload(owner);
        if (e != hipSuccess) return fail(OCH_E_HIP, "row deal tables: %s", hipGetErrorString(e));
    }
    // frames in flight may still read the old tables; on failure the new ones
    // are freed and the old deal stays
    const hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return fail(OCH_E_HIP, "row deal: hipDeviceSynchronize: %s", hipGetErrorString(se));
    p->d_chunk_map.swap(d_map);
    p->d_owner.swap(d_own);
    p->h_chunk_map.swap(map);
    ++p->deal_serial;
    if (!chunk_shard) {                        // back to round-robin
        p->deal_n = p->deal_h = p->deal_chunk = p->deal_max = 0;
        p->deal_table.clear();
        return OCH_OK;
    }
    p->deal_h = height;
    p->deal_chunk = row_chunk;
    p->deal_n = n_shards;
    p->deal_max = max_chunks;
    p->deal_table.assign(chunk_shard, chunk_shard + n_chunks);
    return OCH_OK;
}

OCH_API int och_gpu_slice_rows(const och_gpu_pool *p, int height, int row_chunk, int n_shards, int *rows)
{
    if (!p || !rows) return fail(OCH_E_INVALID, "NULL argument");
    *rows = p->slice_rows(height, row_chunk, n_shards);
    return OCH_OK;
}

OCH_API int och_gpu_chunk_costs(och_gpu_pool *p, const och_camera *cams, int n_views, int row_chunk, float *costs)
{
    OCH_ENTRY();
    if (!p || !cams || !costs || row_chunk <= 0) return fail(OCH_E_INVALID, "bad chunk-cost arguments");
    if (n_views < 1 || n_views > OCH_MAX_VIEWS) return fail(OCH_E_INVALID, "n_views %d outside 1..%d", n_views, OCH_MAX_VIEWS);
    if (int vs = check_views(cams, n_views)) return vs;
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    // one whole-frame render, natural 8x8-tile order, every workgroup timed
    const int W = cams[0].width, H = cams[0].height;
    // tiles per workgroup exactly as launch_as sizes the grid kernel's grid
    const uint32_t tiles = (uint32_t)n_views * ((uint32_t)(W + 7) / 8) * ((uint32_t)(H + 7) / 8),
                   per_block = (uint32_t)p->opt_block / 64;
    const uint32_t n_blocks = (tiles + per_block - 1) / per_block;
    const size_t frame_bytes = ((size_t)n_views * H * W * 4 + 255) & ~(size_t)255;
    int st = ensure_scratch(p, frame_bytes + (size_t)n_blocks * 4);
    if (st != OCH_OK) return st;
    const och::DevFrame f = make_frame(p, cams, n_views, reinterpret_cast<uint32_t *>(p->scratch.d), nullptr, H, 0, 1);
    // The grid kernel writes the costs: every launched workgroup overwrites its 0xFFFFFFFF, so a
    // block the launch did not cover is caught below instead of being read as
    // uninitialised scratch.
    std::vector<uint32_t> c;
    st = cost_render(p, reinterpret_cast<uint32_t *>(p->scratch.d + frame_bytes), n_blocks, c,
                     [&](const och::Schedule &sc) { return och::launch_render(p->dev(), f, sc, p->stream()); }, &f);
    if (st != OCH_OK) return st;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (c[b] == 0xFFFFFFFFu) return fail(OCH_E_INVALID, "chunk-cost render left workgroup %u untimed", b);
    const std::vector<float> spread = och::plan::spread_chunk_costs(c, n_views, W, H, per_block, row_chunk);
    std::copy(spread.begin(), spread.end(), costs);
    return OCH_OK;
}

OCH_API int och_deal_chunks(const float *costs, int n_chunks, int n_shards, const float *weights, int32_t *chunk_shard)
{
    if (!costs || !chunk_shard || n_chunks <= 0 || n_shards <= 0) return fail(OCH_E_INVALID, "bad deal arguments");
    std::vector<double> w(n_shards, 1.0);
    double w_sum = 0.0, w_max = 0.0;
    for (int s = 0; s < n_shards; ++s) {
        if (weights) w[s] = weights[s];
        if (!(w[s] > 0.0)) return fail(OCH_E_INVALID, "shard %d weight %g is not positive", s, w[s]);
        w_sum += w[s];
        w_max = std::max(w_max, w[s]);
    }
    // a shard holds at most its weighted share of the chunks plus two, which
    // bounds the padding of the equal-size slices an all-gather needs
    const int cap = (int)std::ceil(n_chunks * w_max / w_sum) + 2;
    std::vector<int> order(n_chunks);
    for (int k = 0; k < n_chunks; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return costs[a] > costs[b]; });
    std::vector<double> load(n_shards, 0.0);
    std::vector<int> count(n_shards, 0);
    for (int k : order) {             // longest processing time first, onto the least loaded shard (per weight)
        int best = -1;
        double best_score = 0.0;
        for (int s = 0; s < n_shards; ++s) {
            if (count[s] >= cap) continue;
            const double score = (load[s] + std::max(0.0f, costs[k])) / w[s];
            if (best < 0 || score < best_score || (score == best_score && count[s] < count[best])) {
                best = s;
                best_score = score;
            }
        }
        chunk_shard[k] = best;
        load[best] += std::max(0.0f, costs[k]);
        ++count[best];
    }
    return OCH_OK;
}

OCH_API int och_gpu_render_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices,
                                     int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    return render_views(p, cams, n_views, rgba_slices, row_chunk, shard, n_shards, false);
}

OCH_API int och_gpu_render_bounce_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint32_t *rgba_slices,
                                            int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    return render_views(p, cams, n_views, rgba_slices, row_chunk, shard, n_shards, true);
}

OCH_API int och_gpu_render_ssaa_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, int s, uint32_t *rgba,
                                          size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cams || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    return render_ssaa_views(p, cams, n_views, nullptr, s, rgba, capacity_pixels);
}

OCH_API int och_light_check(const och_light *l)
{
    if (!l) return fail(OCH_E_INVALID, "light is NULL");
    if (l->flags & ~(OCH_LIGHT_SUN | OCH_LIGHT_AO)) return fail(OCH_E_INVALID, "unknown light flags 0x%x", l->flags);
    if (l->flags & OCH_LIGHT_SUN) {
        const float *s = l->sun_dir;
        if (!std::isfinite(s[0]) || !std::isfinite(s[1]) || !std::isfinite(s[2]))
            return fail(OCH_E_INVALID, "sun_dir is not finite");
        if (s[0] == 0.0F && s[1] == 0.0F && s[2] == 0.0F) return fail(OCH_E_INVALID, "sun_dir is zero");
    }
    if ((l->flags & OCH_LIGHT_AO) && !(std::isfinite(l->ao_reach) && l->ao_reach > 0.0F))
        return fail(OCH_E_INVALID, "ao_reach %g: must be finite and > 0", (double)l->ao_reach);
    if (l->sun_shade < 0 || l->sun_shade > 256) return fail(OCH_E_INVALID, "sun_shade %d outside 0..256", l->sun_shade);
    if (l->ao_shade < 0 || l->ao_shade > 64) return fail(OCH_E_INVALID, "ao_shade %d outside 0..64", l->ao_shade);
    if (l->sun_shade + 4 * l->ao_shade > 256)
        return fail(OCH_E_INVALID, "sun_shade %d + 4 * ao_shade %d exceeds 256", l->sun_shade, l->ao_shade);
    return OCH_OK;
}

namespace {

// och_gpu_render_lit_views_dev / _lit_masks_views_dev / _lit_codes_views_dev:
// exactly one of rgba, masks and codes.
int render_lit_views(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light, uint32_t *rgba,
                     uint8_t *masks, size_t capacity_pixels, int row_chunk, int shard, int n_shards,
                     uint16_t *codes = nullptr)
{
    // every refusal comes before anything is written or launched
    if (!p || !cams || !light || (!rgba && !masks && !codes)) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int cs = codes ? needs_code_palette(p, "lit codes") : OCH_OK) return cs;
    if (int fs = frame_args(cams, n_views, row_chunk, shard, n_shards)) return fs;
    const int W = cams[0].width, H = cams[0].height;
    const size_t pixels = (size_t)n_views * p->slice_rows(H, row_chunk, n_shards) * W;
    if (capacity_pixels < pixels)
        return fail(OCH_E_INVALID, "the buffer holds %zu pixels, %d slices of %d x %d need %zu", capacity_pixels, n_views,
                    W, p->slice_rows(H, row_chunk, n_shards), pixels);
    if (int rs = check_ready(p)) return rs;
    DeviceGuard g(p->device);
    const och::DevFrame f = make_frame(p, cams, n_views, rgba, nullptr, row_chunk, shard, n_shards);
    // the primary render's plan of this grid, never its split form
    if (codes) return CAMERA_LAUNCH(p, f, false, false, och::launch_render_lit_codes(p->dev(), f, sc, *light, codes, p->stream()));
    return CAMERA_LAUNCH(p, f, false, false, och::launch_render_lit(p->dev(), f, sc, *light, masks, p->stream()));
}

}  // namespace

OCH_API int och_gpu_render_lit_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                         uint32_t *rgba_slices, size_t capacity_pixels, int row_chunk, int shard,
                                         int n_shards)
{
    OCH_ENTRY();
    if (!rgba_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, rgba_slices, nullptr, capacity_pixels, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_render_lit_masks_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views,
                                               const och_light *light, uint8_t *mask_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    if (!mask_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, nullptr, mask_slices, capacity_pixels, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_render_lit_codes_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views,
                                               const och_light *light, uint16_t *code_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards)
{
    OCH_ENTRY();
    if (!code_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_lit_views(p, cams, n_views, light, nullptr, nullptr, capacity_pixels, row_chunk, shard, n_shards,
                            code_slices);
}

OCH_API int och_gpu_shade_lit_unshard_views_dev(och_gpu_pool *p, const uint16_t *gathered, uint32_t *frames, int width,
                                                int height, int row_chunk, int n_shards, int n_views,
                                                const och_light *light)
{
    OCH_ENTRY();
    if (int ls = och_light_check(light)) return ls;
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, true)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_shade_lit_unshard(gathered, frames, p->d_code_table.d, width, height, row_chunk, n_shards,
                                          p->slice_rows(height, row_chunk, n_shards), n_views,
                                          p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr,
                                          light->sun_shade, light->ao_shade, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_render_lit(och_gpu_pool *p, const och_camera *cam, const och_light *light, uint32_t *rgba,
                               size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int vs = och::check_views(cam, 1)) return vs;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width, cam->height, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *o) { return och_gpu_render_lit_views_dev(p, cam, 1, light, o, pixels, cam->height, 0, 1); });
}

OCH_API int och_gpu_render_lit_ssaa_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                              int s, uint32_t *rgba, size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cams || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;      // before the s check
    return render_ssaa_views(p, cams, n_views, light, s, rgba, capacity_pixels);
}

OCH_API int och_gpu_render_lit_ssaa(och_gpu_pool *p, const och_camera *cam, const och_light *light, int s, uint32_t *rgba,
                                    size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !light || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int as = ssaa_args(cam, 1, s)) return as;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width / s, cam->height / s, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *o) { return och_gpu_render_lit_ssaa_views_dev(p, cam, 1, light, s, o, pixels); });
}

OCH_API int och_gpu_render_steps_dev(och_gpu_pool *p, const och_camera *cams, int n_views, int n_steps,
                                     void *const *streams, uint32_t *const *frames, int n_buffers,
                                     void *const *start_events, void *const *stop_events, int row_chunk, int bounce)
{
    OCH_ENTRY();
    if (!p || !cams || !streams || !frames) return fail(OCH_E_INVALID, "NULL argument");
    if (int as = loop_args(n_steps, n_buffers, start_events, stop_events, frames)) return as;
    // The frame loop of update_image (ORT/test_och_h_octree.cpp:437-457), one
    // launch per frame, issued here rather than by the caller's interpreter.
    // The pool's stream is restored afterwards, also after a failure.
    FrameLoopScope loop{p};
    int st = OCH_OK;
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        loop.frame(streams[b], start_events, stop_events, k);
        st = render_views(p, cams, n_views, frames[b], row_chunk, 0, 1, bounce != 0);
    }
    return st;
}

OCH_API int och_gpu_render_lit_steps_dev(och_gpu_pool *p, const och_camera *cams, int n_views, const och_light *light,
                                         int n_steps, void *const *streams, uint32_t *const *frames, int n_buffers,
                                         void *const *start_events, void *const *stop_events, int row_chunk)
{
    OCH_ENTRY();
    if (!p || !cams || !light || !streams || !frames) return fail(OCH_E_INVALID, "NULL argument");
    if (int ls = och_light_check(light)) return ls;
    if (int as = loop_args(n_steps, n_buffers, start_events, stop_events, frames)) return as;
    if (int vs = och::check_views(cams, n_views)) return vs;
    // och_gpu_render_steps_dev's loop, each frame a lit frame as one shard
    const size_t pixels = (size_t)n_views * (size_t)cams[0].width * (size_t)cams[0].height;
    FrameLoopScope loop{p};
    int st = OCH_OK;
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        loop.frame(streams[b], start_events, stop_events, k);
        st = render_lit_views(p, cams, n_views, light, frames[b], nullptr, pixels, row_chunk, 0, 1);
    }
    return st;
}

int och::sharded_steps(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views, int n_steps,
                       void *const *streams, uint8_t *const *slices, uint8_t *const *gathered, uint32_t *const *frames,
                       int n_buffers, void *const *start_events, void *const *stop_events, int row_chunk, int bounce,
                       int exchange, bool codes, const och_light *light)
{
    if (!p || !comm || !cams || !streams || !slices) return fail(OCH_E_INVALID, "NULL argument");
    if (light && bounce) return fail(OCH_E_INVALID, "lit and bounce together are out of scope");
    if (light)
        if (int ls = och_light_check(light)) return ls;
    if (n_steps < 0 || n_buffers < 1) return fail(OCH_E_INVALID, "n_steps %d / n_buffers %d", n_steps, n_buffers);
    if (n_views < 1 || n_views > OCH_MAX_VIEWS || row_chunk <= 0) return fail(OCH_E_INVALID, "bad views / row_chunk");
    if (exchange < OCH_EXCHANGE_ALL_GATHER || exchange > OCH_EXCHANGE_GATHER)
        return fail(OCH_E_INVALID, "unknown exchange %d", exchange);
    if ((start_events == nullptr) != (stop_events == nullptr))
        return fail(OCH_E_INVALID, "start_events and stop_events: both or neither");
    int n_ranks = 0, rank = 0, device = -1;
    if (int cs = och::comm_ranks(comm, &n_ranks, &rank, &device)) return cs;
    if (device != p->device) return fail(OCH_E_INVALID, "communicator on device %d, pool on device %d", device, p->device);
    const bool receives = exchange != OCH_EXCHANGE_GATHER || rank == 0;
    const bool shades = exchange == OCH_EXCHANGE_ALL_GATHER || rank == 0;
    // Everything a frame needs is checked before the first is queued: a rank
    // that stops part way leaves its peers' collectives without a partner.
    for (int b = 0; b < n_buffers; ++b) {
        if (!slices[b]) return fail(OCH_E_INVALID, "slices[%d] is NULL", b);
        if (receives && (!gathered || !gathered[b])) return fail(OCH_E_INVALID, "rank %d needs gathered[%d]", rank, b);
        if (shades && (!frames || !frames[b])) return fail(OCH_E_INVALID, "rank %d needs frames[%d]", rank, b);
    }
    if (int vs = check_views(cams, n_views)) return vs;
    if (codes && shades && !p->d_code_table.d)
        return fail(OCH_E_INVALID, "no code table: set a palette of at most %d voxel ids", OCH_CODE_MAX_VOXELS);
    // lit codes: the rendering rank needs the palette too (render_lit_views would refuse mid-window)
    if (int cs = codes && light ? needs_code_palette(p, "lit codes") : OCH_OK) return cs;
    const int W = cams[0].width, H = cams[0].height;
    const size_t pixels = (size_t)n_views * p->slice_rows(H, row_chunk, n_ranks) * W;
    const size_t bytes = pixels * (codes ? (light ? 2 : 1) : 4);
    DeviceGuard g(p->device);
    // Per frame: render -> exchange -> shade, all on the frame's stream, so
    // the three are ordered on the device and the host never waits.  A
    // buffer set is reused only behind the previous frame on its stream.
    int st = OCH_OK;
    bool issued = false;                     // a collective of this window is queued
    FrameLoopScope loop{p};
    for (int k = 0; k < n_steps && st == OCH_OK; ++k) {
        const int b = k % n_buffers;
        const hipStream_t s = static_cast<hipStream_t>(streams[b]);
        loop.frame(streams[b], start_events, stop_events, k);
        if (light)
            st = render_lit_views(p, cams, n_views, light, codes ? nullptr : reinterpret_cast<uint32_t *>(slices[b]),
                                  nullptr, pixels, row_chunk, rank, n_ranks,
                                  codes ? reinterpret_cast<uint16_t *>(slices[b]) : nullptr);
        else
            st = render_views(p, cams, n_views, codes ? nullptr : reinterpret_cast<uint32_t *>(slices[b]), row_chunk,
                              rank, n_ranks, bounce != 0, codes ? slices[b] : nullptr);
        if (st == OCH_OK) {
            st = exchange == OCH_EXCHANGE_GATHER
                     ? och::comm_gather(comm, slices[b], receives ? gathered[b] : nullptr, bytes, 0, s)
                     : och::comm_all_gather(comm, slices[b], gathered[b], bytes, s);
            issued = issued || st == OCH_OK;
        }
        if (st == OCH_OK && shades)
            st = !codes ? och_gpu_unshard_views_dev(p, reinterpret_cast<const uint32_t *>(gathered[b]), frames[b], W, H,
                                                    row_chunk, n_ranks, n_views)
                 : light ? och_gpu_shade_lit_unshard_views_dev(p, reinterpret_cast<const uint16_t *>(gathered[b]),
                                                               frames[b], W, H, row_chunk, n_ranks, n_views, light)
                         : och_gpu_shade_unshard_views_dev(p, gathered[b], frames[b], W, H, row_chunk, n_ranks, n_views);
    }
    if (st != OCH_OK && issued) {
        // The peers' collectives of this window can no longer all complete.
        // Aborting here does not unblock the peers: their callers must abort
        // theirs (bench.py's watchdog, or the process exiting).  A failure
        // before this rank queued any collective leaves the communicator as
        // it was (every rank failing alike keeps a consistent one).
        och::comm_abort(comm);               // leaves the error text alone
        return fail(st, "%s (communicator aborted: the window stopped part way)", och_last_error());
    }
    return st;
}

OCH_API int och_gpu_render_sharded_steps_dev(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views,
                                             int n_steps, void *const *streams, uint8_t *const *slices,
                                             uint8_t *const *gathered, uint32_t *const *frames, int n_buffers,
                                             void *const *start_events, void *const *stop_events, int row_chunk,
                                             int bounce, int exchange)
{
    OCH_ENTRY();
    return och::sharded_steps(p, comm, cams, n_views, n_steps, streams, slices, gathered, frames, n_buffers, start_events,
                              stop_events, row_chunk, bounce, exchange, true, nullptr);
}

OCH_API int och_gpu_render_lit_sharded_steps_dev(och_gpu_pool *p, och_comm *comm, const och_camera *cams, int n_views,
                                                 int n_steps, void *const *streams, uint8_t *const *slices,
                                                 uint8_t *const *gathered, uint32_t *const *frames, int n_buffers,
                                                 void *const *start_events, void *const *stop_events, int row_chunk,
                                                 const och_light *light, int exchange)
{
    OCH_ENTRY();
    if (!light) return fail(OCH_E_INVALID, "light is NULL");
    return och::sharded_steps(p, comm, cams, n_views, n_steps, streams, slices, gathered, frames, n_buffers, start_events,
                              stop_events, row_chunk, 0, exchange, true, light);
}

OCH_API int och_gpu_render_codes_views_dev(och_gpu_pool *p, const och_camera *cams, int n_views, uint8_t *code_slices,
                                           int row_chunk, int shard, int n_shards, int bounce)
{
    OCH_ENTRY();
    if (!code_slices) return fail(OCH_E_INVALID, "NULL argument");
    return render_views(p, cams, n_views, nullptr, row_chunk, shard, n_shards, bounce != 0, code_slices);
}

OCH_API int och_gpu_shade_unshard_views_dev(och_gpu_pool *p, const uint8_t *gathered, uint32_t *frames, int width,
                                            int height, int row_chunk, int n_shards, int n_views)
{
    OCH_ENTRY();
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, true)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_shade_unshard(gathered, frames, p->d_code_table.d, width, height, row_chunk, n_shards,
                                      p->slice_rows(height, row_chunk, n_shards), n_views,
                                      p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_render_dev(och_gpu_pool *p, const och_camera *cam, uint32_t *rgba_slice, int row_chunk, int shard,
                               int n_shards)
{
    OCH_ENTRY();
    if (!cam) return fail(OCH_E_INVALID, "NULL camera");
    return och_gpu_render_views_dev(p, cam, 1, rgba_slice, row_chunk, shard, n_shards);
}

OCH_API int och_gpu_unshard_views_dev(och_gpu_pool *p, const uint32_t *gathered, uint32_t *frames, int width,
                                      int height, int row_chunk, int n_shards, int n_views)
{
    OCH_ENTRY();
    if (int as = unshard_args(p, gathered, frames, width, height, row_chunk, n_shards, n_views, false)) return as;
    DeviceGuard g(p->device);
    OCH_HIP(och::launch_unshard(gathered, frames, width, height, row_chunk, n_shards,
                                p->slice_rows(height, row_chunk, n_shards), n_views,
                                p->deal_for(height, row_chunk, n_shards) ? p->d_owner.d : nullptr, p->stream()));
    return OCH_OK;
}

OCH_API int och_gpu_unshard_dev(och_gpu_pool *p, const uint32_t *gathered, uint32_t *frame, int width, int height,
                                int row_chunk, int n_shards)
{
    OCH_ENTRY();
    return och_gpu_unshard_views_dev(p, gathered, frame, width, height, row_chunk, n_shards, 1);
}

OCH_API int och_gpu_render(och_gpu_pool *p, const och_camera *cam, uint32_t *rgba)
{
    OCH_ENTRY();
    if (!p || !cam || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    // no capacity argument, and a scratch of exactly the frame
    return to_host(p, (size_t)cam->width * cam->height, 0, rgba,
                   [&](uint32_t *scratch) { return och_gpu_render_dev(p, cam, scratch, cam->height, 0, 1); });
}

OCH_API int och_gpu_render_ssaa(och_gpu_pool *p, const och_camera *cam, int s, uint32_t *rgba, size_t capacity_pixels)
{
    OCH_ENTRY();
    if (!p || !cam || !rgba) return fail(OCH_E_INVALID, "NULL argument");
    if (int as = ssaa_args(cam, 1, s)) return as;
    if (int rs = check_ready(p)) return rs;
    size_t pixels;
    if (int cs = host_capacity(capacity_pixels, cam->width / s, cam->height / s, pixels)) return cs;
    return to_host(p, pixels, 4, rgba,
                   [&](uint32_t *scratch) { return och_gpu_render_ssaa_views_dev(p, cam, 1, s, scratch, pixels); });
}
