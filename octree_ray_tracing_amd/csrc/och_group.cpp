// och_group.cpp -- multi-GPU frames from ONE host process:
// a reference host in C++ (ORT/test_och_h_octree.cpp:437-457 renders one
// frame per OnUserUpdate) drives every GPU of the node.
//
//   * each device holds a replica of the read-only node pool (one H2D upload);
//   * rows are dealt in chunks of row_chunk rows over the devices
//     (och_shard_rows, or och_frame_group_plan's cost deal); each device
//     renders its slice -- raygen, traversal and shading fused -- as 1-byte
//     colour codes (or RGBA8 words for palettes of more than
//     OCH_CODE_MAX_VOXELS ids); lit frames (och_frame_group_render_lit) as
//     2-byte lit codes, or lit RGBA8 words for such palettes;
//   * one RCCL all-gather over xGMI (ncclCommInitAll over the devices) gives
//     every device all slices, and one kernel per device shades + unshards
//     them into the [views][H][W] RGBA8 frames (olc::Pixel layout).
// Each device has its own issuing thread (one thread per GPU),
// which enqueues its device's window of frames -- render, all-gather on its
// own communicator, shade -- through och::sharded_steps (och_api.cpp), the
// window of the one-process-per-GPU path; the calling thread posts the window
// to every worker and returns once all of them have enqueued it, so the
// devices' launch costs overlap instead of adding up.  Frames rotate over up to
// kMaxSets buffer sets, each with its own stream per device, so several
// frames can be in flight (och_frame_group_render_steps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "och_host.h"
#include "och_rccl.h"

using och::DeviceGuard;
using och::fail;

namespace {

constexpr int kMaxSets = 8;

// One frame in flight on one device: its stream, this device's slices, all
// devices' slices, the frames.
struct BufferSet {
    hipStream_t stream = nullptr;
    och::DevBuf<uint8_t> slice, gathered;
    och::DevBuf<uint32_t> frames;
};

// One host thread bound to one device: runs the jobs posted to it, one at a
// time, and reports each job's status (and its thread-local error text).
class DeviceWorker {
  public:
    explicit DeviceWorker(int device) : device_(device), thread_([this] { loop(); }) {}
    ~DeviceWorker()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            quit_ = true;
        }
        cv_.notify_all();
        thread_.join();
    }
    void post(std::function<int()> job)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            job_ = std::move(job);
            busy_ = true;
        }
        cv_.notify_all();
    }
    // Wait for the posted job; its status, and its error text on failure.
    int wait(std::string &error)
    {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [this] { return !busy_; });
        error = error_;
        return status_;
    }

  private:
    void loop()
    {
        const bool dev_ok = hipSetDevice(device_) == hipSuccess;
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [this] { return busy_ || quit_; });
            if (quit_) return;
            std::function<int()> job = std::move(job_);
            l.unlock();
            int st = dev_ok ? job() : och::report(OCH_E_HIP, "worker thread could not select its device");
            std::string err = st == OCH_OK ? std::string() : std::string(och_last_error());
            l.lock();
            status_ = st;
            error_ = std::move(err);
            busy_ = false;
            cv_.notify_all();
        }
    }

    int device_;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    bool busy_ = false, quit_ = false;
    int status_ = OCH_OK;
    std::string error_;
    std::thread thread_;   // last: starts after the members it reads
};

}  // namespace

struct och_frame_group {
    int n = 0;
    std::vector<int> devices;
    std::vector<och_gpu_pool *> pools;
    std::vector<och_comm *> comms;
    std::vector<std::unique_ptr<DeviceWorker>> workers;
    std::vector<std::array<BufferSet, kMaxSets>> sets;   // per device; the first n_sets have a stream
    int n_sets = 0;
    size_t slice_bytes = 0, frame_bytes = 0;             // what every set in use holds at least
    int width = 0, height = 0, n_views = 0;
    int last_set = 0;        // the buffer set of the last frame
    bool rendered = false;
    // a device's frame failed after others may have queued their all-gathers:
    // the communicators were aborted and the group refuses further frames
    bool broken = false;
};

namespace {

// Run job(r) on every device's worker thread; the first failure is reported
// (with its device) on the calling thread.
int run_on_devices(och_frame_group *g, const std::function<int(int)> &job)
{
    for (int r = 0; r < g->n; ++r) g->workers[r]->post([&job, r] { return job(r); });
    int st = OCH_OK, first = 0;
    std::string first_error;
    for (int r = 0; r < g->n; ++r) {
        std::string err;
        const int s = g->workers[r]->wait(err);
        if (s != OCH_OK && st == OCH_OK) {
            st = s;
            first = r;
            first_error = std::move(err);
        }
    }
    return st == OCH_OK ? OCH_OK : fail(st, "device %d: %s", g->devices[first], first_error.c_str());
}

int sync_all(och_frame_group *g)
{
    for (int r = 0; r < g->n; ++r) {
        if (int st = och_gpu_synchronize(g->pools[r])) return st;
        DeviceGuard dg(g->devices[r]);
        if (!dg.ok) return fail(OCH_E_HIP, "cannot select device %d", g->devices[r]);
        for (int b = 0; b < g->n_sets; ++b) OCH_HIP(hipStreamSynchronize(g->sets[r][b].stream));
    }
    return OCH_OK;
}

// n_sets buffer sets for n_views frames of W x H, slices of rows x W in
// `elem`-byte pixels, and one stream per set and device.
int ensure_buffers(och_frame_group *g, int W, int H, int n_views, int row_chunk, size_t elem, int n_sets)
{
    int slice_rows = 0;
    if (och_gpu_slice_rows(g->pools[0], H, row_chunk, g->n, &slice_rows) != OCH_OK) return OCH_E_INVALID;
    const size_t slice = (size_t)n_views * (size_t)slice_rows * W * elem;
    const size_t frame = (size_t)n_views * H * W * 4;
    if (n_sets <= g->n_sets && slice <= g->slice_bytes && frame <= g->frame_bytes) return OCH_OK;
    if (int st = sync_all(g)) return st;     // frames in flight use the buffers that grow below
    g->slice_bytes = g->frame_bytes = 0;     // until every set holds the new sizes
    const int sets = std::max(n_sets, g->n_sets);
    for (int r = 0; r < g->n; ++r) {
        DeviceGuard dg(g->devices[r]);
        if (!dg.ok) return fail(OCH_E_HIP, "cannot select device %d", g->devices[r]);
        for (int b = 0; b < sets; ++b) {
            BufferSet &s = g->sets[r][b];
            hipError_t e = s.stream ? hipSuccess : hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = s.slice.reserve(slice);
            if (e == hipSuccess) e = s.gathered.reserve(slice * g->n);
            if (e == hipSuccess) e = s.frames.reserve(frame / 4);
            if (e != hipSuccess) return fail(OCH_E_NOMEM, "frame group buffers: %s", hipGetErrorString(e));
        }
    }
    g->n_sets = sets;
    g->slice_bytes = slice;
    g->frame_bytes = frame;
    return OCH_OK;
}

// Abort every device's communicator (ncclCommAbort): after one device's
// window failed, the others' all-gathers of that frame have no partner and
// would hold their streams forever.  (The failed window already aborted its own.)
void abort_comms(och_frame_group *g)
{
    for (och_comm *c : g->comms) och::comm_abort(c);
    g->broken = true;
}

// light (optional): lit frames -- 2-byte lit codes when the palette fits, lit
// RGBA8 slices and a plain unshard otherwise.
int render_steps(och_frame_group *g, const och_camera *cams, int n_views, int n_steps, int n_sets, int row_chunk,
                 int bounce, const och_light *light = nullptr)
{
    if (!g || !cams || n_views < 1 || n_views > OCH_MAX_VIEWS || row_chunk < 1 || n_steps < 0 || n_sets < 1 ||
        n_sets > kMaxSets)
        return fail(OCH_E_INVALID, "bad frame group render arguments");
    if (g->broken) return fail(OCH_E_HIP, "frame group unusable after a failed frame (communicators aborted)");
    if (light)
        if (int ls = och_light_check(light)) return ls;
    if (int vs = och::check_views(cams, n_views)) return vs;
    const int W = cams[0].width, H = cams[0].height;
    // Indexed colour when the palette allows it (a quarter of the RGBA8 bytes on xGMI).
    int n_vox = 0;
    int st = och::pool_palette_size(g->pools[0], &n_vox);
    if (st != OCH_OK) return st;
    const bool codes = n_vox <= OCH_CODE_MAX_VOXELS;
    st = ensure_buffers(g, W, H, n_views, row_chunk, codes ? (light ? 2 : 1) : 4, n_sets);
    if (st != OCH_OK) return st;
    if (n_steps == 0) return OCH_OK;
    // the shade of every device needs its code table (checked before any frame is queued)
    if (codes)
        for (int r = 0; r < g->n; ++r) {
            int nv = 0;
            if (och::pool_palette_size(g->pools[r], &nv) != OCH_OK || nv < 1)
                return fail(OCH_E_INVALID, "device %d has no palette", g->devices[r]);
        }
    st = run_on_devices(g, [&](int r) {
        const och::EntryScope entry("och_frame_group_render_steps");   // this thread's, for och_discarded_error
        void *streams[kMaxSets];
        uint8_t *slices[kMaxSets], *gathered[kMaxSets];
        uint32_t *frames[kMaxSets];
        for (int b = 0; b < n_sets; ++b) {
            BufferSet &s = g->sets[r][b];
            streams[b] = s.stream;
            slices[b] = s.slice.d;
            gathered[b] = s.gathered.d;
            frames[b] = s.frames.d;
        }
        // one thread per communicator: no RCCL group call is needed
        return och::sharded_steps(g->pools[r], g->comms[r], cams, n_views, n_steps, streams, slices, gathered, frames,
                                  n_sets, nullptr, nullptr, row_chunk, bounce, OCH_EXCHANGE_ALL_GATHER, codes, light);
    });
    if (st != OCH_OK) {
        abort_comms(g);                      // leaves the error text alone
        return fail(st, "%s (communicators aborted; destroy the group)", och_last_error());
    }
    g->width = W;
    g->height = H;
    g->n_views = n_views;
    g->last_set = (n_steps - 1) % n_sets;
    g->rendered = true;
    return OCH_OK;
}

}  // namespace

OCH_API int och_frame_group_create(const int *devices, int n_devices, const uint32_t *nodes, uint32_t n_nodes,
                                   uint32_t root, int depth, int index_base, float miss_t, och_frame_group **out)
{
    if (!out || !nodes || n_devices < 1 || n_devices > 64) return fail(OCH_E_INVALID, "bad frame group arguments");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(OCH_E_NODEV, "no HIP device visible");
    std::vector<int> devs(n_devices);
    if (!devices) {                          // the first n_devices gfx950 devices, in HIP order
        std::vector<int> all(ndev);
        int n950 = 0;
        if (och_device_list(all.data(), ndev, &n950) != OCH_OK || n950 < n_devices)
            return fail(OCH_E_NODEV, "%d gfx950 devices asked, %d visible", n_devices, n950);
        for (int r = 0; r < n_devices; ++r) devs[r] = all[r];
    }
    for (int r = 0; r < n_devices; ++r) {
        if (devices) devs[r] = devices[r];
        if (devs[r] < 0 || devs[r] >= ndev) return fail(OCH_E_NODEV, "device %d not visible", devs[r]);
        for (int q = 0; q < r; ++q)
            if (devs[q] == devs[r]) return fail(OCH_E_INVALID, "a device appears twice in the group");
    }
    const och::Rccl &R = och::rccl();
    if (!R.ok) return fail(OCH_E_NODEV, "%s", R.error.c_str());
    auto *g = new och_frame_group;
    g->n = n_devices;
    g->devices = devs;
    g->pools.assign(n_devices, nullptr);
    g->sets = decltype(g->sets)(n_devices);
    for (int r = 0; r < n_devices; ++r) {
        const int st = och_gpu_pool_create(nodes, n_nodes, root, depth, index_base, miss_t, devs[r], &g->pools[r]);
        if (st != OCH_OK) {
            const std::string msg = och_last_error();
            och_frame_group_destroy(g);
            return fail(st, "device %d: %s", devs[r], msg.c_str());
        }
    }
    std::vector<ncclComm_t> raw(n_devices, nullptr);
    const ncclResult_t nr = R.comm_init_all(raw.data(), n_devices, devs.data());
    if (nr != ncclSuccess) {
        och_frame_group_destroy(g);
        return fail(OCH_E_HIP, "ncclCommInitAll: %s", R.error_string(nr));
    }
    for (int r = 0; r < n_devices; ++r) g->comms.push_back(och::comm_adopt(raw[r], n_devices, r, devs[r]));
    for (int r = 0; r < n_devices; ++r) g->workers.emplace_back(new DeviceWorker(devs[r]));
    *out = g;
    return OCH_OK;
}

OCH_API int och_frame_group_destroy(och_frame_group *g)
{
    if (!g) return OCH_OK;
    (void)sync_all(g);
    g->workers.clear();                      // joins the issuing threads
    for (och_comm *c : g->comms) och_comm_destroy(c);
    // the pools before the streams: pool destroy synchronises the stream its pool names
    for (och_gpu_pool *p : g->pools)
        if (p) och_gpu_pool_destroy(p);
    int st = OCH_OK;
    for (int r = 0; r < g->n; ++r) {
        DeviceGuard dg(g->devices[r]);
        if (!dg.ok) st = fail(OCH_E_HIP, "cannot select device %d", g->devices[r]);
        for (BufferSet &s : g->sets[r]) {
            (void)s.slice.release();
            (void)s.gathered.release();
            (void)s.frames.release();
            if (s.stream) (void)hipStreamDestroy(s.stream);
        }
    }
    delete g;
    return st;
}

OCH_API int och_frame_group_size(const och_frame_group *g, int *n_devices)
{
    if (!g || !n_devices) return fail(OCH_E_INVALID, "NULL argument");
    *n_devices = g->n;
    return OCH_OK;
}

OCH_API int och_frame_group_pool(och_frame_group *g, int rank, och_gpu_pool **pool)
{
    if (!g || !pool || rank < 0 || rank >= g->n) return fail(OCH_E_INVALID, "bad rank");
    *pool = g->pools[rank];
    return OCH_OK;
}

OCH_API int och_frame_group_set_palette(och_frame_group *g, const uint32_t *rgba, uint32_t n_voxels)
{
    if (!g) return fail(OCH_E_INVALID, "NULL group");
    for (och_gpu_pool *p : g->pools) {
        const int st = och_gpu_set_palette(p, rgba, n_voxels);
        if (st != OCH_OK) return st;
    }
    return OCH_OK;
}

OCH_API int och_frame_group_set_option(och_frame_group *g, int option, int value)
{
    if (!g) return fail(OCH_E_INVALID, "NULL group");
    for (och_gpu_pool *p : g->pools) {
        const int st = och_gpu_set_option(p, option, value);
        if (st != OCH_OK) return st;
    }
    return OCH_OK;
}

OCH_API int och_frame_group_plan(och_frame_group *g, const och_camera *cams, int n_views, int row_chunk)
{
    OCH_ENTRY();
    if (!g || !cams || row_chunk < 1 || n_views < 1) return fail(OCH_E_INVALID, "bad plan arguments");
    if (g->broken) return fail(OCH_E_HIP, "frame group unusable after a failed frame (communicators aborted)");
    if (int st = sync_all(g)) return st;     // frames in flight may read the deal and the plans
    if (g->n > 1) {
        // deal the row chunks by their cost in one timed render of these views
        // (device 0), instead of round-robin, so every device gets an equal
        // share.  The deal is set on every pool or on none: a group whose
        // pools disagree would unshard slices into the wrong rows.
        const int H = cams[0].height, n_chunks = (H + row_chunk - 1) / row_chunk;
        std::vector<float> costs(n_chunks);
        std::vector<int32_t> deal(n_chunks);
        int st = och_gpu_chunk_costs(g->pools[0], cams, n_views, row_chunk, costs.data());
        if (st == OCH_OK) st = och_deal_chunks(costs.data(), n_chunks, g->n, nullptr, deal.data());
        for (int r = 0; r < g->n && st == OCH_OK; ++r)
            st = och_gpu_set_row_deal(g->pools[r], H, row_chunk, g->n, deal.data());
        if (st != OCH_OK) {
            const std::string msg = och_last_error();
            for (int r = 0; r < g->n; ++r) (void)och_gpu_set_row_deal(g->pools[r], H, row_chunk, g->n, nullptr);
            return fail(st, "%s (every device back to round-robin chunks)", msg.c_str());
        }
    }
    for (int r = 0; r < g->n; ++r) {
        int st = och_gpu_plan_views(g->pools[r], cams, n_views, row_chunk, r, g->n);
        if (st == OCH_OK) st = och_gpu_set_option(g->pools[r], OCH_OPT_TILE_ORDER, 2);
        if (st != OCH_OK) return st;
    }
    return OCH_OK;
}

OCH_API int och_frame_group_render(och_frame_group *g, const och_camera *cams, int n_views, int row_chunk, int bounce)
{
    OCH_ENTRY();
    return render_steps(g, cams, n_views, 1, 1, row_chunk, bounce);
}

OCH_API int och_frame_group_render_steps(och_frame_group *g, const och_camera *cams, int n_views, int n_steps,
                                         int n_buffers, int row_chunk, int bounce)
{
    OCH_ENTRY();
    return render_steps(g, cams, n_views, n_steps, n_buffers, row_chunk, bounce);
}

OCH_API int och_frame_group_render_lit(och_frame_group *g, const och_camera *cams, int n_views, int row_chunk,
                                       const och_light *light)
{
    OCH_ENTRY();
    if (!light) return fail(OCH_E_INVALID, "light is NULL");
    return render_steps(g, cams, n_views, 1, 1, row_chunk, 0, light);
}

OCH_API int och_frame_group_render_lit_steps(och_frame_group *g, const och_camera *cams, int n_views, int n_steps,
                                             int n_buffers, int row_chunk, const och_light *light)
{
    OCH_ENTRY();
    if (!light) return fail(OCH_E_INVALID, "light is NULL");
    return render_steps(g, cams, n_views, n_steps, n_buffers, row_chunk, 0, light);
}

OCH_API int och_frame_group_frames_dev(och_frame_group *g, int rank, uint32_t **frames)
{
    if (!g || !frames || rank < 0 || rank >= g->n) return fail(OCH_E_INVALID, "bad rank");
    if (!g->rendered) return fail(OCH_E_INVALID, "nothing rendered yet");
    *frames = g->sets[rank][g->last_set].frames.d;
    return OCH_OK;
}

OCH_API int och_frame_group_download(och_frame_group *g, int rank, uint32_t *rgba)
{
    if (!g || !rgba || rank < 0 || rank >= g->n) return fail(OCH_E_INVALID, "bad rank");
    if (!g->rendered) return fail(OCH_E_INVALID, "nothing rendered yet");
    DeviceGuard dg(g->devices[rank]);
    if (!dg.ok) return fail(OCH_E_HIP, "cannot select device %d", g->devices[rank]);
    const BufferSet &s = g->sets[rank][g->last_set];
    const size_t bytes = (size_t)g->n_views * g->height * g->width * 4;
    OCH_HIP(hipMemcpyAsync(rgba, s.frames.d, bytes, hipMemcpyDeviceToHost, s.stream));
    OCH_HIP(hipStreamSynchronize(s.stream));
    return OCH_OK;
}

OCH_API int och_frame_group_synchronize(och_frame_group *g)
{
    if (!g) return fail(OCH_E_INVALID, "NULL group");
    return sync_all(g);
}
