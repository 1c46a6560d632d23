// och_gpu.hpp -- header-only C++ host mirror over the C ABI (och_gpu.h).
//
// Gives a reference user the same call shapes they had:
//   tree.sse_trace(ox, oy, oz, dx, dy, dz, hit_direction, hit_voxel, hit_time)
//                                               ORT/och_h_octree.h:292, :449-452
//   camera.update_position() + window.update_image()
//                                               ORT/test_och_h_octree.cpp:87-138, :437-457
// with the work done by the gfx950 kernels.  Errors throw och::gpu::error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <array>
#include <utility>
#include <vector>

#include "och_gpu.h"

namespace och {
namespace gpu {

// och::direction (ORT/och_tree_helper.h:7-18).
enum class direction : int32_t {
    x_pos = 0, y_pos = 1, z_pos = 2, x_neg = 3, y_neg = 4, z_neg = 5, exit = 6, inside = 7, error = 8
};

// Which voxels a conditional stroke touches (OCH_WHEN_*): those whose id is, or is not, `match`.
enum class when : int { is = OCH_WHEN_IS, is_not = OCH_WHEN_IS_NOT };

struct error : std::runtime_error {
    int status;
    error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(int status, const char *what)
{
    if (status != OCH_OK) throw error(status, std::string(what) + ": " + och_last_error());
}

// HIP indices of the visible gfx950 devices (och_device_list).
inline std::vector<int> devices()
{
    int n = 0;
    check(och_device_list(nullptr, 0, &n), "och_device_list");
    std::vector<int> d(n);
    if (n) check(och_device_list(d.data(), n, &n), "och_device_list");
    return d;
}

struct float3 {
    float x, y, z;
};

// A node pool resident on one GPU.  Construct from the reference's own table
// (h_octree: table->nodes, capacity, root_idx, Depth) or from och_build_terrain.
class tree {
public:
    tree(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base = 1,
         float miss_t = __builtin_inff(), int device = -1)
    {
        check(och_gpu_pool_create(nodes, n_nodes, root, depth, index_base, miss_t, device, &pool_), "och_gpu_pool_create");
    }
    // A pool the library made (world::make_pool); the tree owns it.
    explicit tree(och_gpu_pool *adopted) : pool_(adopted) {}
    tree(const tree &) = delete;
    tree &operator=(const tree &) = delete;
    ~tree() { och_gpu_pool_destroy(pool_); }

    // h_octree::sse_trace, one ray (synchronous; fine for the pick ray of :536).
    void sse_trace(float ox, float oy, float oz, float dx, float dy, float dz, direction &hit_direction,
                   uint32_t &hit_voxel, float &hit_time) const
    {
        int32_t d = 0;
        check(och_gpu_trace(pool_, ox, oy, oz, dx, dy, dz, &d, &hit_voxel, &hit_time), "och_gpu_trace");
        hit_direction = static_cast<direction>(d);
    }
    void sse_trace(float3 o, float3 d, direction &hit_direction, uint32_t &hit_voxel, float &hit_time) const
    {
        sse_trace(o.x, o.y, o.z, d.x, d.y, d.z, hit_direction, hit_voxel, hit_time);
    }

    // Many rays at once (the per-pixel loop's calls, batched).  width > 0: the
    // rays are a camera's, a row-major image that many rays wide (x + y * W,
    // ORT/test_och_h_octree.cpp:135), traced 8x8 tiles per wave
    // (och_gpu_trace_batch_image); same records either way.
    void trace_batch(float3 origin, const std::vector<float3> &dirs, std::vector<direction> &dir_out,
                     std::vector<uint32_t> &voxel_out, std::vector<float> &t_out, uint32_t width = 0) const
    {
        const uint32_t n = static_cast<uint32_t>(dirs.size());
        std::vector<int32_t> d(n);
        voxel_out.resize(n);
        t_out.resize(n);
        if (width)
            check(och_gpu_trace_batch_image(pool_, &origin.x, 0, &dirs[0].x, n, width, d.data(), voxel_out.data(),
                                            t_out.data()),
                  "och_gpu_trace_batch_image");
        else
            check(och_gpu_trace_batch(pool_, &origin.x, 0, &dirs[0].x, n, d.data(), voxel_out.data(), t_out.data()),
                  "och_gpu_trace_batch");
        dir_out.resize(n);
        for (uint32_t i = 0; i < n; ++i) dir_out[i] = static_cast<direction>(d[i]);
    }

    void set_palette(const std::vector<uint32_t> &rgba)
    {
        check(och_gpu_set_palette(pool_, rgba.data(), static_cast<uint32_t>(rgba.size() / 6)), "och_gpu_set_palette");
    }

    // update_position + update_image into an olc::Sprite-compatible RGBA8 buffer
    // (memcpy it into GetDrawTarget()->GetData(), olcPixelGameEngine.h:945).
    void render(const och_camera &cam, uint32_t *rgba) const { check(och_gpu_render(pool_, &cam, rgba), "och_gpu_render"); }

    // The same frame supersampled: cam is the camera of the sample grid (width
    // and height multiples of s = 2, 4 or 8), rgba takes (width / s) x
    // (height / s) pixels, each the rounded mean of its s x s samples
    // (och_gpu_render_ssaa).
    void render_ssaa(const och_camera &cam, int s, std::vector<uint32_t> &rgba) const
    {
        rgba.resize(static_cast<size_t>(cam.width / (s > 0 ? s : 1)) * static_cast<size_t>(cam.height / (s > 0 ? s : 1)));
        check(och_gpu_render_ssaa(pool_, &cam, s, rgba.data(), rgba.size()), "och_gpu_render_ssaa");
    }
    void render_ssaa(const och_camera &cam, int s, uint32_t *rgba, size_t capacity_pixels) const
    {
        check(och_gpu_render_ssaa(pool_, &cam, s, rgba, capacity_pixels), "och_gpu_render_ssaa");
    }

    // The same frame with every face hit shaded by sun shadow and ambient
    // occlusion, primary and secondary rays in one launch (och_gpu_render_lit;
    // och_gpu.h has the definition of every bit).
    void render_lit(const och_camera &cam, const och_light &light, std::vector<uint32_t> &rgba) const
    {
        rgba.resize(static_cast<size_t>(cam.width > 0 ? cam.width : 0) * static_cast<size_t>(cam.height > 0 ? cam.height : 0));
        check(och_gpu_render_lit(pool_, &cam, &light, rgba.data(), rgba.size()), "och_gpu_render_lit");
    }
    void render_lit(const och_camera &cam, const och_light &light, uint32_t *rgba, size_t capacity_pixels) const
    {
        check(och_gpu_render_lit(pool_, &cam, &light, rgba, capacity_pixels), "och_gpu_render_lit");
    }

    // The lit frame supersampled: cam is the camera of the sample grid, as for
    // render_ssaa; every sample is render_lit's colour, shaded before the mean,
    // all in one launch (och_gpu_render_lit_ssaa).
    void render_lit_ssaa(const och_camera &cam, const och_light &light, int s, std::vector<uint32_t> &rgba) const
    {
        rgba.resize(static_cast<size_t>(cam.width / (s > 0 ? s : 1)) * static_cast<size_t>(cam.height / (s > 0 ? s : 1)));
        check(och_gpu_render_lit_ssaa(pool_, &cam, &light, s, rgba.data(), rgba.size()), "och_gpu_render_lit_ssaa");
    }
    void render_lit_ssaa(const och_camera &cam, const och_light &light, int s, uint32_t *rgba, size_t capacity_pixels) const
    {
        check(och_gpu_render_lit_ssaa(pool_, &cam, &light, s, rgba, capacity_pixels), "och_gpu_render_lit_ssaa");
    }

    // Lit codes, the lit frame's exchange format between GPUs (device buffers,
    // asynchronous on the pool's stream): this shard's slices as one uint16 per
    // pixel, code | mask << 8 (och_gpu_render_lit_codes_views_dev) ...
    void render_lit_codes(const std::vector<och_camera> &cams, const och_light &light, uint16_t *code_slices,
                          size_t capacity_pixels, int row_chunk, int shard = 0, int n_shards = 1) const
    {
        check(och_gpu_render_lit_codes_views_dev(pool_, cams.data(), static_cast<int>(cams.size()), &light, code_slices,
                                                 capacity_pixels, row_chunk, shard, n_shards),
              "och_gpu_render_lit_codes_views_dev");
    }
    // ... and every shard's gathered slices shaded into [views][H][W] RGBA8
    // frames, the words render_lit writes (och_gpu_shade_lit_unshard_views_dev).
    void shade_lit_unshard(const uint16_t *gathered, uint32_t *frames, int width, int height, int row_chunk,
                           int n_shards, int n_views, const och_light &light) const
    {
        check(och_gpu_shade_lit_unshard_views_dev(pool_, gathered, frames, width, height, row_chunk, n_shards, n_views,
                                                  &light),
              "och_gpu_shade_lit_unshard_views_dev");
    }

    och_gpu_pool *handle() const { return pool_; }

private:
    och_gpu_pool *pool_ = nullptr;
};

// h_octree::set / at (ORT/och_h_octree.h:176-258) with a device mirror that is
// refreshed by uploading only the slots the edits wrote.
class editor {
public:
    editor(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, uint32_t capacity)
        : depth_(depth)
    {
        check(och_editor_create(nodes, n_nodes, root, depth, capacity, &ed_), "och_editor_create");
    }
    editor(const editor &) = delete;
    editor &operator=(const editor &) = delete;
    ~editor() { och_editor_destroy(ed_); }

    void set(int x, int y, int z, uint32_t v) { check(och_editor_set(ed_, x, y, z, v), "och_editor_set"); }
    uint32_t at(int x, int y, int z) const { return och_editor_at(ed_, x, y, z); }
    uint32_t get_root() const
    {
        och_editor_stats st;
        och_editor_info(ed_, &st);
        return st.root;
    }

    // The device pool that mirrors this editor; refresh it with flush().
    tree make_tree(int device = -1) const
    {
        const uint32_t *words = nullptr;
        uint32_t slots = 0, root = 0;
        check(och_editor_nodes(ed_, &words, &slots, &root), "och_editor_nodes");
        return tree(words, slots, root, depth_, 1, __builtin_inff(), device);
    }
    void flush(tree &t) { check(och_editor_flush(ed_, t.handle()), "och_editor_flush"); }

    och_editor *handle() const { return ed_; }

private:
    och_editor *ed_ = nullptr;
    int depth_;
};

// A pool built into host memory (och_build_voxels); owns its nodes.
class host_pool {
public:
    host_pool() = default;
    host_pool(host_pool &&o) noexcept : pool_(o.pool_) { o.pool_ = och_host_pool{}; }
    host_pool &operator=(host_pool &&o) noexcept
    {
        std::swap(pool_, o.pool_);
        return *this;
    }
    host_pool(const host_pool &) = delete;
    host_pool &operator=(const host_pool &) = delete;
    ~host_pool() { och_host_pool_free(&pool_); }

    const och_host_pool &get() const { return pool_; }
    och_host_pool *out() { return &pool_; }

private:
    och_host_pool pool_{};
};

// A DAG from the caller's voxels: a list of (x, y, z, id) records that act as
// successive h_octree::set calls, or a dense grid (och_voxel_params).
inline host_pool build_voxels(const och_voxel_params &params)
{
    host_pool p;
    check(och_build_voxels(&params, p.out()), "och_build_voxels");
    return p;
}

// A batch of set() records applied to an existing 1-based pool (och_edit_params):
// the canonical pool of its voxels after the records, as build_voxels returns it.
inline host_pool edit_voxels(const och_edit_params &params)
{
    host_pool p;
    check(och_edit_voxels(&params, p.out()), "och_edit_voxels");
    return p;
}

// A box of a host pool's voxels as a dense grid, x fastest, then y, then z
// (och_pool_read_box): the grid och_voxel_params takes back.
inline void read_box(const och_host_pool &pool, const int32_t lo[3], const int32_t hi[3], int kind, void *grid,
                     size_t capacity_bytes)
{
    check(och_pool_read_box(pool.nodes, pool.n_nodes, pool.root, pool.depth, pool.index_base, lo, hi, kind, grid,
                            capacity_bytes),
          "och_pool_read_box");
}

// The voxels that differ between two host pools of one depth and index_base
// (och_pool_diff): records of (x, y, z, id under b) in ascending Morton order;
// records = nullptr gives the stats alone.
inline och_diff_stats pool_diff(const och_host_pool &a, const och_host_pool &b, void *records = nullptr, uint64_t capacity = 0)
{
    och_diff_stats st;
    check(och_pool_diff(a.nodes, a.n_nodes, a.root, b.nodes, b.n_nodes, b.root, a.depth, a.index_base, records, capacity, &st),
          "och_pool_diff");
    return st;
}

// The maximal aligned cubes of the box lo <= (x, y, z) < hi clipped to a tree of
// `depth` (och_box_cubes, host only): their Morton keys and heights in
// ascending height and key, with the per-height counts of the cubes and of the
// cells that straddle the box (22 entries each).
struct box_cube_list {
    std::vector<uint64_t> keys;
    std::vector<uint8_t> heights;
    uint64_t cubes_per_height[22], cells_per_height[22];
};
inline box_cube_list box_cubes(const int32_t lo[3], const int32_t hi[3], int depth)
{
    box_cube_list out;
    uint64_t n = 0;
    check(och_box_cubes(lo, hi, depth, nullptr, nullptr, 0, out.cubes_per_height, out.cells_per_height, &n), "och_box_cubes");
    out.keys.resize(n);
    out.heights.resize(n);
    if (n)
        check(och_box_cubes(lo, hi, depth, out.keys.data(), out.heights.data(), n, out.cubes_per_height, out.cells_per_height, &n),
              "och_box_cubes");
    return out;
}

// The same of a ball (och_sphere_cubes, host only): centre2 is twice the
// centre in voxels, diameter counts voxels.  The counts come from the walk
// itself, whose cost follows the ball's surface.
inline box_cube_list sphere_cubes(const int32_t centre2[3], uint32_t diameter, int depth)
{
    box_cube_list out;
    uint64_t n = 0;
    check(och_sphere_cubes(centre2, diameter, depth, nullptr, nullptr, 0, out.cubes_per_height, out.cells_per_height, &n),
          "och_sphere_cubes");
    out.keys.resize(n);
    out.heights.resize(n);
    if (n)
        check(och_sphere_cubes(centre2, diameter, depth, out.keys.data(), out.heights.data(), n, out.cubes_per_height,
                               out.cells_per_height, &n),
              "och_sphere_cubes");
    return out;
}

// A world that stays on one GPU between brush strokes (och_world_*): edit()
// applies a record list as edit_voxels would, flush() publishes the stroke's
// new nodes to a tree made by make_pool(), download() gives the canonical pool;
// at() and read_box() ask it what it holds, tighten() makes its box exact;
// snapshot(), checkout() and release() keep earlier states, diff() compares two;
// paint_box() and paint_sphere() are the strokes conditional on the old voxel.
class world {
public:
    world(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, uint32_t capacity = 0, int device = -1)
    {
        check(och_world_create(nodes, n_nodes, root, depth, capacity, device, &w_), "och_world_create");
    }
    world(const world &) = delete;
    world &operator=(const world &) = delete;
    ~world() { och_world_destroy(w_); }

    // One stroke: n records of (x, y, z, id); OCH_E_CAPACITY leaves the world as it was (compact() and retry).
    void edit(const uint32_t *records, uint64_t n, bool on_device = false)
    {
        check(och_world_edit(w_, records, n, on_device ? 1 : 0), "och_world_edit");
    }
    tree make_pool()
    {
        och_gpu_pool *p = nullptr;
        check(och_world_pool_create(w_, &p), "och_world_pool_create");
        return tree(p);
    }
    void flush(tree &t) { check(och_world_flush(w_, t.handle()), "och_world_flush"); }
    host_pool download()
    {
        host_pool p;
        check(och_world_download(w_, p.out()), "och_world_download");
        return p;
    }
    void compact() { check(och_world_compact(w_), "och_world_compact"); }
    // The voxels at n coordinates of (x, y, z) under the current root, 0 outside the tree; complete on return.
    void at(const int32_t *coords, uint64_t n, uint32_t *ids, bool on_device = false)
    {
        check(och_world_at(w_, coords, n, ids, on_device ? 1 : 0), "och_world_at");
    }
    // The box [lo, hi) as a grid, x fastest (och_pool_read_box's bytes); kind is OCH_VOXELS_GRID_U8 or _U32.
    void read_box(const int32_t lo[3], const int32_t hi[3], int kind, void *grid, size_t capacity_bytes, bool on_device = false)
    {
        check(och_world_read_box(w_, lo, hi, kind, grid, capacity_bytes, on_device ? 1 : 0), "och_world_read_box");
    }
    // The box made exact; the stats carry it (box_lo, box_hi; hi exclusive).
    och_world_stats tighten()
    {
        check(och_world_tighten(w_), "och_world_tighten");
        return info();
    }
    och_world_stats info() const
    {
        och_world_stats st;
        check(och_world_info(w_, &st), "och_world_info");
        return st;
    }
    // Remember the current root: a handle for checkout() and diff(), live until release().
    uint64_t snapshot()
    {
        uint64_t s = 0;
        check(och_world_snapshot(w_, &s), "och_world_snapshot");
        return s;
    }
    // Make a snapshot the current state again (undo / redo): O(1), nothing is launched.
    void checkout(uint64_t s) { check(och_world_checkout(w_, s), "och_world_checkout"); }
    void release(uint64_t s) { check(och_world_release(w_, s), "och_world_release"); }
    // What differs between two snapshots (OCH_WORLD_CURRENT: the current state): records of (x, y, z, id
    // under to) in ascending Morton order, what edit() takes; records = nullptr gives the stats alone.
    och_diff_stats diff(uint64_t from, uint64_t to = OCH_WORLD_CURRENT, void *records = nullptr, uint64_t capacity = 0,
                        bool on_device = false)
    {
        och_diff_stats st;
        check(och_world_diff(w_, from, to, records, capacity, on_device ? 1 : 0, &st), "och_world_diff");
        return st;
    }
    // Every voxel of the box [lo, hi) becomes id (0 removes), as edit() of the box's records would leave
    // the world, at a cost that follows the box's surface; OCH_E_CAPACITY leaves the world as it was.
    och_region_stats fill_box(const int32_t lo[3], const int32_t hi[3], uint32_t id)
    {
        och_region_stats st;
        check(och_world_fill_box(w_, lo, hi, id, &st), "och_world_fill_box");
        return st;
    }
    // Inside the box the content of the snapshot, outside it the current content: undo for a region.
    och_region_stats restore_box(uint64_t snapshot, const int32_t lo[3], const int32_t hi[3])
    {
        och_region_stats st;
        check(och_world_restore_box(w_, snapshot, lo, hi, &st), "och_world_restore_box");
        return st;
    }
    // The same two strokes for a ball: centre2 is twice the centre in voxels, diameter counts voxels.
    och_region_stats fill_sphere(const int32_t centre2[3], uint32_t diameter, uint32_t id)
    {
        och_region_stats st;
        check(och_world_fill_sphere(w_, centre2, diameter, id, &st), "och_world_fill_sphere");
        return st;
    }
    och_region_stats restore_sphere(uint64_t snapshot, const int32_t centre2[3], uint32_t diameter)
    {
        och_region_stats st;
        check(och_world_restore_sphere(w_, snapshot, centre2, diameter, &st), "och_world_restore_sphere");
        return st;
    }

    // Inside the box a voxel v becomes id where the predicate holds (when::is: v == match, when::is_not:
    // v != match) and stays otherwise: paint is (is_not, 0), fill-under (is, 0), replace (is, m).
    och_paint_stats paint_box(const int32_t lo[3], const int32_t hi[3], uint32_t id, gpu::when w = gpu::when::is_not, uint32_t match = 0)
    {
        och_paint_stats st;
        check(och_world_paint_box(w_, lo, hi, static_cast<int>(w), match, id, &st), "och_world_paint_box");
        return st;
    }
    och_paint_stats paint_sphere(const int32_t centre2[3], uint32_t diameter, uint32_t id, gpu::when w = gpu::when::is_not,
                                 uint32_t match = 0)
    {
        och_paint_stats st;
        check(och_world_paint_sphere(w_, centre2, diameter, static_cast<int>(w), match, id, &st), "och_world_paint_sphere");
        return st;
    }

    och_world *handle() const { return w_; }

private:
    och_world *w_ = nullptr;
};

// Every GPU of the node from one host thread: a pool replica
// per device, row chunks dealt round-robin, one RCCL all-gather, shading on
// every device.  frames(rank) is device rank's [views][H][W] RGBA8 copy.
class frame_group {
public:
    frame_group(const std::vector<int> &devices, const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth,
                int index_base = 1, float miss_t = __builtin_inff())
    {
        check(och_frame_group_create(devices.data(), static_cast<int>(devices.size()), nodes, n_nodes, root, depth,
                                     index_base, miss_t, &g_),
              "och_frame_group_create");
    }
    frame_group(const frame_group &) = delete;
    frame_group &operator=(const frame_group &) = delete;
    ~frame_group() { och_frame_group_destroy(g_); }

    int size() const
    {
        int n = 0;
        check(och_frame_group_size(g_, &n), "och_frame_group_size");
        return n;
    }
    void set_palette(const std::vector<uint32_t> &rgba)
    {
        check(och_frame_group_set_palette(g_, rgba.data(), static_cast<uint32_t>(rgba.size() / 6)),
              "och_frame_group_set_palette");
    }
    void set_option(och_option option, int value)
    {
        check(och_frame_group_set_option(g_, option, value), "och_frame_group_set_option");
    }
    // Cost-planned launch order for frames of these cameras' geometry.
    void plan(const std::vector<och_camera> &cams, int row_chunk = 8)
    {
        check(och_frame_group_plan(g_, cams.data(), static_cast<int>(cams.size()), row_chunk), "och_frame_group_plan");
    }
    // One frame of every view, asynchronous on all devices.
    void render(const std::vector<och_camera> &cams, int row_chunk = 8, bool bounce = false)
    {
        check(och_frame_group_render(g_, cams.data(), static_cast<int>(cams.size()), row_chunk, bounce ? 1 : 0),
              "och_frame_group_render");
    }
    // n_steps frames, up to n_buffers in flight, each device's issued by its own
    // thread; frames() / download() then give the last one.
    void render_steps(const std::vector<och_camera> &cams, int n_steps, int n_buffers = 3, int row_chunk = 8,
                      bool bounce = false)
    {
        check(och_frame_group_render_steps(g_, cams.data(), static_cast<int>(cams.size()), n_steps, n_buffers,
                                           row_chunk, bounce ? 1 : 0),
              "och_frame_group_render_steps");
    }
    // The two render calls with a light: lit frames (tree::render_lit's words),
    // exchanged as 2-byte lit codes when the palette fits the codes.
    void render_lit(const std::vector<och_camera> &cams, const och_light &light, int row_chunk = 8)
    {
        check(och_frame_group_render_lit(g_, cams.data(), static_cast<int>(cams.size()), row_chunk, &light),
              "och_frame_group_render_lit");
    }
    void render_lit_steps(const std::vector<och_camera> &cams, const och_light &light, int n_steps, int n_buffers = 3,
                          int row_chunk = 8)
    {
        check(och_frame_group_render_lit_steps(g_, cams.data(), static_cast<int>(cams.size()), n_steps, n_buffers,
                                               row_chunk, &light),
              "och_frame_group_render_lit_steps");
    }
    uint32_t *frames(int rank) const
    {
        uint32_t *p = nullptr;
        check(och_frame_group_frames_dev(g_, rank, &p), "och_frame_group_frames_dev");
        return p;
    }
    void download(int rank, uint32_t *rgba) const { check(och_frame_group_download(g_, rank, rgba), "och_frame_group_download"); }
    void synchronize() const { check(och_frame_group_synchronize(g_), "och_frame_group_synchronize"); }

private:
    och_frame_group *g_ = nullptr;
};

// The library's RCCL communicator for one process per GPU: rank 0 makes the
// id (unique_id()), the launcher hands it to every rank (MPI_Bcast, a file,
// torch.distributed), every rank constructs comm(id, n_ranks, rank, device).
class comm {
public:
    using id_t = std::array<uint8_t, OCH_COMM_ID_BYTES>;
    static id_t unique_id()
    {
        id_t id{};
        check(och_comm_unique_id(id.data()), "och_comm_unique_id");
        return id;
    }
    comm(const id_t &id, int n_ranks, int rank, int device)
    {
        check(och_comm_create(id.data(), n_ranks, rank, device, &c_), "och_comm_create");
    }
    comm(const comm &) = delete;
    comm &operator=(const comm &) = delete;
    ~comm() { och_comm_destroy(c_); }
    och_comm *handle() const { return c_; }

private:
    och_comm *c_ = nullptr;
};

// tree_camera's per-frame state (pos :55, dir :53, fov :95).
struct camera {
    float3 pos{1.5F, 1.5F, 1.5F};
    float yaw = 0.0F, pitch = 0.0F, fov = 1.25F;
    int width = 640, height = 360;

    och_camera update_position() const
    {
        och_camera c;
        check(och_camera_setup(pos.x, pos.y, pos.z, yaw, pitch, fov, width, height, &c), "och_camera_setup");
        return c;
    }
};

}  // namespace gpu
}  // namespace och
