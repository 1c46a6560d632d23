/*
 * och_gpu.h -- C ABI of the MI355X (gfx950) sparse-voxel-octree ray caster.
 *
 * Drop-in boundary for the reference's hot path (ORT/ = Octree_Ray_Tracing/):
 *
 *   void h_octree<L,D>::sse_trace(float ox, float oy, float oz,
 *                                 float dx, float dy, float dz,
 *                                 och::direction& hit_direction,
 *                                 uint32_t& hit_voxel, float& hit_time) const;
 *                                                   ORT/och_h_octree.h:292, :449
 *   void octree::sse_trace(...)                     ORT/och_octree.h:56-58, ORT/och_octree.cpp:167
 *   tree_camera::update_position()  (ray generator) ORT/test_och_h_octree.cpp:87-138
 *   tree_window::update_image() + trace_pixel()     ORT/test_och_h_octree.cpp:437-457, :64-85
 *
 * Every entry point returns an och_status (0 = OK).  Host buffers belong to
 * the caller; device memory belongs to the pool.  Functions suffixed _dev take
 * device pointers and enqueue on the pool's HIP stream without synchronising.
 * Results are bit-identical to the reference CPU tracer run with the same
 * RCPPS table (och_gpu_set_rcp_lut / och_host_rcp_lut).
 */
#ifndef OCH_GPU_H
#define OCH_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCH_GPU_ABI_VERSION 1
#define OCH_MAX_VIEWS 8

#if defined(__GNUC__)
#define OCH_API __attribute__((visibility("default")))
#else
#define OCH_API
#endif

typedef enum och_status {
    OCH_OK = 0,
    OCH_E_INVALID = -1,     /* bad argument / precondition */
    OCH_E_HIP = -2,         /* HIP runtime error (see och_last_error) */
    OCH_E_NODEV = -3,       /* no gfx950 device visible */
    OCH_E_RCP_MODEL = -4,   /* host RCPPS is not representable as a mantissa table */
    OCH_E_NOMEM = -5,
    OCH_E_CAPACITY = -6     /* builder: node table full (reference: exit(0), ORT/och_h_octree.h:112-116) */
} och_status;

/* och::direction, ORT/och_tree_helper.h:7-18: the ray-travel sign on the
 * axis whose face was crossed last; exit = miss, inside = origin in a voxel. */
typedef enum och_direction {
    OCH_X_POS = 0, OCH_Y_POS = 1, OCH_Z_POS = 2,
    OCH_X_NEG = 3, OCH_Y_NEG = 4, OCH_Z_NEG = 5,
    OCH_EXIT = 6, OCH_INSIDE = 7, OCH_ERROR = 8
} och_direction;

/* Indexed-colour frame codes (1 byte per pixel, the multi-GPU exchange format
 * of och_gpu_render_codes_views_dev): 6 * (voxel - 1) + direction for a hit
 * face with a palette entry, the three fixed colours of trace_pixel
 * (ORT/test_och_h_octree.cpp:76-84, magenta for an id without a palette
 * entry), | OCH_CODE_BLOCKED when a config-5 secondary ray was blocked.
 * Needs a palette of at most OCH_CODE_MAX_VOXELS voxel ids. */
#define OCH_CODE_MAGENTA 125
#define OCH_CODE_INSIDE 126
#define OCH_CODE_SKY 127
#define OCH_CODE_BLOCKED 128
#define OCH_CODE_MAX_VOXELS 20

typedef struct och_gpu_pool och_gpu_pool;

/* Camera uniforms of tree_camera::update_position (ORT/test_och_h_octree.cpp:87-115),
 * computed ONCE per frame on the host (sinf/cosf/tanf of this host's libm)
 * by och_camera_setup; the per-pixel part runs on the GPU. */
typedef struct och_camera {
    float pos[3];        /* ray origin, tree occupies [1,2)^3 (ORT/test_och_h_octree.cpp:55) */
    float rot[9];        /* t_x_fx, t_x_fy, t_x_fz, t_y_fx, ..., t_z_fz (:107-115) */
    float fov_factor;    /* 1 / tanf(fov / 2) (:97) */
    float aspect;        /* (float)W / (float)H (:89) */
    float view_x;        /* 2.0F / (float)W (:91) */
    float view_y;        /* 2.0F / (float)H (:93) */
    int32_t width, height;
} och_camera;

typedef struct och_pool_info {
    uint64_t device_bytes;   /* node pool bytes resident in HBM */
    uint32_t n_nodes;        /* nodes uploaded (incl. the padding slot of 1-based pools) */
    uint32_t root;
    int32_t depth;
    int32_t index_base;
    float miss_t;
    int32_t rcp_log2_entries;
    int32_t device;
} och_pool_info;

/* ------------------------------------------------------------ runtime */
OCH_API int och_abi_version(void);
OCH_API const char *och_last_error(void);      /* thread-local message of the last failure */
/* Every kernel launch first clears its thread's pending HIP error: one left by
 * an earlier HIP call of the thread (another library's, e.g. RCCL's
 * communicator init) would otherwise be reported as the launch's own.  The
 * error is kept, not dropped: the first one cleared since the last reset, in
 * any thread -- its hipError_t in *hip_error (0 = none), the number cleared in
 * *count, and into what (what_cap bytes, may be NULL) its name and the C-ABI
 * entry and launcher that found it.  reset != 0 clears the record after
 * reading.  Any argument may be NULL. */
OCH_API int och_discarded_error(int *hip_error, int *count, char *what, size_t what_cap, int reset);
OCH_API int och_device_count(int *count);       /* visible gfx950 devices */
/* HIP indices of the visible gfx950 devices, in HIP order: up to capacity of
 * them into devices[], their total into *count. */
OCH_API int och_device_list(int *devices, int capacity, int *count);

/* ------------------------------------------------------------ RCPPS model */
/* Capture this host CPU's _mm_rcp_ps (the reference's reciprocal,
 * ORT/och_h_octree.h:316) as a 2^k table over the mantissa of inputs in [-2,-1),
 * after checking that the result depends only on the top k mantissa bits and
 * that other exponents shift the result exponent.  lut must hold 1<<23 entries
 * (worst case); *log2_entries receives k.  Returns OCH_E_RCP_MODEL if the host
 * instruction does not follow the model (then pass an explicit table). */
OCH_API int och_host_rcp_lut(uint32_t *lut, int *log2_entries);
/* Same model evaluated on the host, for a single input bit pattern. */
OCH_API uint32_t och_rcp_from_lut(uint32_t xbits, const uint32_t *lut, int log2_entries);
/* Largest relative error |r * x - 1| of a table over x in [-2, -1).  A pool
 * whose table exceeds 2^-10 (x86 RCPPS: within 1.5 * 2^-12) does not use the
 * cull's approximate camera test, only its exact per-ray test (OCH_OPT_CULL),
 * so records stay the reference's under any table. */
OCH_API int och_rcp_lut_error(const uint32_t *lut, int log2_entries, double *max_rel_error);

/* ------------------------------------------------------------ node pools */
/* Upload a node pool.  nodes = n_nodes x 8 uint32 child slots exactly as the
 * reference lays them out (ORT/och_h_octree.h:38-40): interior slots hold node
 * indices, the leaf level holds voxel ids, 0 = empty.
 *   index_base 1: h_octree -- indices are 1-based into nodes[] (the
 *                 reference's table->nodes with root_idx, ORT/och_h_octree.h:93-95);
 *   index_base 0: octree   -- 0-based, root = 0 (ORT/och_octree.cpp:207).
 * miss_t: hit_time reported for a miss (+INF for h_octree, :429; 0.0F for
 * octree, ORT/och_octree.cpp:302).  depth = number of levels (1..22).
 * The pool starts with this host's RCPPS table (och_host_rcp_lut); override
 * with och_gpu_set_rcp_lut.  device < 0 selects the current HIP device. */
OCH_API int och_gpu_pool_create(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth,
                                int index_base, float miss_t, int device, och_gpu_pool **out);
OCH_API int och_gpu_pool_destroy(och_gpu_pool *pool);
OCH_API int och_gpu_pool_info(const och_gpu_pool *pool, och_pool_info *info);
/* Re-upload nodes [first, first+count) (pool numbering) and set a new root --
 * mirrors h_octree::set's path copy (ORT/och_h_octree.h:176-237) after an edit. */
OCH_API int och_gpu_pool_update(och_gpu_pool *pool, uint32_t first, uint32_t count,
                                const uint32_t *nodes, uint32_t root);
OCH_API int och_gpu_set_rcp_lut(och_gpu_pool *pool, const uint32_t *lut, int log2_entries);
/* Palette: n_voxels x 6 RGBA8 colours (olc::Pixel layout, r in the low byte),
 * ordered x_pos..z_neg per voxel id 1..n (ORT/och_voxel.cpp:195-305). */
OCH_API int och_gpu_set_palette(och_gpu_pool *pool, const uint32_t *rgba, uint32_t n_voxels);
/* Enqueue all later work on a caller-owned HIP stream (hipStream_t); NULL is
 * HIP's null stream (torch's default stream).  Until called, the pool uses a
 * non-blocking stream of its own. */
OCH_API int och_gpu_set_stream(och_gpu_pool *pool, void *hip_stream);
OCH_API int och_gpu_synchronize(och_gpu_pool *pool);
/* Launch options of trace/render kernels.  Every launch is a grid of one ray
 * per thread.  Ids 0, 2, 3, 7, 9, 12 and 13 belonged to arms measured slower
 * on every scene and retired in round 5 (persistent and refill schedules,
 * in-block wave merging, the per-node voxel-box skip, the column cull;
 * DESIGN.md section 8): setting or reading them fails with OCH_E_INVALID. */
typedef enum och_option {
    OCH_OPT_BLOCK = 1,         /* threads per workgroup: 64..1024, multiple of 64 (default 64) */
    OCH_OPT_LAYOUT = 4,        /* 0 = the caller's node layout; 1 = packed (default when the DAG has < 2^24
                                  (node, level) pairs): per-level breadth-first ids, interior slots carry the
                                  child's occupancy mask so only descents and hits touch memory */
    OCH_OPT_TILE_ORDER = 5,    /* camera rays (render): 0 = 8x8-pixel tiles row-major; 1 = 64x64-pixel supertiles,
                                  each handed to one XCD so neighbouring rays share that XCD's L2; 2 = the launch
                                  order planned by och_gpu_plan_views (costliest tiles first) for frames of the
                                  planned geometry, else 0; 3 = that plan grouped per XCD.  Dispatch order only:
                                  frames are identical */
    OCH_OPT_BOUNCE_COMPACT = 6,/* config 5: 1 (default) = compact each block's secondary rays into its first lanes
                                  (wave ballot/popcount + LDS queue) before tracing them; 0 = trace each in place;
                                  2 = per block, compact when that packs the block's secondary rays into fewer
                                  waves than hold them, else in place.  Lit frames (och_gpu_render_lit_views_dev, _lit_ssaa_views_dev):
                                  0 = every hit lane walks its own pixel's secondary rays, 1 or 2 = the block's
                                  hit pixels are compacted and their rays dealt over its lanes; same bytes */
    OCH_OPT_CULL = 8,          /* 1 (default) = a ray whose walk provably never enters the bounding box of the
                                  pool's voxels (och_pool_occupied_box) is recorded as the miss it would end in,
                                  without walking (camera rays: a cheaper conservative test first, before the
                                  ray's setup); exact, for launches that do not count
                                  PUSHes.  0 = every ray walks.  2 = diagnostic: launches that count PUSHes
                                  cull too, a culled ray counting 0 (the PUSHes the culled launch walks) */
    OCH_OPT_TIMING = 10,       /* per-launch timing of trace/render kernels (och_gpu_last_kernel_ms):
                                  1 (default) = recorded by the kernel's own dispatch (hipExtLaunchKernel: no
                                  packets between two launches of a stream); 2 = hipEventRecord before and
                                  after the launch; 0 = not timed */
    OCH_OPT_PLAN = 11,         /* shape of och_gpu_plan_views' launch order (set before planning): 0 =
                                  costliest first; P in 1..99 = the costliest P % first, the rest in natural
                                  order (default 10); 100 = costliest and cheapest alternating */
    OCH_OPT_SPLIT = 14,        /* heavy-tile split (set before och_gpu_plan_views; renders with OCH_OPT_TILE_ORDER
                                  2, block 64, packed layout): the planned tiles whose cost reaches this % of the
                                  costliest one's walk each ray over OCH_OPT_SPLIT_SEGS lanes, a lane entering
                                  only every S-th present cell of level OCH_OPT_SPLIT_LEVEL along the ray, the
                                  lowest one's hit kept -- the same records, a lone
                                  frame no longer waiting on its few longest rays.  0 = off */
    OCH_OPT_SPLIT_SEGS = 15,   /* lanes per ray of a split tile: 2, 4 (default), 8 or 16 */
    OCH_OPT_SPLIT_LEVEL = 16,  /* the level whose cells are the split's segments (default 6) */
    OCH_OPT_SPLIT_TILES = 17   /* read only: tiles split by the current plan */
} och_option;
OCH_API int och_gpu_set_option(och_gpu_pool *pool, int option, int value);
OCH_API int och_gpu_get_option(const och_gpu_pool *pool, int option, int *value);
/* Diagnostics: later trace/render launches write one record per wave into a
 * device buffer of capacity_waves x 4 uint64: {start, end} (s_memrealtime,
 * 100 MHz), HW_ID | XCC_ID << 32, rays finished.  NULL turns it off. */
OCH_API int och_gpu_set_stamp_buffer(och_gpu_pool *pool, uint64_t *stamps, uint32_t capacity_waves);
/* Diagnostics: HIP's occupancy answer (workgroups per CU) for kind 0 = render
 * grid kernel or 2 = trace grid kernel, at the pool's block size and stack
 * depth (kind 1, the retired persistent kernel, fails). */
OCH_API int och_gpu_occupancy(const och_gpu_pool *pool, int kind, int *blocks_per_cu);
/* Duration of the most recent trace/render kernel launched on the pool,
 * measured with HIP events on the stream it ran on (blocks until it ends).
 * OCH_E_INVALID if that launch was not timed (OCH_OPT_TIMING 0, n = 0, or it
 * recorded the caller's events). */
OCH_API int och_gpu_last_kernel_ms(och_gpu_pool *pool, float *ms);
/* The next trace/render launch on the pool records these HIP events
 * (hipEvent_t, created by the caller; either may be NULL) at its kernel's
 * start and end, through the dispatch itself, instead of the pool's own.
 * One launch only; a call that launches nothing (n = 0) leaves them
 * unrecorded.  For frame timers: no event packets between the launches of a
 * stream. */
OCH_API int och_gpu_set_launch_events(och_gpu_pool *pool, void *start_event, void *stop_event);

/* ------------------------------------------------------------ tracing */
/* Reference signature: one ray, synchronous (the pick ray of
 * ORT/test_och_h_octree.cpp:536).  Requires origin in (1,2)^3. */
OCH_API int och_gpu_trace(och_gpu_pool *pool, float ox, float oy, float oz, float dx, float dy, float dz,
                          int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time);
/* Batch of n rays, host buffers, synchronous.  origin_stride 0 = one shared
 * origin (3 floats), 3 = one origin per ray.  dirs: n x 3 floats (och::float3
 * AoS, ORT/test_och_h_octree.cpp:49).  Outputs: n each. */
OCH_API int och_gpu_trace_batch(och_gpu_pool *pool, const float *origin, int origin_stride,
                                const float *dirs, uint32_t n,
                                int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time);
/* Same with device buffers, asynchronous on the pool stream.  push_count
 * (optional, may be NULL) receives the PUSH iterations (child fetches) per ray. */
OCH_API int och_gpu_trace_batch_dev(och_gpu_pool *pool, const float *origin, int origin_stride,
                                    const float *dirs, uint32_t n,
                                    int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time,
                                    uint32_t *push_count);

/* och_gpu_trace_batch_dev for rays laid out as a row-major image `width`
 * rays wide (a camera's rays as update_position stores them, x + y * W,
 * ORT/test_och_h_octree.cpp:135): each wavefront walks an 8x8 tile of
 * neighbouring rays instead of 64 consecutive rays of one row, so its lanes
 * share the DAG's top nodes and finish after similar walks.  n need not be a
 * multiple of width (the last row is partial).  Records in the caller's
 * order, bit-identical to och_gpu_trace_batch_dev.  With OCH_OPT_TILE_ORDER
 * >= 2, batches of the geometry planned by och_gpu_plan_batch_tiled dispatch
 * their costliest tiles first. */
OCH_API int och_gpu_trace_batch_tiled_dev(och_gpu_pool *pool, const float *origin, int origin_stride,
                                          const float *dirs, uint32_t n, uint32_t width,
                                          int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time,
                                          uint32_t *push_count);
/* och_gpu_trace_batch for a camera's rays in the reference's layout, a
 * row-major image `width` rays wide (x + y * W, ORT/test_och_h_octree.cpp:135):
 * host buffers, synchronous, traced as och_gpu_trace_batch_tiled_dev traces
 * them (8x8 tiles per wave; the plan of och_gpu_plan_batch_tiled when one
 * exists for this geometry).  Records in the caller's order, bit-identical to
 * och_gpu_trace_batch. */
OCH_API int och_gpu_trace_batch_image(och_gpu_pool *pool, const float *origin, int origin_stride,
                                      const float *dirs, uint32_t n, uint32_t width,
                                      int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time);
/* Plan the launch order of tiled batches of n rays `width` wide (block size
 * included in the key): one timed trace of these rays, then
 * costliest tiles first.  Synchronous; a plan stays valid while the rays
 * change (it orders dispatch only). */
OCH_API int och_gpu_plan_batch_tiled(och_gpu_pool *pool, const float *origin, int origin_stride,
                                     const float *dirs, uint32_t n, uint32_t width);

/* Config 5 (BASELINE configs[4]): each primary ray that hits a voxel face
 * spawns one secondary ray -- from o + d*t - offset, the point half a voxel in
 * front of the hit face (get_directional_hit_offset, ORT/test_och_h_octree.cpp:
 * 487-502, as the editor's placement point :385), along d mirrored on the hit
 * axis -- traced by the same traversal.  Build-defined: the reference renders
 * primary rays only.  Secondary records: direction -1, voxel 0, t 0 when the
 * primary ray did not hit (exit / inside).  push_count (optional) receives the
 * PUSH iterations of both rays.  Device buffers, asynchronous on the pool stream. */
OCH_API int och_gpu_trace_bounce_batch_dev(och_gpu_pool *pool, const float *origin, int origin_stride,
                                           const float *dirs, uint32_t n,
                                           int32_t *hit_direction, uint32_t *hit_voxel, float *hit_time,
                                           int32_t *bounce_direction, uint32_t *bounce_voxel, float *bounce_time,
                                           uint32_t *push_count);

/* ------------------------------------------------------------ camera / frame */
/* tree_camera::update_position's per-frame constants (ORT/test_och_h_octree.cpp:89-115):
 * yaw = camera.dir.x, pitch = camera.dir.y, fov = 1.25F in the reference. */
OCH_API int och_camera_setup(float px, float py, float pz, float yaw, float pitch, float fov,
                             int width, int height, och_camera *cam);
/* Per-pixel ray directions (row-major, x + y*W) into a device buffer of W*H*3 floats. */
OCH_API int och_gpu_raygen_dev(och_gpu_pool *pool, const och_camera *cam, float *dirs);
/* One frame of update_position + update_image (ORT/test_och_h_octree.cpp:437-457):
 * raygen, trace and shade fused, RGBA8 into a host W*H buffer. */
OCH_API int och_gpu_render(och_gpu_pool *pool, const och_camera *cam, uint32_t *rgba);
/* Sharded device render: rows are dealt in chunks of row_chunk rows round-robin
 * over n_shards; this call renders shard `shard` into `rgba_slice`, a compact
 * buffer of och_shard_rows(H, row_chunk, n_shards) x W pixels. n_shards = 1,
 * row_chunk = H renders the whole frame. */
OCH_API int och_gpu_render_dev(och_gpu_pool *pool, const och_camera *cam, uint32_t *rgba_slice,
                               int row_chunk, int shard, int n_shards);
OCH_API int och_shard_rows(int height, int row_chunk, int n_shards);
/* Several cameras of equal size in one launch (stereo / multi-view frames):
 * view v's slice goes to rgba_slices + v * och_shard_rows(H, row_chunk, n_shards) * W.
 * One launch keeps the GPU busy with other views while a view's slowest rays finish.
 *
 * Every camera render (this one, the bounce, codes, supersampled and lit forms,
 * och_gpu_plan_views) runs a table of 8-byte tile descriptors, one per wave,
 * which the pool makes on the first launch of a geometry (size, views, row
 * chunk, shard, block, launch order, row deal) and keeps for the next frames;
 * nothing in it depends on the cameras.  A descriptor holds columns, rows and
 * slice rows in 16 bits: frames of more than 65 535 columns, rows or slice
 * rows, or of 2^25 or more tiles, are refused with OCH_E_INVALID. */
OCH_API int och_gpu_render_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views, uint32_t *rgba_slices,
                                     int row_chunk, int shard, int n_shards);
/* Plan the launch order of frames of this geometry (size, views, sharding,
 * block, bounce compaction): one render of these cameras per kernel (primary
 * and config-5 bounce frames) times every workgroup, and later renders with
 * OCH_OPT_TILE_ORDER = 2 dispatch the costliest tiles first, so a frame does
 * not end on a few late grazing tiles.  Synchronous.  A plan made from one
 * camera stays valid (and approximately right) while the camera moves;
 * re-plan at will. */
OCH_API int och_gpu_plan_views(och_gpu_pool *pool, const och_camera *cams, int n_views, int row_chunk, int shard,
                               int n_shards);
/* Config 5 frame: och_gpu_render_views_dev with one bounce per hit; a hit
 * pixel keeps its face colour when its secondary ray escapes (exit) and is
 * halved (RGB >> 1, alpha kept) when the secondary ray is blocked. */
OCH_API int och_gpu_render_bounce_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                            uint32_t *rgba_slices, int row_chunk, int shard, int n_shards);
/* Supersampled frames, s x s samples per pixel (s = 2, 4 or 8), resolved in
 * the render kernel: cams are the cameras of the sample grid (equal width and
 * height, both multiples of s), and view v's frame of (width / s) x (height / s)
 * RGBA8 words goes to rgba + v * (width / s) * (height / s).  With F the frame
 * och_gpu_render_views_dev writes for the same cameras (one shard), each byte is
 *   out[Y][X].c = (sum over j, i < s of F[s Y + j][s X + i].c + s * s / 2) >> (2 log2 s):
 * the box mean of the stored 8-bit channels, rounded half up; no gamma, no
 * jitter, alpha 0xFF.  capacity_pixels is what rgba holds, in pixels; a smaller
 * buffer, another s, a size that is no multiple of s, views of unequal size
 * and a pool left torn by a failed flush are refused (OCH_E_INVALID) before
 * anything is written.  One shard, whole frames; launch options change the
 * dispatch only (OCH_OPT_TILE_ORDER 2 uses och_gpu_plan_views' plan for these
 * cameras with row_chunk = height, never its split form).
 * _views_dev: device buffer, asynchronous on the pool's stream;
 * och_gpu_render_ssaa: one camera into a host buffer, synchronous. */
OCH_API int och_gpu_render_ssaa_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views, int s,
                                          uint32_t *rgba, size_t capacity_pixels);
OCH_API int och_gpu_render_ssaa(och_gpu_pool *pool, const och_camera *cam, int s, uint32_t *rgba,
                                size_t capacity_pixels);
/* Lit frames: och_gpu_render_views_dev's frame with every face hit shaded by
 * sun shadow and ambient occlusion, primary and secondary rays in one launch.
 * Build-defined, like config 5: the reference renders primary rays only.
 *
 * A pixel is lit only when its primary record is a face hit (direction <
 * OCH_EXIT, an id without a palette entry included); sky and INSIDE pixels
 * are the plain render's.  All secondary rays start at config 5's secondary
 * origin p: per axis q = o + d * t (product rounded, then the sum), and on the
 * hit axis a = direction % 3, p = q -+ voxel_dim / 2 (- for direction < 3).
 *   Sun ray (OCH_LIGHT_SUN): from p along sun_dir, the direction towards the
 *     sun, as given (not normalised).  The face is turned towards the sun iff
 *     sun_dir[a] < 0 for direction < 3, sun_dir[a] > 0 otherwise (the record's
 *     direction is the ray's travel sign; the normal opposes it).  A face
 *     turned away is self-shadowed: no ray, shadowed.  Otherwise the pixel is
 *     shadowed iff the sun ray's record is not OCH_EXIT (INSIDE blocks).
 *   AO rays (OCH_LIGHT_AO), k = 0..3: with b = (a + 1) % 3, c = (a + 2) % 3,
 *     d[a] = -1 for direction < 3 else +1, d[b] = k & 1 ? -1 : +1,
 *     d[c] = k & 2 ? -1 : +1 (length sqrt 3 each, so one bound on t is one
 *     distance).  Ray k is occluded iff its record is not OCH_EXIT and is
 *     OCH_INSIDE or has t < ao_reach (float compare).
 * Mask byte of a pixel: bits 0..3 AO ray k occluded, bit 4 shadowed, bit 5
 * self-shadowed (bit 4 set too); 0x80 for a pixel that is not a face hit; the
 * bits of a ray kind that was not requested are 0.  Shade: with
 * w = 256 - sun_shade * [bit 4] - ao_shade * popcount(bits 0..3), each of R, G,
 * B becomes (c * w + 128) >> 8 and alpha is kept; w = 256 is the identity, so
 * flags = 0 gives och_gpu_render_views_dev's frame word for word.
 *
 * och_light_check (host only): OCH_E_INVALID for unknown flags, OCH_LIGHT_SUN
 * with a non-finite or all-zero sun_dir, OCH_LIGHT_AO with ao_reach not finite
 * or not > 0, sun_shade outside 0..256, ao_shade outside 0..64, or
 * sun_shade + 4 * ao_shade > 256.
 *
 * och_gpu_render_lit_views_dev writes RGBA8 slices, _lit_masks_views_dev the
 * mask bytes (1 B per pixel), both laid out as och_gpu_render_views_dev lays
 * out its slices (view v at v * och_gpu_slice_rows(...) * W pixels; the pool's
 * row deal honoured), so they compose with och_gpu_unshard_views_dev.
 * capacity_pixels is what the buffer holds, in pixels: a smaller buffer, a
 * light och_light_check refuses, views of unequal size and a pool left torn by
 * a failed flush are refused (OCH_E_INVALID) before anything is written.
 * Launch options change the dispatch only (OCH_OPT_TILE_ORDER 2 uses
 * och_gpu_plan_views' plan of exactly this grid, never its split form;
 * OCH_OPT_BOUNCE_COMPACT picks how the secondary rays are dealt over lanes).
 * _views_dev: device buffers, asynchronous on the pool's stream;
 * och_gpu_render_lit: one camera, whole frame, host buffer, synchronous.
 * Across GPUs a lit frame travels as lit codes (below): och_gpu_render_lit_
 * codes_views_dev, och_gpu_shade_lit_unshard_views_dev, the windows
 * och_gpu_render_lit_steps_dev / _lit_sharded_steps_dev and
 * och_frame_group_render_lit.
 * Out of scope: lit and bounce together, more than four AO rays, supersampled
 * lit frames through the sharded paths.  Lit and supersampled frames together
 * on one GPU: och_gpu_render_lit_ssaa_views_dev below. */
enum { OCH_LIGHT_SUN = 1, OCH_LIGHT_AO = 2 };
typedef struct och_light {
    float sun_dir[3];    /* towards the sun; traced as given */
    float ao_reach;      /* an AO ray is occluded by a hit with t < ao_reach */
    int32_t sun_shade;   /* 0..256 */
    int32_t ao_shade;    /* 0..64, per occluded AO ray */
    int32_t flags;       /* OCH_LIGHT_SUN | OCH_LIGHT_AO */
} och_light;
OCH_API int och_light_check(const och_light *light);
OCH_API int och_gpu_render_lit_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views, const och_light *light,
                                         uint32_t *rgba_slices, size_t capacity_pixels, int row_chunk, int shard,
                                         int n_shards);
OCH_API int och_gpu_render_lit_masks_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                               const och_light *light, uint8_t *mask_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards);
OCH_API int och_gpu_render_lit(och_gpu_pool *pool, const och_camera *cam, const och_light *light, uint32_t *rgba,
                               size_t capacity_pixels);
/* Lit codes: the lit frame's exchange format between GPUs, one little-endian
 * uint16 per pixel, code | mask << 8.  code is the OCH_CODE_* byte
 * och_gpu_render_codes_views_dev (bounce = 0) writes for the pixel (a palette
 * index, OCH_CODE_MAGENTA, _INSIDE or _SKY; never | OCH_CODE_BLOCKED); mask is
 * the byte och_gpu_render_lit_masks_views_dev writes for it under the same
 * light.  The lit word of a pixel is the code table's word shaded by the mask
 * as above; a mask of 0x80 has w = 256, so one formula serves every pixel and
 * flags = 0 gives the plain sharded frame word for word.  The whole mask
 * travels, not the shade level: the shading rank may use other weights than
 * the rendering ranks were given.  2 B per pixel, half of RGBA8; a lossless
 * single byte does not exist (some 123 codes x 10 shade levels > 256).
 * och_gpu_render_lit_codes_views_dev: slices laid out as the mask slices, 2 B
 * per pixel; och_gpu_render_lit_views_dev's refusals, and a palette of more
 * than OCH_CODE_MAX_VOXELS ids (or none), all before anything is written; the
 * same plan rule.  och_gpu_shade_lit_unshard_views_dev: gathered lit codes
 * [n_shards][n_views][rows][W] -> RGBA8 frames [n_views][H][W], every word the
 * one och_gpu_render_lit_views_dev writes under light (only its sun_shade and
 * ao_shade are read); refuses a light och_light_check refuses and a pool
 * without a code table. */
OCH_API int och_gpu_render_lit_codes_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                               const och_light *light, uint16_t *code_slices, size_t capacity_pixels,
                                               int row_chunk, int shard, int n_shards);
OCH_API int och_gpu_shade_lit_unshard_views_dev(och_gpu_pool *pool, const uint16_t *gathered, uint32_t *frames,
                                                int width, int height, int row_chunk, int n_shards, int n_views,
                                                const och_light *light);
/* Supersampled lit frames, s x s lit samples per pixel (s = 2, 4 or 8),
 * traced, shaded and resolved in one launch; the sample-resolution frame is
 * never stored.  cams are the cameras of the sample grid (equal width and
 * height, both multiples of s), and view v's frame of (width / s) x
 * (height / s) RGBA8 words goes to rgba + v * (width / s) * (height / s).
 * With F the frames och_gpu_render_lit_views_dev writes for the same cameras
 * and the same light as one shard with row_chunk = height, each byte is
 *   out[Y][X].c = (sum over j, i < s of F[s Y + j][s X + i].c + s * s / 2) >> (2 log2 s):
 * och_gpu_render_ssaa_views_dev's rule on the lit frame -- shade first, then
 * the mean.  Everything else is the lit definition's: sky and INSIDE samples
 * enter with the plain render's colour, alpha is 0xFF, no gamma, no jitter;
 * the secondary origin, the ray directions, the mask rules, ao_reach (in
 * units of t, not of output pixels) and the shade are unchanged.  So
 * light.flags = 0 gives och_gpu_render_ssaa_views_dev's frame word for word.
 * capacity_pixels is what rgba holds, in pixels.  Refused (OCH_E_INVALID)
 * before anything is written: another s, a size that is no multiple of s,
 * views of unequal size, n_views outside 1..OCH_MAX_VIEWS, a smaller buffer, a
 * light och_light_check refuses, NULL pointers and a pool left torn by a
 * failed flush.  Launch options change the dispatch only (OCH_OPT_TILE_ORDER 2
 * uses och_gpu_plan_views' plan for these cameras with row_chunk = height,
 * never its split form; OCH_OPT_BOUNCE_COMPACT as for lit frames).
 * _views_dev: device buffer, asynchronous on the pool's stream;
 * och_gpu_render_lit_ssaa: one camera into a host buffer, synchronous.
 * Out of scope: a mask output, shards and row deals, colour-code slices and
 * the RCCL exchange paths, frame groups, lit and bounce together. */
OCH_API int och_gpu_render_lit_ssaa_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                              const och_light *light, int s, uint32_t *rgba, size_t capacity_pixels);
OCH_API int och_gpu_render_lit_ssaa(och_gpu_pool *pool, const och_camera *cam, const och_light *light, int s,
                                    uint32_t *rgba, size_t capacity_pixels);
/* The frame loop (update_image once per frame, ORT/test_och_h_octree.cpp:
 * 437-457) issued natively: n_steps whole frames of the same cameras
 * (och_gpu_render_views_dev, or _bounce_views_dev with bounce = 1; one shard),
 * frame k on streams[k % n_buffers] into frames[k % n_buffers] (each
 * n_views * H * W RGBA8 words), so up to n_buffers frames are in flight and a
 * frame reuses a buffer only behind the previous frame on that stream.  With
 * start_events / stop_events (n_steps hipEvent_t each, or both NULL) the
 * dispatch of frame k records start_events[k] and stop_events[k].
 * Asynchronous; the pool's stream is left as it was. */
OCH_API int och_gpu_render_steps_dev(och_gpu_pool *pool, const och_camera *cams, int n_views, int n_steps,
                                     void *const *streams, uint32_t *const *frames, int n_buffers,
                                     void *const *start_events, void *const *stop_events, int row_chunk,
                                     int bounce);
/* The same loop with every frame a lit frame (och_gpu_render_lit_views_dev as
 * one shard); the light is checked before the first frame is queued. */
OCH_API int och_gpu_render_lit_steps_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                         const och_light *light, int n_steps, void *const *streams,
                                         uint32_t *const *frames, int n_buffers, void *const *start_events,
                                         void *const *stop_events, int row_chunk);
/* Row deal: instead of round-robin, row chunk g of frames `height` rows tall
 * (chunks of row_chunk rows over n_shards) belongs to shard chunk_shard[g],
 * for ceil(height / row_chunk) chunks; each shard's chunks keep their order.
 * Render, plan, shade and unshard calls of exactly this geometry use it.  A
 * slice then holds och_gpu_slice_rows rows -- the largest shard's chunks, the
 * others' slices padded -- so slices stay equal for an all-gather.  Every
 * rank must set the same deal.  chunk_shard = NULL restores round-robin.
 * Waits for the device (frames in flight may read the old tables). */
OCH_API int och_gpu_set_row_deal(och_gpu_pool *pool, int height, int row_chunk, int n_shards, const int32_t *chunk_shard);
/* Rows per slice for this geometry under the pool's deal (och_shard_rows without one). */
OCH_API int och_gpu_slice_rows(const och_gpu_pool *pool, int height, int row_chunk, int n_shards, int *rows);
/* The cost of every row chunk of these views: one timed render of the whole
 * frame (every workgroup timed, shader clocks), spread over its tiles' rows.
 * costs: ceil(height / row_chunk) floats.  Synchronous. */
OCH_API int och_gpu_chunk_costs(och_gpu_pool *pool, const och_camera *cams, int n_views, int row_chunk, float *costs);
/* Host only: deal n_chunks chunks of the given costs over n_shards, longest
 * first onto the shard with the least cost per weight (weights NULL = all 1;
 * a shard with other fixed work, e.g. the display rank's shading, gets a
 * smaller weight), at most ceil(n_chunks * max weight / sum) + 2 chunks per
 * shard.  Deterministic: the same costs give the same deal on every rank. */
OCH_API int och_deal_chunks(const float *costs, int n_chunks, int n_shards, const float *weights, int32_t *chunk_shard);
/* Reassemble n_shards gathered slices (slice s at gathered + s*rows*W) into a
 * full W*H frame on the device. */
OCH_API int och_gpu_unshard_dev(och_gpu_pool *pool, const uint32_t *gathered, uint32_t *frame,
                                int width, int height, int row_chunk, int n_shards);
/* Multi-view form: gathered = [n_shards][n_views][rows][W] (each rank's
 * och_gpu_render_views_dev output, all-gathered), frames = [n_views][H][W]. */
OCH_API int och_gpu_unshard_views_dev(och_gpu_pool *pool, const uint32_t *gathered, uint32_t *frames,
                                      int width, int height, int row_chunk, int n_shards, int n_views);

/* Indexed-colour form of och_gpu_render_views_dev / _bounce_views_dev (bounce
 * = 0 / 1): the same pixels as OCH_CODE_* bytes, a quarter of the RGBA8 bytes
 * to all-gather between ranks.  OCH_E_INVALID when the pool's palette has
 * more than OCH_CODE_MAX_VOXELS ids. */
OCH_API int och_gpu_render_codes_views_dev(och_gpu_pool *pool, const och_camera *cams, int n_views,
                                           uint8_t *code_slices, int row_chunk, int shard, int n_shards,
                                           int bounce);
/* och_gpu_unshard_views_dev for gathered code slices, shading each code to
 * the RGBA8 word the RGBA render would have written (bit-identical frames). */
OCH_API int och_gpu_shade_unshard_views_dev(och_gpu_pool *pool, const uint8_t *gathered, uint32_t *frames,
                                            int width, int height, int row_chunk, int n_shards, int n_views);

/* ------------------------------------------------------------ multi-GPU frames, one process */
/* SURVEY §8(e) for a C++ host: one process, one thread, every GPU of the node.
 * Each device holds a replica of the pool; rows are dealt in chunks of
 * row_chunk rows round-robin over the devices (och_shard_rows); every device
 * renders its slice, one RCCL all-gather (ncclCommInitAll over the devices,
 * xGMI) hands every device all slices, and each device shades + unshards them
 * into [n_views][H][W] RGBA8 frames -- the frames och_gpu_render_views_dev
 * would write, bit for bit.  Slices travel as 1-byte colour codes when the
 * palette has at most OCH_CODE_MAX_VOXELS ids, as RGBA8 otherwise.  RCCL is
 * loaded on first use (dlopen; an RCCL already in the process is reused);
 * OCH_E_NODEV when it cannot be.  devices = NULL means the first n_devices gfx950 devices (och_device_list).
 * Replaces the per-pixel loop of ORT/test_och_h_octree.cpp:437-457 across GPUs.
 * och_frame_group_plan also deals the row chunks by cost (och_gpu_chunk_costs,
 * och_deal_chunks) so that every device gets an equal share of the work. */
typedef struct och_frame_group och_frame_group;
OCH_API int och_frame_group_create(const int *devices, int n_devices, const uint32_t *nodes, uint32_t n_nodes,
                                   uint32_t root, int depth, int index_base, float miss_t, och_frame_group **out);
OCH_API int och_frame_group_destroy(och_frame_group *group);
OCH_API int och_frame_group_size(const och_frame_group *group, int *n_devices);
/* The pool replica on device `rank` (RCPPS table, stamps; owned by the group). */
OCH_API int och_frame_group_pool(och_frame_group *group, int rank, och_gpu_pool **pool);
OCH_API int och_frame_group_set_palette(och_frame_group *group, const uint32_t *rgba, uint32_t n_voxels);
OCH_API int och_frame_group_set_option(och_frame_group *group, int option, int value);
/* och_gpu_plan_views on every device for this geometry, then OCH_OPT_TILE_ORDER = 2. */
OCH_API int och_frame_group_plan(och_frame_group *group, const och_camera *cams, int n_views, int row_chunk);
/* Enqueue one frame of n_views equal-size cameras on every device (bounce = 1:
 * config 5's secondary rays).  Asynchronous; frames are valid once the
 * group is synchronised (or downloaded). */
OCH_API int och_frame_group_render(och_frame_group *group, const och_camera *cams, int n_views, int row_chunk,
                                   int bounce);
/* Device pointer of device `rank`'s [n_views][H][W] RGBA8 frames (valid until the next render). */
OCH_API int och_frame_group_frames_dev(och_frame_group *group, int rank, uint32_t **frames);
/* Copy device `rank`'s frames to a host buffer of n_views*H*W words (synchronous). */
OCH_API int och_frame_group_download(och_frame_group *group, int rank, uint32_t *rgba);
OCH_API int och_frame_group_synchronize(och_frame_group *group);
/* n_steps frames of the same cameras issued natively: frame k renders,
 * exchanges and shades into buffer set k % n_buffers of every device, on
 * that set's stream, so up to n_buffers frames are in flight (n_buffers
 * 1..8).  Asynchronous.  och_frame_group_frames_dev / _download then give
 * buffer set (n_steps - 1) % n_buffers: the last frame. */
OCH_API int och_frame_group_render_steps(och_frame_group *group, const och_camera *cams, int n_views, int n_steps,
                                         int n_buffers, int row_chunk, int bounce);
/* The two render calls with a light: lit frames, the words
 * och_gpu_render_lit_views_dev writes.  Slices travel as 2-byte lit codes when
 * the palette has at most OCH_CODE_MAX_VOXELS ids, as lit RGBA8 words
 * otherwise.  A light och_light_check refuses is refused before anything is
 * queued. */
OCH_API int och_frame_group_render_lit(och_frame_group *group, const och_camera *cams, int n_views, int row_chunk,
                                       const och_light *light);
OCH_API int och_frame_group_render_lit_steps(och_frame_group *group, const och_camera *cams, int n_views, int n_steps,
                                             int n_buffers, int row_chunk, const och_light *light);

/* ------------------------------------------------------------ multi-GPU frames, one process per GPU */
/* SURVEY §8(e) with one process per GPU (the driver's torch.distributed
 * launch, MPI, ...): the library's own RCCL communicator over the ranks.
 * Rank 0 calls och_comm_unique_id; the caller hands the OCH_COMM_ID_BYTES
 * bytes to every rank by its own means (torch.distributed broadcast, MPI_Bcast,
 * a file); every rank then calls och_comm_create with its device (collective:
 * returns once all ranks joined).  RCCL is loaded on first use, as for the
 * frame group; OCH_E_NODEV when it cannot be. */
#define OCH_COMM_ID_BYTES 128
typedef struct och_comm och_comm;
OCH_API int och_comm_unique_id(uint8_t *id);
OCH_API int och_comm_create(const uint8_t *id, int n_ranks, int rank, int device, och_comm **out);
OCH_API int och_comm_destroy(och_comm *comm);
/* OCH_OK when RCCL can be loaded (no communicator made): lets every rank agree
 * that all can join before any of them blocks in och_comm_create. */
OCH_API int och_comm_available(void);
/* ncclCommAbort, callable from another thread (a watchdog): a collective whose
 * peer never comes stops blocking its stream.  The handle stays valid for
 * och_comm_destroy; later calls on it fail.  Aborting one rank does not
 * unblock the others: each rank's caller aborts its own. */
OCH_API int och_comm_abort(och_comm *comm);
OCH_API int och_comm_info(const och_comm *comm, int *n_ranks, int *rank, int *device);
/* recv = [n_ranks][bytes]: every rank's `bytes` (ncclAllGather), enqueued on stream. */
OCH_API int och_comm_all_gather(och_comm *comm, const void *send, void *recv, size_t bytes, void *stream);
/* Only rank `root` receives recv = [n_ranks][bytes]; the others send (recv may be NULL there).
 * One ncclSend / ncclRecv group per call: the root receives from every rank, its own slice
 * included (a send to itself, skipped when send already sits at recv + root * bytes). */
OCH_API int och_comm_gather(och_comm *comm, const void *send, void *recv, size_t bytes, int root, void *stream);

/* Exchange of a sharded frame (och_gpu_render_sharded_steps_dev). */
enum {
    OCH_EXCHANGE_ALL_GATHER = 0,   /* every rank receives every slice (ncclAllGather), every rank shades */
    OCH_EXCHANGE_DISPLAY = 1,      /* every rank receives every slice, only rank 0 (the display) shades */
    OCH_EXCHANGE_GATHER = 2        /* only rank 0 receives the slices (ncclSend / ncclRecv) and shades */
};
/* The sharded frame loop of update_image (ORT/test_och_h_octree.cpp:437-457)
 * on one rank, issued natively: n_steps frames of the same cameras, frame k on
 * streams[k % n_buffers]:
 *   1. this rank's row chunks of the n_views cameras as colour codes
 *      (och_gpu_render_codes_views_dev, shard = the comm's rank, n_shards = its
 *      size) into slices[b]: [n_views][rows][W] bytes, rows = och_gpu_slice_rows;
 *   2. the exchange into gathered[b]: [n_ranks][n_views][rows][W] bytes;
 *   3. where this rank shades (`exchange` above): shade + unshard into frames[b],
 *      [n_views][H][W] RGBA8 -- the frames och_gpu_render_views_dev writes.
 * gathered / frames may be NULL (or hold NULL entries) on ranks that do not
 * receive / shade.  start_events / stop_events (n_steps each, or both NULL):
 * recorded by frame k's render dispatch.  Every rank must issue the same
 * n_steps.  Asynchronous; the pool's stream is left as it was. */
OCH_API int och_gpu_render_sharded_steps_dev(och_gpu_pool *pool, och_comm *comm, const och_camera *cams, int n_views,
                                             int n_steps, void *const *streams, uint8_t *const *slices,
                                             uint8_t *const *gathered, uint32_t *const *frames, int n_buffers,
                                             void *const *start_events, void *const *stop_events, int row_chunk,
                                             int bounce, int exchange);
/* The same window for lit frames: step 1 writes lit codes
 * (och_gpu_render_lit_codes_views_dev; slices[b] holds 2 B per pixel), step 2
 * moves 2 * n_views * rows * W bytes per rank in any of the three exchanges,
 * step 3 is och_gpu_shade_lit_unshard_views_dev -- the frames
 * och_gpu_render_lit_views_dev writes.  The light, the buffers, the palette
 * and the code table are checked before the first frame is queued. */
OCH_API int och_gpu_render_lit_sharded_steps_dev(och_gpu_pool *pool, och_comm *comm, const och_camera *cams,
                                                 int n_views, int n_steps, void *const *streams,
                                                 uint8_t *const *slices, uint8_t *const *gathered,
                                                 uint32_t *const *frames, int n_buffers, void *const *start_events,
                                                 void *const *stop_events, int row_chunk, const och_light *light,
                                                 int exchange);

/* ------------------------------------------------------------ builder */
/* The demo terrain (ORT/test_och_h_octree.cpp:561-787) built in parallel
 * bottom-up, hash-consed to the same canonical DAG h_octree produces.
 * Output pool is breadth-first (root first, levels contiguous), 1-based with
 * slot 0 unused when dedup = 1 (an h_octree pool), or an expanded 0-based tree
 * with root 0 when dedup = 0 (an och::octree pool). */
typedef struct och_terrain_params {
    int32_t depth;          /* 1..12: dim = 1 << depth */
    int32_t tunnels;        /* apply the remove(tree, tunnels) pass (:786) */
    int32_t dedup;          /* 1 = h_octree DAG, 0 = pointer octree */
    int32_t rand_kind;      /* 0 = glibc rand() default seed, 1 = MSVC rand() */
    int32_t threads;        /* 0 = all hardware threads */
    int32_t use_gpu;        /* 1: voxelise 32^3 bricks on the current GPU (depth >= 5; smaller trees
                               are built on the host); a DAG (dedup = 1) is also hash-consed on
                               the GPU, an expanded tree allocated by host threads;
                               OCH_E_NODEV if no GPU can run the kernels.  0: host threads only.
                               Both give the same pool, slot for slot. */
} och_terrain_params;

typedef struct och_host_pool {
    uint32_t *nodes;        /* n_nodes x 8 */
    uint32_t n_nodes;
    uint32_t root;
    int32_t depth;
    int32_t index_base;
    uint64_t solid_voxels;  /* statistics */
    uint64_t voxel_hist[8]; /* count per voxel id 0..7 (solid ids) */
    uint64_t tree_nodes;    /* nodes of the expanded tree (h_octree nodecnt) */
    double build_seconds;
} och_host_pool;

OCH_API int och_build_terrain(const och_terrain_params *params, och_host_pool *out);
OCH_API void och_host_pool_free(och_host_pool *pool);

/* A DAG from the caller's voxels, in the form och_build_terrain(dedup = 1)
 * returns: 1-based, root 1 (root 0 and one zero node for a world without
 * voxels), breadth-first in first-occurrence order, no empty node.  That form
 * depends on the content alone: the GPU and the host path, every record order
 * and both input kinds give the same pool, slot for slot.
 * A list's records act as successive h_octree::set calls: a later record for a
 * coordinate replaces an earlier one, id 0 removes the voxel, a coordinate
 * outside [0, dim) is ignored.  Ids are any uint32.
 * solid_voxels = the distinct non-zero voxels, voxel_hist[k] those of id k
 * (k = 1..7; [0] stays 0), tree_nodes = the expanded tree's nodes.
 * OCH_E_INVALID: depth outside 1..21, a grid deeper than 10 (u8) / 9 (u32), a
 * list of 2^31 records or more, device data without use_gpu.  OCH_E_CAPACITY:
 * the caller's capacity is too small.  OCH_BUILD_TRACE=1 prints phase times. */
enum { OCH_VOXELS_LIST = 0, OCH_VOXELS_GRID_U8 = 1, OCH_VOXELS_GRID_U32 = 2 };
typedef struct och_voxel_params {
    int32_t depth;       /* 1..21: dim = 1 << depth (3 * depth bits of Morton key fit 64) */
    int32_t kind;
    const void *data;    /* LIST: n x 4 uint32 (x, y, z, id), AoS.  GRID_*: dim^3 ids, x fastest, then y, then z */
    uint64_t n;          /* LIST: records, < 2^31.  GRID_*: ignored */
    int32_t on_device;   /* data is device memory of the current device (use_gpu = 1 only), its
                            writes complete: the build reads it on a stream of its own */
    int32_t use_gpu;     /* as och_terrain_params.use_gpu: 1 = current GPU, OCH_E_NODEV without one; 0 = host threads */
    int32_t threads;     /* host path; 0 = all */
    uint32_t capacity;   /* node ids to reserve, id 0 included; 0 = the exact bound, tree_nodes + 1.
                            Less is enough when subtrees are shared: the unique nodes + 1 on the GPU */
} och_voxel_params;
OCH_API int och_build_voxels(const och_voxel_params *params, och_host_pool *out);

/* A batch of voxel edits applied to an existing pool.  Let V be the pool's
 * voxels (every (x, y, z) where och_pool_at is non-zero) and V' be V after the
 * records, applied in order as h_octree::set calls (a later record wins, id 0
 * removes, a coordinate outside [0, dim) is ignored, ids are any uint32).  The
 * result is the canonical pool of V' in och_build_voxels' form, slot for slot
 * the pool och_build_voxels gives for V listed in any order followed by the
 * records; its statistics are those of the result.  GPU and host path give the
 * same bytes.
 * The input pool need not be canonical: only nodes reachable from root are
 * read; duplicates, any slot order, unused or garbage slots and reachable
 * all-zero nodes (which count as no node) are accepted, so n = 0 canonicalises
 * an editor's slot array (och_editor_nodes).  A node must lie at one height.
 * Refused before *out is touched -- OCH_E_INVALID: depth outside 1..21,
 * n >= 2^31, on_device without use_gpu, nodes NULL with n_nodes > 0, records
 * NULL with n > 0, root > n_nodes, an interior node's child word > n_nodes, a
 * node reachable at two heights.  OCH_E_CAPACITY: the caller's capacity is too
 * small.  OCH_E_NOMEM, OCH_E_NODEV, OCH_E_HIP as the builders.
 * Every call uploads, adopts, renumbers and returns the whole pool in host
 * memory; nothing stays on the device between calls (och_world, below, is
 * the same editor over a store that does stay).
 * OCH_BUILD_TRACE=1 prints phase times ("edit gpu " / "edit host "). */
typedef struct och_edit_params {
    const uint32_t *nodes;  /* the pool to edit, host memory: n_nodes x 8, 1-based (h_octree form) */
    uint32_t n_nodes;
    uint32_t root;          /* 0 = a world without voxels */
    int32_t depth;          /* 1..21 */
    const void *records;    /* n x 4 uint32 (x, y, z, id), as OCH_VOXELS_LIST */
    uint64_t n;             /* < 2^31; 0 = canonicalise only */
    int32_t on_device;      /* records are device memory (use_gpu = 1 only), writes complete */
    int32_t use_gpu, threads;
    uint32_t capacity;      /* node ids to reserve, id 0 included; 0 = the bound: the reachable input
                               nodes + one id per row of the records' own tree (the level counts of
                               the unique in-range keys, id 0 included) + 1.  Less is enough when
                               nodes are shared: the distinct nodes of both trees + 1 on the GPU */
} och_edit_params;
OCH_API int och_edit_voxels(const och_edit_params *params, och_host_pool *out);

/* The packed device layout (OCH_OPT_LAYOUT 1) of a pool, on the host: node 0
 * is zero padding, ids are breadth-first per level, interior slots hold
 * child_id | child_mask << 24, leaf-level slots voxel ids; *out_root =
 * root_id | root_mask << 24.  out = NULL only reports *out_nodes. */
OCH_API int och_pool_pack(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                          uint32_t *out, uint32_t out_capacity, uint32_t *out_nodes, uint32_t *out_root);
/* Bounding box of every non-empty leaf voxel reachable from root, in voxel
 * units: voxel (x, y, z) lies in it iff lo <= (x, y, z) < hi per axis.
 * Returns OCH_OK with lo = hi = {0, 0, 0} for a pool without voxels. */
OCH_API int och_pool_occupied_box(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                                  int32_t lo[3], int32_t hi[3]);
/* h_octree::at over any pool (ORT/och_h_octree.h:239-258). */
OCH_API uint32_t och_pool_at(const uint32_t *nodes, uint32_t root, int depth, int index_base,
                             int x, int y, int z);
/* A box of voxels as a dense grid, on the host, from any pool: the cell of
 * (x, y, z), lo <= (x, y, z) < hi per axis, is grid[((z - lo[2]) * ny +
 * (y - lo[1])) * nx + (x - lo[0])] with (nx, ny, nz) = hi - lo -- x fastest,
 * then y, then z, the layout och_build_voxels takes, so a whole tree read and
 * fed back as a grid rebuilds the same pool.  kind is OCH_VOXELS_GRID_U8 or
 * OCH_VOXELS_GRID_U32.  A cell inside [0, dim) holds och_pool_at of its
 * coordinate, a cell outside holds 0: the box may reach past the tree on any
 * side and lo may be negative (extents and the volume are 64-bit).  A box with
 * hi == lo on some axis writes nothing and returns OCH_OK.
 * Refused before anything is written -- OCH_E_INVALID: a NULL pointer, another
 * kind, index_base outside 0 and 1, a pool och_pool_occupied_box refuses,
 * hi[a] < lo[a], a volume times the cell size above capacity_bytes.
 * With OCH_VOXELS_GRID_U8 an id above 255 inside the box gives OCH_E_INVALID,
 * the text naming the id, and the grid's contents are then unspecified (this
 * cannot be known before reading); no value is ever truncated.
 * och_world_read_box, below, gives the same bytes from a resident world. */
OCH_API int och_pool_read_box(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, int index_base,
                              const int32_t lo[3], const int32_t hi[3], int kind, void *grid, size_t capacity_bytes);

/* What a diff reports (och_pool_diff here, och_world_diff below). */
typedef struct och_diff_stats {
    uint64_t n;                    /* voxels whose id differs between the two roots */
    uint64_t pairs;                /* node positions expanded, the root's included */
    int32_t box_lo[3], box_hi[3];  /* box of those voxels, [lo, hi); lo = hi = 0 when n = 0 */
} och_diff_stats;                  /* 40 bytes */
/* The voxels that differ between two host pools of one depth and index_base:
 * for every coordinate where the voxel under (nodes_a, root_a) differs from the
 * one under (nodes_b, root_b), one record (x, y, z, id under b), 4 x uint32 in
 * the OCH_VOXELS_LIST layout, id 0 = the voxel was removed; in ascending Morton
 * order (key = x bit 0, y bit 1, z bit 2 per level).  Applied as edits to a's
 * content the records give b's.  The pools need not be canonical; an all-zero
 * node counts as no node.  capacity counts records; records = NULL is the
 * summary form: only *stats.  och_world_diff gives the same records, n and box
 * for the same two contents; `pairs` here is the positions this walk visited,
 * which prunes only where both arguments are the same array and the ids are
 * equal, so it is not comparable with the world's.
 * Refused before anything is written -- OCH_E_INVALID: NULL stats or nodes,
 * index_base outside 0 and 1, depth outside 1..21, a pool
 * och_pool_occupied_box refuses, 2^31 differing voxels or more.
 * OCH_E_CAPACITY: records != NULL and n > capacity; *stats is complete and
 * nothing has been written to records. */
OCH_API int och_pool_diff(const uint32_t *nodes_a, uint32_t n_a, uint32_t root_a,
                          const uint32_t *nodes_b, uint32_t n_b, uint32_t root_b, int depth, int index_base,
                          void *records, uint64_t capacity, och_diff_stats *stats);

/* ------------------------------------------------------------ world */
/* A DAG that stays on one GPU between brush strokes: the node store
 * och_edit_voxels builds per call (nodes, levels, hash table), kept, with the
 * current root, a stream and the stroke's work buffers.  och_world_edit applies
 * a list of records to it as och_edit_voxels would and replaces the root;
 * och_world_flush publishes the new nodes to a pool made by
 * och_world_pool_create, which traces and renders like any other pool.
 * The store is append-only: a stroke only adds nodes, so every earlier root,
 * and every frame in flight that walks from one, stays valid, and a flush
 * waits for no kernel.  Ids are handed out in claim order and mean something
 * only inside one world and generation; och_world_download gives the canonical
 * pool.  What strokes no longer reach stays in the store until
 * och_world_compact.
 * GPU only (OCH_E_NODEV without a device), 1-based pools, depth 1..21, one
 * thread at a time per world, like the editor.  After a HIP failure inside a
 * stroke the world is broken: every later call on it but och_world_destroy
 * returns OCH_E_INVALID; pools keep what their last flush gave them.
 * OCH_BUILD_TRACE=1 prints phase times ("world ").
 * Out of scope: worlds replicated across GPUs, frame groups and the sharded
 * paths; 0-based pools; depth 22.  Earlier roots (undo, checkout, the diff of
 * two roots) are the history section below. */
typedef struct och_world och_world;

typedef struct och_world_stats {
    uint32_t capacity;    /* ids, id 0 included */
    uint32_t used;        /* ids handed out, id 0 included */
    uint32_t root;        /* store id (0 = no voxels); means something only inside this world and generation */
    int32_t depth, device;
    uint64_t strokes;     /* edits applied since create */
    uint64_t generation;  /* +1 per och_world_compact: store ids of another generation mean nothing */
    int32_t box_lo[3], box_hi[3];  /* a superset of the voxels' box, [lo, hi); lo = hi = 0: none.
                                      Exact right after och_world_tighten */
} och_world_stats;

/* Adopt a pool: what och_edit_voxels accepts as its pool (host memory,
 * 1-based, not necessarily canonical; n_nodes = 0 or root = 0: an empty world
 * to paint into), with its refusals before anything is touched
 * (OCH_E_INVALID: depth outside 1..21, nodes NULL with n_nodes > 0,
 * root > n_nodes, a child word past the end, a node at two heights).
 * capacity = ids to reserve, id 0 included and fixed for the world's life;
 * 0 = twice the reachable nodes + 64 * depth.  OCH_E_CAPACITY: fewer than the
 * reachable nodes + 1; OCH_E_INVALID: 2^29 - 1 or more.  device < 0: the
 * current one.  The box starts as och_pool_occupied_box of the nodes. */
OCH_API int och_world_create(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth, uint32_t capacity,
                             int device, och_world **out);
OCH_API int och_world_destroy(och_world *world);
OCH_API int och_world_info(const och_world *world, och_world_stats *info);
/* One stroke: n records as OCH_VOXELS_LIST (host memory, or device memory of
 * the world's device with its writes complete; n < 2^31, n = 0 is a no-op)
 * with och_edit_voxels' semantics -- in order, last wins, id 0 removes, out of
 * range ignored, any uint32 id.  Nothing of the pool is uploaded, reached,
 * adopted, renumbered, counted or downloaded.
 * OCH_E_CAPACITY, with the world unchanged, when used + the level counts of
 * the stroke's unique in-range keys > capacity: one id per row of the
 * records' own tree, ignoring what the rows share with the store, so the
 * answer depends on the records alone.  Call och_world_compact and retry.
 * The box grows by the box of the stroke's surviving in-range records with
 * id != 0 -- surviving: after last wins, so a coordinate set and then removed
 * within one list does not count; removals never shrink it
 * (och_world_tighten does). */
OCH_API int och_world_edit(och_world *world, const void *records, uint64_t n, int on_device);
/* A pool of the current world on the world's device: index_base 1, the
 * world's depth, miss t = +INF, capacity slots (och_pool_info.n_nodes), its
 * raw layout the store's rows, its packed layout (capacity <= 2^24; raw only
 * above) numbered like them.  The caller destroys it, before or after the
 * world.  It has no host mirror: och_gpu_pool_update and och_editor_flush on
 * it return OCH_E_INVALID.  Everything else about a pool works unchanged. */
OCH_API int och_world_pool_create(och_world *world, och_gpu_pool **out);
/* Publish the strokes since the pool's last flush: the ids handed out since
 * then are copied and packed on the device, then both roots and the box are
 * published.  Complete on return.  The ids written are reached by no root
 * published before, so launches in flight are not waited for -- except after a
 * compaction, which renumbers: the flush then waits for all work on the device
 * and rewrites the pool whole (a failure then leaves the pool torn, as a
 * failed och_editor_flush does, until a later flush succeeds; any other failed
 * flush leaves the pool showing its last one).  OCH_E_INVALID for a pool not
 * made from this world. */
OCH_API int och_world_flush(och_world *world, och_gpu_pool *pool);
/* The canonical pool of the world's voxels with its statistics, slot for slot
 * what och_build_voxels / och_edit_voxels give for the same content; freed
 * with och_host_pool_free.  The world is unchanged: the save path. */
OCH_API int och_world_download(och_world *world, och_host_pool *out);
/* Drop what neither the root nor a live snapshot (below) reaches: the
 * reachable nodes interned into a fresh store of the same capacity.  Content
 * (the current root's and every snapshot's), box and capacity are unchanged
 * and every handle stays valid; `used` becomes the distinct nodes reachable
 * from all of them + 1, generation + 1; every pool is rewritten whole by its
 * next flush.  A failure leaves the old store and every handle in place. */
OCH_API int och_world_compact(och_world *world);

/* ------------------------------------------------------------ world: reading back */
/* Asking a resident world what it holds, on its GPU, under its current root:
 * every stroke applied so far counts, flushed to a pool or not.  The store is
 * append-only, so a query waits for nothing but its own kernel.  All three
 * calls are synchronous: the world's stream is synchronised and the results
 * are complete on return.  och_world_at and och_world_read_box only read: a
 * HIP failure in them is reported (OCH_E_HIP) and leaves the world usable, as
 * in och_world_download.  OCH_BUILD_TRACE=1 prints their phase times too.
 * Out of scope: queries on an och_gpu_pool instead of the world; asynchronous
 * queries on a caller's stream; run-length or sparse output; shrinking the box
 * inside a stroke.  An older root is read by checking its snapshot out first
 * (och_world_checkout, below: O(1)). */

/* h_octree::at for n coordinates: coords is n x 3 int32 (x, y, z), AoS, and
 * ids[i] becomes the voxel at coordinate i.  A coordinate outside [0, dim)
 * gives 0 -- unlike och_pool_at, which does not range-check.  on_device != 0:
 * both buffers are memory of the world's device, their writes complete (the
 * kernel runs on the world's stream); otherwise both are host memory.
 * n = 0 is a no-op.  OCH_E_INVALID, whatever the world: n >= 2^31, a NULL
 * buffer with n > 0; then a NULL or broken world. */
OCH_API int och_world_at(och_world *world, const int32_t *coords, uint64_t n, uint32_t *ids, int on_device);
/* och_pool_read_box of the world's current content, byte for byte: the
 * layout, the overhang (cells outside [0, dim) read 0), the empty box, the
 * refusals before anything is written (a NULL lo, hi or grid, another kind,
 * hi[a] < lo[a], a volume times the cell size above capacity_bytes; then a
 * NULL or broken world) and OCH_E_INVALID naming an id above 255 met under
 * OCH_VOXELS_GRID_U8, the grid's contents then unspecified.  on_device
 * applies to grid only (memory of the world's device; lo and hi are host
 * memory); a host grid goes through a device buffer the world allocates on
 * demand and keeps.  A box that meets the tree in 2^32 aligned 4x4x4 bricks
 * or more is refused (OCH_E_INVALID). */
OCH_API int och_world_read_box(och_world *world, const int32_t lo[3], const int32_t hi[3], int kind, void *grid,
                               size_t capacity_bytes, int on_device);
/* Make the world's box exact: och_pool_occupied_box of what
 * och_world_download would return; a world without voxels reports
 * lo = hi = 0.  The next och_world_flush of each pool publishes it.  Later
 * strokes grow it by their own boxes again, so it is exact right after this
 * call and a superset afterwards.  No traced record depends on which superset
 * of the voxels' box a pool holds, so frames are unchanged.
 * The first call allocates 16 bytes per id of the world's capacity (256 MiB at
 * capacity 2^24), kept for the world's life, and fills it for every id in use;
 * later calls only visit the ids handed out since, a call after
 * och_world_compact starts over.  OCH_E_NOMEM leaves the box and the world as
 * they were; a HIP failure breaks the world, as in a stroke. */
OCH_API int och_world_tighten(och_world *world);

/* ------------------------------------------------------------ world: history */
/* The store is append-only, so every earlier state of a world is still intact
 * on the GPU: a snapshot remembers one, a checkout makes it current again
 * (undo; strokes after it branch off, and the state left behind stays
 * reachable through its own snapshot: redo), and och_world_diff answers what
 * changed between two of them at a cost that follows the change, not the world.
 * A snapshot is a handle: handles start at 1 per world, are never reused and
 * mean something only for that world; two snapshots of one state are two
 * handles.  It keeps the root, its child mask and the world's box as they are
 * at the call, and lives until och_world_release or och_world_destroy;
 * och_world_compact keeps what live snapshots reach.
 * Out of scope: snapshots across och_world_destroy, or their serialisation; a
 * diff between two worlds or between generations; och_world_at /
 * och_world_read_box of a snapshot (check it out first); asynchronous diffs;
 * replicated worlds themselves (diff(A, B) applied as one och_world_edit turns
 * a replica holding A into B: this is their primitive); frame groups and the
 * sharded paths. */
#define OCH_WORLD_CURRENT 0ull            /* as `from` / `to` / `snapshot`: the world's current root */
#define OCH_WORLD_MAX_SNAPSHOTS 65536
/* Remember the current root.  OCH_E_INVALID: a NULL snapshot, a NULL or broken
 * world; OCH_E_CAPACITY: OCH_WORLD_MAX_SNAPSHOTS are live already. */
OCH_API int och_world_snapshot(och_world *world, uint64_t *snapshot);
/* Make the snapshot's root, mask and box the world's again: O(1), nothing is
 * launched; used, strokes, generation and the store do not change.  The box is
 * the one the world had at the snapshot, a superset of that content
 * (och_world_tighten makes it exact); the next och_world_flush of each pool
 * publishes the root.  OCH_WORLD_CURRENT is a no-op.  OCH_E_INVALID, the text
 * naming the handle: an unknown or released one. */
OCH_API int och_world_checkout(och_world *world, uint64_t snapshot);
/* Forget a snapshot; what only it reached goes with the next och_world_compact.
 * OCH_E_INVALID: an unknown or released handle, OCH_WORLD_CURRENT. */
OCH_API int och_world_release(och_world *world, uint64_t snapshot);
/* The live handles in ascending order: up to `capacity` of them into ids
 * (NULL with capacity 0: count only), the total in *count. */
OCH_API int och_world_snapshots(const och_world *world, uint64_t *ids, uint32_t capacity, uint32_t *count);
/* och_pool_diff of the contents under two roots of this world, on its GPU:
 * the same records in the same (ascending Morton) order, the same n and box.
 * from / to are snapshot handles or OCH_WORLD_CURRENT.  capacity counts
 * records; on_device != 0: records is memory of the world's device, otherwise
 * host memory, reached through a device buffer the world keeps; records = NULL
 * is the summary form: only *stats.  Two ids at one height are equal exactly
 * when their subtrees hold the same voxels, so the walk expands only positions
 * whose subtrees differ: `pairs`, the frontier sizes summed over the levels,
 * is the sum over h = 1..depth of the distinct values of key >> 3h over the
 * differing voxels' Morton keys, and roots with equal ids give n = 0, pairs = 0
 * and no launch.  Synchronous on the world's stream (one 8-byte read-back per
 * level); the buffers are kept, grown on demand.  It only reads: a HIP failure
 * is OCH_E_HIP and leaves the world usable.
 * Refused, nothing written -- OCH_E_INVALID: NULL stats, a NULL or broken
 * world, an unknown handle, a level's frontier or an n of 2^31 or more.
 * OCH_E_CAPACITY: records != NULL and n > capacity; *stats is complete and
 * nothing has been written to records. */
OCH_API int och_world_diff(och_world *world, uint64_t from, uint64_t to, void *records, uint64_t capacity,
                           int on_device, och_diff_stats *stats);

/* ------------------------------------------------------------ world: regions */
/* Strokes whose shape is a box, at a cost that follows the box's surface.  A
 * box is a union of maximal aligned cubes, and a cube of side 2^h that lies
 * wholly inside it is one child word at height h: 0 for a clear, the id of the
 * uniform subtree of that height for a fill, the word another root holds there
 * for a restore.  Only the cells that straddle the box's faces get new rows.
 * Both strokes are append-only like och_world_edit: frames in flight and other
 * snapshots stay valid, OCH_E_CAPACITY leaves the world unchanged, and a HIP
 * failure inside them breaks the world.  The part of a box outside the tree is
 * ignored; hi[a] <= lo[a] on an axis, or nothing left after clipping, is a
 * stroke that changes nothing (strokes + 1, OCH_OK, stats all 0), as an edit
 * whose records all lie outside the tree.
 * A ball (och_world_fill_sphere, och_world_restore_sphere) is the second
 * shape: the same cubes, cells and levels, classified against a sphere.
 * Strokes conditional on the old voxel (och_world_paint_box, _paint_sphere)
 * close the section.
 * Out of scope: shapes other than boxes and balls; copying a box to another
 * place; replicated worlds. */
typedef struct och_region_stats {
    uint64_t cubes;      /* child words written: the maximal aligned cubes inside the box that were emitted */
    uint64_t cells;      /* straddling cells expanded = rows rebuilt, summed over the levels */
    uint64_t new_ids;    /* ids the stroke consumed */
    int32_t  lo[3], hi[3];  /* the box after clipping to [0, dim); lo = hi = 0: nothing inside the tree */
} och_region_stats;      /* 48 bytes */

/* Host only, no device: the maximal aligned cubes of lo <= (x, y, z) < hi
 * clipped to a tree of `depth` (1..21) -- the cubes of side 2^h, aligned to
 * 2^h, that lie inside the box while their parent cube does not.  keys[i] is
 * cube i's Morton key at its height heights[i] (its corner is the key's
 * coordinates times 2^h; key = x bit 0, y bit 1, z bit 2 per level), in
 * ascending height and ascending key within a height: the order in which the
 * region strokes inject them.  cubes_per_height[h] counts them; cells_per_height[H]
 * counts the cells of side 2^H that straddle the box (meet it without lying
 * inside): the rows a fill rebuilds.  Both arrays hold 22 entries (heights
 * 0..21; the whole tree is one cube at height depth) and either may be NULL;
 * *count is the cubes' total.  keys = heights = NULL with capacity 0 gives the
 * counts only, from closed forms.  OCH_E_INVALID: a NULL lo, hi or count,
 * depth outside 1..21, only one of keys and heights; OCH_E_CAPACITY: more
 * cubes than capacity, the counts complete and nothing written to keys. */
OCH_API int och_box_cubes(const int32_t lo[3], const int32_t hi[3], int depth,
                          uint64_t *keys, uint8_t *heights, uint64_t capacity,
                          uint64_t cubes_per_height[22], uint64_t cells_per_height[22], uint64_t *count);
/* Set every voxel of the box to id (0 removes; any uint32): the world is left
 * exactly as och_world_edit of the box's records would leave it, content and
 * canonical och_world_download alike, without a record: for any box
 * stats.cubes and stats.cells are och_box_cubes' totals.  A box that covers
 * the whole tree makes the root the uniform subtree of height depth, or 0.
 * OCH_E_CAPACITY, with the world unchanged, when used + cells + T > capacity,
 * T = the greatest height with a cube for id != 0 (the uniform subtrees made
 * on the way), else 0: the answer depends on the box alone.  OCH_E_INVALID: a
 * NULL lo or hi, a NULL or broken world, a height with 2^31 entries or more.
 * id != 0 grows the world's box by the clipped box; a clear leaves it
 * (och_world_tighten makes it exact).  One read-back, of the store's head. */
OCH_API int och_world_fill_box(och_world *world, const int32_t lo[3], const int32_t hi[3], uint32_t id,
                               och_region_stats *stats /* may be NULL */);
/* Inside the clipped box the content of `snapshot`, outside it the current
 * content.  The snapshot is a live handle of this world; OCH_WORLD_CURRENT is
 * a stroke that changes nothing.  The walk drops every cell whose ids under
 * the two roots are equal (och_world_diff's rule), so the cost follows the
 * part of the box's surface and interior that differs: stats.cubes counts the
 * maximal cubes inside the box whose content differs, stats.cells the
 * straddling cells whose content inside the box differs.  A box that covers
 * the whole tree makes the snapshot's root the current one (cubes = 1 when the
 * roots differ).  A restore that finds no differing cube -- OCH_WORLD_CURRENT,
 * equal roots, a box outside the tree, or two states that differ outside the
 * box only -- changes nothing but strokes (+ 1): it consumes no id, is never
 * refused for capacity and leaves the world's box as it is.  Otherwise:
 * OCH_E_CAPACITY, with the world unchanged, when used + the straddling cells
 * the walk expanded (those whose two ids differ, the root cell included; at
 * least stats.cells) > capacity, and the world's box grows by the part of the
 * clipped box inside the snapshot's box (a whole-tree restore consumes no id
 * and is never refused).  OCH_E_INVALID: a NULL lo or hi, a NULL or broken
 * world, an unknown or released handle, a height with 2^31 differing cubes or
 * 2^28 differing cells or more.  One 8-byte read-back per level on
 * the way down, one of 4 bytes per level on the way up; the buffers are kept
 * and grown on demand, as och_world_diff's. */
OCH_API int och_world_restore_box(och_world *world, uint64_t snapshot, const int32_t lo[3], const int32_t hi[3],
                                  och_region_stats *stats /* may be NULL */);

/* A ball, in integers and half-voxel units: voxel (x, y, z) has its centre at
 * (2x+1, 2y+1, 2z+1); centre2[3] is twice the ball's centre (so it may sit on
 * a voxel's centre, face, edge or corner) and `diameter` counts voxels.  The
 * voxel is in the ball iff
 *   (2x+1-centre2[0])^2 + (2y+1-centre2[1])^2 + (2z+1-centre2[2])^2 <= diameter^2.
 * |centre2[a]| <= 2^24 and diameter <= 2^24, else OCH_E_INVALID: every offset
 * then stays below 2^24.4 and the sum below 2^51, exact in 64-bit integers,
 * and the range still reaches a ball over a whole tree of depth 21.  The
 * aligned cube [c, c + 2^h)^3 is classified per axis, a = 2c+1-centre2 and
 * b = 2(c+2^h)-1-centre2: its farthest offset is max(|a|, |b|), its nearest
 * min(|a|, |b|) where a and b have one sign, else 0 for an odd and 1 for an
 * even centre2[a]; inside iff the farthest offsets' squares sum to at most
 * diameter^2, outside iff the nearest offsets' squares sum to more, straddling
 * otherwise (it then holds a voxel inside and a voxel outside; a voxel never
 * straddles).  The ball's axis box, lo[a] = ceil((centre2[a] - diameter - 1) / 2),
 * hi[a] = floor((centre2[a] + diameter - 1) / 2) + 1, clipped to the tree, is
 * a loose superset of its voxels: the lo and hi of the stats, and what the
 * world's box grows by.
 *
 * och_sphere_cubes: och_box_cubes for a ball, its contract in every respect
 * (host only; ascending height, then ascending key; counts only without keys
 * and heights; OCH_E_CAPACITY with complete counts and nothing written;
 * OCH_E_INVALID for a NULL centre2 or count, depth outside 1..21, only one of
 * keys and heights), and OCH_E_INVALID for the argument range above.  There
 * are no closed forms: the counts come from the top-down walk itself, counts
 * only included, so a call costs what the ball's surface holds (cubes + 8 *
 * cells classifications), not its volume. */
OCH_API int och_sphere_cubes(const int32_t centre2[3], uint32_t diameter, int depth,
                             uint64_t *keys, uint8_t *heights, uint64_t capacity,
                             uint64_t cubes_per_height[22], uint64_t cells_per_height[22], uint64_t *count);
/* Set every voxel of the ball to id (0 removes; any uint32): the world is left
 * exactly as och_world_edit of the ball's records would leave it, content and
 * canonical och_world_download alike; a record stroke of the same ball
 * afterwards consumes no id.  stats.cubes and stats.cells are
 * och_sphere_cubes' totals, stats.lo and stats.hi the clipped axis box (all 0
 * where that is empty).  A ball that covers the tree makes the root the
 * uniform subtree of height depth, or 0.  OCH_E_CAPACITY, with the world
 * unchanged, when used + cells + T > capacity, T = the greatest height with a
 * cube for id != 0, else 0; checked after the walk and before the first
 * intern: the answer depends on ball and depth alone.  cubes = 0 -- no voxel
 * of the ball lies in the tree: an empty axis box, diameter 0 with an even
 * centre2 component, ... -- changes nothing but strokes (+ 1), is never
 * refused for capacity and leaves the world's box alone.  id != 0 with
 * cubes > 0 grows the world's box by the clipped axis box; a clear leaves it.
 * OCH_E_INVALID: a NULL centre2, a NULL or broken world, the argument range,
 * a height with 2^31 entries or more, a frontier of 2^28 cells or more.
 * The walk keeps its counts on the device: two read-backs a stroke, of the
 * walk's totals by height and of the store's head; where a level outgrew the
 * sizes the walk was launched with, the walk (which interns nothing) runs
 * again with larger ones. */
OCH_API int och_world_fill_sphere(och_world *world, const int32_t centre2[3], uint32_t diameter, uint32_t id,
                                  och_region_stats *stats /* may be NULL */);
/* Inside the ball the content of `snapshot`, outside it the current content:
 * och_world_restore_box' contract word for word with "box" read as "ball".
 * The walk drops every child whose two words are equal; cubes and cells count
 * only what differs; a restore that finds no differing cube changes nothing
 * but strokes and is never refused; OCH_E_CAPACITY, with the world unchanged,
 * when used + the straddling cells the walk expanded > capacity; the world's
 * box grows by the clipped axis box inside the snapshot's box only when a cube
 * differed; a ball over the whole tree makes the snapshot's root current, with
 * cubes = 1.  OCH_E_INVALID as och_world_restore_box, and a NULL centre2 or
 * the argument range.  One 8-byte read-back per level on the way down, one of
 * 4 bytes per level on the way up: the cost follows what differs, not the
 * ball's surface. */
OCH_API int och_world_restore_sphere(och_world *world, uint64_t snapshot, const int32_t centre2[3], uint32_t diameter,
                                     och_region_stats *stats /* may be NULL */);

/* Conditional strokes: inside the shape a voxel whose current id is v becomes
 * pred(v) ? id : v, with pred(v) = (v == match) for OCH_WHEN_IS and
 * (v != match) for OCH_WHEN_IS_NOT.  Paint the solid voxels: (IS_NOT, 0, id);
 * fill under, the empty ones only: (IS, 0, id); replace a material: (IS, m, n);
 * erase it: (IS, m, 0); keep only it: (IS_NOT, m, 0).
 *
 * The world is left exactly as och_world_edit would leave it given the records
 * {(x, y, z, id) : voxel in the shape, in the tree, pred(current id)}, content
 * and canonical och_world_download alike; that record stroke afterwards
 * consumes no id and leaves the root where it is.  Shape, clipping, argument
 * ranges, the ball's integer inequality and the axis box are
 * och_world_fill_box' and och_world_fill_sphere's.  Append-only like every
 * stroke; a HIP failure breaks the world.
 *
 * A cube inside the shape is one child word and its new word a function of the
 * subtree the old word names, evaluated once per distinct node of the DAG: the
 * cost follows the shape's surface plus the distinct nodes under it, never its
 * volume.  Heights: a voxel is 0, a node of height h >= 1 has children of
 * height h - 1.  A cube's word is what the current root holds at its position
 * (an interior word at or above the capacity reads as 0).  A cube of height h
 * is open when the stroke can touch it: always for h >= 1 and word != 0,
 * otherwise (an empty cube, a voxel) iff pred(word).  stats.cells counts the
 * straddling open cells the walk expanded, the root cell included; stats.cubes
 * the open cubes inside the shape whose parent is not (a shape that covers the
 * tree: one cube of height depth, no cell).  N_h is the set of distinct
 * non-empty nodes of height h >= 1 that are a counted cube's word or a
 * non-zero child of a member of N_(h+1); stats.nodes = sum |N_h|.  T = the
 * greatest height of a counted cube when pred(0) and id != 0 (the uniform
 * subtrees empty positions turn into), else 0.  All of these depend on the
 * world's content, the shape and the predicate alone.
 *
 * cubes = 0 changes nothing but strokes (+ 1): no id, never refused for
 * capacity, the world's box left alone.  OCH_E_CAPACITY, with the world
 * unchanged, when used + cells + nodes + T > capacity; checked after the walk
 * and the map's way down, before the first intern.  The world's box grows by
 * the clipped (axis) box only when pred(0), id != 0 and cubes > 0: no other
 * conditional stroke makes an empty voxel solid.  OCH_E_INVALID: a `when`
 * other than 0 or 1, a NULL or broken world, NULL pointers, the ball's
 * argument range, a height with 2^31 or more cubes, candidates or nodes, a
 * frontier of 2^28 or more cells.  One 8-byte read-back per level of the walk,
 * one of 4 bytes per height of the map and per level on the way up. */
#define OCH_WHEN_IS      0   /* voxels whose current id == match   (match 0: the empty ones) */
#define OCH_WHEN_IS_NOT  1   /* voxels whose current id != match   (match 0: the solid ones) */

typedef struct och_paint_stats {
    uint64_t cubes;     /* open maximal cubes inside the shape */
    uint64_t cells;     /* open straddling cells the walk expanded, the root cell included */
    uint64_t nodes;     /* distinct nodes mapped, summed over the heights */
    uint64_t new_ids;   /* ids the stroke consumed */
    int32_t  lo[3], hi[3];   /* the clipped (axis) box, as och_region_stats */
} och_paint_stats;           /* 56 bytes */

OCH_API int och_world_paint_box(och_world *world, const int32_t lo[3], const int32_t hi[3], int when, uint32_t match,
                                uint32_t id, och_paint_stats *stats /* may be NULL */);
OCH_API int och_world_paint_sphere(och_world *world, const int32_t centre2[3], uint32_t diameter, int when, uint32_t match,
                                   uint32_t id, och_paint_stats *stats /* may be NULL */);

/* ------------------------------------------------------------ editor */
/* Interactive editing (the demo's place/remove, ORT/test_och_h_octree.cpp:
 * 301-435): h_octree::set / at (ORT/och_h_octree.h:176-258) over a host pool of
 * `capacity` slots (1-based, slot s at nodes[(s-1)*8]) that a device pool of
 * the same size mirrors.  An edit path-copies at most `depth` new nodes into
 * freed or never-used slots and frees dead ones; och_editor_flush uploads the
 * runs of slots written since the last flush, raw and packed layouts alike.
 * Traced records equal the reference's after the same edits (slot numbering
 * differs: the reference places nodes by hash, :110-160). */
typedef struct och_editor och_editor;

typedef struct och_editor_stats {
    uint32_t capacity;      /* slots */
    uint32_t live_nodes;    /* distinct nodes reachable from the root */
    uint32_t high_water;    /* highest slot ever handed out */
    uint32_t root;
    int32_t depth;
    uint32_t dirty_first;   /* lowest slot written since the last flush */
    uint32_t dirty_count;   /* distinct slots written since the last flush (0 = none) */
} och_editor_stats;

/* Adopt a 1-based pool (e.g. och_build_terrain's; root 0 = empty tree).
 * OCH_E_INVALID for an out-of-range child or an empty interior node,
 * OCH_E_CAPACITY if its nodes do not fit in capacity slots. */
OCH_API int och_editor_create(const uint32_t *nodes, uint32_t n_nodes, uint32_t root, int depth,
                              uint32_t capacity, och_editor **out);
OCH_API int och_editor_destroy(och_editor *editor);
/* h_octree::set: voxel (x,y,z) := v (0 removes).  Out-of-range coordinates are
 * ignored, as in the reference.  OCH_E_CAPACITY (tree unchanged) when fewer
 * than depth slots are free; the reference exit(0)s (ORT/och_h_octree.h:112-116). */
OCH_API int och_editor_set(och_editor *editor, int x, int y, int z, uint32_t v);
OCH_API uint32_t och_editor_at(const och_editor *editor, int x, int y, int z);
OCH_API int och_editor_info(const och_editor *editor, och_editor_stats *info);
/* The slot array (capacity x 8, valid until the next edit) and root: pass
 * them to och_gpu_pool_create to make the mirroring device pool. */
OCH_API int och_editor_nodes(const och_editor *editor, const uint32_t **nodes, uint32_t *n_slots, uint32_t *root);
/* Upload the dirty slots, then the root, to a pool made from this editor
 * (index_base 1, same depth, capacity slots).  Slots are rewritten in place,
 * so the flush first waits for ALL work on the pool's device (every stream).
 * Only a pool this editor's last flush wrote, untouched since, gets the
 * windowed upload; any other pool (a new one, one another editor or
 * och_gpu_pool_update wrote, or one a failed flush left behind) is written
 * whole, its packed layout replaced by one numbered like the slots.  The root
 * is published after every slot it reaches.  A flush that fails after it
 * began writing leaves slots half written (slots are reused in place), so it
 * marks the pool torn: traces, renders and och_gpu_pool_update on it return
 * OCH_E_INVALID until a later flush of this editor succeeds. */
OCH_API int och_editor_flush(och_editor *editor, och_gpu_pool *pool);

#ifdef __cplusplus
}
#endif
#endif /* OCH_GPU_H */
