/*
 * align3d_hip.h — C ABI of the MI355X (gfx950) implementation of align3d's ICP hot path.
 *
 * The reference (otaviog/align3d, Rust) has no FFI of its own: the hot path sits behind ordinary
 * public Rust API.  Every entry point below names the Rust item it stands in for (file:line under
 * the reference checkout).  A Rust shim that keeps `MultiscaleAlign::new/align` and `MsIcpParams`
 * binds exactly these symbols (INTEGRATION.md shows the `extern "C"` block).
 *
 * Conventions
 *  - plain pointers and sizes only; all structs are POD with fixed-width members;
 *  - every function returns an a3d_status; nothing throws or aborts across the boundary.  Where the
 *    reference panics (`expect`, `unwrap`) the status says why and the shim re-raises;
 *  - "host" pointers are ordinary process memory, "device" pointers are HIP device memory of the
 *    context's GPU;
 *  - a context owns one HIP stream; calls on one context are serialised on that stream and the
 *    functions that return results to host memory synchronise it before returning.
 *  - poses are nalgebra `Isometry3<f32>` storage: translation xyz + unit quaternion (i, j, k, w)
 *    (src/transform.rs:18).
 */
#ifndef ALIGN3D_HIP_H
#define ALIGN3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A3D_ABI_VERSION 1
/* a3d_point_cloud_render_device: the largest half-width, in pixels, of a row's footprint (at most 17 x 17 per row). */
#define A3D_RENDER_MAX_HALF_WIDTH 8

typedef enum a3d_status {
  A3D_OK = 0,
  /* MultiscaleAlign::new length mismatch (src/icp/multiscale.rs:30-34) and any malformed argument. */
  A3D_INVALID_PARAMETER = 1,
  /* target without intensity map / normals, source without intensities (src/icp/image_icp.rs:44-57),
     point cloud without normals (src/icp/pcl_icp.rs:50-58): the reference `expect`s. */
  A3D_MISSING_FIELD = 2,
  /* GaussNewton::solve() == None (count == 0 or Cholesky failed; src/optim/gaussnewton.rs:84-93):
     the reference `unwrap`s (src/icp/image_icp.rs:152, src/icp/pcl_icp.rs:96). */
  A3D_SOLVE_FAILED = 3,
  /* any HIP runtime failure, including "no device"; a3d_last_error() has the text. */
  A3D_HIP_ERROR = 4,
  /* NaN coordinate while building the kd-tree (partial_cmp().unwrap(), src/kdtree.rs:43). */
  A3D_NAN_IN_INPUT = 5,
  /* bilateral slice result not representable as u16 (num::cast().unwrap(), src/bilateral/grid.rs:129). */
  A3D_CAST_OVERFLOW = 6
} a3d_status;

/* IcpParams (src/icp/icp_params.rs:8-23), field for field. */
typedef struct a3d_icp_params {
  uint64_t max_iterations;
  float weight;
  float color_weight;
  float max_point_to_plane_distance; /* never read by the reference either */
  float max_distance;
  float max_normal_angle;
  float max_color_distance;
} a3d_icp_params;

/* Transform = Isometry3<f32> (src/transform.rs:18). */
typedef struct a3d_pose {
  float t[3];
  float q[4]; /* i, j, k, w */
} a3d_pose;

/* Borrowed view of a RangeImage (src/range_image/structure.rs:20-36) exactly as the Rust struct
 * holds it in standard layout, so a shim passes `as_ptr()` with no copies.  Host pointers. */
typedef struct a3d_range_image_view {
  const float* points;        /* [height][width][3], 12-byte stride (Array2<Vector3<f32>>) */
  const uint8_t* mask;        /* [height][width] */
  const float* normals;       /* [height][width][3] or NULL (Option) */
  const uint8_t* intensities; /* [height*width] or NULL (Option) */
  const float* intensity_map; /* [(height+2)][(width+2)] or NULL (IntensityMap.map, src/intensity_map.rs:8) */
  double fx, fy, cx, cy;      /* CameraIntrinsics (src/camera.rs:7-20); cast to f32 at use */
  uint64_t width, height;     /* array dims (the reference never reads intrinsics.width/height on this path) */
} a3d_range_image_view;

/* Borrowed view of a PointCloud (src/pointcloud.rs:8-12). Host pointers. */
typedef struct a3d_point_cloud_view {
  const float* points;  /* [len][3] */
  const float* normals; /* [len][3] or NULL */
  uint64_t len;
} a3d_point_cloud_view;

/* One GaussNewton<6> accumulator as read back for tests (src/optim/gaussnewton.rs:9-14). */
typedef struct a3d_gn_state {
  float hessian[36]; /* row-major 6x6, both triangles filled */
  float gradient[6];
  float squared_residual_sum;
  uint64_t count;
} a3d_gn_state;

/* RangeImageBuilder (src/range_image/builder.rs:7-14). */
typedef struct a3d_builder_params {
  uint32_t with_normals;     /* RangeImage::compute_normals on level 0 */
  uint32_t with_intensity;   /* compute_intensity + compute_intensity_map on every level */
  uint32_t use_bilateral;    /* with_bilateral_filter(Some(BilateralFilter::new(sigma_space, sigma_color))) */
  uint32_t pad;
  double sigma_space, sigma_color;
  uint64_t pyramid_levels;
  float blur_sigma;
  uint32_t pad2;
} a3d_builder_params;

typedef struct a3d_context a3d_context;
typedef struct a3d_device_image a3d_device_image;       /* one RangeImage resident in HBM */
typedef struct a3d_multiscale a3d_multiscale;           /* MultiscaleAlign */
typedef struct a3d_multiscale_batch a3d_multiscale_batch; /* P independent MultiscaleAlign jobs */
typedef struct a3d_multi_context a3d_multi_context;     /* one a3d_context per device of a device list */
typedef struct a3d_multiscale_multi_batch a3d_multiscale_multi_batch; /* P MultiscaleAlign jobs over several GPUs */
typedef struct a3d_kdtree a3d_kdtree;                   /* R3dTree */
typedef struct a3d_pcl_icp a3d_pcl_icp;                 /* Icp */
typedef struct a3d_pcl_icp_batch a3d_pcl_icp_batch;     /* P independent Icp jobs over resident clouds */

/* ---- library / context -------------------------------------------------------------------
 * Threading: a context owns one HIP stream, its scratch regions, the pool of pyramid arenas and the cached
 * single-pair ICP engine; calls that take the same context (directly or through a handle created on it) must not
 * run concurrently.  Different contexts, also on the same GPU, may be used from different threads at the same time
 * (this is how frame builds overlap alignments); freeing an image from another thread than the one using its
 * context is allowed.  The reference's objects are re-entrant because they borrow host memory; here a thread that
 * wants its own concurrent `align` creates its own context.  Results are complete when a call returns, except
 * a3d_multiscale_batch_align with no host outputs, which only enqueues (a3d_context_synchronize waits).
 * Lifetime of images: the objects that read images (a3d_multiscale, a3d_multiscale_batch) borrow them like the
 * reference's `&'a Vec<RangeImage>`; an image must not be freed while a host-synchronous call on it is running.
 * After an enqueue-only batch_align the images MAY be freed right away: a3d_range_image_free waits for the batch's
 * launches (also when batch and image live on different contexts / streams) before the memory is recycled.
 * Lifetime of contexts: every handle created on a context (a3d_multiscale, batches, kd-trees, Icp objects) must be
 * freed before a3d_context_destroy.  Images are the exception — they are data and tend to outlive the code that made
 * them: a3d_context_destroy with images of that context still alive waits for the context's work, refuses new work
 * on it, and the context's memory (the pyramid arenas those images live in, its streams) is released when the last
 * such image is freed; a3d_range_image_free on them stays valid. */

uint32_t a3d_abi_version(void);
/* HIP devices visible to the process (0 without a GPU): the device list a3d_multi_context_create is given. */
a3d_status a3d_device_count(int32_t* out_count);
/* Text of the most recent failure on the calling thread ("" if none). */
const char* a3d_last_error(void);
const char* a3d_status_string(a3d_status s);

/* Binds HIP device `device_index`, creates the context's stream. A3D_HIP_ERROR if there is no GPU. */
a3d_status a3d_context_create(int32_t device_index, a3d_context** out_ctx);
/* The same with a stream priority: < 0 the device's highest, 0 the default, > 0 its lowest.  A frame-builder context
 * that shares the GPU with a batch alignment wants the highest: its many short kernels are then dispatched ahead of
 * the alignment's long ones instead of queueing behind them (the build is the dependent chain of the two). */
a3d_status a3d_context_create_with_priority(int32_t device_index, int32_t priority, a3d_context** out_ctx);
/* How the ICP pixel pass of the alignments created on `ctx` is cut into blocks (no reference counterpart: the
 * reference's own sums depend on the order rayon delivers its 75 chunks in, src/icp/image_icp.rs:96,143-148).
 *   tiles_per_pair == 0 (default): throughput tiling — the number of blocks a (pair, level) is cut into follows the
 *     batch size, so that every batch fills the chip; the f32 sums of a pair are then associated differently in a
 *     batch of 64, a batch of 32 and alone, and its pose can differ in the last bits (more where the reference's
 *     parameters are not contractive).
 *   tiles_per_pair  > 0: pinned tiling — every pair's level is cut into that many blocks (fewer when the level is
 *     small), from the pair's OWN size: a pair's pose is bit-identical alone, in any batch, at any position of a
 *     batch, next to images of other sizes, on one stream group or three.  24 is what the throughput tiling gives a
 *     64-pair batch of 640x480 images at level 0, so a 64-pair batch loses nothing at level 0; small batches lose
 *     parallelism (a lone pair runs on 24 blocks instead of ~120).
 * Takes effect for batches created or re-bound and single alignments started after the call. */
a3d_status a3d_context_set_tiling(a3d_context* ctx, uint32_t tiles_per_pair);
/* The same, naming which of the context's four streams (created in order: consecutive hardware queues, i.e. compute pipes
 * 0..3 when the process's streams are created by this library context by context) is its main stream; -1 = the default
 * order of a3d_context_create_with_priority.  For a SECOND aligning context on one GPU (alignments in flight on separate
 * streams, align3d_amd/odometry.py): main_slot 1 or 2 keeps its launch chain off the first context's pipe. */
a3d_status a3d_context_create_on_pipe(int32_t device_index, int32_t priority, int32_t main_slot, a3d_context** out_ctx);
/* An aligning context and the builder context (highest priority) that feeds it, created back to back.  Which compute
 * pipe of the GPU a HIP stream lands on follows the order in which the process creates its streams, and a pipe
 * dispatches one big grid at a time: created as a pair, the builder's kernel stream sits on the pipe of the aligner's
 * idle copy stream, beside (not behind) the three streams a batch alignment's pair groups run on.  Created at
 * unrelated moments, it lands wherever the process's stream count happens to point (measured: 11 k instead of 14 k
 * frame pairs/s in the streaming loop).  Destroy both with a3d_context_destroy. */
a3d_status a3d_context_create_pair(int32_t device_index, a3d_context** out_aligner, a3d_context** out_builder);
/* Waits for the context's work and releases its streams and scratch regions.  Every other handle created on the context
 * must have been freed.  Images may still be alive ("Lifetime of contexts" above): the context then only refuses new
 * work, and its pyramid arenas and streams go when the last of those images is freed. */
a3d_status a3d_context_destroy(a3d_context* ctx);
a3d_status a3d_context_synchronize(a3d_context* ctx);
/* The context's hipStream_t, for callers that want to order their own work after ours. */
void* a3d_context_stream(a3d_context* ctx);
/* The HIP device the context was created on (-1 for a null context): what a rank of a multi-process job checks against
 * its LOCAL_RANK before it does any work (bench.py). */
int32_t a3d_context_device(a3d_context* ctx);
/* The compute units of that device (0 for a null context): the number the launch geometries are sized by (one block per
 * CU for Icp and IcpBatch), which a test needs to say how many blocks a pass is cut into. */
int32_t a3d_context_num_cus(a3d_context* ctx);

/* hipEvent pair on the context stream: start, ..., stop -> elapsed milliseconds (stop synchronises). */
a3d_status a3d_timer_start(a3d_context* ctx);
a3d_status a3d_timer_stop(a3d_context* ctx, float* out_ms);

/* Raw device memory on the context's GPU (bench / tests keep inputs resident with these). */
a3d_status a3d_malloc(a3d_context* ctx, size_t bytes, void** out_device_ptr);
a3d_status a3d_free(a3d_context* ctx, void* device_ptr);
/* Page-locked host memory (hipHostMalloc): frames handed to a3d_range_image_build_pyramid from such a buffer are
 * copied by DMA at the PCIe rate instead of through the runtime's pageable staging path. */
a3d_status a3d_host_alloc(a3d_context* ctx, size_t bytes, void** out_host_ptr);
a3d_status a3d_host_free(a3d_context* ctx, void* host_ptr);
a3d_status a3d_memcpy_h2d(a3d_context* ctx, void* dst_device, const void* src_host, size_t bytes);
a3d_status a3d_memcpy_d2h(a3d_context* ctx, void* dst_host, const void* src_device, size_t bytes);
a3d_status a3d_memcpy_d2d(a3d_context* ctx, void* dst_device, const void* src_device, size_t bytes);

/* ---- parameters (host only, no GPU needed) ---------------------------------------------- */

/* IcpParams::default() (src/icp/icp_params.rs:33-43). */
void a3d_icp_params_default(a3d_icp_params* out);
/* MsIcpParams::default() (src/icp/icp_params.rs:112-133): writes 3 entries, index 0 = finest level. */
void a3d_ms_icp_params_default(a3d_icp_params out[3]);

/* ---- range images resident on the device ------------------------------------------------- */

/* Copies a RangeImage into HBM in the kernels' layout.  `view->normals`, `intensities`,
 * `intensity_map` may be NULL; what is missing only matters to the call that needs it. */
a3d_status a3d_range_image_upload(a3d_context* ctx, const a3d_range_image_view* view,
                                  a3d_device_image** out_image);
/* The same for a whole pyramid (`&[RangeImage]` as MultiscaleAlign::align receives it, src/icp/multiscale.rs:51):
 * `n_levels` views -> `n_levels` resident images that share ONE arena from the context's pool, one asynchronous copy
 * per array straight from the caller's memory (DMA when it is page-locked, a3d_host_alloc), one synchronisation.
 * A steady stream of upload / align / free calls allocates nothing.  Free each image with a3d_range_image_free. */
a3d_status a3d_range_image_upload_pyramid(a3d_context* ctx, const a3d_range_image_view* views, uint64_t n_levels,
                                          a3d_device_image** out_images);
a3d_status a3d_range_image_free(a3d_device_image* image);

/* RangeImage::compute_normals (src/range_image/structure.rs:184-262) on a resident image;
 * afterwards the image "has normals". */
a3d_status a3d_range_image_compute_normals(a3d_device_image* image);
/* Reads the resident normals back: [height][width][3] f32. */
a3d_status a3d_range_image_download_normals(a3d_device_image* image, float* out_normals);

/* RangeImageBuilder::default() (src/range_image/builder.rs:16-26): normals, intensity, no bilateral
 * filter, 3 levels, blur sigma 1; the sigmas are BilateralFilter::default()'s. */
void a3d_builder_params_default(a3d_builder_params* out);
/* RangeImageBuilder::build(frame) (src/range_image/builder.rs:74-91) on the device: depth u16 [h][w] and
 * rgb u8 [h][w][3] come from host memory, every level of the pyramid stays resident.  out_levels receives
 * params->pyramid_levels handles (index 0 = full resolution); free each with a3d_range_image_free.
 * The pyramid's RGB blur restates image-0.24.7's imageops::blur (parity unpinned). */
a3d_status a3d_range_image_build_pyramid(a3d_context* ctx, const a3d_builder_params* params,
                                         const uint16_t* depth, const uint8_t* rgb, uint64_t width,
                                         uint64_t height, double fx, double fy, double cx, double cy,
                                         double depth_scale, a3d_device_image** out_levels);
/* The same for n_frames frames of one stream (same size, intrinsics and depth scale) in ONE launch sequence: every
 * kernel of the builder has a frame dimension, so up to 48 frames cost the 10 launches one frame costs (a frame stream is
 * launch-bound otherwise).  depth_frames / rgb_frames: n_frames host pointers (page-locked buffers from a3d_host_alloc
 * are copied by DMA).  out_levels: [n_frames][params->pyramid_levels] handles, frame-major.  All or nothing: on
 * failure no handle is returned.  The call returns when every pyramid is complete. */
a3d_status a3d_range_image_build_pyramids(a3d_context* ctx, const a3d_builder_params* params, uint64_t n_frames,
                                          const uint16_t* const* depth_frames, const uint8_t* const* rgb_frames,
                                          uint64_t width, uint64_t height, double fx, double fy, double cx, double cy,
                                          double depth_scale, a3d_device_image** out_levels);
/* Instrumentation for the roofline of the frame builder: what the most recent a3d_range_image_build_pyramids call on
 * this context processed — out_stats = {frames, cells of their bilateral grids (GH x GW x GD, src/bilateral/grid.rs:37-56),
 * 12^3-cell blur tiles the splat marked, first-channel tiles written as zeros}. */
a3d_status a3d_context_last_build_stats(a3d_context* ctx, uint64_t out_stats[4]);
/* Instrumentation: when on, every chunk (up to 48 frames) of a3d_range_image_build_pyramids is bracketed by a hipEvent
 * pair on the context's stream, recorded behind the wait for the chunk's upload: a3d_context_last_build_kernel_ms is the
 * sum of those brackets for the most recent build — the device time of the builder's kernels without the PCIe copies
 * (a live figure for the builder's roofline; rocprofv3 --kernel-trace shows the same kernels one by one). */
a3d_status a3d_context_set_build_profiling(a3d_context* ctx, int32_t on);
a3d_status a3d_context_last_build_kernel_ms(a3d_context* ctx, float* out_ms);
a3d_status a3d_range_image_size(const a3d_device_image* image, uint64_t* out_width, uint64_t* out_height);
/* Reads resident arrays back (each pointer nullable): points [h][w][3], mask [h][w], normals [h][w][3],
 * intensities [h*w], intensity_map [(h+2)][(w+2)], colors [h][w][3] u8, intrinsics fx fy cx cy. */
a3d_status a3d_range_image_download(a3d_device_image* image, float* points, uint8_t* mask, float* normals,
                                    uint8_t* intensities, float* intensity_map, uint8_t* colors,
                                    double out_intrinsics[4]);

/* RangeImage::compute_normals (src/range_image/structure.rs:184-262) on n resident images of one size and one context
 * in ONE launch per 64 images; enqueue-only like a3d_range_image_compute_normals (results are ordered on the context's
 * stream; a3d_range_image_download_normals / a3d_context_synchronize wait).  An odometry or mapping host that keeps its
 * range images resident recomputes the normals of a whole window of frames at the stencil's HBM rate instead of paying
 * one launch per frame. */
a3d_status a3d_range_image_compute_normals_batch(a3d_device_image* const* images, uint64_t n);

/* PointCloud::from(&RangeImage) (src/range_image/structure.rs:375-406): mask != 0, row-major.  d_points / d_normals:
 * DEVICE [capacity][3] f32 on the image's GPU (d_normals may be NULL; A3D_MISSING_FIELD if it is not and the image has
 * no normals).  Points and normals are copied bit for bit.  Host-synchronous; *out_len = number of points written.
 * capacity >= width * height is always enough; a smaller one that the cloud does not fit gives A3D_INVALID_PARAMETER,
 * *out_len = the point count, and nothing written.  The result is an a3d_point_cloud_view of device pointers for
 * a3d_pcl_icp_new_device / a3d_pcl_icp_align_device / a3d_kdtree_new_device. */
a3d_status a3d_range_image_to_point_cloud(const a3d_device_image* image, float* d_points, float* d_normals,
                                          uint64_t capacity, uint64_t* out_len);
/* The same for n images of one context in one pass (structure.rs:375-406 for each): per-image output pointers and
 * capacities (d_normals may be NULL, or hold NULL entries), lengths into out_lens[n].  If any image does not fit its
 * capacity, A3D_INVALID_PARAMETER and nothing is written for any image (out_lens still holds every count).  n == 0:
 * A3D_OK, nothing touched. */
a3d_status a3d_range_image_to_point_clouds(const a3d_device_image* const* images, uint64_t n, float* const* d_points,
                                           float* const* d_normals, const uint64_t* capacities, uint64_t* out_lens);
/* Whether the resident image carries normals (RangeImage::normals is Some): 1 or 0.  No device work. */
a3d_status a3d_range_image_has_normals(const a3d_device_image* image, int32_t* out_has_normals);
/* Whether the resident image carries colours (RangeImage::colors is Some: every builder image, and an uploaded one after
 * a3d_range_image_set_colors): 1 or 0.  No device work. */
a3d_status a3d_range_image_has_colors(const a3d_device_image* image, int32_t* out_has_colors);
/* a3d_range_image_to_point_clouds with the colours of the kept pixels (structure.rs:392-398: the same mask as the points).
 * d_colors: NULL (then this is a3d_range_image_to_point_clouds), or n entries of which each is NULL (no colours written
 * for that image) or a DEVICE buffer of capacities[i] rows of [3] u8, RGB: row k is the colour of the k-th pixel with
 * mask != 0 in row-major order, byte for byte; no byte at or past 3 * out_lens[i] is written.  A non-NULL entry for an
 * image without colours is A3D_MISSING_FIELD, decided for the whole batch before anything is launched, as for normals.
 * Points, normals, the capacity rule (all or nothing) and the two launches are those of the entry above. */
a3d_status a3d_range_image_to_point_clouds_rgb(const a3d_device_image* const* images, uint64_t n, float* const* d_points,
                                               float* const* d_normals, uint8_t* const* d_colors,
                                               const uint64_t* capacities, uint64_t* out_lens);

/* RangeImage::colors = Some(..) (src/range_image/structure.rs:20-36): host rgb [h][w][3] u8 -> the resident image's
 * colours, in an allocation of their own that is freed with the image.  Host-synchronous.  An image that already has
 * colours (every builder image) gives A3D_INVALID_PARAMETER. */
a3d_status a3d_range_image_set_colors(a3d_device_image* image, const uint8_t* rgb);
/* RangeImage::compute_intensity + compute_intensity_map (src/range_image/structure.rs:266-297) in place on n resident
 * images of one context; their sizes may differ (one launch for the batch).  Enqueue-only like
 * a3d_range_image_compute_normals_batch.  An image without colours gives A3D_MISSING_FIELD (nothing is enqueued for any
 * image); an image without intensities or a map gets them in allocations of their own.  n == 0: A3D_OK. */
a3d_status a3d_range_image_compute_intensity(a3d_device_image* const* images, uint64_t n);
/* RangeImage::pyramid(levels, sigma) (src/range_image/structure.rs:309-351) for n resident images of one context and one
 * size.  out_levels[n][levels - 1] receives NEW handles for levels 1 .. levels - 1, image-major (level 0 is the caller's
 * image and is not copied); the coarser levels of one image share one pooled arena.  Points and mask are picked from the
 * source pixels with mask == 1, normals only if level 0 has normals, colours blurred and halved only if it has colours,
 * intrinsics scaled by 0.5 per level.  with_intensity != 0: intensities and map on EVERY level, level 0 in place (the
 * builder's semantics, builder.rs:83-88); A3D_MISSING_FIELD without colours.  The builder's limits: levels in
 * 1 .. 16, a coarsest side of at least 2, a finite sigma, sigma <= 3 when levels > 1; sigma <= 0 means 1.  Mixed
 * contexts or sizes and null handles: A3D_INVALID_PARAMETER.  All or nothing: on failure no handle is returned and
 * level 0 is untouched.  Host-synchronous: every pyramid is complete on return.  n == 0: A3D_OK, nothing touched. */
a3d_status a3d_range_image_pyramids(const a3d_device_image* const* level0, uint64_t n, uint64_t levels, float blur_sigma,
                                    uint32_t with_intensity, a3d_device_image** out_levels);

/* RangeImage::compute_normals, host in / host out convenience form. */
a3d_status a3d_compute_normals(a3d_context* ctx, const float* points, const uint8_t* mask,
                               uint64_t width, uint64_t height, float* out_normals);

/* ---- ImageIcp (src/icp/image_icp.rs:19-165) ---------------------------------------------- */

/* ImageIcp::new(params, target) + initial_transform + align(source): all iterations run on the
 * device; returns best_transform.  init_pose NULL = Transform::eye().  Target and source may differ in size and
 * intrinsics: the loop runs over the source's pixels, and only the target's intrinsics and size enter the projection
 * and its bounds test (image_icp.rs:107-109). */
a3d_status a3d_image_icp_align(a3d_context* ctx, const a3d_icp_params* params,
                               const a3d_device_image* target, const a3d_device_image* source,
                               const a3d_pose* init_pose, a3d_pose* out_pose);

/* One pass of the per-pixel body (src/icp/image_icp.rs:101-139) from `pose`, returning the two
 * merged accumulators before add_weighted (the state GaussNewton holds at image_icp.rs:148).  Used for per-iteration
 * parity and by bench.py's live-pixel count. */
a3d_status a3d_image_icp_accumulate(a3d_context* ctx, const a3d_icp_params* params,
                                    const a3d_device_image* target, const a3d_device_image* source,
                                    const a3d_pose* pose, a3d_gn_state* out_geom,
                                    a3d_gn_state* out_color);

#ifdef A3D_DIAGNOSTICS /* exported by the diagnostics build only (csrc/Makefile `diag`: libalign3d_hip_diag.so) */
/* a3d_image_icp_accumulate through a cross-check kernel in which EVERY per-pixel value — the Jacobians
 * (src/icp/cost_function.rs:33-57), CameraIntrinsics::project_grad (src/camera.rs:82-89) and the products of
 * GaussNewton::step (src/optim/gaussnewton.rs:47-77) — is computed with the reference's own unfused operations and
 * IEEE divisions; only the order of the additions differs.  The product kernel fuses those (they only feed the sums). */
a3d_status a3d_image_icp_accumulate_exact(a3d_context* ctx, const a3d_icp_params* params, const a3d_device_image* target,
                                          const a3d_device_image* source, const a3d_pose* pose,
                                          a3d_gn_state* out_geom, a3d_gn_state* out_color);
/* The same pass through the opt-in merged-accumulator kernel (A3D_ICP_ACCUM=merged: a thread sums
 * geom.add_weighted(color, weight, color_weight) (src/optim/gaussnewton.rs:115-121) directly, from the weighted
 * Jacobians), returning that merged accumulator: H, g, the weighted residual sum and the combined count.  Test hook. */
a3d_status a3d_image_icp_accumulate_weighted(a3d_context* ctx, const a3d_icp_params* params,
                                             const a3d_device_image* target, const a3d_device_image* source,
                                             const a3d_pose* pose, a3d_gn_state* out_state);
/* Level 0 of a device-built pyramid: the u16 depth plane its points were back-projected from (width * height, 0 =
 * invalid), the f32 back-projection constants {fx, fy, cx, cy, depth scale} and whether the image carries
 * points_from_depth (the alignment kernel then rebuilds level-0 points from the plane).  A3D_MISSING_FIELD for any other
 * image.  Test hook. */
a3d_status a3d_range_image_download_depth16(a3d_device_image* image, uint16_t* out_depth, float out_backproject[5],
                                            int32_t* out_points_from_depth);
/* Whether the image ICP kernel may rebuild the points of a width x height depth image back-projected with {fx, fy, cx, cy,
 * depth scale} in straight-line code: the host proof the alignment applies to every level-0 image before it takes its
 * depth plane (1 = proven, 0 = its points are read).  No device work.  Test hook. */
a3d_status a3d_backproject_proven(uint32_t width, uint32_t height, const float backproject[5], int32_t* out_proven);
/* Whether that kernel may also divide by the image's two focal lengths in three operations (q = a y, r = fma(-f, q, a),
 * q + r y with y = RN(1 / f)) instead of five: a3d_backproject_proven and, for fx and for fy, the exhaustive sweep over
 * the 2^23 mantissas of the numerator that the alignment runs once per focal length and context (1 = every quotient is
 * the IEEE one).  Tens of milliseconds per focal length, no device work.  Test hook. */
a3d_status a3d_backproject_short_division_proven(uint32_t width, uint32_t height, const float backproject[5],
                                                 int32_t* out_proven);
/* The dot-product cut that stands in for the reference's normal-angle gate: a correspondence whose dot product d
 * satisfies -1 <= d <= *out is rejected, which is |acos(d)| > thr when `strict` (point-cloud ICP) and |acos(d)| >= thr
 * otherwise (image ICP).  The host bisection the ICP launches use.  No device work.  Test hook. */
a3d_status a3d_acos_gate_threshold(float thr, int32_t strict, float* out);
#endif /* A3D_DIAGNOSTICS */

/* ---- instrumentation that SHIPS in the product library -------------------------------------------------------
 * The four entry points below (a3d_image_icp_align_trace, a3d_selftest_transform, a3d_selftest_division and, further
 * down, a3d_multiscale_batch_persistent_levels) and the timing getters (…_last_kernel_ms, …_last_level_ms, …_last_timing,
 * a3d_context_last_build_*) have no reference counterpart.  They are part of the product library on purpose: they run or
 * time the PRODUCT's own device functions (the iteration tail's pose arithmetic, the shared-reciprocal division, the
 * launches of an alignment), so the parity tests and bench.py check and time the code that ships — no second kernel sits
 * behind any of them.  What only exists to cross-check the product (exact-arithmetic accumulate, merged accumulators,
 * every A3D_* environment knob and the kernel variants behind them) is compiled into the diagnostics build alone
 * (#ifdef A3D_DIAGNOSTICS above). */
/* Instrumentation (no reference counterpart): a3d_image_icp_align that also writes, per iteration,
 * [residual, t(3), q_ijkw(4)] of the transform after that iteration's update; out_trace holds
 * 8 * params->max_iterations floats. */
a3d_status a3d_image_icp_align_trace(a3d_context* ctx, const a3d_icp_params* params,
                                     const a3d_device_image* target, const a3d_device_image* source,
                                     const a3d_pose* init_pose, a3d_pose* out_pose, float* out_trace);

/* Instrumentation: the pose arithmetic of the iteration tail run ON THE DEVICE for n items (host arrays in and out):
 *   out_composed[i] = Transform::exp(&LieGroup::Se3(updates6[i])) * poses[i]   (src/transform.rs:44-108, 205-220;
 *                     poses == NULL: identity), evaluated by the very device functions the ICP kernels' tail calls
 *                     (minimax sin / cos up to theta = pi/4, libm above; the theta^2 < 1e-16 Taylor branch);
 *   out_points3[i]  = Transform::transform_vector(out_composed[i], points3[i])  (src/transform.rs:138-145);
 *   out_normals3[i] = Transform::transform_normal(out_composed[i], points3[i])  (src/transform.rs:147-153).
 * Lets the reference's own known answers (src/transform.rs:321-411) be checked against the device code. */
a3d_status a3d_selftest_transform(a3d_context* ctx, const float* updates6, const a3d_pose* poses, const float* points3,
                                  uint64_t n, a3d_pose* out_composed, float* out_points3, float* out_normals3);
/* Instrumentation: the ICP kernels divide with a reciprocal shared between the quotients of one pixel
 * (same arithmetic as a correctly rounded f32 division); this runs that routine on n caller-drawn
 * (numerator, denominator) pairs on the device and counts results that differ from IEEE `/`. */
a3d_status a3d_selftest_division(a3d_context* ctx, const float* numerators, const float* denominators,
                                 uint64_t n, uint64_t* out_mismatches);
/* Instrumentation: fills every byte of the context's memory that is idle between calls with `byte` (0 .. 255), so a test
 * can show that a result does not depend on what an earlier call left there.  Host-synchronous: waits for the context's
 * stream, copy stream and side streams, then fills each allocated scratch region over its whole size, every pooled image
 * arena (slab slices included) and every spare kd-tree / Icp block, and forgets that the bilateral grid region is
 * clean, as a growth of that region does.  Live images, cached tables, voxel maps, trees and whatever else a handle
 * owns are not touched.  The contents of that memory between calls are unspecified anyway (growth discards them).
 * Not thread-safe against the context: the regions and the grid key are changed with no lock held, so no other call on
 * this context may run at the same time (image and handle frees from other threads, which take the pool's lock, may).
 * out_bytes: the bytes filled, [0..5] the scratch regions, [6] pooled arenas, [7] spare blocks. */
a3d_status a3d_selftest_fill_scratch(a3d_context* ctx, uint32_t byte, uint64_t out_bytes[8]);

/* ---- MultiscaleAlign (src/icp/multiscale.rs:7-68) ---------------------------------------- */

/* MultiscaleAlign::new(params, &target_pyramid): A3D_INVALID_PARAMETER unless
 * n_params == n_levels (multiscale.rs:30-34).  Index 0 = finest level.  Borrows the images. */
a3d_status a3d_multiscale_new(a3d_context* ctx, const a3d_icp_params* params, uint64_t n_params,
                              const a3d_device_image* const* target_pyramid, uint64_t n_levels,
                              a3d_multiscale** out);
/* MultiscaleAlign::align(&source_pyramid): coarsest level first, each level starts from the
 * previous level's result; a shorter source pyramid truncates like izip! (multiscale.rs:54-64).  A source level may
 * differ from its target level in size and intrinsics; only the target's enter the projection (image_icp.rs:107-109). */
a3d_status a3d_multiscale_align(a3d_multiscale* ms, const a3d_device_image* const* source_pyramid,
                                uint64_t n_source_levels, a3d_pose* out_pose);
/* The same with the source pyramid as the reference holds it: `&[RangeImage]` in HOST memory (src/icp/multiscale.rs:51).
 * One call uploads and aligns: the arrays go up on the context's copy stream, coarsest level first, and the launches of
 * a level wait for that level's arrays only, so the coarse levels iterate under the upload of the fine ones (0.65 against
 * 0.84 ms for upload-then-align at 640x480, 3 levels x 15 iterations, page-locked arrays).  Nothing stays resident.
 * At most 16 levels (A3D_INVALID_PARAMETER beyond — a 17-level pyramid needs an image side of 2^17 pixels; a3d_multiscale_align
 * over resident images has no such limit). */
a3d_status a3d_multiscale_align_host(a3d_multiscale* ms, const a3d_range_image_view* source_pyramid,
                                     uint64_t n_source_levels, a3d_pose* out_pose);
a3d_status a3d_multiscale_free(a3d_multiscale* ms);

/* P independent MultiscaleAlign::new(params, target_p).align(source_p) jobs run as one launch
 * sequence (grid = pairs x tiles).  target/source are [n_pairs][n_levels] row-major handle tables.  Sizes and
 * intrinsics may differ between pairs and, inside a pair, between target and source: only the target's enter the
 * projection (image_icp.rs:107-109); the source's own width and back-projection constants serve its pixel loop. */
a3d_status a3d_multiscale_batch_new(a3d_context* ctx, const a3d_icp_params* params,
                                    uint64_t n_params, uint64_t n_pairs, uint64_t n_levels,
                                    const a3d_device_image* const* target_pyramids,
                                    const a3d_device_image* const* source_pyramids,
                                    a3d_multiscale_batch** out);
/* Runs every pair.  out_poses_host: [n_pairs] or NULL.  out_matrices_device: [n_pairs][16] f32
 * row-major 4x4 in device memory (the buffer the RCCL gather sends) or NULL.
 * out_status_host: per-pair A3D_OK / A3D_SOLVE_FAILED, [n_pairs] or NULL.  With
 * out_poses_host == NULL and out_status_host == NULL the call only enqueues (no host sync). */
a3d_status a3d_multiscale_batch_align(a3d_multiscale_batch* batch, a3d_pose* out_poses_host,
                                      float* out_matrices_device, int32_t* out_status_host);
/* Results of the most recent pass of `batch` (the way to read an enqueue-only batch_align): host-synchronous, but
 * waits for that pass only, not for work enqueued on the context since (another batch's pass: two batches
 * alternating over a stream of rounds keep the GPU busy while the host reads the previous round). */
a3d_status a3d_multiscale_batch_results(a3d_multiscale_batch* batch, a3d_pose* out_poses_host, int32_t* out_status_host);
/* Points an existing batch at other pyramids (same pair and level counts, same layout as _new): the next
 * batch_align runs on them.  A stream of batches reuses one object and allocates nothing per batch.  Waits for this
 * batch's own earlier passes only. */
a3d_status a3d_multiscale_batch_rebind(a3d_multiscale_batch* batch, const a3d_device_image* const* target_pyramids,
                                       const a3d_device_image* const* source_pyramids);
a3d_status a3d_multiscale_batch_free(a3d_multiscale_batch* batch);
/* Instrumentation: when on, every launch of the per-pixel kernel is bracketed by its own hipEvent pair
 * on the stream it is launched on, and a3d_multiscale_batch_last_kernel_ms returns the sum of those durations
 * for the most recent batch_align (divide by the launch count for the average launch).  A batch splits its
 * pairs into a3d_multiscale_batch_concurrency() groups whose launches run on separate HIP streams at the same
 * time, so that sum can exceed the wall time reported by a3d_multiscale_batch_last_timing. */
a3d_status a3d_multiscale_batch_set_profiling(a3d_multiscale_batch* batch, int32_t on);
a3d_status a3d_multiscale_batch_last_kernel_ms(a3d_multiscale_batch* batch, float* out_kernel_ms);
/* The same sum for one pyramid level.  Levels that ran inside the persistent kernel (one launch per stream group
 * for all their iterations) are timed by that kernel's own clock stamps: per group, from the first pair entering the
 * level to the last pair leaving it; their `launches` are iterations x groups. */
a3d_status a3d_multiscale_batch_last_level_ms(a3d_multiscale_batch* batch, uint32_t level, float* out_ms,
                                              uint32_t* out_launches);
/* Which levels the most recent batch_align ran inside the persistent kernel (bit l = level l): always 0 in the product
 * library (the persistent kernel is a diagnostics-build variant, measured slower); see "instrumentation that ships". */
a3d_status a3d_multiscale_batch_persistent_levels(a3d_multiscale_batch* batch, uint32_t* out_mask);
a3d_status a3d_multiscale_batch_concurrency(a3d_multiscale_batch* batch, uint32_t* out_streams);
/* Time of the most recent batch_align on the device, between hipEvents recorded on the context
 * stream around its launches, and the share of it spent in the per-pixel kernel (sum of that
 * kernel's launches / number of launches). */
a3d_status a3d_multiscale_batch_last_timing(a3d_multiscale_batch* batch, float* out_total_ms,
                                            uint64_t* out_pixel_kernel_launches);

/* ---- P independent MultiscaleAlign jobs over a device list (one host process, several GPUs) ---------------
 * The path shards over independent frame pairs only (no intra-pair sharding): pair j of P goes to device
 * floor(j D / P) — contiguous blocks, 512 pairs over 8 GPUs = 64 each — every device runs its block as one
 * a3d_multiscale_batch on its own context, enqueued by its own host thread, and ONE gather collects the 4x4 poses
 * (16 f32 per pair) into a buffer on the first device (device-to-device copies over xGMI).  The images of a pair
 * must be resident on the device that owns the pair: build or upload them through a3d_multi_context_device(mc, d). */

/* Block [begin, end) of n_items owned by `device` of n_devices (remainders go to the first devices).  Host only. */
a3d_status a3d_multi_shard_range(uint64_t n_items, uint64_t n_devices, uint64_t device, uint64_t* out_begin,
                                 uint64_t* out_end);
/* One context per entry of device_ids (an id may repeat: several contexts = streams on one GPU). */
a3d_status a3d_multi_context_create(const int32_t* device_ids, uint64_t n_devices, a3d_multi_context** out);
a3d_status a3d_multi_context_destroy(a3d_multi_context* mc);
uint64_t a3d_multi_context_size(const a3d_multi_context* mc);
/* The context of entry `index` (borrowed; NULL if out of range): frames of the pairs that entry owns are built on it. */
a3d_context* a3d_multi_context_device(a3d_multi_context* mc, uint64_t index);
/* MultiscaleAlign::new for every pair, as a3d_multiscale_batch_new: [n_pairs][n_levels] handle tables in global pair
 * order.  A3D_INVALID_PARAMETER if an image lives on another device than the owner of its pair. */
a3d_status a3d_multiscale_batch_new_multi(a3d_multi_context* mc, const a3d_icp_params* params, uint64_t n_params,
                                          uint64_t n_pairs, uint64_t n_levels,
                                          const a3d_device_image* const* target_pyramids,
                                          const a3d_device_image* const* source_pyramids,
                                          a3d_multiscale_multi_batch** out);
/* Runs every pair on its device and gathers.  Each output is nullable: out_poses_host [n_pairs], out_matrices_host
 * [n_pairs][16] f32 row-major 4x4, out_status_host [n_pairs], *out_matrices_device0 = the gathered [n_pairs][16]
 * buffer on the first device (owned by the batch, overwritten by the next call).  Returns when all are complete. */
a3d_status a3d_multiscale_multi_batch_align(a3d_multiscale_multi_batch* batch, a3d_pose* out_poses_host,
                                            float* out_matrices_host, int32_t* out_status_host,
                                            const float** out_matrices_device0);
a3d_status a3d_multiscale_multi_batch_free(a3d_multiscale_multi_batch* batch);

/* ---- PointCloud resident on the device (src/pointcloud.rs:8-52) ---------------------------- */

/* Both entries take views whose `points` / `normals` are DEVICE pointers on ctx's GPU ([len][3] f32) and are
 * host-synchronous like a3d_range_image_to_point_clouds: complete on return, so buffers may be freed right after.  Per
 * point the value is Transform::transform_vector / transform_normal (src/transform.rs:138-153) in the reference's own
 * operation order, bit for bit; quaternions are used as given (the reference does not validate them either).  Decided on
 * the host before anything is launched: n == 0 is A3D_OK and touches nothing; a cloud with len == 0 may have null
 * pointers and contributes nothing; a len or a batch of 2^31 points' worth of tiles or more is A3D_INVALID_PARAMETER. */

/* &Transform * &PointCloud (src/pointcloud.rs:40-52) for n resident clouds in one launch.
 * poses_host: n poses, or NULL = copy bit for bit.  d_out_normals may be NULL (no normals
 * written); an entry that is non-NULL while clouds[i].normals is NULL -> A3D_MISSING_FIELD.
 * Output i may be exactly input i (points on points, normals on normals: in place); any other overlap of an output with
 * an input or with another output is A3D_INVALID_PARAMETER. */
a3d_status a3d_point_clouds_transform_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                             const a3d_pose* poses_host, uint64_t n, float* const* d_out_points,
                                             float* const* d_out_normals);
/* The same, written back to back in cloud order then point order into one cloud:
 * cloud i starts at sum(len[0..i)).  *out_len = total.  capacity < total ->
 * A3D_INVALID_PARAMETER, *out_len = total, nothing written.  d_out_normals non-NULL requires
 * normals on every cloud with len > 0 (else A3D_MISSING_FIELD).  The output may overlap no input. */
a3d_status a3d_point_clouds_merge_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                         const a3d_pose* poses_host, uint64_t n, float* d_out_points, float* d_out_normals,
                                         uint64_t capacity, uint64_t* out_len);
/* Colours on resident clouds.  A cloud's colours are [len][3] u8, RGB (the reference's Array1<Vector3<u8>>,
 * src/pointcloud.rs:8-12), in a DEVICE buffer of their own beside points and normals.  a3d_point_cloud_view does not
 * carry them: they cross the ABI as an array of n pointers parallel to the views, where a NULL array or a NULL entry
 * means "this cloud has no colours" (inputs) or "write no colours" (outputs).  A colour is a payload: it never decides
 * which point is kept, and a pose does not touch it (&Transform * &PointCloud clones the colours, pointcloud.rs:49: copy
 * the buffer with a3d_memcpy_d2d; there is no transform entry for them).  Colour buffers need no alignment, and no entry
 * writes a byte past the rows it reports. */

/* a3d_point_clouds_merge_device with colours: the colours of cloud i start at byte 3 * sum(len[0..i)) of d_out_colors
 * (room for `capacity` rows).  A non-NULL d_out_colors requires colours on every cloud with len > 0 (else
 * A3D_MISSING_FIELD); with d_out_colors NULL, d_colors is ignored and the call is a3d_point_clouds_merge_device.  The
 * colour output may overlap no input and no other output (A3D_INVALID_PARAMETER).  One launch. */
a3d_status a3d_point_clouds_merge_rgb_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                             const uint8_t* const* d_colors, const a3d_pose* poses_host, uint64_t n,
                                             float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                             uint64_t capacity, uint64_t* out_len);

/* Voxel-grid downsampling of n resident clouds, each exactly as if it were passed alone, in a number of launches that
 * does not depend on n; host-synchronous like the two entries above.  Of the points of a cloud that share a cell of the
 * grid of pitch voxel_size anchored at origin (NULL = (0,0,0)), the one nearest to the cell's centre is kept (ties: the
 * lowest index); the kept points are written in input order and copied bit for bit, normals too.  The rule of
 * src/range_image/resize.rs:4-40 (one real sample per cell, never an average) with the cell centre in place of the cell
 * mean, which makes the result independent of the order of the points.  In f32, every operation rounded on its own:
 *   c_k = floorf((p_k - o_k) / v); the point is DROPPED unless every c_k is finite and in [-2^20, 2^20) (so NaN and
 *   infinite coordinates never reach a kd-tree build); cell key (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20);
 *   ctr_k = (c_k + 0.5f) * v + o_k, d_k = p_k - ctr_k, dist = (d_x * d_x + d_y * d_y) + d_z * d_z;
 *   the winner of a key minimises bits(dist) << 32 | index.
 * d_out_points[i]: room for capacities[i] points; d_out_normals (NULL, or NULL entries: no normals written; a non-NULL
 * entry while clouds[i].normals is NULL -> A3D_MISSING_FIELD); d_out_index (NULL, or NULL entries): the input index of
 * each kept point, capacities[i] u32.  out_lens[i] = kept points, out_dropped[i] (NULL ok) = dropped points of cloud i.
 * capacities[i] >= len_i always suffices; if any cloud's result does not fit the call returns A3D_INVALID_PARAMETER with
 * every count in out_lens (and out_dropped) and NOTHING written to any output.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx, d_clouds,
 * d_out_points, capacities or out_lens, a voxel_size that is not finite or <= 0, a non-finite origin, a cloud of 2^32
 * points or more (or within one tile, < 2^21 points, of it), any overlap of an output (its first min(len_i,
 * capacities[i]) elements) with an input or another output — there is no in-place form — are A3D_INVALID_PARAMETER.  A
 * cloud with len == 0 may have null pointers and yields out_lens[i] = 0.
 * Scratch memory (context-owned, grow-only, shared with the calls above): 16 bytes per slot of each cloud's hash table,
 * whose slot count is the smallest power of two >= 2 * len_i (so 32 to 64 bytes per point), plus len_i / 8 bytes of
 * flags, 4 bytes per 1024 points and 104 bytes per cloud. */
a3d_status a3d_point_clouds_voxel_downsample_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                    float voxel_size, const float origin[3], float* const* d_out_points,
                                                    float* const* d_out_normals, uint32_t* const* d_out_index,
                                                    const uint64_t* capacities, uint64_t* out_lens, uint64_t* out_dropped);
/* The same with colours: the kept rows' colours go out in input order beside their points, d_out_colors[i] having room for
 * capacities[i] rows of [3] u8.  The normals' rules apply: d_colors and d_out_colors may be NULL or hold NULL entries; a
 * non-NULL output for a cloud without colours is A3D_MISSING_FIELD; the colour buffers (inputs by 3 * len_i bytes, outputs
 * by 3 * min(len_i, capacities[i])) are part of the overlap check; nothing is written if any result does not fit.  Points,
 * normals, indices, counts and the launches are those of the entry above, which is this one with NULL colours. */
a3d_status a3d_point_clouds_voxel_downsample_rgb_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                                        const uint8_t* const* d_colors, uint64_t n, float voxel_size,
                                                        const float origin[3], float* const* d_out_points,
                                                        float* const* d_out_normals, uint8_t* const* d_out_colors,
                                                        uint32_t* const* d_out_index, const uint64_t* capacities,
                                                        uint64_t* out_lens, uint64_t* out_dropped);

/* Voxel-grid downsampling by cell MEAN: the sibling of the two entries above for users who expect what PCL's VoxelGrid
 * and Open3D's voxel_down_sample return, the centroid of each cell with the mean normal and the mean colour.  n resident
 * clouds, each exactly as if it were passed alone, in a number of launches that does not depend on n; host-synchronous.
 * The offsets are rounded to a lattice and summed in integers, so the result is the same bits under any permutation of a
 * cloud's rows (as a multiset of rows) and the same bits as tests/voxel_mean_restatement.py.  The rule.  All f32
 * operations are rounded on their own (correctly rounded / and sqrt), f64 operations likewise.  Per call: v = voxel_size
 * finite and > 0, a finite origin o (NULL = (0,0,0)); host constants in f32: s = 32768.0f / v and u = v / 32768.0f.
 *   1. Cell.  c_k and the cell key of a3d_point_clouds_voxel_downsample_device, unchanged.  A point it refuses is dropped
 *      and counted.
 *   2. Offsets.  ctr_k = (c_k + 0.5f) * v + o_k and d_k = p_k - ctr_k, as that entry computes them.
 *      q_k = (int) rintf(d_k * s), ties to even.  Per cell, in int64: N = sum 1 and S_k = sum q_k.  |q_k| stays near 2^14;
 *      with len < 2^32 nothing can overflow.
 *   3. Mean point.  If N == 1 the cell's only row is copied bit for bit: point, normal and colour.  Otherwise
 *      m_k = (float)((double)S_k / (double)N) and out_k = ctr_k + m_k * u, with ctr taken from the cell's representative
 *      (step 6).
 *   4. Mean normal (only when normals are written, N > 1).  A row's normal is counted iff its three components are finite
 *      and |n_k| <= 2.  r_k = (int) rintf(n_k * 1048576.0f), and T_k = sum r_k in int64 over the counted rows; each sum
 *      stays <= 2^53, so it is exact in f64.  L = sqrt((T_x*T_x + T_y*T_y) + T_z*T_z) in f64.
 *      out_n_k = L > 0 ? (float)((double)T_k / L) : 0.  A zero normal stays in the cloud: every aligner's angle gate
 *      rejects it, as after a3d_point_clouds_estimate_normals_device.
 *   5. Mean colour (only when colours are written, N > 1).  Per channel C = sum c in u64, and out_c = (2 C + N) / (2 N)
 *      in integer division, which rounds half up.
 *   6. Order, index, count.  A cell's representative is its lowest input index.  Output rows are in ascending order of
 *      representative, which is first-occurrence order.  d_out_index[i][row] is that index, strictly increasing;
 *      d_out_counts[i][row] = N as u32.
 * So out_lens, out_dropped and the set of cells are those of a3d_point_clouds_voxel_downsample_device with the same v and
 * o, a cloud whose cells are all singletons comes back bit for bit in input order, and each output coordinate differs
 * from the exact mean of its cell by at most v * 2^-15 + 2 ulp32(M), M the largest absolute input or origin coordinate.
 * The outputs, their NULL forms, capacities, A3D_MISSING_FIELD for a normals or colour output of a cloud that lacks the
 * field, and every check made on the host before anything is launched are those of
 * a3d_point_clouds_voxel_downsample_rgb_device; d_out_counts (NULL, or NULL entries: not written; capacities[i] u32) is
 * one more output of the overlap check.  If any cloud's rows do not fit its capacity the call returns
 * A3D_INVALID_PARAMETER with every count in out_lens (and out_dropped) and NOTHING written to any output.
 * Scratch memory (context-owned, grow-only, shared with the calls above): what the nearest-point entry takes, plus 20
 * bytes per point (a 16-byte record of the counting sort by cell and a 4-byte row number) and 96 bytes per 64 points. */
a3d_status a3d_point_clouds_voxel_mean_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                              const uint8_t* const* d_colors, uint64_t n, float voxel_size,
                                              const float origin[3], float* const* d_out_points,
                                              float* const* d_out_normals, uint8_t* const* d_out_colors,
                                              uint32_t* const* d_out_index, uint32_t* const* d_out_counts,
                                              const uint64_t* capacities, uint64_t* out_lens, uint64_t* out_dropped);

/* Normals of n resident clouds from their own neighbourhoods, each exactly as if it were passed alone, in a number of
 * launches that does not depend on n; host-synchronous like the entries above.  For clouds that have no pixel grid to take
 * normals from (a lidar scan, an uploaded cloud, a voxel map's extract).  Per point: the eigenvector of the smallest
 * eigenvalue of the scatter matrix of its neighbours, oriented towards the cloud's viewpoint.  The rule, every f32
 * operation rounded on its own, with r2 = radius * radius and s = 32768.0f / radius computed on the host:
 *   1. grid of pitch radius at the origin (the downsample's cell and key); a point whose key is refused (NaN, infinite,
 *      outside +-2^20 cells) is DROPPED: nobody's neighbour, normal (0,0,0), count 0, curvature 0;
 *   2. the neighbours of point i are the kept points j of its cloud (i included) whose cell coordinates each differ from
 *      i's by at most 1 and whose d = p_j - p_i has (d_x*d_x + d_y*d_y) + d_z*d_z <= r2;
 *   3. q_k = (int) rintf(d_k * s);  N = sum 1, S_k = sum q_k, M_kl = sum q_k q_l in int64: no order dependence;
 *   4. A_kl = (double)N * (double)M_kl - (double)S_k * (double)S_l;  mx = max |A_kl|;  the row is VALID iff
 *      N >= min_neighbors and mx > 0, else normal 0 and curvature 0 (the count is still reported);
 *      B = (float) ldexp(A, -e) with e the exponent of frexp(mx);
 *   5. cyclic Jacobi in f32, exactly 6 sweeps over the pairs (0,1), (0,2), (1,2), each skipped iff a_pq == 0:
 *      theta = (a_qq - a_pp) / (2 a_pq), t = (theta < 0 ? -1 : 1) / (|theta| + sqrtf(theta*theta + 1)),
 *      c = 1 / sqrtf(t*t + 1), s = t*c;  a_pp -= t*a_pq, a_qq += t*a_pq, a_pq = 0;  a_op' = c*a_op - s*a_oq,
 *      a_oq' = s*a_op + c*a_oq;  V_kp' = c*V_kp - s*V_kq, V_kq' = s*V_kp + c*V_kq (V starts as the identity);
 *   6. n = the column of V at the smallest diagonal entry (ties: lowest index), divided by
 *      sqrtf((n_x*n_x + n_y*n_y) + n_z*n_z);  curvature = lambda_min / ((l_0 + l_1) + l_2), or 0 if that sum is not > 0;
 *   7. w = viewpoint - p_i (orient_by_normals != 0: the row's existing normal), dot = (n_x*w_x + n_y*w_y) + n_z*w_z,
 *      n is negated iff dot < 0.
 * A row with a zero normal takes no part in any alignment (its angle to any normal is pi / 2, which every gate below
 * pi / 2 rejects), so nothing is compacted.  viewpoints_host: [n][3] f32 in host memory, NULL = the origin for every
 * cloud.  d_out_normals[i]: [len_i][3]; d_out_curvature and d_out_counts: NULL, or per cloud NULL / [len_i] (counts: N of
 * step 3).  out_valid[i] = valid rows of cloud i; out_dropped[i] (NULL ok) = dropped rows.
 * d_out_normals[i] == d_clouds[i].normals (in place) is allowed: a thread reads only its own row's old normal, before it
 * writes.  Every other overlap of an output with an input or another output is A3D_INVALID_PARAMETER.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx, d_clouds,
 * d_out_normals or out_valid, a radius that is not finite or <= 0 (or so small that its square is 0 in f32),
 * min_neighbors < 3, a non-finite viewpoint, a cloud of 2^32 points or more (or within one tile, < 2^21 points, of it),
 * NULL points or NULL output normals of a non-empty cloud are A3D_INVALID_PARAMETER; orient_by_normals on a non-empty
 * cloud without normals is A3D_MISSING_FIELD.  A cloud with len == 0 may have null pointers and yields zeros.
 * Scratch memory (context-owned, grow-only, shared with the calls above): the downsample's hash table (32 to 64 bytes per
 * point) plus 16 bytes per point for the cell-ordered copy and 96 bytes per cloud. */
a3d_status a3d_point_clouds_estimate_normals_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                    float radius, uint32_t min_neighbors, const float* viewpoints_host,
                                                    int32_t orient_by_normals, float* const* d_out_normals,
                                                    float* const* d_out_curvature, uint32_t* const* d_out_counts,
                                                    uint64_t* out_valid, uint64_t* out_dropped);

/* Outlier removal for resident clouds: the three entries below.  The radius filter (PCL RadiusOutlierRemoval, Open3D
 * remove_radius_outlier) is the k = 0 form of the knn entry followed by a select on its counts with lo = min_neighbors;
 * the statistical filter (StatisticalOutlierRemoval, remove_statistical_outlier) is the knn entry, the threshold entry
 * and a select on qsum with lo = 0, hi = T.
 *
 * Keep rows by value, in input order: row p of cloud i is kept iff lo[i] <= d_values[i][p] <= hi[i] (lo > hi keeps
 * nothing).  n resident clouds, each exactly as if it were passed alone, in a number of launches that does not depend on n
 * (one upload, two launches); host-synchronous like the entries above.  Kept rows go out in input order, point, normal
 * and colour copied bit for bit; d_out_index holds the input row of each kept row and is strictly increasing.  The
 * coordinates are never looked at: a NaN row with a kept value is kept.  d_values: one device array of len_i u32 per
 * cloud; lo, hi: [n] u32 in host memory.  The outputs, their NULL forms, capacities, A3D_MISSING_FIELD for a normals or
 * colour output of a cloud that lacks the field, and the colour buffers' freedom of alignment are those of
 * a3d_point_clouds_voxel_downsample_rgb_device: if any cloud's rows do not fit its capacity the call returns
 * A3D_INVALID_PARAMETER with every count in out_lens and NOTHING written to any output.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx, d_clouds, d_values,
 * lo, hi, d_out_points, capacities or out_lens, a cloud of 2^32 points or more (or within one tile, < 2^21 points, of
 * it), NULL points, values or output points of a non-empty cloud, any overlap of an output (its first min(len_i,
 * capacities[i]) elements) with an input (the values are one) or another output — there is no in-place form — are
 * A3D_INVALID_PARAMETER.  A cloud with len == 0 may have null pointers and yields out_lens[i] = 0.
 * Scratch memory (context-owned, grow-only, shared with the calls above): len_i / 8 bytes of flags, 4 bytes per 1024
 * points and 104 bytes per cloud. */
a3d_status a3d_point_clouds_select_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                          const uint8_t* const* d_colors, uint64_t n, const uint32_t* const* d_values,
                                          const uint32_t* lo, const uint32_t* hi, float* const* d_out_points,
                                          float* const* d_out_normals, uint8_t* const* d_out_colors,
                                          uint32_t* const* d_out_index, const uint64_t* capacities, uint64_t* out_lens);

/* Neighbour count and sum of the k nearest neighbour distances per row of n resident clouds, each exactly as if it were
 * passed alone, in a number of launches that does not depend on n (one upload, one fill, four launches);
 * host-synchronous.  The rule, every f32 operation rounded on its own, with r2 = radius * radius and s = 32768.0f / radius
 * computed on the host:
 *   1. grid and 2. neighbours: steps 1 and 2 of a3d_point_clouds_estimate_normals_device, word for word (pitch radius;
 *      dropped rows are nobody's neighbour; cell coordinates differ by at most 1; d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2);
 *   3. counts[p] = N, the neighbours of row p, itself included, 0 for a dropped row: bit for bit the d_out_counts of
 *      a3d_point_clouds_estimate_normals_device at the same radius;
 *   4. the OTHERS of row p are its neighbours with a different row index (a duplicate point is an other at distance 0);
 *      for each other, t = (uint32) rintf(sqrtf(d2) * s), which is non-decreasing in d2;
 *   5. qsum[p] = Q = the sum of the k smallest t, or 0xFFFFFFFF if the row is dropped or has fewer than k others; the
 *      multiset of the k smallest values is unique, so Q does not depend on the order in which candidates are met;
 *   6. out_stats[i] = {m, sum Q, sum (Q*Q & 0xFFFFFFFF), sum (Q*Q >> 32)} over the m rows of cloud i whose Q is not
 *      0xFFFFFFFF: u64 integer sums, the same bits on every run and under any permutation of the rows.  r2 is at most
 *      twice the exact square of the radius (a denormal product), so t <= 46342 < 2^16, Q < 2^21 and Q*Q < 2^42 for k <= 32;
 *      with len < 2^32 the four sums stay below 2^32, 2^53, 2^64 and 2^42: none can overflow.
 * 0 <= k <= 32.  k == 0 is the count-only form: no distances are computed, d_out_qsum is not read and the statistics are
 * zeros.  d_out_counts: NULL, or per cloud NULL / [len_i] u32.  d_out_qsum: NULL only if k == 0, else per cloud [len_i] u32.
 * out_stats: [n][4] u64 in host memory, NULL ok.  out_dropped[i] (NULL ok) = dropped rows of cloud i.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx or d_clouds, a radius
 * that is not finite or <= 0 (or so small that its square is 0 in f32), k > 32, a NULL d_out_qsum (or entry of a non-empty
 * cloud) while k > 0, a cloud of 2^32 points or more (or within one tile, < 2^21 points, of it), NULL points of a non-empty
 * cloud, any overlap of an output with an input or another output are A3D_INVALID_PARAMETER.  A cloud with len == 0 may
 * have null pointers and yields zeros.
 * Scratch memory (context-owned, grow-only, shared with the calls above): that of the normals entry (32 to 64 bytes per
 * point of hash table, 16 bytes per point for the cell-ordered copy) and 64 bytes per cloud. */
a3d_status a3d_point_clouds_knn_distance_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                float radius, uint32_t k, uint32_t* const* d_out_counts,
                                                uint32_t* const* d_out_qsum, uint64_t* out_stats, uint64_t* out_dropped);

/* The statistical filter's threshold from one cloud's out_stats of the entry above; host only, no GPU call.  With
 * {m, SQ, lo, hi} = stats and SQ2 = lo + hi * 2^32:  mu = (double)SQ / (double)m;  num = m * SQ2 - SQ * SQ, exact in 128
 * bits (>= 0 and < 2^107);  var = (double)num / ((double)m * (double)(m - 1)), the sample variance as PCL uses it, 0 when
 * m < 2;  T = floor(mu + std_ratio * sqrt(var)), clamped to [0, 0xFFFFFFFE] so that the 0xFFFFFFFF of a row without k
 * others never passes.  m == 0 gives 0.  The filter keeps the rows with 0 <= qsum <= T.  A NULL argument, a std_ratio
 * that is not finite or negative, and statistics outside the bounds stated above (or with num < 0) are
 * A3D_INVALID_PARAMETER. */
a3d_status a3d_knn_distance_threshold(const uint64_t stats[4], double std_ratio, uint32_t* out_hi);

/* Which rows belong together: DBSCAN clusters of n resident clouds, each exactly as if it were passed alone, in a number
 * of launches that does not depend on n (one upload, one fill, eight launches); host-synchronous.  PCL
 * EuclideanClusterExtraction(tolerance) is min_points = 1; Open3D cluster_dbscan(eps, min_points) is (radius, min_points).
 * The rule, every f32 operation rounded on its own, with r2 = radius * radius computed on the host:
 *   1. grid and neighbours: steps 1 and 2 of a3d_point_clouds_knn_distance_device, word for word (pitch radius; dropped
 *      rows are nobody's neighbour; cell coordinates differ by at most 1; d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2, the
 *      same bits seen from either row, so the relation is symmetric);
 *   2. row p is a CORE row iff it is kept and N_p >= min_points, N_p its neighbours, itself included: bit for bit the
 *      counts of the knn entry;
 *   3. two core rows are linked iff they are neighbours; a cluster is a connected component of the core rows under that
 *      link, and its ROOT is its lowest row;
 *   4. a kept row that is not core and has a core neighbour is a BORDER row of the cluster of the core neighbour j that
 *      minimises bits(d2) << 32 | j: the nearest, the lower row on a tie; a border row never links two clusters;
 *   5. every other row is noise (dropped rows; non-core rows without a core neighbour), label 0xFFFFFFFF;
 *   6. clusters are numbered 0 ... C-1 by ascending root: labels[p] = the number of row p's cluster, sizes[c] = the rows
 *      labelled c, border rows included, roots[c] strictly increasing, row_sizes[p] = sizes[labels[p]] and 0 for noise.
 * min_points = 1 makes every kept row core: Euclidean cluster extraction with tolerance radius.  Core rows get the labels
 * Open3D gives them for the same neighbour sets (it numbers clusters by their lowest core index too); a border row with
 * core neighbours in several clusters may land in another of them than Open3D's first-come rule puts it.  Every output is
 * integers decided on integers or on d2 bits: the same on every run.  Under a permutation of the rows the partition of the
 * core rows and the noise set do not change.
 * d_out_labels: per cloud [len_i] u32, required for a non-empty cloud; it goes to a3d_point_clouds_select_device as it is.
 * d_out_row_sizes: NULL, or per cloud NULL / [len_i] u32.  d_out_sizes, d_out_roots: NULL, or per cloud NULL / [len_i] u32
 * of which the first C_i are written and the rest left untouched.  out_clusters[i] = C_i, out_noise[i] = noise rows
 * (dropped ones included), out_dropped[i] = dropped rows: [n] u64 in host memory, each NULL ok.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx, d_clouds or
 * d_out_labels, a radius that is not finite or <= 0 (or so small that its square is 0 in f32), min_points == 0, a cloud of
 * 2^32 points or more (or within one tile, < 2^21 points, of it), NULL points or labels of a non-empty cloud, any overlap
 * of an output ([len_i] u32 each) with an input (points, normals) or another output are A3D_INVALID_PARAMETER.  A cloud with
 * len == 0 may have null pointers and yields zeros.  A union-find loop that ran past its bound (it cannot) is A3D_HIP_ERROR.
 * Scratch memory (context-owned, grow-only, shared with the calls above): that of the knn entry (32 to 64 bytes per point
 * of hash table, 16 for the cell-ordered copy) plus 12 bytes per point (parent, owner, size), 1 / 8 byte per point of flags,
 * 4 bytes per 1024 points and 168 bytes per cloud. */
a3d_status a3d_point_clouds_cluster_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n, float radius,
                                           uint32_t min_points, uint32_t* const* d_out_labels,
                                           uint32_t* const* d_out_row_sizes, uint32_t* const* d_out_sizes,
                                           uint32_t* const* d_out_roots, uint64_t* out_clusters, uint64_t* out_noise,
                                           uint64_t* out_dropped);

/* The dominant plane of n resident clouds (PCL SACSegmentation with SACMODEL_PLANE, Open3D segment_plane), each exactly
 * as if it were passed alone, in a number of launches that does not depend on n: one upload (job table, triples, zeroed
 * words), one fill and four launches (candidates, score, best, flag + moments), and one small upload and one launch more
 * per refinement round; host-synchronous.  There is no early exit by probability: every candidate is scored against every
 * row.  The rule:
 * Every f32 and every f64 operation is rounded on its own.  Divide and sqrt are correctly rounded.
 * Per call: a distance threshold t, f32, finite and > 0, and a number of refinement rounds R with 0 <= R <= 8.
 * Per cloud i: H_i candidate triples (a, b, c) of row numbers, [H_i][3] u32 in HOST memory.  0 <= H_i <= 4096.  Every
 * index is < len_i.
 *   1. Candidate plane of a triple.  The three points are widened to f64.  u = p_b - p_a, v = p_c - p_a.  m = u x v, each
 *      component as u_y*v_z - u_z*v_y.  L = (m_x*m_x + m_y*m_y) + m_z*m_z.  U = (u_x*u_x + u_y*u_y) + u_z*u_z, and V
 *      likewise.  The candidate is DEGENERATE iff two of its indices are equal, or L is not finite, or not
 *      L > (U*V) * 2^-20.  That covers a repeated row, a non-finite row, and three rows whose sine is below 2^-10.
 *      Otherwise n = (float)(m / sqrt(L)) per component, and the plane's point is p_a, in f32 as stored.
 *   2. Distance and inlier, in f32.  e_k = p_k - p_ak, d = (n_x*e_x + n_y*e_y) + n_z*e_z.  Row p is an inlier of the
 *      candidate iff fabsf(d) <= t.  A row with a NaN or an infinity is never an inlier.  The form p - a is deliberate.
 *      n.p + w saves three operations per test and cancels badly for clouds far from the origin.
 *   3. Score.  count[h] is the number of inliers of candidate h over ALL rows of the cloud, and 0 for a degenerate
 *      candidate.  The best candidate maximises count[h] << 32 | (0xFFFFFFFF - h): the most inliers, the lowest h on a
 *      tie.  If every candidate is degenerate, or H_i == 0 or len_i == 0, there is no plane: flags all 0, plane four
 *      zeros, best = 0xFFFFFFFF, status A3D_OK.
 *   4. Flags.  flags[p] = 1 iff p is an inlier of the current plane (n, point), else 0.  After step 3 the current plane
 *      is the best candidate's.
 *   5. Refit moments over the rows with flag 1, all in integers.  s = 64.0f / t in f32.  q_k = (int) rintf(e_k * s), ties
 *      to even, with e from step 2 against the current plane's point.  A flagged row takes part iff
 *      fabsf(e_k * s) <= 1048576.0f for all three k.  N = sum 1, S_k = sum q_k, and for the six products P = q_k q_l, with
 *      |P| <= 2^40: Lo_kl = sum (P & 0x7FFFFFFF), Hi_kl = sum (P >> 31), an arithmetic shift.  So
 *      M_kl = Hi_kl * 2^31 + Lo_kl exactly.  With len < 2^32, N, S, Lo and Hi each fit 64 bits, so no order of summation
 *      can matter.  The record is 16 u64 words: N, S[3], Lo[6], Hi[6] in the order xx, xy, xz, yy, yz, zz.
 *   6. Plane from moments, on the HOST (a3d_plane_from_moments).  A_kl = N*M_kl - S_k*S_l, exact in 128-bit integers
 *      (|A| < 2^105).  Each A_kl converted to f64, round to nearest even.  mx = max |A_kl|.  The refit is VALID iff N >= 3
 *      and mx > 0.  Then steps 4 (scaling by frexp's exponent) to 6 (normal = column of the smallest diagonal entry,
 *      normalised) of the rule of a3d_point_clouds_estimate_normals_device: six cyclic Jacobi sweeps in f32.  Centroid in
 *      f64: c_k = (double)a_k + ((double)S_k / (double)N) / (double)s, with a the point that the moments were taken
 *      against.  d = -((n_x*c_x + n_y*c_y) + n_z*c_z) in f64, with n widened.  The four numbers are negated iff d < 0.
 *      This is the side the origin is on: the default viewpoint of the normals call.  If the refit is not valid, the
 *      plane is the current plane itself: its f32 normal widened, and c = a; d and the sign follow in the same way.
 *   7. Refinement, R times.  The current plane becomes the plane of step 6: normal (float)n, point (float)c.  Steps 4 and
 *      5 are repeated against it, then step 6.  R = 0 is the inliers of the best candidate and the model refitted to them
 *      (Open3D's behaviour).
 * Every count, flag and moment is an integer decided on f32 bits that no order can change: the same on every run, and under
 * a permutation of the rows (the triples mapped through it) the same counts, best and plane, and the permuted flags.
 * triples: [n] host pointers to [H_i][3] u32 (NULL ok where H_i == 0); n_triples: [n] u32, the H_i.  d_out_flags: per cloud
 * [len_i] u32, required for a non-empty cloud; it goes to a3d_point_clouds_select_device as it is: lo = hi = 1 is the plane,
 * lo = hi = 0 is the rest.  d_out_counts: NULL, or per cloud NULL / [H_i] u32, count[h] of step 3; words past H_i are left
 * untouched.  out_planes: [n][4] f64 (n_x, n_y, n_z, d: n.x + d = 0), required.  out_best[i] = the best candidate's h,
 * out_inliers[i] = the flagged rows of the last round, out_refit_rows[i] = N of the last moments: [n] u64, each NULL ok.
 * All of these are host memory.
 * Decided on the host before anything is launched (nothing is touched): n == 0 is A3D_OK; a NULL ctx, d_clouds, triples,
 * n_triples, d_out_flags or out_planes, a t that is not finite or <= 0 (or so small that 64 / t is not finite in f32),
 * refine > 8, H_i > 4096, NULL triples of a cloud with H_i > 0, a triple index >= len_i (so every H_i > 0 on an empty cloud),
 * a cloud of 2^32 points or more, NULL points or flags of a non-empty cloud, any overlap of an output (flags [len_i] u32,
 * counts [H_i] u32) with an input (points, normals) or another output are A3D_INVALID_PARAMETER.  A cloud with len == 0 may
 * have null pointers and has no plane.
 * Scratch memory (context-owned, grow-only, shared with the calls above): 48 bytes per candidate (triple, plane, counter),
 * 64 bytes per cloud and 136 bytes per cloud and round. */
a3d_status a3d_point_clouds_segment_plane_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n, float t,
                                                 uint32_t refine, const uint32_t* const* triples, const uint32_t* n_triples,
                                                 uint32_t* const* d_out_flags, uint32_t* const* d_out_counts,
                                                 double* out_planes, uint64_t* out_best, uint64_t* out_inliers,
                                                 uint64_t* out_refit_rows);

/* The candidate triples the wrappers give the entry above; host only, no GPU call.  For candidate h and k in 0..2:
 * z = seed + (3h + k + 1) * 0x9E3779B97F4A7C15 mod 2^64, then the splitmix64 finaliser (z ^= z >> 30;
 * z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31), and the index is
 * ((z >> 32) * len) >> 32.  A counter-based rule of our own, not the generator of PCL or Open3D: candidate h does not depend
 * on H.  Repeated indices are allowed: such a candidate is degenerate by the rule above.  out_triples: [H][3] u32.  H == 0
 * is A3D_OK and writes nothing; a NULL out_triples, len == 0, len >= 2^32 and H > 4096 are A3D_INVALID_PARAMETER. */
a3d_status a3d_plane_hypotheses(uint64_t seed, uint64_t len, uint64_t H, uint32_t* out_triples);

/* Step 6 of the rule above, from one record of step 5; host only, no GPU call.  moments: N, S[3], Lo[6], Hi[6]; point: the
 * point a the moments were taken against; t: the call's threshold (s = 64.0f / t); fallback_normal: the current plane's
 * normal, which an invalid refit keeps.  out_plane: (n_x, n_y, n_z, d).  *out_valid (NULL ok) = 1 iff the refit was valid.
 * A NULL moments, point, fallback_normal or out_plane, a t that is not finite or <= 0 (or with 64 / t not finite), and
 * moments that no call can have produced (N >= 2^32, |S_k| > N * 2^20, Lo_kl > N * (2^31 - 1), |Hi_kl| > N * 2^9) are
 * A3D_INVALID_PARAMETER. */
a3d_status a3d_plane_from_moments(const uint64_t moments[16], const float point[3], float t, const float fallback_normal[3],
                                  double out_plane[4], uint32_t* out_valid);

/* A persistent voxel map: the hash table of the downsample above kept between calls, so that resident clouds go in frame
 * by frame (a3d_voxel_map_insert) instead of merge + downsample of the whole map per frame.  The contract:
 *   After any sequence of inserts, the map's contents equal a3d_point_clouds_merge_device(all inserted clouds under their
 *   poses, in insertion order) followed by a3d_point_clouds_voxel_downsample_device(voxel_size, origin): points, normals,
 *   order and winner indices, however the inserts were grouped into calls and whatever the table's size history was.
 * Sequence numbers: point i of cloud j of a call gets seq = total + sum(len[0..j)) + i, where total is the number of points
 * ever offered to the map; dropped points (the downsample's drop rule) consume a number too, so seq is the point's index
 * in the merged cloud, and the winner of a cell minimises bits(dist) << 32 | seq over everything inserted so far.
 * Reservation: the table is open-addressing with a power-of-two slot count; before it launches, an insert of L points
 * makes sure slots >= 2 * (cells + L) and otherwise moves the map into the next sufficient power of two (one growth).  The
 * table is allocated by the first insert that offers a point, at max(that rule, 2 * reserve_cells, 64) slots, which is no
 * growth.  Device memory: 16 + 12 (+ 12 with normals) (+ 4 with colours) bytes per slot, from the context's block pool.
 * Limits: total + L must stay below 2^32 - 2^21 (one tile span), else A3D_INVALID_PARAMETER and nothing changes;
 * a3d_voxel_map_retain renumbers a long-lived map, and removes cells by place and by age.  The map is also a spatial index:
 * a3d_voxel_map_nearest_device and a3d_voxel_map_icp_align_device (below) read it without an extract or a kd-tree build.
 * Colours (a3d_voxel_map_new_rgb): a map may keep the winner's colour per cell, and the contract extends word for word:
 * after any sequence of inserts a3d_voxel_map_extract_rgb equals a3d_point_clouds_merge_rgb_device of everything inserted
 * followed by a3d_point_clouds_voxel_downsample_rgb_device, colours included.  After a retain the map is a new map into
 * which the surviving rows, colours too, went as one cloud.  Nearest, align and accumulate never read colours.
 * A map of MEANS (a3d_voxel_map_new_mean) keeps a3d_point_clouds_voxel_mean_device's rule instead of the nearest-point rule,
 * as running integer sums per slot, and the contract carries over word for word: after any sequence of inserts
 * a3d_voxel_map_extract_mean equals a3d_point_clouds_merge_rgb_device of everything inserted followed by
 * a3d_point_clouds_voxel_mean_device(voxel_size, origin): points, normals, colours, order, representative indices and
 * counts, bit for bit, however the inserts were grouped (every term of every sum is an integer, so no order of addition
 * can matter; poses are applied before a point or a normal is quantised, the bits the merge writes).  A cell's
 * representative is its lowest seq, rows are in ascending representative, a cell with one point holds that point's row
 * bit for bit.  The count of a cell is kept in 64 bits and exported as u32, saturating; the normal sums are exact in f64
 * up to 2^32 points per cell, as in the batch rule.  Every other call takes a map of means through the same entry:
 * insert (two launches, as on a nearest-point map), extract, retain, nearest, icp_*, render, clear, get_stats; the
 * readers see the mean row where they saw the winner's.  Retain on a map of means: the box is tested on the stored row,
 * the mean; min_seq on the representative's seq (age by last observation is not kept); the survivors keep their rows,
 * sums and counts and are numbered 0 ... k-1 in their old order, and later inserts go on summing into them.  Such a map
 * is then NOT a new map into which the surviving rows went as one cloud: it is the mean downsample of every point ever
 * offered to the surviving cells, in their original order, followed by whatever comes later.  Six launches.  Device memory
 * of a map of means, per slot: the above plus 8 (count) + 24 (lattice sums) (+ 24 with normals) (+ 24 with colours) + 4
 * (the number of the last insert call that touched the cell): 64 bytes for points alone, 100 with normals, 128 with both.
 * Multi-GPU maps are NOT built.
 * Every call is host-synchronous (one wait, at its end) and ordered on the context's stream; a map belongs to its context
 * and must be freed before it. */
typedef struct a3d_voxel_map a3d_voxel_map;
typedef struct a3d_voxel_map_stats {
  uint64_t cells;         /* occupied cells */
  uint64_t slots;         /* slots of the table (0 before the first point) */
  uint64_t total;         /* points ever offered, dropped ones included: the next sequence number */
  uint64_t dropped_total; /* of those, dropped by the drop rule */
  uint64_t growths;       /* times the table was moved into a larger one */
} a3d_voxel_map_stats;

/* A new, empty map of pitch voxel_size anchored at origin (NULL = (0,0,0)); with_normals != 0: the map keeps a normal per
 * cell and every inserted cloud must have normals.  reserve_cells (0 allowed, < 2^32): cells the first table has room for
 * without growing.  Decided on the host, nothing is launched or allocated on the device: a NULL ctx or out, a voxel_size
 * that is not finite or <= 0, a non-finite origin are A3D_INVALID_PARAMETER. */
a3d_status a3d_voxel_map_new(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                             uint64_t reserve_cells, a3d_voxel_map** out);
/* The same; with_colors != 0: the map keeps a colour per cell and every inserted cloud must have colours.  A map made by
 * a3d_voxel_map_new has no colours. */
a3d_status a3d_voxel_map_new_rgb(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                                 int with_colors, uint64_t reserve_cells, a3d_voxel_map** out);
/* The same arguments and errors; the map is a map of means (above): per cell the centroid, the mean normal and the mean
 * colour of everything offered to it, by the rule of a3d_point_clouds_voxel_mean_device.  The mode is fixed for the map's
 * life. */
a3d_status a3d_voxel_map_new_mean(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                                  int with_colors, uint64_t reserve_cells, a3d_voxel_map** out);
/* Inserts n resident clouds (device pointers on the map's context) under poses_host[i] (NULL = as they are, bit for bit;
 * otherwise Transform::transform_vector / transform_normal as a3d_point_clouds_merge_device).  out_dropped (NULL ok): [n],
 * the dropped points of each cloud; out_cells (NULL ok): the map's occupied cells afterwards.
 * Decided on the host before anything is launched, and then nothing is inserted from the whole call: n == 0 is A3D_OK and
 * touches nothing; a NULL map or d_clouds, a cloud of 2^32 points or more, NULL points of a non-empty cloud and the limit
 * above are A3D_INVALID_PARAMETER; a non-empty cloud without normals offered to a map with normals is A3D_MISSING_FIELD.
 * A cloud with len == 0 may have null pointers.  A3D_HIP_ERROR if the table ever filled up (it cannot). */
a3d_status a3d_voxel_map_insert(a3d_voxel_map* map, const a3d_point_cloud_view* d_clouds, const a3d_pose* poses_host,
                                uint64_t n, uint64_t* out_dropped, uint64_t* out_cells);
/* The same with the clouds' colours (d_colors: NULL, or n DEVICE pointers to [len][3] u8 of which some may be NULL).  A
 * non-empty cloud without colours offered to a map with colours is A3D_MISSING_FIELD, decided on the host: nothing from
 * the call is inserted; so a3d_voxel_map_insert on such a map is refused for any non-empty cloud.  A map without colours
 * ignores d_colors. */
a3d_status a3d_voxel_map_insert_rgb(a3d_voxel_map* map, const a3d_point_cloud_view* d_clouds, const uint8_t* const* d_colors,
                                    const a3d_pose* poses_host, uint64_t n, uint64_t* out_dropped, uint64_t* out_cells);
/* Writes the occupied cells' rows in ascending seq — the order the downsample gives on the merged cloud, the same bits on
 * every run — into d_out_points (room for `capacity` points), d_out_normals (NULL ok; non-NULL on a map without normals
 * -> A3D_MISSING_FIELD) and d_out_index (NULL ok): the seq of each row, u32.  *out_len = cells.  capacity < cells ->
 * A3D_INVALID_PARAMETER, *out_len = cells, nothing written.  A NULL map, d_out_points or out_len, or outputs whose first
 * `capacity` rows overlap one another, are A3D_INVALID_PARAMETER.  The map is not changed; inserts may continue.
 * Scratch memory (context-owned, shared with the calls above): total / 8 bytes of bitmap and total / 16 of prefixes. */
a3d_status a3d_voxel_map_extract(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint32_t* d_out_index,
                                 uint64_t capacity, uint64_t* out_len);
/* The same with the rows' colours into d_out_colors (NULL ok; room for `capacity` rows of [3] u8; non-NULL on a map
 * without colours -> A3D_MISSING_FIELD).  capacity < cells writes nothing.  The colour output takes part in the overlap
 * check by its first 3 * capacity bytes; bytes at or past 3 * cells are never written. */
a3d_status a3d_voxel_map_extract_rgb(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                     uint32_t* d_out_index, uint64_t capacity, uint64_t* out_len);
/* The same with the cells' counts into d_out_counts (NULL ok; room for `capacity` u32): the points ever offered to each
 * row's cell, saturating at 2^32 - 1; d_out_index is then each cell's representative, its lowest seq.  A non-NULL
 * d_out_counts on a nearest-point map is A3D_INVALID_PARAMETER (it keeps no counts); with d_out_counts NULL the call is
 * a3d_voxel_map_extract_rgb on either kind of map.  The counts take part in the overlap check by 4 * capacity bytes. */
a3d_status a3d_voxel_map_extract_mean(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                      uint32_t* d_out_index, uint32_t* d_out_counts, uint64_t capacity, uint64_t* out_len);
/* Rebuilds the map from the cells that survive and numbers them anew.  A cell survives iff its winner's seq >= min_seq
 * and, if a box is given, its stored row p has box_min[k] <= p[k] <= box_max[k] for k = 0, 1, 2: plain f32 comparisons
 * on the stored bits (the cell centre plays no part).  box_min and box_max are both NULL (no box) or both given; infinite
 * bounds are allowed (a one-sided box); box_min[k] > box_max[k] keeps nothing; min_seq >= total removes everything; no
 * box and min_seq == 0 is a pure compaction.  The contract:
 *   Let the survivors be the k rows of a3d_voxel_map_extract that pass the rule, in extract order.  After the call the map
 *   is indistinguishable from a new map of the same voxel_size, origin, with_normals and reserve_cells into which those k
 *   rows, points, normals and colours, were inserted as ONE cloud without a pose.
 * (A cell's stored row is the very f32 point its key and bits(dist) were computed from, so offering it again without a pose
 * gives the same key and the same distance.)  So: extract returns the k rows bit for bit with indices 0 ... k-1;
 * get_stats gives cells = total = k and dropped_total = 0; growths is unchanged (a retain is no growth); for k > 0, slots
 * is the smallest power of two >= max(2 k, 2 * reserve_cells, 64); every later insert, extract and retain gives exactly
 * what it would give on that new map, and the next point offered gets seq k: the 2^32 - 2^21 limit recedes with every
 * retain.  For k == 0 the call has the effect of a3d_voxel_map_clear: the allocation is kept and slots is what it was.
 * Marks: a caller that ages by frame records `total` at frame boundaries, and the renumbering invalidates those records.
 * out_marks[i] (i < n_marks) = the number of survivors whose OLD seq is < marks[i]: the same boundary in the new numbering;
 * a mark >= the old total gives k.  marks NULL with n_marks == 0 is fine.  *out_removed (NULL ok) = cells before - k.
 * Decided on the host before anything is launched: a NULL map, one of box_min / box_max NULL alone, a NaN bound, marks or
 * out_marks NULL with n_marks > 0 (or n_marks >= 2^32) are A3D_INVALID_PARAMETER.  On a map that holds no table yet:
 * A3D_OK, removed 0, every out_mark 0.  On ANY failure, one of the device included (A3D_HIP_ERROR), the map is unchanged:
 * the old table is only read, and stays the map's if the new one cannot be allocated or built.
 * Five launches whatever cells and slots are.  Scratch memory as the extract: total / 8 bytes of bitmap and total / 16 of
 * prefixes (and 16 bytes per mark).  Device memory: the new table's block is sized for the cells BEFORE the call (k is
 * known only at the call's one wait; the table inside it has the slots stated above): memory follows one retain later. */
a3d_status a3d_voxel_map_retain(a3d_voxel_map* map, const float box_min[3], const float box_max[3], uint64_t min_seq,
                                const uint64_t* marks, uint64_t n_marks, uint64_t* out_marks, uint64_t* out_removed);
a3d_status a3d_voxel_map_get_stats(const a3d_voxel_map* map, a3d_voxel_map_stats* out);
/* Empties the map and keeps its allocation: cells, total and dropped_total are 0 again (sequence numbers restart). */
a3d_status a3d_voxel_map_clear(a3d_voxel_map* map);
void a3d_voxel_map_free(a3d_voxel_map* map);

/* Aligning against the map.  The association rule, the definition everything below is tested against:
 *   For a query point q, after its optional pose (Transform::transform_vector, as a3d_voxel_map_insert applies it):
 *   c_k = floorf((q_k - o_k) / v) as above; if q fails the drop rule (a c_k not finite or outside [-2^20, 2^20)) it has
 *   no correspondence.  The candidates are the stored rows of the occupied cells c + d, d in {-1, 0, 1}^3.  A neighbour
 *   whose coordinate leaves [-2^20, 2^20) on any axis is skipped; that is decided per axis, before the key is packed: a
 *   borrow or carry never reaches another axis's field of the key.  For a candidate row r, in f32 with every operation
 *   rounded on its own: d = q - r, d2 = (d_x * d_x + d_y * d_y) + d_z * d_z.  The winner minimises
 *   bits(d2) << 32 | seq, the word form the map already uses (d2 is never negative or NaN here).  The result therefore
 *   does not depend on slot order, table size, growth history or timing.  If no candidate exists the result is seq
 *   0xFFFFFFFF and d2 +inf.
 * In plain words: the exact nearest stored row wherever that row lies within about one cell of q.  The claim is rigorous
 * for distances <= 0.75 v when |q - o| / v < 2^12, because the rounding of the cell coordinate is then far below a
 * quarter cell; farther rows are simply not found.  This is NOT the reference's R3dTree::nearest, which scans a single
 * leaf and is approximate: there is no parity with Icp over a3d_voxel_map_extract's cloud, only the rule above.
 * Search radii above one cell, several sources per call, colour terms and a point-to-point cost are NOT built.
 * All entries are host-synchronous and ordered on the context's stream like the other map calls; the map is never
 * modified, so inserts and retains may follow.  A map whose table has more than 2^32 slots (over 120 GiB) is refused with
 * A3D_INVALID_PARAMETER by all of them: slot indices are 32-bit in these kernels. */

/* The association for m resident queries: d_queries [m][3] f32, pose_host NULL = the queries as they are, bit for bit;
 * d_out_seq [m] u32 and d_out_dist2 [m] f32.  m == 0 is A3D_OK and touches nothing; a map without a table (nothing
 * inserted yet) fills the outputs with "none".  Decided on the host before any launch: a NULL map, or with m > 0 a NULL
 * d_queries, d_out_seq or d_out_dist2, m >= 2^31, and outputs that overlap each other or the queries are
 * A3D_INVALID_PARAMETER. */
a3d_status a3d_voxel_map_nearest_device(a3d_voxel_map* map, const float* d_queries, uint64_t m, const a3d_pose* pose_host,
                                        uint32_t* d_out_seq, float* d_out_dist2);
/* Frame-to-map ICP: Icp::align's loop (src/icp/pcl_icp.rs:59-106) with the association above in place of the kd-tree,
 * started from initial_host (NULL = Transform::eye()) instead of eye(): the returned pose maps the source AS GIVEN into
 * the map's frame, the caller does not transform the cloud first.  The gates (max_distance squared against d2, the strict
 * normal-angle gate), the residual, the Jacobian, the weight, max_iterations (0 returns the initial pose bit for bit), the
 * best-pose rule and the solve-failure status are exactly a3d_pcl_icp_align_device's: A3D_SOLVE_FAILED when no point
 * passes, with the pose reached so far in out_pose.  d_source: DEVICE pointers on the map's context, read during the call.
 * The launch geometry follows the source length and the device only, never the table's slot count: the sums of an
 * iteration depend on the map's contents alone.  The working buffers (two states, two partial sets, the out pose; a few
 * hundred bytes per CU) belong to the map: allocated on first use, freed with it.
 * Decided on the host before any launch, in this order: a NULL map, params, d_source, d_source->points or out_pose
 * -> A3D_INVALID_PARAMETER; a source with len == 0 or len >= 2^31 -> A3D_INVALID_PARAMETER; a map without normals ->
 * A3D_MISSING_FIELD; a source without normals -> A3D_MISSING_FIELD. */
a3d_status a3d_voxel_map_icp_align_device(a3d_voxel_map* map, const a3d_icp_params* params,
                                          const a3d_point_cloud_view* d_source, const a3d_pose* initial_host,
                                          a3d_pose* out_pose);
/* One pass of that per-point loop under `pose` (NULL = eye), summed in f64 as a3d_pcl_icp_accumulate: test hook.  The
 * same refusals. */
a3d_status a3d_voxel_map_icp_accumulate_device(a3d_voxel_map* map, const a3d_icp_params* params,
                                               const a3d_point_cloud_view* d_source, const a3d_pose* pose,
                                               a3d_gn_state* out_state);
/* Instrumentation: device time (ms) of the iteration launches of the most recent a3d_voxel_map_icp_align_device. */
a3d_status a3d_voxel_map_icp_last_device_ms(a3d_voxel_map* map, float* out_ms);

/* ---- PinholeCamera::project_to_image over a cloud (src/camera.rs:177-202) ------------------ */

/* Renders a resident cloud into the resident RangeImage a pinhole camera would see: the inverse of
 * a3d_range_image_to_point_cloud, with PinholeCamera::project_to_image (src/camera.rs:177-202) applied to every row.
 * d_cloud: DEVICE pointers on the context's GPU ([len][3] f32 points, normals or NULL), d_colors: DEVICE [len][3] u8 or
 * NULL, all read during the call only.  world_to_camera_host: PinholeCamera's world_to_camera (the inverse of the
 * camera_to_world given to PinholeCamera::new), NULL = none.  fx, fy, cx, cy are cast to f32 once.  The rule, all of it in
 * f32 with every operation rounded on its own; for each row k, in this order:
 *   1. p = transform_vector(world_to_camera, points[k]) (src/transform.rs:138-145); without a pose p = points[k] verbatim.
 *   2. z = p.z; the row is dropped unless z > 0 and z < +inf (a NaN fails both).
 *   3. u = p.x * fx / z + cx, v = p.y * fy / z + cy (CameraIntrinsics::project, camera.rs:64-70).
 *   4. ui = round(u), vi = round(v), halves away from zero (f32::round, camera.rs:194); the row is dropped unless
 *      0 <= ui < width and 0 <= vi < height compared as f32 (camera.rs:196): -0.0 passes, NaN and infinities fail.  This is
 *      not the (u + 0.5) as i32 of the ICP kernels: u = 0.49999997 lands in column 0 here.
 *   5. The footprint's half-widths are 0 for radius == 0, else hx = min(floor(radius * fx / z), 8) and
 *      hy = min(floor(radius * fy / z), 8) (the product is rounded, then divided; 8 = A3D_RENDER_MAX_HALF_WIDTH).
 *   6. The footprint is columns [ui - hx, ui + hx] x rows [vi - hy, vi + hy] clipped to the image; a row whose centre
 *      pixel is outside the image is dropped whole (the reference's None).
 *   7. Every pixel of the footprint is offered the key bits(z) << 32 | k, and a pixel's winner is the MINIMUM key: the
 *      nearest surface, and on equal z bits the lowest row (z > 0 and finite, so its bits are monotone).
 * A pixel with winner k gets mask 1, point p of step 1 (the true transformed point, not a pixel-centre back-projection:
 * with radius > 0 one row may fill many pixels with the same point and normal, a surfel to point-to-plane ICP), normal
 * transform_normal(world_to_camera, normals[k]) (verbatim without a pose), colour colors[k] byte for byte and index k; a
 * pixel without a winner gets mask 0, +0 points and normals, colour 0, 0, 0 and index 0xFFFFFFFF.  The result does not
 * depend on launch geometry, scheduling or how often the call runs.
 * *out_image: an ordinary image on ctx (a3d_range_image_free) that carries fx, fy, cx, cy as given, has normals iff
 * d_cloud->normals is not NULL and colours iff d_colors is not NULL (a non-NULL d_colors for a cloud that has none is the
 * caller's business: the view does not know), and has no intensities and no map: a3d_range_image_compute_intensity /
 * a3d_range_image_pyramids add them as for an uploaded image with colours.  d_out_index: NULL, or DEVICE [height][width]
 * u32 for the index plane.  Host-synchronous; three launches whatever the sizes; width * height * 8 bytes of context
 * scratch for the z-buffer.  len == 0 is A3D_OK with an all-empty image.
 * Decided on the host before anything is launched or allocated (A3D_INVALID_PARAMETER, *out_image untouched): a NULL ctx,
 * d_cloud or out_image; width or height 0, or width * height >= 2^31; a non-finite intrinsic, or (float)fx <= 0 or
 * (float)fy <= 0; a radius that is NaN, infinite or negative; len > 2^32 - 2; NULL points with len > 0; an index plane
 * that overlaps the cloud.  On any failure *out_image is untouched and no memory is kept. */
a3d_status a3d_point_cloud_render_device(a3d_context* ctx, const a3d_point_cloud_view* d_cloud, const uint8_t* d_colors,
                                         const a3d_pose* world_to_camera_host /* NULL: none */,
                                         double fx, double fy, double cx, double cy, uint64_t width, uint64_t height,
                                         float radius, uint32_t* d_out_index /* NULL, or DEVICE [h][w] */,
                                         a3d_device_image** out_image);
/* PinholeCamera::project_to_image (src/camera.rs:177-202) over the live map: bit for bit, the index plane included,
 * a3d_point_cloud_render_device applied to what a3d_voxel_map_extract_rgb would return now (the row index is the extract's
 * row); the image has normals iff the map has them and colours iff the map has them; an empty map gives an all-empty
 * image.  The extract goes into context scratch inside the call (cells * 27 bytes behind the z-buffer) and the same
 * kernels run on it.  The same refusals as above with `map` in place of ctx and d_cloud; the map is never changed. */
a3d_status a3d_voxel_map_render(a3d_voxel_map* map, const a3d_pose* world_to_camera_host, double fx, double fy, double cx,
                                double cy, uint64_t width, uint64_t height, float radius, uint32_t* d_out_index,
                                a3d_device_image** out_image);

/* ---- Dense TSDF volume: fuse resident range images, raycast a model image ------------------- */

/* A truncated signed distance volume of nx x ny x nz voxels of pitch v, the centre of voxel (0, 0, 0) at `origin` in the
 * world, owned by its context like a voxel map.  Storage, x fastest: one 8-byte record {f32 D, f32 W} per voxel (D: the
 * fused distance in units of the truncation tau, W: the number of observations, an integer held exactly in f32) and, with
 * colours, a plane of one u32 r | g << 8 | b << 16 per voxel.  A new or cleared volume is all zero bytes (clearing is one
 * fill); W == 0 is "never observed".  All device arithmetic below is f32 with every operation rounded on its own; poses go
 * through Transform::transform_vector / transform_normal (src/transform.rs:138-153), the quaternion form.  Every call is
 * host-synchronous and ordered on the context's stream; results depend neither on launch geometry nor on how often a call
 * runs.  The surface leaves the volume as a triangle mesh or a point cloud through a3d_tsdf_volume_extract_surface below.
 * Hashed or sparse volumes, marching cubes, along-ray distances, weights by angle or depth and de-integration are NOT built.
 * a3d_tsdf_volume_new: decided on the host before anything is allocated (A3D_INVALID_PARAMETER, *out untouched): a NULL
 * ctx, origin or out; a dimension outside [2, 1024]; voxel_size, truncation or an origin component that is not finite;
 * voxel_size <= 0 or truncation <= 0; max_weight outside [1, 2^24].  Device memory: 8 (+ 4 with colours) bytes per voxel. */
typedef struct a3d_tsdf_volume a3d_tsdf_volume;
a3d_status a3d_tsdf_volume_new(a3d_context* ctx, uint64_t nx, uint64_t ny, uint64_t nz, float voxel_size,
                               const float origin[3], float truncation, uint64_t max_weight, int with_colors,
                               a3d_tsdf_volume** out);
void a3d_tsdf_volume_free(a3d_tsdf_volume* volume);
/* Every record and colour back to zero bytes; the allocation stays. */
a3d_status a3d_tsdf_volume_clear(a3d_tsdf_volume* volume);
/* What the volume was made with (any output may be NULL). */
a3d_status a3d_tsdf_volume_info(const a3d_tsdf_volume* volume, uint64_t out_dims[3], float* out_voxel_size,
                                float* out_truncation, float out_origin[3], uint64_t* out_max_weight,
                                int32_t* out_with_colors);
/* Fuses n >= 1 resident images, image f seen from world_to_camera_host[f] (PinholeCamera's world_to_camera), in order.
 * The rule, per voxel (i, j, k), for f = 0 ... n-1 in that order (fx, fy, cx, cy: image f's intrinsics cast to f32 once):
 *   1. pw = (ox + (float)i * v, oy + (float)j * v, oz + (float)k * v).
 *   2. pc = transform_vector(world_to_camera[f], pw); z = pc.z; the frame is skipped unless z > 0 and z < +inf.
 *   3. u = pc.x * fx / z + cx, v_ = pc.y * fy / z + cy; ui = round(u), vi = round(v_), halves away from zero; skipped unless
 *      0 <= ui < width and 0 <= vi < height compared as f32: steps 3-4 of a3d_point_cloud_render_device
 *      (src/camera.rs:177-202).
 *   4. skipped if mask[vi][ui] == 0; dz = points[vi][ui].z; skipped unless dz > 0 and dz < +inf.
 *   5. sdf = dz - z; skipped if sdf < -tau; d = min(1, sdf / tau).
 *   6. Wn = W + 1; D = (D * W + d) / Wn; W = min(Wn, max_weight).
 *   7. with colours, per channel c of the voxel and c_in of colors[vi][ui]: c = (u8)floor((c * W_old + c_in) / Wn + 0.5),
 *      W_old the W step 6 started from.
 * One thread per voxel keeps the record in registers over the frames of a launch: a call costs one read and at most one
 * write of the volume per 64 frames (the host cuts n into chunks of at most 64, in order; the result is the rule's
 * whatever the cut), and a voxel no frame touched is not written.
 * Decided on the host before anything is launched, and then the volume is unchanged: a NULL volume, images, poses or
 * image, n == 0, an image of another context -> A3D_INVALID_PARAMETER; an image without colours offered to a volume with
 * colours -> A3D_MISSING_FIELD. */
a3d_status a3d_tsdf_volume_integrate(a3d_tsdf_volume* volume, const a3d_device_image* const* images,
                                     const a3d_pose* world_to_camera_host, uint64_t n);
/* The model image a pinhole camera at camera_to_world_host sees: one ray per pixel, sampled at fixed depths.  The rule, per
 * pixel (row, col), with the intrinsics cast to f32 once, g(p) = (transform_vector(camera_to_world, p) - origin) / v per
 * component, and world_to_camera = (q* = (-i, -j, -k, w), -(q* rotating t)) computed once on the host in f32:
 *   1. xn = ((float)col - cx) / fx, yn = ((float)row - cy) / fy.
 *   2. sample k = 0 ... K-1 is at z_k = z_near + (float)k * step (not accumulated), at g_k = g((xn * z_k, yn * z_k, z_k));
 *      K = floor((z_far - z_near) / step) + 1, computed on the host in f64 from the f32 values.
 *   3. tri(g), the trilinear sample: i0 = floor(g.x), j0, k0 likewise; valid iff 0 <= i0 and i0 + 1 <= nx - 1, the same
 *      for j0 and k0, tested in f32 (a NaN fails), AND all eight corner voxels have W > 0; its value is
 *      lerp(a, b, t) = a + t * (b - a) over the corners' D along x first, then y, then z, with t = g - floor(g).
 *   4. walking k upwards, an invalid sample forgets the previous one; a valid sample D after a valid sample D_prev:
 *      D_prev > 0 and D <= 0 is a HIT; D_prev <= 0 and D > 0 ends the ray without one (it left a surface from behind); a
 *      first valid sample with D <= 0 is never a hit.
 *   5. on a hit: s = D_prev / (D_prev - D), z* = z_prev + (z_k - z_prev) * s; the pixel gets mask 1 and the point
 *      p* = (xn * z*, yn * z*, z*).
 *   6. the normal: g* = g(p*), G = (tri(g* + ex) - tri(g* - ex), the same with ey, with ez) at unit voxel offsets,
 *      len = sqrt(Gx * Gx + Gy * Gy + Gz * Gz) summed left to right; +0 if one of the six samples is invalid or len is 0 or
 *      not finite (every aligner's angle gate rejects it; the mask stays 1), else transform_normal(world_to_camera, G / len).
 *      D grows towards the camera: a wall seen head-on gets (0, 0, -1), RangeImage::compute_normals' sign
 *      (src/range_image/structure.rs:250).
 *   7. the colour is that of voxel round(g*), halves away from zero, clamped into the volume; 0, 0, 0 without colours.
 *   8. a pixel without a hit gets mask 0, +0 points and normals and colour 0, 0, 0.
 * There is no empty-space skipping: it would change which samples a ray sees.  *out_image: an ordinary image on the
 * volume's context (a3d_range_image_free) that carries fx, fy, cx, cy as given, always has normals, has colours iff the
 * volume has them and no intensities.  One thread per pixel, one launch.
 * Decided on the host before anything is launched or allocated (A3D_INVALID_PARAMETER, *out_image untouched): a NULL
 * volume, pose or out_image; the camera refusals of a3d_point_cloud_render_device; z_near, z_far or step not finite,
 * z_near <= 0, z_far <= z_near, step <= 0; K > 4096. */
a3d_status a3d_tsdf_volume_raycast(a3d_tsdf_volume* volume, const a3d_pose* camera_to_world_host, double fx, double fy,
                                   double cx, double cy, uint64_t width, uint64_t height, float z_near, float z_far,
                                   float step, a3d_device_image** out_image);
/* The volume to HOST memory, for tests: out_records [nz][ny][nx][2] f32 (D, W), out_colors [nz][ny][nx] u32 (NULL ok; non-NULL
 * on a volume without colours -> A3D_MISSING_FIELD).  A NULL volume or out_records is A3D_INVALID_PARAMETER. */
a3d_status a3d_tsdf_volume_download(a3d_tsdf_volume* volume, float* out_records, uint32_t* out_colors);
/* The inverse of a3d_tsdf_volume_download: every record (and, with `colors`, every colour) of the volume from HOST memory,
 * bit for bit, NaN included: records [nz][ny][nx][2] f32 (D, W), colors [nz][ny][nx] u32 (NULL: the colours stay as they
 * are; non-NULL on a volume without colours -> A3D_MISSING_FIELD).  A NULL volume or records is A3D_INVALID_PARAMETER.  It
 * restores a saved volume, and lets a test set any field: exact zeros, -0, ties, holes.  W is an integer count in
 * [0, 2^24]: after an upload of a W that is negative, not an integer or not finite, the results of integrate and raycast
 * are unspecified.  Any D, NaN and the infinities included, follows the rules as they are written; a hit whose D_prev is
 * +inf has s = NaN, so its point is NaN and its colour is unspecified. */
a3d_status a3d_tsdf_volume_upload(a3d_tsdf_volume* volume, const float* records, const uint32_t* colors);
/* The volume's surface, independent of any viewpoint: a vertex on every crossing edge, with the field's gradient as its
 * normal and a voxel's colour, and (want_faces != 0) triangles by marching TETRAHEDRA on the Kuhn split of every cell, not
 * marching cubes: the split matches across neighbouring cells, has no ambiguous case and its table is derived from the
 * paragraph below, at the price of about twice the triangles.  The rule, all of it f32, every operation rounded on its own:
 *   1. Voxel (i, j, k) is VALID iff W >= min_weight and |D| < +inf (a NaN fails both); a valid voxel is INSIDE iff D <= 0
 *      (-0 is inside: the side the raycast's hit test uses).
 *   2. Edge class c = 1 ... 7 has the offset e_c = (c & 1, c >> 1 & 1, c >> 2 & 1).  Voxel a OWNS the edges from a to
 *      b = a + e_c for every c whose b lies in the volume: three axis edges, three face diagonals, one body diagonal.  An
 *      edge CROSSES iff both ends are valid and exactly one is inside.
 *   3. The vertex of a crossing edge: t = Da / (Da - Db); the voxel coordinate g* = ((float)i + t * ex, (float)j + t * ey,
 *      (float)k + t * ez) with e_c as floats; the point is origin + g* * v per component, in the WORLD frame.  The normal is
 *      step 6 of the raycast rule taken at g* directly with no pose applied: G from six tri() samples at unit voxel
 *      offsets (tri unchanged, its W > 0 test included), len = sqrt(Gx * Gx + Gy * Gy + Gz * Gz) summed left to right, the
 *      normal G / len, or +0 where a sample is invalid or len is 0 or not finite; it points towards growing D, out of the
 *      surface.  The colour is that of voxel round(g*), halves away from zero, clamped into the volume (step 7 there).
 *   4. Vertices are ordered by ascending (voxel number with x fastest, class); a vertex's rank is its index.  The point-cloud
 *      form (want_faces == 0) keeps classes 1, 2 and 4 only, the axis edges (Open3D's extract_point_cloud points), in the
 *      same relative order; the mesh form keeps all seven.
 *   5. Triangles.  A cell a (0 <= i < nx - 1, likewise j and k) gives triangles iff all eight corners are valid.  Its six
 *      tetrahedra come from the axis permutations (p, q, r) in the order xyz, xzy, yxz, yzx, zxy, zyx: v0 = a, v1 = a + e_p,
 *      v2 = v1 + e_q, v3 = a + (1, 1, 1) (e_p: the unit step along axis p).  Every tetrahedron edge is an owned edge of its
 *      lower end, so a triangle corner is (owner voxel, class).  With S the set of inside vertices: |S| = 0 or 4 gives no
 *      triangle; |S| = 1 or 3: the lone vertex L and the others A < B < C (local numbers) give the triangle on the edges
 *      LA, LB, LC; |S| = 2: inside P < Q and outside A < B give the quad PA, PB, QB, QA, split into (PA, PB, QB) and
 *      (PA, QB, QA).  Winding: with the crossings put at the edge midpoints of the unit cell, if
 *      (p1 - p0) x (p2 - p0) . (centroid of the outside vertices - centroid of the inside vertices) is negative the last
 *      two corners are swapped, each triangle of a quad by the same test: counter-clockwise seen from outside.  The 6 x 16
 *      table this gives is plain data in tsdf_surface.hip.  Triangles are ordered by ascending (cell's voxel number,
 *      tetrahedron, triangle); degenerate ones (t is 0 or 1 where a D is exactly 0) are kept.
 * Outputs, DEVICE memory on the volume's context: d_out_points [vertex_capacity][3] f32, d_out_normals the same or NULL,
 * d_out_colors [vertex_capacity][3] u8 or NULL (non-NULL on a volume without colours -> A3D_MISSING_FIELD), d_out_faces
 * [face_capacity][3] u32 vertex indices; with want_faces == 0 the face arguments are ignored and *out_faces is 0.
 * *out_vertices / *out_faces: the counts.  NULL d_out_points and d_out_faces with capacities 0 is a COUNT-ONLY call: only
 * the counting passes run and the status is A3D_OK.  Otherwise, if either count exceeds its capacity the call returns
 * A3D_INVALID_PARAMETER with both counts set and NOTHING written; a count of 2^32 - 1 or more is refused the same way (in
 * a count-only call too).  Decided on the host before any launch (A3D_INVALID_PARAMETER, the counts untouched): a NULL
 * volume or count pointer; min_weight outside [1, 2^24]; a NULL d_out_points with a vertex capacity above 0 or with
 * another vertex output; a NULL d_out_faces with a face capacity above 0; outputs (taken at their capacities) that overlap
 * each other or the volume.  Host-synchronous; four launches at most whatever the volume's size (count, one block's scan
 * of the block sums, vertices, triangles) and two waits; 5 bytes of context scratch per voxel (a mask byte and two 16-bit
 * offsets inside the voxel's block of 256) plus 12 bytes per block.  Neither result depends on launch geometry, on
 * scheduling, on what scratch holds or on how often the call runs; the volume is never changed. */
a3d_status a3d_tsdf_volume_extract_surface(a3d_tsdf_volume* volume, uint64_t min_weight, int want_faces, float* d_out_points,
                                           float* d_out_normals /* NULL ok */, uint8_t* d_out_colors /* NULL ok */,
                                           uint64_t vertex_capacity, uint32_t* d_out_faces, uint64_t face_capacity,
                                           uint64_t* out_vertices, uint64_t* out_faces);

/* ---- Aligning against the volume: the field query and point-to-SDF ICP ---------------------- */

/* A signed distance field is an alignment target with no association step: it tells every point how far it is from the
 * surface and in which direction (the frame-to-model tracker of Bylow et al. and Canelhas' SDF tracker).  The rule, for a
 * query point q in the WORLD frame, after its optional pose (Transform::transform_vector); all of it f32, every operation
 * rounded on its own:
 *   1. g = (q - origin) / v per component: the raycast rule's g() without the camera.
 *   2. D = tri(g), step 3 of the raycast rule unchanged: the inside-the-volume test in f32, all eight corners W > 0, the
 *      lerp order x, y, z.  An invalid sample means NO VALUE.
 *   3. The sample is NO CORRESPONDENCE unless |D| < 1: at the truncation the field is clamped and carries no direction.
 *      A NaN fails.
 *   4. The gradient is step 6 of the raycast rule at g: G = (tri(g + ex) - tri(g - ex), the same with ey, with ez) at unit
 *      voxel offsets, len = sqrt(Gx * Gx + Gy * Gy + Gz * Gz) summed left to right; no correspondence if one of the six
 *      samples is invalid or len is 0 or not finite; otherwise n = G / len, in the WORLD frame (nothing is rotated back).
 *      D grows towards free space, so n points out of the surface, the way a frame cloud's normals do.
 *   5. d = D * tau is the signed metric distance; the associated point is t = (q.x - d * n.x, q.y - d * n.y,
 *      q.z - d * n.z), its normal is n and its squared distance is d2 = d * d.
 * Where the volume was fused from range images D is the PROJECTIVE distance along the viewing rays, so d overstates the
 * distance to a surface seen at a slant; near the surface the zero set and the direction are what the alignment uses.
 * This is NOT Icp over a3d_tsdf_volume_extract_surface's point cloud, which associates by a kd-tree: there is no parity
 * with it, only the rule above.  Weights by distance or angle, a robust kernel, colour terms, several sources per call, a
 * coarse-to-fine schedule and an analytic one-cell gradient are NOT built.
 * All entries are host-synchronous and ordered on the context's stream like the other volume calls; the volume is never
 * written, so clear, upload and integrate may follow. */

/* The field query of steps 1-5 for m resident points, one launch: d_queries [m][3] f32, pose_host NULL = the queries as
 * they are, bit for bit; d_out_distance [m] f32 gets d and d_out_normals [m][3] f32 gets n.  A point with no value gets
 * the distance bits 0x7FC00000 and the normal +0, +0, +0.  A point with a value but no direction (|D| >= 1 or a failure
 * of step 4) keeps its d and gets the +0 normal; a d that is a NaN (an uploaded NaN or infinity among the corners) is
 * written as 0x7FC00000 too, and d = -0 is kept as -0.  Clearance and collision queries against the fused model are this
 * call.  m == 0 is A3D_OK and touches nothing.  Decided on the host before any launch: a NULL volume, or with m > 0 a NULL
 * d_queries, d_out_distance or d_out_normals, m >= 2^31, and outputs that overlap each other or the queries are
 * A3D_INVALID_PARAMETER. */
a3d_status a3d_tsdf_volume_sample_device(a3d_tsdf_volume* volume, const float* d_queries, uint64_t m,
                                         const a3d_pose* pose_host, float* d_out_distance, float* d_out_normals);
/* Frame-to-model ICP: Icp::align's loop (src/icp/pcl_icp.rs:59-106) with the field query above in place of the kd-tree,
 * started from initial_host (NULL = Transform::eye()): the returned pose maps the source AS GIVEN into the volume's world
 * frame.  Per source point: p = q is the point under the pose, sn its normal under the pose (transform_normal), and the
 * associated point t, its normal n and d2 of step 5 go through the per-point tail of a3d_pcl_icp_align_device as it is:
 * the gate max_distance squared against d2 (reject iff d2 > it), the strict normal-angle gate on sn . n, the residual
 * (t - p) . n, the Jacobian [n, p x n], the weight, max_iterations (0 returns the initial pose bit for bit), the best-pose
 * rule and the solve-failure status: A3D_SOLVE_FAILED when no point passes, with the pose reached so far in out_pose.
 * d_source: DEVICE pointers on the volume's context, read during the call.  The launch geometry follows the source length
 * and the device only, never the volume's size.  The working buffers (two states, two partial sets, the out pose; a few
 * hundred bytes per CU) belong to the volume: allocated on first use, freed with it.
 * Decided on the host before any launch, in this order: a NULL volume, params, d_source, d_source->points or out_pose
 * -> A3D_INVALID_PARAMETER; a source with len == 0 or len >= 2^31 -> A3D_INVALID_PARAMETER; a source without normals ->
 * A3D_MISSING_FIELD. */
a3d_status a3d_tsdf_volume_icp_align_device(a3d_tsdf_volume* volume, const a3d_icp_params* params,
                                            const a3d_point_cloud_view* d_source, const a3d_pose* initial_host,
                                            a3d_pose* out_pose);
/* One pass of that per-point loop under `pose` (NULL = eye), summed in f64 as a3d_pcl_icp_accumulate: test hook.  The
 * same refusals. */
a3d_status a3d_tsdf_volume_icp_accumulate_device(a3d_tsdf_volume* volume, const a3d_icp_params* params,
                                                 const a3d_point_cloud_view* d_source, const a3d_pose* pose,
                                                 a3d_gn_state* out_state);
/* Instrumentation: device time (ms) of the iteration launches of the most recent a3d_tsdf_volume_icp_align_device. */
a3d_status a3d_tsdf_volume_icp_last_device_ms(a3d_tsdf_volume* volume, float* out_ms);

/* ---- R3dTree (src/kdtree.rs:19-106) ------------------------------------------------------- */

/* R3dTree::new(&points): `points` [n][3] f32 in host memory are uploaded and the tree is built ON THE DEVICE
 * (kdtree_select.hip: per level the point of rank len / 2 in the reference's own order and a partition around it, the
 * last levels sorted in LDS; leaf <= 16, mid = len / 2 — the same tree, bit for bit, as the reference's recursive build
 * with a stable sort per node). */
a3d_status a3d_kdtree_new(a3d_context* ctx, const float* points, uint64_t n, a3d_kdtree** out);
/* The same over points that are already resident: d_points [n][3] f32 in device memory of the context's GPU (the
 * layout of PointCloud::points, src/pointcloud.rs:8-12).  Read during the call only; the same tree, bit for bit. */
a3d_status a3d_kdtree_new_device(a3d_context* ctx, const void* d_points, uint64_t n, a3d_kdtree** out);
/* Instrumentation: which build made the tree: 1 selection build (kdtree_select.hip: the product's), 3 the same with one
 * more launch per upper level that places oversized median buckets chip-wide (a cloud from a depth image: a wall of
 * tens of thousands of equal coordinates; a new context's builds have it, drop it after four builds in a row without such a
 * bucket and take it up again with the next one — the tree is the same either way); diagnostics build only: 0 host build,
 * 2 sorting build (the cross-checks). */
a3d_status a3d_kdtree_build_path(a3d_kdtree* tree, int32_t* out_path);
/* Instrumentation: device time (ms) of the build's launches (first kernel to last, hipEvents on the context's stream;
 * without the upload of host points and without the allocation of the tree's arrays). */
a3d_status a3d_kdtree_build_ms(a3d_kdtree* tree, float* out_ms);
/* R3dTree::nearest for m queries (leaf-only search, no backtracking).  Host pointers.
 * out_indices are indices into the `points` given to a3d_kdtree_new. */
a3d_status a3d_kdtree_nearest(a3d_kdtree* tree, const float* queries, uint64_t m,
                              uint64_t* out_indices, float* out_sqr_distances);
/* Same with queries and results resident: d_queries [m][3] f32, d_indices [m] u32, d_sqr [m] f32. */
a3d_status a3d_kdtree_nearest_device(a3d_kdtree* tree, const void* d_queries, uint64_t m,
                                     void* d_indices, void* d_sqr_distances);
a3d_status a3d_kdtree_free(a3d_kdtree* tree);
/* Instrumentation: tree shape {leaves, internal nodes, depth of the deepest leaf}. */
a3d_status a3d_kdtree_stats(a3d_kdtree* tree, uint64_t out3[3]);
/* Instrumentation: the tree as laid out in HBM.  out_split: [2^depth - 1] f32 split values in heap order;
 * out_leaves: [2^depth * 16][4] f32 {x, y, z, index bits}, +inf in unused slots.  Either may be null; the
 * element counts are returned in out_counts {splits, leaf slots} (call with null arrays to size the buffers). */
a3d_status a3d_kdtree_download(a3d_kdtree* tree, float* out_split, float* out_leaves, uint64_t out_counts[2]);

/* ---- Icp (src/icp/pcl_icp.rs:15-108) ------------------------------------------------------ */

/* Icp::new(params, &target): builds the kd-tree over target.points; A3D_MISSING_FIELD is
 * deferred to align like the reference. */
a3d_status a3d_pcl_icp_new(a3d_context* ctx, const a3d_icp_params* params,
                           const a3d_point_cloud_view* target, a3d_pcl_icp** out);
/* Icp::align(&source): starts from Transform::eye() (initial_transform is ignored, pcl_icp.rs:59). */
a3d_status a3d_pcl_icp_align(a3d_pcl_icp* icp, const a3d_point_cloud_view* source,
                             a3d_pose* out_pose);
/* Icp::new / Icp::align over clouds that are already resident: the view's `points` / `normals` are DEVICE pointers
 * (same layout: [len][3] f32, src/pointcloud.rs:8-12) on the context's GPU.  The target's arrays are read during
 * a3d_pcl_icp_new_device only (tree and leaf normals are copies); the source's during a3d_pcl_icp_align_device, which
 * is host-synchronous like a3d_pcl_icp_align.  Same tree, same pose bits as the host-pointer forms; no PCIe traffic
 * except the 32-byte result (benches/bench_icp.rs:9-39 without the copies). */
a3d_status a3d_pcl_icp_new_device(a3d_context* ctx, const a3d_icp_params* params,
                                  const a3d_point_cloud_view* d_target, a3d_pcl_icp** out);
a3d_status a3d_pcl_icp_align_device(a3d_pcl_icp* icp, const a3d_point_cloud_view* d_source,
                                    a3d_pose* out_pose);
/* One pass of the per-point body (pcl_icp.rs:68-92) from `pose`: test hook. */
a3d_status a3d_pcl_icp_accumulate(a3d_pcl_icp* icp, const a3d_point_cloud_view* source,
                                  const a3d_pose* pose, a3d_gn_state* out_state);
/* Instrumentation: device time (ms) of the iteration launches of the most recent a3d_pcl_icp_align. */
a3d_status a3d_pcl_icp_last_device_ms(a3d_pcl_icp* icp, float* out_ms);
a3d_status a3d_pcl_icp_free(a3d_pcl_icp* icp);

/* P independent Icp::new(params, &target_p).align(&source_p) (src/icp/pcl_icp.rs:31-107) over clouds that are resident
 * in device memory, run as one launch sequence: every iteration is ONE launch for all pairs (grid = blocks per pair x
 * pairs).  Per pair the behaviour is a3d_pcl_icp_new_device + a3d_pcl_icp_align_device's: the same tree bit for bit, start
 * from Transform::eye(), the same per-point arithmetic; the block partials are grouped differently, so poses agree with
 * the one-pair form to rounding, not bit for bit.  Results do not depend on the order of the pairs in the batch. */

/* Icp::new for every pair (pcl_icp.rs:31-38): d_targets [n_pairs] views whose `points` / `normals` are DEVICE pointers,
 * read during this call only (trees and leaf normals are copies).  The trees are built back to back on the context's
 * stream and the call waits for the device once, after the last one.  One a3d_icp_params for all pairs.
 * Before anything is launched: a target with 0 or >= 2^31 points is A3D_INVALID_PARAMETER; a target without normals is
 * A3D_MISSING_FIELD (the `expect` of pcl_icp.rs:50-53, raised here instead of at align time); after the builds a NaN
 * coordinate is A3D_NAN_IN_INPUT.  The message names the pair.  n_pairs == 0 is A3D_OK: an empty batch that never
 * touches the context and whose align is a no-op. */
a3d_status a3d_pcl_icp_batch_new_device(a3d_context* ctx, const a3d_icp_params* params, uint64_t n_pairs,
                                        const a3d_point_cloud_view* d_targets, a3d_pcl_icp_batch** out);
/* Icp::align for every pair (pcl_icp.rs:47-107): d_sources [n_pairs] views of DEVICE pointers, read until the pass is
 * complete.  out_poses_host / out_status_host: [n_pairs] or NULL; with both NULL the call only enqueues (no host
 * sync; a3d_pcl_icp_batch_results reads the pass).  Returns A3D_OK when the pass ran: a pair whose
 * GaussNewton::solve() is None (pcl_icp.rs:96 `unwrap`s) has status A3D_SOLVE_FAILED, keeps the pose it had reached and
 * does not disturb the other pairs.  Before anything is launched: a source with len == 0 (or >= 2^31) is
 * A3D_INVALID_PARAMETER, a source without normals A3D_MISSING_FIELD (pcl_icp.rs:54-58); the message names the pair. */
a3d_status a3d_pcl_icp_batch_align_device(a3d_pcl_icp_batch* batch, const a3d_point_cloud_view* d_sources,
                                          a3d_pose* out_poses_host, int32_t* out_status_host);
/* Results of the most recent pass of `batch` (the same contract as a3d_multiscale_batch_results): waits for that pass
 * only. */
a3d_status a3d_pcl_icp_batch_results(a3d_pcl_icp_batch* batch, a3d_pose* out_poses_host, int32_t* out_status_host);
/* Instrumentation: device time (ms) of the most recent pass, between hipEvents round its launches (as
 * a3d_pcl_icp_last_device_ms); waits for that pass. */
a3d_status a3d_pcl_icp_batch_last_device_ms(a3d_pcl_icp_batch* batch, float* out_ms);
/* Drop for the batch (the Icp objects of pcl_icp.rs:15-20 and their R3dTree). */
a3d_status a3d_pcl_icp_batch_free(a3d_pcl_icp_batch* batch);

/* ---- BilateralFilter<u16> (src/bilateral/edge_aware_filter.rs:30-135, grid.rs:32-162) ----- */

/* BilateralFilter::default() sigmas (edge_aware_filter.rs:30-36). */
void a3d_bilateral_default_sigmas(double* out_sigma_space, double* out_sigma_color);
/* BilateralFilter::new(sigma_space, sigma_color).filter(&image): u16 [height][width] in and out,
 * host pointers.  out_grid_dims (nullable) receives GH, GW, GD. */
a3d_status a3d_bilateral_filter_u16(a3d_context* ctx, const uint16_t* image, uint64_t width,
                                    uint64_t height, double sigma_space, double sigma_color,
                                    uint16_t* out_image, uint64_t out_grid_dims[3]);
/* The same filter (edge_aware_filter.rs:126-135) for images that are already in DEVICE memory: n_images images
 * [n][height][width] u16 in, the same layout out (d_out may not alias d_images); the shape of benches/bench_bilateral.rs
 * without PCIe in it.  Images below 2^24 pixels.  With a3d_context_set_build_profiling on, the device time of the call's
 * launch sequences is left in a3d_context_last_build_kernel_ms. */
a3d_status a3d_bilateral_filter_u16_device(a3d_context* ctx, const uint16_t* d_images, uint64_t n_images,
                                           uint64_t width, uint64_t height, double sigma_space, double sigma_color,
                                           uint16_t* d_out);

#ifdef __cplusplus
}
#endif
#endif /* ALIGN3D_HIP_H */
