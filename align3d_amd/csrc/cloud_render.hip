// PinholeCamera::project_to_image (src/camera.rs:177-202) over a whole resident cloud: the inverse of
// PointCloud::from(&RangeImage).  A cloud (or the live voxel map) and a pinhole camera at a pose give the resident
// RangeImage that camera would see: per pixel the nearest row that projects onto it, with its point, normal and colour.
// The rule is stated in align3d_hip.h (a3d_point_cloud_render_device); all of it is f32, every operation rounded on its
// own, and the winner of a pixel is the minimum of bits(z) << 32 | row over all rows, so the image does not depend on
// launch geometry, scheduling or how often the call runs.
//
// Three launches whatever the sizes, no LDS, no block waits on another:
//  1. the z-buffer ([h][w] u64 in the context's scratch region 5) is filled with ~0;
//  2. render_splat_kernel: one thread per row of the cloud (coalesced 12-byte loads as cloud_transform.hip); the row is
//     moved into the camera's frame, projected, rounded, and every pixel of its footprint gets a no-return 64-bit
//     atomic min of the key (relaxed, agent scope: a pixel's rows come from every XCD).  Keys only ever decrease, so a
//     plain agent-scope load that finds a smaller key already stored may skip the atomic (SplatForm::CHECKED: measured
//     slower, kept in the diagnostics build);
//  3. render_resolve_kernel: one thread per pixel reads the winner's row again and recomputes its point and normal with
//     the same inlined functions (camera_point / camera_normal), hence the bits step 2 keyed, and writes points, mask,
//     normals, colours (three byte stores, store_color) and the optional index plane; a pixel without a winner gets zeros.
// The map form extracts into the same scratch region inside the call and runs the same kernels on that cloud.
#include <cmath>
#include <vector>

#include "cloud_batch.hpp"
#include "voxel_map.hpp"

using namespace a3d;

namespace {

constexpr uint32_t RD_THREADS = 256;
constexpr uint64_t RD_EMPTY = ~0ull;       // a z-buffer slot no row has reached (no key equals it: row <= 2^32 - 2)
constexpr uint32_t RD_NO_ROW = 0xFFFFFFFFu;  // the index plane of a pixel without a winner
constexpr size_t RD_COLOR_SLACK = 16;      // bytes readable past a colour plane's end, as a3d_range_image_set_colors leaves
constexpr float RD_MAX_HALF = (float)A3D_RENDER_MAX_HALF_WIDTH;

#define RD_GLOBAL __attribute__((address_space(1)))

// How a footprint pixel is offered its key.  Measured on MI355X (scripts/cloud_render_probe.py): the load
// that may skip the atomic puts an L2 round trip in front of every pixel of a lane's footprint loop, and the map at
// radius v / 2 into 640 x 480 takes 3.1 x the time of the atomics alone, which the memory side absorbs in flight.
enum class SplatForm : uint32_t { ATOMIC = 0, CHECKED = 1 };
constexpr SplatForm RD_SPLAT = SplatForm::ATOMIC;

struct RenderJob {
  const float* points;
  const float* normals;   // null: the image has no normals
  const uint8_t* colors;  // null: the image has no colours
  uint32_t len, width, height, has_pose;
  float fx, fy, cx, cy, radius, pad;
  Pose pose;
};

// Step 1 of the rule: row k in the camera's frame (verbatim without a pose).  ONE definition for the splat, which keys
// the pixel with bits(z), and the resolve, which stores the point.
__device__ __forceinline__ V3 camera_point(const RenderJob& j, uint32_t k) {
  const f32x3 p = *(const RD_GLOBAL f32x3_u*)((const RD_GLOBAL float*)j.points + 3 * (size_t)k);
  const V3 v{p.x, p.y, p.z};
  return j.has_pose ? transform_vector(j.pose, v) : v;
}
__device__ __forceinline__ V3 camera_normal(const RenderJob& j, uint32_t k) {
  const f32x3 n = *(const RD_GLOBAL f32x3_u*)((const RD_GLOBAL float*)j.normals + 3 * (size_t)k);
  const V3 v{n.x, n.y, n.z};
  return j.has_pose ? transform_normal(j.pose, v) : v;
}

template <SplatForm FORM>
__global__ void __launch_bounds__(RD_THREADS) render_splat_kernel(const RenderJob j, unsigned long long* __restrict__ zbuf) {
  const uint64_t k64 = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
  if (k64 >= j.len) return;
  const uint32_t k = (uint32_t)k64;
  const V3 p = camera_point(j, k);
  const float z = p.z;
  if (!(z > 0.0f && z < INFINITY)) return;  // (NaN fails both)
  // CameraIntrinsics::project (camera.rs:64-70): the product first, then the IEEE quotient, then the sum
  const float u = p.x * j.fx / z + j.cx, v = p.y * j.fy / z + j.cy;
  const float ui = roundf(u), vi = roundf(v);  // f32::round: halves away from zero
  // camera.rs:196: compared as f32; -0.0 passes, NaN and the infinities fail
  if (!(ui >= 0.0f && ui < (float)j.width && vi >= 0.0f && vi < (float)j.height)) return;
  float hx = 0.0f, hy = 0.0f;
  if (j.radius != 0.0f) {
    hx = fminf(floorf(j.radius * j.fx / z), RD_MAX_HALF);
    hy = fminf(floorf(j.radius * j.fy / z), RD_MAX_HALF);
  }
  // ui < width < 2^31 and 0 <= hx <= 8: everything below fits a 64-bit integer with room to spare
  const int64_t col = (int64_t)ui, row = (int64_t)vi, dx = (int64_t)hx, dy = (int64_t)hy;
  const int64_t c0 = std::max<int64_t>(col - dx, 0), c1 = std::min<int64_t>(col + dx, (int64_t)j.width - 1);
  const int64_t r0 = std::max<int64_t>(row - dy, 0), r1 = std::min<int64_t>(row + dy, (int64_t)j.height - 1);
  const unsigned long long key = (unsigned long long)__float_as_uint(z) << 32 | k;
  for (int64_t r = r0; r <= r1; ++r) {
    unsigned long long* line = zbuf + (size_t)r * j.width;  // (r < height, c < width: inside the [h][w] plane)
    for (int64_t c = c0; c <= c1; ++c) {
      if (FORM == SplatForm::CHECKED &&
          __hip_atomic_load(line + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
        continue;  // keys only decrease: this one can no longer win
      (void)__hip_atomic_fetch_min(line + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // result unused: no return
    }
  }
}

__global__ void __launch_bounds__(RD_THREADS)
    render_resolve_kernel(const RenderJob j, const unsigned long long* __restrict__ zbuf, uint32_t npx,
                          float* __restrict__ out_points, uint8_t* __restrict__ out_mask, float* __restrict__ out_normals,
                          uint8_t* __restrict__ out_colors, uint32_t* __restrict__ out_index) {
  const uint32_t px = blockIdx.x * RD_THREADS + threadIdx.x;
  if (px >= npx) return;
  const unsigned long long key = zbuf[px];
  const bool won = key != RD_EMPTY;
  const uint32_t k = (uint32_t)key;
  f32x3 p{0.f, 0.f, 0.f}, n{0.f, 0.f, 0.f};
  uint32_t rgb = 0;
  if (won && k < j.len) {  // (a key always names a row of the cloud; kept as a bound on every load)
    const V3 v = camera_point(j, k);
    p = f32x3{v.x, v.y, v.z};
    if (out_normals) {
      const V3 w = camera_normal(j, k);
      n = f32x3{w.x, w.y, w.z};
    }
    if (out_colors) rgb = load_color(j.colors, k);
  }
  *(RD_GLOBAL f32x3_u*)((RD_GLOBAL float*)out_points + 3 * (size_t)px) = p;
  out_mask[px] = won ? 1 : 0;
  if (out_normals) *(RD_GLOBAL f32x3_u*)((RD_GLOBAL float*)out_normals + 3 * (size_t)px) = n;
  if (out_colors) store_color(out_colors, px, rgb);
  if (out_index) out_index[px] = won ? k : RD_NO_ROW;
}

SplatForm splat_setting() {
  uint32_t v = (uint32_t)RD_SPLAT;
  if (const char* env = A3D_DIAG_ENV("A3D_CLOUD_RENDER_SPLAT"))  // diagnostics build: the variant the probe times
    if (*env) v = (uint32_t)atoi(env);
  return v == 0 ? SplatForm::ATOMIC : v == 1 ? SplatForm::CHECKED : RD_SPLAT;
}

}  // namespace

// What the render entries (and the TSDF raycast, tsdf.hip) decide about the camera before anything is allocated or launched.
a3d_status a3d::check_camera(double fx, double fy, double cx, double cy, uint64_t width, uint64_t height, float radius) {
  A3D_REQUIRE(width >= 1 && height >= 1 && width < (1ull << 31) && height < (1ull << 31) && width * height < (1ull << 31),
              A3D_INVALID_PARAMETER, "render: the image has at least one pixel and fewer than 2^31");
  A3D_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), A3D_INVALID_PARAMETER,
              "render: the intrinsics must be finite");
  A3D_REQUIRE(std::isfinite((float)fx) && std::isfinite((float)fy) && std::isfinite((float)cx) && std::isfinite((float)cy) &&
                  (float)fx > 0.0f && (float)fy > 0.0f,
              A3D_INVALID_PARAMETER, "render: fx and fy must be positive (and finite) as f32");
  A3D_REQUIRE(std::isfinite(radius) && radius >= 0.0f, A3D_INVALID_PARAMETER, "render: the radius is finite and >= 0");
  return A3D_OK;
}

namespace {

// The image's arena, the three launches and the one wait.  `zbuf`: [h][w] u64 of the context's scratch.  The cloud's
// arrays may lie in that scratch region too (the map form).
a3d_status render_cloud(a3d_context* ctx, const a3d_point_cloud_view& cloud, const uint8_t* d_colors,
                        const a3d_pose* world_to_camera_host, double fx, double fy, double cx, double cy, uint32_t width,
                        uint32_t height, float radius, unsigned long long* zbuf, uint32_t* d_out_index,
                        a3d_device_image** out_image) {
  const size_t npx = (size_t)width * height;
  const bool with_normals = cloud.normals != nullptr, with_colors = d_colors != nullptr;
  size_t total = 0;
  auto take = [&](size_t bytes) {
    const size_t at = total;
    total += pad256(bytes);
    return at;
  };
  const size_t off_points = take(npx * 12), off_mask = take(npx);
  const size_t off_normals = with_normals ? take(npx * 12) : 0;
  const size_t off_colors = with_colors ? take(npx * 3 + RD_COLOR_SLACK) : 0;
  DeviceArena* arena = new DeviceArena();
  if (ctx_arena_acquire(ctx, total, arena) != A3D_OK) {
    delete arena;
    return A3D_HIP_ERROR;
  }
  a3d_device_image* im = new a3d_device_image();
  im->ctx = ctx, im->arena = arena;
  ++arena->refs;
  char* base = (char*)arena->base;
  im->width = width, im->height = height;
  im->fx64 = fx, im->fy64 = fy, im->cx64 = cx, im->cy64 = cy;
  im->fx = (float)fx, im->fy = (float)fy, im->cx = (float)cx, im->cy = (float)cy;
  im->points = (float*)(base + off_points), im->mask = (uint8_t*)(base + off_mask);
  if (with_normals) im->normals = (float*)(base + off_normals), im->has_normals = true;
  if (with_colors) im->colors = (uint8_t*)(base + off_colors);

  RenderJob j{};
  j.points = cloud.points, j.normals = cloud.normals, j.colors = d_colors;
  j.len = (uint32_t)cloud.len, j.width = width, j.height = height;
  j.fx = im->fx, j.fy = im->fy, j.cx = im->cx, j.cy = im->cy, j.radius = radius;
  if (world_to_camera_host) j.has_pose = 1, j.pose = pose_from_c(world_to_camera_host);

  hipStream_t s = ctx->stream;
  bool ok = hipMemsetAsync(zbuf, 0xFF, npx * 8, s) == hipSuccess;
  if (ok && j.len > 0) {
    const dim3 grid((uint32_t)(((uint64_t)j.len + RD_THREADS - 1) / RD_THREADS)), block(RD_THREADS);
#ifdef A3D_DIAGNOSTICS  // (the product library holds the one variant it launches)
    if (splat_setting() != RD_SPLAT)
      hipLaunchKernelGGL(render_splat_kernel<RD_SPLAT == SplatForm::CHECKED ? SplatForm::ATOMIC : SplatForm::CHECKED>, grid,
                         block, 0, s, j, zbuf);
    else
#endif
      hipLaunchKernelGGL(render_splat_kernel<RD_SPLAT>, grid, block, 0, s, j, zbuf);
    ok = hipGetLastError() == hipSuccess;
  }
  if (ok) {
    const dim3 grid((uint32_t)((npx + RD_THREADS - 1) / RD_THREADS)), block(RD_THREADS);
    hipLaunchKernelGGL(render_resolve_kernel, grid, block, 0, s, j, (const unsigned long long*)zbuf, (uint32_t)npx, im->points,
                       im->mask, im->normals, im->colors, d_out_index);
    ok = hipGetLastError() == hipSuccess;
  }
  // host-synchronous: the image is complete on return (its arena needs no fence), the cloud may be freed right after
  if (hipStreamSynchronize(s) != hipSuccess) ok = false;
  if (!ok) {
    set_error("render: HIP failure: %s", hipGetErrorString(hipGetLastError()));
    a3d_range_image_free(im);
    return A3D_HIP_ERROR;
  }
  *out_image = im;
  return A3D_OK;
}

}  // namespace

extern "C" {

a3d_status a3d_point_cloud_render_device(a3d_context* ctx, const a3d_point_cloud_view* d_cloud, const uint8_t* d_colors,
                                         const a3d_pose* world_to_camera_host, double fx, double fy, double cx, double cy,
                                         uint64_t width, uint64_t height, float radius, uint32_t* d_out_index,
                                         a3d_device_image** out_image) {
  A3D_REQUIRE(ctx && d_cloud && out_image, A3D_INVALID_PARAMETER, "null argument");
  A3D_TRY(check_camera(fx, fy, cx, cy, width, height, radius));
  A3D_REQUIRE(d_cloud->len <= 0xFFFFFFFEull, A3D_INVALID_PARAMETER, "a3d_point_cloud_render_device: more than 2^32 - 2 rows");
  A3D_REQUIRE(d_cloud->len == 0 || d_cloud->points, A3D_INVALID_PARAMETER, "null points pointer");
  const a3d_point_cloud_view cloud = *d_cloud;  // (len == 0: nothing is read, the fields only say what the image has)
  const uint64_t npx = width * height;
  if (d_out_index) {  // the index plane is the one output the caller owns: it may not lie over the cloud it is made from
    RangeRecorder ranges;
    ranges.out(d_out_index, npx * 4);
    ranges.in(cloud.points, cloud.len * 12), ranges.in(cloud.normals, cloud.len * 12), ranges.in(d_colors, cloud.len * 3);
    A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
                "a3d_point_cloud_render_device: the index plane overlaps the cloud");
  }
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 5, pad256(npx * 8), &region));
  return render_cloud(ctx, cloud, d_colors, world_to_camera_host, fx, fy, cx, cy, (uint32_t)width, (uint32_t)height, radius,
                      (unsigned long long*)region, d_out_index, out_image);
}

a3d_status a3d_voxel_map_render(a3d_voxel_map* map, const a3d_pose* world_to_camera_host, double fx, double fy, double cx,
                                double cy, uint64_t width, uint64_t height, float radius, uint32_t* d_out_index,
                                a3d_device_image** out_image) {
  A3D_REQUIRE(map && out_image, A3D_INVALID_PARAMETER, "null argument");
  A3D_TRY(check_camera(fx, fy, cx, cy, width, height, radius));
  a3d_context* ctx = map->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // scratch region 5: the z-buffer | the extract's points | normals | colours (the extract's own temporaries are region 3's)
  const uint64_t npx = width * height, cells = map->cells, rows = std::max<uint64_t>(cells, 1);
  const size_t z_bytes = pad256(npx * 8), p_bytes = pad256(rows * 12), c_bytes = pad256(rows * 3);
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 5, z_bytes + p_bytes + (map->with_normals ? p_bytes : 0) + (map->with_colors ? c_bytes : 0), &region));
  char* base = (char*)region;
  float* d_points = (float*)(base + z_bytes);
  float* d_normals = map->with_normals ? (float*)(base + z_bytes + p_bytes) : nullptr;
  uint8_t* d_colors = map->with_colors ? (uint8_t*)(base + z_bytes + p_bytes + (map->with_normals ? p_bytes : 0)) : nullptr;
  uint64_t len = 0;
  // (read-only on the map, host-synchronous; the row index of the image is the extract's row)
  A3D_TRY(a3d_voxel_map_extract_rgb(map, d_points, d_normals, d_colors, nullptr, cells, &len));
  a3d_point_cloud_view cloud{d_points, d_normals, len};
  return render_cloud(ctx, cloud, d_colors, world_to_camera_host, fx, fy, cx, cy, (uint32_t)width, (uint32_t)height, radius,
                      (unsigned long long*)region, d_out_index, out_image);
}

}  // extern "C"
