// A dense truncated signed distance volume: resident range images are fused into it (KinectFusion's projective update, a
// running mean along the viewing ray) and a pinhole camera raycasts a dense model image out of it.  The rules are stated
// in align3d_hip.h (a3d_tsdf_volume_integrate / a3d_tsdf_volume_raycast); all of it is f32, every operation rounded on its
// own, and neither result depends on launch geometry or on how often a call runs: a voxel is written by its own thread
// only, a pixel by its own thread only, and nothing is summed across threads.
//
//  * tsdf_integrate_kernel: one thread per voxel, voxels numbered with x fastest, so a wave reads (and writes) 64 records,
//    512 contiguous bytes, whatever nx is.  The frame loop runs INSIDE the thread with the record in registers: up to 64
//    frames cost one read and at most one write of the volume, and a voxel no frame touched is not stored.  The frames'
//    constants (pose, intrinsics, plane pointers) are a job table in the context's scratch region 3, read through
//    wave-uniform addresses.  No frustum culling by block: the product path holds nothing that could change a bit.
//  * tsdf_raycast_kernel: one thread per pixel, one launch; K fixed-depth samples, eight records per sample, no
//    empty-space skipping (it would change which samples a ray sees).  The image is built as cloud_render.hip builds its
//    own (an arena of the context's pool), so it is a first-class a3d_device_image.
#include <cmath>
#include <vector>

#include "tsdf.hpp"

using namespace a3d;

namespace {

constexpr uint32_t TS_THREADS = 256;
constexpr uint32_t TS_MIN_DIM = 2, TS_MAX_DIM = 1024;  // 2^30 voxels at most: a voxel's number fits 32 bits
constexpr uint64_t TS_CHUNK = 64;                      // frames per launch
constexpr double TS_MAX_SAMPLES = 4096.0;
constexpr size_t TS_COLOR_SLACK = 16;  // bytes readable past a colour plane's end, as a3d_range_image_set_colors leaves

struct TsdfFrame {
  const float* points;    // [h][w][3], the camera's frame
  const uint8_t* mask;    // [h][w]
  const uint8_t* colors;  // [h][w][3] or null
  uint32_t width, height;
  float fx, fy, cx, cy;
  Pose pose;  // world_to_camera
  uint32_t pad;
};

template <bool COLORS>
__global__ void __launch_bounds__(TS_THREADS)
    tsdf_integrate_kernel(const TsdfGrid g, const TsdfFrame* __restrict__ frames, uint32_t n_frames) {
  const uint32_t idx = blockIdx.x * TS_THREADS + threadIdx.x;  // (total <= 2^30: no wrap)
  if (idx >= g.total) return;
  const uint32_t i = idx % g.nx, line = idx / g.nx, j = line % g.ny, k = line / g.ny;
  const V3 pw{g.ox + (float)i * g.v, g.oy + (float)j * g.v, g.oz + (float)k * g.v};
  const float2 rec = g.records[idx];
  float D = rec.x, W = rec.y;
  uint32_t rgb = 0;
  bool touched = false;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const TsdfFrame& fr = frames[f];  // (a wave-uniform address)
    const V3 pc = transform_vector(fr.pose, pw);
    const float z = pc.z;
    if (!(z > 0.0f && z < INFINITY)) continue;  // (NaN fails both)
    // CameraIntrinsics::project (camera.rs:64-70) and f32::round, as render_splat_kernel
    const float u = pc.x * fr.fx / z + fr.cx, v_ = pc.y * fr.fy / z + fr.cy;
    const float ui = roundf(u), vi = roundf(v_);
    if (!(ui >= 0.0f && ui < (float)fr.width && vi >= 0.0f && vi < (float)fr.height)) continue;
    const size_t px = (size_t)(uint32_t)vi * fr.width + (uint32_t)ui;  // (inside the [h][w] planes)
    if (fr.mask[px] == 0) continue;
    const float dz = fr.points[3 * px + 2];
    if (!(dz > 0.0f && dz < INFINITY)) continue;
    const float sdf = dz - z;
    if (sdf < -g.tau) continue;
    const float d = fminf(1.0f, sdf / g.tau);
    const float Wn = W + 1.0f;
    if (COLORS) {
      if (!touched) rgb = g.colors[idx];
      const uint32_t in = load_color(fr.colors, px);
      uint32_t out = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float old = (float)((rgb >> (8 * c)) & 0xFFu), add = (float)((in >> (8 * c)) & 0xFFu);
        out |= ((uint32_t)floorf((old * W + add) / Wn + 0.5f) & 0xFFu) << (8 * c);
      }
      rgb = out;
    }
    D = (D * W + d) / Wn;
    W = fminf(Wn, g.max_weight);
    touched = true;
  }
  if (touched) {
    g.records[idx] = float2{D, W};
    if (COLORS) g.colors[idx] = rgb;
  }
}

struct RayJob {
  Pose camera_to_world, world_to_camera;
  float fx, fy, cx, cy, z_near, step;
  uint32_t width, height, samples;
};

// g(p) of the rule: a camera-frame point in voxel coordinates.
__device__ __forceinline__ V3 voxel_coordinate(const TsdfGrid& g, const RayJob& j, V3 pc) {
  const V3 pw = transform_vector(j.camera_to_world, pc);
  return V3{(pw.x - g.ox) / g.v, (pw.y - g.oy) / g.v, (pw.z - g.oz) / g.v};
}

__global__ void __launch_bounds__(TS_THREADS)
    tsdf_raycast_kernel(const TsdfGrid g, const RayJob j, uint32_t npx, float* __restrict__ out_points,
                        uint8_t* __restrict__ out_mask, float* __restrict__ out_normals, uint8_t* __restrict__ out_colors) {
  const uint32_t px = blockIdx.x * TS_THREADS + threadIdx.x;
  if (px >= npx) return;
  const uint32_t row = px / j.width, col = px % j.width;
  const float xn = ((float)col - j.cx) / j.fx, yn = ((float)row - j.cy) / j.fy;
  bool have_prev = false, hit = false;
  float D_prev = 0.0f, z_prev = 0.0f, D = 0.0f, z_k = 0.0f;
  for (uint32_t k = 0; k < j.samples; ++k) {
    z_k = j.z_near + (float)k * j.step;
    if (!tri(g, voxel_coordinate(g, j, V3{xn * z_k, yn * z_k, z_k}), &D)) {
      have_prev = false;
      continue;
    }
    if (have_prev) {
      if (D_prev > 0.0f && D <= 0.0f) {
        hit = true;
        break;
      }
      if (D_prev <= 0.0f && D > 0.0f) break;  // it left a surface from behind
    }
    have_prev = true, D_prev = D, z_prev = z_k;
  }
  f32x3 p{0.f, 0.f, 0.f}, n{0.f, 0.f, 0.f};
  uint32_t rgb = 0;
  if (hit) {
    const float s = D_prev / (D_prev - D);
    const float zs = z_prev + (z_k - z_prev) * s;
    const V3 ps{xn * zs, yn * zs, zs};
    p = f32x3{ps.x, ps.y, ps.z};
    const V3 gs = voxel_coordinate(g, j, ps);
    float xp, xm, yp, ym, zp, zm;
    // (bitwise on purpose: all six samples are taken, as the rule states them)
    const bool all = tri(g, V3{gs.x + 1.0f, gs.y, gs.z}, &xp) & tri(g, V3{gs.x - 1.0f, gs.y, gs.z}, &xm) &
                     tri(g, V3{gs.x, gs.y + 1.0f, gs.z}, &yp) & tri(g, V3{gs.x, gs.y - 1.0f, gs.z}, &ym) &
                     tri(g, V3{gs.x, gs.y, gs.z + 1.0f}, &zp) & tri(g, V3{gs.x, gs.y, gs.z - 1.0f}, &zm);
    if (all) {
      const V3 G{xp - xm, yp - ym, zp - zm};
      const float len = sqrtf(G.x * G.x + G.y * G.y + G.z * G.z);
      if (len > 0.0f && len < INFINITY) {
        const V3 w = transform_normal(j.world_to_camera, G / len);
        n = f32x3{w.x, w.y, w.z};
      }
    }
    if (out_colors)
      rgb = g.colors[((size_t)clamped_voxel(gs.z, g.nz) * g.ny + clamped_voxel(gs.y, g.ny)) * g.nx + clamped_voxel(gs.x, g.nx)];
  }
  *(f32x3_u*)(out_points + 3 * (size_t)px) = p;
  out_mask[px] = hit ? 1 : 0;
  *(f32x3_u*)(out_normals + 3 * (size_t)px) = n;
  if (out_colors) store_color(out_colors, px, rgb);
}

// Transform::inverse in f32: q* = (-i, -j, -k, w), t' = -(q* rotating t).
Pose pose_inverse(const Pose& p) {
  const Quat qc{-p.q.i, -p.q.j, -p.q.k, p.q.w};
  const V3 t = rotate(qc, p.t);
  return Pose{{-t.x, -t.y, -t.z}, qc};
}

}  // namespace

extern "C" {

a3d_status a3d_tsdf_volume_new(a3d_context* ctx, uint64_t nx, uint64_t ny, uint64_t nz, float voxel_size,
                               const float origin[3], float truncation, uint64_t max_weight, int with_colors,
                               a3d_tsdf_volume** out) {
  A3D_REQUIRE(ctx && origin && out, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(nx >= TS_MIN_DIM && nx <= TS_MAX_DIM && ny >= TS_MIN_DIM && ny <= TS_MAX_DIM && nz >= TS_MIN_DIM && nz <= TS_MAX_DIM,
              A3D_INVALID_PARAMETER, "a3d_tsdf_volume_new: every dimension lies in [2, 1024]");
  A3D_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.f, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_new: the voxel size must be finite and positive");
  A3D_REQUIRE(std::isfinite(truncation) && truncation > 0.f, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_new: the truncation must be finite and positive");
  A3D_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_new: the origin must be finite");
  A3D_REQUIRE(max_weight >= 1 && max_weight <= TS_MAX_WEIGHT, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_new: max_weight lies in [1, 2^24]");
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  const size_t total = (size_t)nx * ny * nz, rec_bytes = pad256(total * sizeof(float2));
  const size_t bytes = rec_bytes + (with_colors ? pad256(total * 4) : 0);
  void* block = nullptr;
  size_t block_bytes = 0;
  A3D_TRY(ctx_block_alloc(ctx, bytes, &block, &block_bytes));
  hipError_t e = hipMemsetAsync(block, 0, bytes, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    ctx_block_release(ctx, block, block_bytes);
    set_error("a3d_tsdf_volume_new: clearing the volume failed: %s", hipGetErrorString(e));
    return A3D_HIP_ERROR;
  }
  a3d_tsdf_volume* vol = new a3d_tsdf_volume();
  vol->ctx = ctx;
  vol->nx = (uint32_t)nx, vol->ny = (uint32_t)ny, vol->nz = (uint32_t)nz, vol->max_weight = (uint32_t)max_weight;
  vol->v = voxel_size, vol->tau = truncation, vol->ox = origin[0], vol->oy = origin[1], vol->oz = origin[2];
  vol->with_colors = with_colors != 0;
  vol->block = block, vol->block_bytes = block_bytes, vol->used_bytes = bytes;
  vol->records = (float2*)block;
  if (with_colors) vol->colors = (uint32_t*)((char*)block + rec_bytes);
  *out = vol;
  return A3D_OK;
}

void a3d_tsdf_volume_free(a3d_tsdf_volume* volume) {
  if (!volume) return;
  solo_icp_release(volume->ctx, &volume->icp);
  if (volume->block) ctx_block_release(volume->ctx, volume->block, volume->block_bytes);
  delete volume;
}

a3d_status a3d_tsdf_volume_clear(a3d_tsdf_volume* volume) {
  A3D_REQUIRE(volume, A3D_INVALID_PARAMETER, "null argument");
  A3D_HIP_TRY(hipSetDevice(volume->ctx->device));
  A3D_HIP_TRY(hipMemsetAsync(volume->block, 0, volume->used_bytes, volume->ctx->stream));
  A3D_HIP_TRY(hipStreamSynchronize(volume->ctx->stream));
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_info(const a3d_tsdf_volume* volume, uint64_t out_dims[3], float* out_voxel_size,
                                float* out_truncation, float out_origin[3], uint64_t* out_max_weight,
                                int32_t* out_with_colors) {
  A3D_REQUIRE(volume, A3D_INVALID_PARAMETER, "null argument");
  if (out_dims) out_dims[0] = volume->nx, out_dims[1] = volume->ny, out_dims[2] = volume->nz;
  if (out_voxel_size) *out_voxel_size = volume->v;
  if (out_truncation) *out_truncation = volume->tau;
  if (out_origin) out_origin[0] = volume->ox, out_origin[1] = volume->oy, out_origin[2] = volume->oz;
  if (out_max_weight) *out_max_weight = volume->max_weight;
  if (out_with_colors) *out_with_colors = volume->with_colors ? 1 : 0;
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_integrate(a3d_tsdf_volume* volume, const a3d_device_image* const* images,
                                     const a3d_pose* world_to_camera_host, uint64_t n) {
  A3D_REQUIRE(volume && images && world_to_camera_host, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(n >= 1 && n < (1ull << 31), A3D_INVALID_PARAMETER, "a3d_tsdf_volume_integrate: at least one frame (and fewer than 2^31)");
  a3d_context* ctx = volume->ctx;
  std::vector<TsdfFrame> frames(n);
  for (uint64_t f = 0; f < n; ++f) {
    const a3d_device_image* im = images[f];
    A3D_REQUIRE(im, A3D_INVALID_PARAMETER, "a3d_tsdf_volume_integrate: null image");
    A3D_REQUIRE(im->ctx == ctx, A3D_INVALID_PARAMETER, "a3d_tsdf_volume_integrate: the images must live on the volume's context");
    A3D_REQUIRE(im->points && im->mask && im->width >= 1 && im->height >= 1 &&
                    (uint64_t)im->width * im->height < (1ull << 31),
                A3D_INVALID_PARAMETER, "a3d_tsdf_volume_integrate: bad image");
    A3D_REQUIRE(!volume->with_colors || im->colors, A3D_MISSING_FIELD,
                "a3d_tsdf_volume_integrate: an image without colours offered to a volume with colours");
    TsdfFrame& fr = frames[f];
    fr = TsdfFrame{};
    fr.points = im->points, fr.mask = im->mask, fr.colors = volume->with_colors ? im->colors : nullptr;
    fr.width = im->width, fr.height = im->height;
    fr.fx = im->fx, fr.fy = im->fy, fr.cx = im->cx, fr.cy = im->cy;
    fr.pose = pose_from_c(world_to_camera_host + f);
  }
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  void* region = nullptr;  // scratch region 3: the job table of the whole call
  A3D_TRY(ctx_scratch(ctx, 3, pad256(n * sizeof(TsdfFrame)), &region));
  const TsdfFrame* d_frames = (const TsdfFrame*)region;
  hipStream_t s = ctx->stream;
  // (`frames` lives until the wait below)
  A3D_HIP_TRY(hipMemcpyAsync(region, frames.data(), n * sizeof(TsdfFrame), hipMemcpyHostToDevice, s));
  const TsdfGrid g = grid_of(volume);
  const dim3 grid((g.total + TS_THREADS - 1) / TS_THREADS), block(TS_THREADS);
  bool ok = true;
  for (uint64_t first = 0; ok && first < n; first += TS_CHUNK) {  // chunks of at most 64 frames, in order
    const uint32_t count = (uint32_t)std::min<uint64_t>(TS_CHUNK, n - first);
    if (volume->with_colors)
      hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, s, g, d_frames + first, count);
    else
      hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, s, g, d_frames + first, count);
    ok = hipGetLastError() == hipSuccess;
  }
  // host-synchronous: the images may be freed right after (their arenas need no fence)
  if (hipStreamSynchronize(s) != hipSuccess) ok = false;
  if (!ok) {
    set_error("a3d_tsdf_volume_integrate: HIP failure: %s", hipGetErrorString(hipGetLastError()));
    return A3D_HIP_ERROR;
  }
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_raycast(a3d_tsdf_volume* volume, const a3d_pose* camera_to_world_host, double fx, double fy,
                                   double cx, double cy, uint64_t width, uint64_t height, float z_near, float z_far,
                                   float step, a3d_device_image** out_image) {
  A3D_REQUIRE(volume && camera_to_world_host && out_image, A3D_INVALID_PARAMETER, "null argument");
  A3D_TRY(check_camera(fx, fy, cx, cy, width, height, 0.0f));
  A3D_REQUIRE(std::isfinite(z_near) && std::isfinite(z_far) && std::isfinite(step), A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_raycast: z_near, z_far and step must be finite");
  A3D_REQUIRE(z_near > 0.f && z_far > z_near && step > 0.f, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_raycast: 0 < z_near < z_far and step > 0");
  const double samples = std::floor(((double)z_far - (double)z_near) / (double)step) + 1.0;
  A3D_REQUIRE(samples <= TS_MAX_SAMPLES, A3D_INVALID_PARAMETER, "a3d_tsdf_volume_raycast: more than 4096 samples per ray");
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));

  // the image, as render_cloud builds its own (cloud_render.hip)
  const size_t npx = (size_t)width * height;
  const bool with_colors = volume->with_colors;
  size_t total = 0;
  auto take = [&](size_t bytes) {
    const size_t at = total;
    total += pad256(bytes);
    return at;
  };
  const size_t off_points = take(npx * 12), off_mask = take(npx), off_normals = take(npx * 12);
  const size_t off_colors = with_colors ? take(npx * 3 + TS_COLOR_SLACK) : 0;
  DeviceArena* arena = new DeviceArena();
  if (ctx_arena_acquire(ctx, total, arena) != A3D_OK) {
    delete arena;
    return A3D_HIP_ERROR;
  }
  a3d_device_image* im = new a3d_device_image();
  im->ctx = ctx, im->arena = arena;
  ++arena->refs;
  char* base = (char*)arena->base;
  im->width = (uint32_t)width, im->height = (uint32_t)height;
  im->fx64 = fx, im->fy64 = fy, im->cx64 = cx, im->cy64 = cy;
  im->fx = (float)fx, im->fy = (float)fy, im->cx = (float)cx, im->cy = (float)cy;
  im->points = (float*)(base + off_points), im->mask = (uint8_t*)(base + off_mask);
  im->normals = (float*)(base + off_normals), im->has_normals = true;
  if (with_colors) im->colors = (uint8_t*)(base + off_colors);

  RayJob j{};
  j.camera_to_world = pose_from_c(camera_to_world_host);
  j.world_to_camera = pose_inverse(j.camera_to_world);
  j.fx = im->fx, j.fy = im->fy, j.cx = im->cx, j.cy = im->cy, j.z_near = z_near, j.step = step;
  j.width = im->width, j.height = im->height, j.samples = (uint32_t)samples;

  hipStream_t s = ctx->stream;
  const dim3 grid((uint32_t)((npx + TS_THREADS - 1) / TS_THREADS)), block(TS_THREADS);
  hipLaunchKernelGGL(tsdf_raycast_kernel, grid, block, 0, s, grid_of(volume), j, (uint32_t)npx, im->points, im->mask,
                     im->normals, im->colors);
  bool ok = hipGetLastError() == hipSuccess;
  // host-synchronous: the image is complete on return (its arena needs no fence)
  if (hipStreamSynchronize(s) != hipSuccess) ok = false;
  if (!ok) {
    set_error("a3d_tsdf_volume_raycast: HIP failure: %s", hipGetErrorString(hipGetLastError()));
    a3d_range_image_free(im);
    return A3D_HIP_ERROR;
  }
  *out_image = im;
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_download(a3d_tsdf_volume* volume, float* out_records, uint32_t* out_colors) {
  A3D_REQUIRE(volume && out_records, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(!out_colors || volume->with_colors, A3D_MISSING_FIELD, "a3d_tsdf_volume_download: the volume has no colours");
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  const size_t total = (size_t)volume->nx * volume->ny * volume->nz;
  A3D_HIP_TRY(hipMemcpyAsync(out_records, volume->records, total * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
  if (out_colors) A3D_HIP_TRY(hipMemcpyAsync(out_colors, volume->colors, total * 4, hipMemcpyDeviceToHost, ctx->stream));
  A3D_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_upload(a3d_tsdf_volume* volume, const float* records, const uint32_t* colors) {
  A3D_REQUIRE(volume && records, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(!colors || volume->with_colors, A3D_MISSING_FIELD, "a3d_tsdf_volume_upload: the volume has no colours");
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  const size_t total = (size_t)volume->nx * volume->ny * volume->nz;
  A3D_HIP_TRY(hipMemcpyAsync(volume->records, records, total * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
  if (colors) A3D_HIP_TRY(hipMemcpyAsync(volume->colors, colors, total * 4, hipMemcpyHostToDevice, ctx->stream));
  // host-synchronous: the caller's arrays may go right after
  A3D_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return A3D_OK;
}

}  // extern "C"
