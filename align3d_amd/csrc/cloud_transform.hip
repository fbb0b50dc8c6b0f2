// &Transform * &PointCloud (src/pointcloud.rs:40-52 over Transform::transform_vectors / transform_normals,
// src/transform.rs:164-187) on resident clouds, and the same written back to back into one cloud (a map of frames in one
// coordinate system).  Per point k of cloud i: out_points[k] = transform_vector(pose_i, points[k]) and, with normals,
// out_normals[k] = transform_normal(pose_i, normals[k]) — the devmath.hpp functions the ICP kernels call, so the value is
// the reference's f32 bit for bit (no contraction).  A job without a pose copies verbatim: no arithmetic, so NaN
// payloads, -0 and infinities survive.  A merge may also carry the clouds' colours ([len][3] u8): a pose does not touch
// them, they are copied, and cloud i's first row lands at byte 3 * sum(len[0..i)) of the output, at any residue mod 4
// (store_color, cloud_batch.hpp).
//
// One launch over every tile of every cloud of a batch (the job table of cloud_batch.hpp).  A tile is
// XF_THREADS * PPT consecutive points; in round r thread t takes point tile_base + r * XF_THREADS + t, so a wave touches
// one contiguous 768-byte span per array per round.  A thread loads every point (and normal) of its tile before it
// stores any, which puts PPT (2 PPT) independent 12-byte loads in flight per thread and makes an output that is exactly
// its input safe.  A pure streaming pass: no LDS, no atomics, no block waits on another block; 24 B read and 24 B written
// per point with normals against ~60 flops: the bound is HBM bandwidth.
#include <vector>

#include "cloud_batch.hpp"

using namespace a3d;

namespace {

constexpr uint32_t XF_THREADS = 256;
// Points per thread.  Measured on MI355X (scripts/cloud_transform_probe.py) against 1 and 4.
constexpr uint32_t XF_PPT = 2;

// One non-empty cloud of a batch as the kernel sees it (uploaded per call).
struct XformJob {
  const float* points;
  const float* normals;  // read only when out_normals is set
  float* out_points;
  float* out_normals;  // null: no normals are written
  const uint8_t* colors;  // read only when out_colors is set
  uint8_t* out_colors;    // null: no colours are written (the merge's alone: a transform's result copies its buffer)
  uint32_t len, first_tile, has_pose, pad;
  Pose pose;
  uint32_t pad2;
};
static_assert(sizeof(XformJob) == 96, "XformJob layout");

// The arrays' pointers come out of the job table, where the compiler only knows them as generic addresses (flat_load /
// flat_store); they are device memory, and saying so gives global_load_dwordx3 / global_store_dwordx3.
#define XF_GLOBAL __attribute__((address_space(1)))

// (no __restrict__ on the arrays: an output may be exactly its input; every load of a thread precedes its stores)
template <uint32_t PPT>
__global__ void __launch_bounds__(XF_THREADS) cloud_transform_kernel(const XformJob* __restrict__ jobs, uint32_t n_jobs) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const XformJob& j = jobs[ji];
  const XF_GLOBAL float* points = (const XF_GLOBAL float*)j.points;
  const XF_GLOBAL float* normals = (const XF_GLOBAL float*)j.normals;
  XF_GLOBAL float* out_points = (XF_GLOBAL float*)j.out_points;
  XF_GLOBAL float* out_normals = (XF_GLOBAL float*)j.out_normals;
  const uint32_t len = j.len;
  const uint32_t k0 = (tile - j.first_tile) * (XF_THREADS * PPT) + threadIdx.x;
  f32x3 p[PPT], n[PPT];
#pragma unroll
  for (uint32_t r = 0; r < PPT; ++r) {
    const uint32_t k = k0 + r * XF_THREADS;
    p[r] = n[r] = f32x3{0.f, 0.f, 0.f};
    if (k < len) {
      p[r] = *(const XF_GLOBAL f32x3_u*)(points + 3 * (size_t)k);
      if (out_normals) n[r] = *(const XF_GLOBAL f32x3_u*)(normals + 3 * (size_t)k);
    }
  }
  if (j.has_pose) {
    const Pose pose = j.pose;
#pragma unroll
    for (uint32_t r = 0; r < PPT; ++r) {
      const V3 v = transform_vector(pose, V3{p[r].x, p[r].y, p[r].z});
      p[r] = f32x3{v.x, v.y, v.z};
      if (out_normals) {
        const V3 w = transform_normal(pose, V3{n[r].x, n[r].y, n[r].z});
        n[r] = f32x3{w.x, w.y, w.z};
      }
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < PPT; ++r) {
    const uint32_t k = k0 + r * XF_THREADS;
    if (k < len) {
      *(XF_GLOBAL f32x3_u*)(out_points + 3 * (size_t)k) = p[r];
      if (out_normals) *(XF_GLOBAL f32x3_u*)(out_normals + 3 * (size_t)k) = n[r];
    }
  }
  if (j.out_colors) {  // (uniform over the block; the colour output overlaps no input)
    const XF_GLOBAL uint8_t* colors = (const XF_GLOBAL uint8_t*)j.colors;
    XF_GLOBAL uint8_t* out_colors = (XF_GLOBAL uint8_t*)j.out_colors;
    uint8_t c[PPT][3];
#pragma unroll
    for (uint32_t r = 0; r < PPT; ++r) {
      const uint32_t k = k0 + r * XF_THREADS;
      if (k < len)
        for (uint32_t b = 0; b < 3; ++b) c[r][b] = colors[3 * (size_t)k + b];
    }
#pragma unroll
    for (uint32_t r = 0; r < PPT; ++r) {
      const uint32_t k = k0 + r * XF_THREADS;
      if (k < len)
        for (uint32_t b = 0; b < 3; ++b) out_colors[3 * (size_t)k + b] = c[r][b];
    }
  }
}

uint32_t points_per_thread_setting() {
  uint32_t v = XF_PPT;
  if (const char* env = A3D_DIAG_ENV("A3D_CLOUD_TRANSFORM_PPT"))  // diagnostics build: the variants the probe times
    if (*env) v = (uint32_t)atoi(env);
  return v == 1 || v == 2 || v == 4 ? v : XF_PPT;
}

// Uploads the job table and runs the one launch; complete on return.
a3d_status run_jobs(a3d_context* ctx, std::vector<XformJob>& jobs, uint32_t ppt) {
  uint64_t tiles = 0;
  const uint32_t tile_points = XF_THREADS * ppt;
  for (XformJob& j : jobs) {
    j.first_tile = (uint32_t)tiles;
    tiles += (j.len + tile_points - 1) / tile_points;
    A3D_REQUIRE(tiles < (1ull << 31), A3D_INVALID_PARAMETER, "batch too large");
  }
  if (jobs.empty()) return A3D_OK;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 3, jobs.size() * sizeof(XformJob), &region));
  hipStream_t s = ctx->stream;
  A3D_HIP_TRY(hipMemcpyAsync(region, jobs.data(), jobs.size() * sizeof(XformJob), hipMemcpyHostToDevice, s));
  const XformJob* d_jobs = (const XformJob*)region;
  const dim3 grid((uint32_t)tiles), block(XF_THREADS);
#ifdef A3D_DIAGNOSTICS  // (the product library holds the one variant it launches)
  if (ppt == 1) hipLaunchKernelGGL(cloud_transform_kernel<1>, grid, block, 0, s, d_jobs, (uint32_t)jobs.size());
  else if (ppt == 4) hipLaunchKernelGGL(cloud_transform_kernel<4>, grid, block, 0, s, d_jobs, (uint32_t)jobs.size());
  else
#endif
    hipLaunchKernelGGL(cloud_transform_kernel<XF_PPT>, grid, block, 0, s, d_jobs, (uint32_t)jobs.size());
  A3D_HIP_TRY(hipGetLastError());
  // host-synchronous: the caller may free inputs and outputs right after
  A3D_HIP_TRY(hipStreamSynchronize(s));
  return A3D_OK;
}

}  // namespace

extern "C" {

a3d_status a3d_point_clouds_transform_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                             const a3d_pose* poses_host, uint64_t n, float* const* d_out_points,
                                             float* const* d_out_normals) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(ctx && d_clouds && d_out_points, A3D_INVALID_PARAMETER, "null argument");
  std::vector<XformJob> jobs;
  RangeRecorder ranges;
  jobs.reserve(n), ranges.reserve(4 * n);
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    if (c.len == 0) continue;  // contributes nothing; its pointers may be null
    A3D_REQUIRE(c.len < (1ull << 31), A3D_INVALID_PARAMETER, "a cloud of 2^31 points or more");
    A3D_REQUIRE(c.points && d_out_points[i], A3D_INVALID_PARAMETER, "null points or output pointer");
    float* out_normals = d_out_normals ? d_out_normals[i] : nullptr;
    A3D_REQUIRE(!out_normals || c.normals, A3D_MISSING_FIELD, "cloud has no normals");
    XformJob j{};
    j.points = c.points, j.normals = out_normals ? c.normals : nullptr;
    j.out_points = d_out_points[i], j.out_normals = out_normals;
    j.len = (uint32_t)c.len;
    if (poses_host) j.has_pose = 1, j.pose = pose_from_c(&poses_host[i]);
    jobs.push_back(j);
    // an output that is exactly its own input (in place) stands for both; everything else must be disjoint
    if (j.points != j.out_points) ranges.in(j.points, c.len * 12);
    if (j.normals != j.out_normals) ranges.in(j.normals, c.len * 12);
    ranges.out(j.out_points, c.len * 12), ranges.out(j.out_normals, c.len * 12);
  }
  A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
              "a3d_point_clouds_transform_device: an output overlaps an input or another output (only output i == input i "
              "is allowed)");
  return run_jobs(ctx, jobs, points_per_thread_setting());
}

a3d_status a3d_point_clouds_merge_rgb_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                             const uint8_t* const* d_colors, const a3d_pose* poses_host, uint64_t n,
                                             float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                             uint64_t capacity, uint64_t* out_len) {
  if (n == 0) {
    if (out_len) *out_len = 0;
    return A3D_OK;
  }
  A3D_REQUIRE(ctx && d_clouds && d_out_points && out_len, A3D_INVALID_PARAMETER, "null argument");
  std::vector<XformJob> jobs;
  RangeRecorder ranges;
  jobs.reserve(n), ranges.reserve(3 * n + 3);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    if (c.len == 0) continue;
    A3D_REQUIRE(c.len < (1ull << 31), A3D_INVALID_PARAMETER, "a cloud of 2^31 points or more");
    A3D_REQUIRE(c.points, A3D_INVALID_PARAMETER, "null points pointer");
    A3D_REQUIRE(!d_out_normals || c.normals, A3D_MISSING_FIELD, "a cloud of the merge has no normals");
    const uint8_t* colors = d_out_colors && d_colors ? d_colors[i] : nullptr;
    A3D_REQUIRE(!d_out_colors || colors, A3D_MISSING_FIELD, "a cloud of the merge has no colours");
    XformJob j{};
    j.points = c.points, j.normals = d_out_normals ? c.normals : nullptr;
    j.out_points = d_out_points + 3 * total, j.out_normals = d_out_normals ? d_out_normals + 3 * total : nullptr;
    j.colors = colors, j.out_colors = d_out_colors ? d_out_colors + 3 * total : nullptr;
    j.len = (uint32_t)c.len;
    if (poses_host) j.has_pose = 1, j.pose = pose_from_c(&poses_host[i]);
    jobs.push_back(j);
    ranges.in(j.points, c.len * 12), ranges.in(j.normals, c.len * 12), ranges.in(j.colors, c.len * 3);
    total += c.len;
  }
  if (capacity < total) {
    *out_len = total;
    set_error("a3d_point_clouds_merge_device: capacity %llu is smaller than the %llu points of the clouds (nothing was written)",
              (unsigned long long)capacity, (unsigned long long)total);
    return A3D_INVALID_PARAMETER;
  }
  ranges.out(d_out_points, total * 12), ranges.out(d_out_normals, total * 12), ranges.out(d_out_colors, total * 3);
  A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
              "a3d_point_clouds_merge_device: the output overlaps an input (or its own normals or colours)");
  A3D_TRY(run_jobs(ctx, jobs, points_per_thread_setting()));
  *out_len = total;
  return A3D_OK;
}

a3d_status a3d_point_clouds_merge_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, const a3d_pose* poses_host,
                                         uint64_t n, float* d_out_points, float* d_out_normals, uint64_t capacity,
                                         uint64_t* out_len) {
  return a3d_point_clouds_merge_rgb_device(ctx, d_clouds, nullptr, poses_host, n, d_out_points, d_out_normals, nullptr,
                                           capacity, out_len);
}

}  // extern "C"
