// PointCloud::from(&RangeImage) (src/range_image/structure.rs:375-406) on resident images: an order-preserving
// compaction.  A pixel is kept iff mask != 0 (structure.rs:381: not the mask == 1 of get_point), kept pixels come out in
// row-major order, points and normals are copied verbatim (no arithmetic: NaN payloads, -0 and inf survive), and an image
// without normals gives a cloud without normals (the reference's Option, structure.rs:384-390).  Colours ([h][w][3] u8)
// pass the same mask (structure.rs:392-398) when the caller asks for them: three bytes per kept pixel, moved by the
// thread that moves the point (store_color, cloud_batch.hpp).
//
// Two launches over every tile of every image of a batch (the job table of cloud_batch.hpp), no block waiting on another:
//  1. cloud_count_kernel: each block counts the kept pixels of its tile (reads the mask only) and adds them to its
//     image's total;
//  2. cloud_write_kernel: each block sums its image's earlier tile counts for its offset, ranks its own pixels with a
//     64-bit ballot and mbcnt plus a scan of the per-wave counts in LDS, and writes [len][3] f32 with 12-byte vector
//     stores.
// A tile is one or more chunks of 2048 pixels (8 rounds of 256), at most CLOUD_MAX_TILES tiles per image.
#include <vector>

#include "cloud_batch.hpp"

using namespace a3d;

namespace {

constexpr uint32_t CLOUD_THREADS = 256;
constexpr uint32_t CLOUD_WAVES = CLOUD_THREADS / 64;
constexpr uint32_t CLOUD_ROUNDS = 8;
constexpr uint32_t CLOUD_CHUNK = CLOUD_ROUNDS * CLOUD_THREADS;  // pixels per chunk
constexpr uint32_t CLOUD_MAX_TILES = 4096;                      // tiles per image at most

// One image of a batch as the kernels see it (uploaded per call into the context's scratch region 3).
struct CloudJob {
  const float* points;
  const uint8_t* mask;
  const float* normals;   // null: no normals are written
  const uint16_t* depth16;  // non-null: points_from_depth (common.hpp), the points are rebuilt from this plane
  float* out_points;
  float* out_normals;
  const uint8_t* colors;  // null: no colours are written
  uint8_t* out_colors;
  uint64_t capacity;
  uint32_t npx, width, first_tile, n_tiles, chunks_per_tile, pad;
  float bp_fx, bp_fy, bp_cx, bp_cy, depth_scale, pad2;
};

// Pass 1: tile_counts[tile] = kept pixels of the tile; lens[image] += the same (lens zeroed by the host upload).
__global__ void __launch_bounds__(CLOUD_THREADS)
    cloud_count_kernel(const CloudJob* __restrict__ jobs, uint32_t n_jobs, uint32_t* __restrict__ tile_counts,
                       unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_wave[CLOUD_WAVES];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const uint8_t* __restrict__ mask = jobs[ji].mask;
  const uint32_t npx = jobs[ji].npx, span = jobs[ji].chunks_per_tile * CLOUD_CHUNK;
  const uint32_t px0 = (tile - jobs[ji].first_tile) * span, px_end = min(npx, px0 + span);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t c = 0;  // wave-uniform
  for (uint32_t p = px0 + threadIdx.x; p - threadIdx.x < px_end; p += CLOUD_THREADS) {
    const bool keep = p < px_end && mask[p] != 0;
    c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(keep));
  }
  if (lane == 0) s_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (uint32_t w = 0; w < CLOUD_WAVES; ++w) total += s_wave[w];
    tile_counts[tile] = total;
    if (total) atomicAdd(&lens[ji], (unsigned long long)total);
  }
}

// Pass 2: every kept pixel of the tile to out[offset + rank].  Nothing is written anywhere if any image of the batch
// has more kept pixels than its capacity (the host then returns A3D_INVALID_PARAMETER).
__global__ void __launch_bounds__(CLOUD_THREADS)
    cloud_write_kernel(const CloudJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ tile_counts,
                       const unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_wave[CLOUD_ROUNDS][CLOUD_WAVES];
  __shared__ uint32_t s_base, s_over;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const CloudJob& j = jobs[ji];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t = tile - j.first_tile;
  if (wave == 0) {
    uint32_t s = 0;
    for (uint32_t k = lane; k < t; k += 64) s += tile_counts[j.first_tile + k];
    bool over = false;
    for (uint32_t k = lane; k < n_jobs; k += 64) over |= lens[k] > jobs[k].capacity;
    s = wave_sum(s);
    const bool any_over = __builtin_amdgcn_ballot_w64(over) != 0ull;
    if (lane == 0) s_base = s, s_over = any_over ? 1u : 0u;
  }
  __syncthreads();
  if (s_over) return;
  const uint8_t* __restrict__ mask = j.mask;
  const uint16_t* __restrict__ depth16 = j.depth16;
  const float* __restrict__ points = j.points;
  const float* __restrict__ normals = j.normals;
  float* __restrict__ out_points = j.out_points;
  float* __restrict__ out_normals = j.out_normals;
  const uint8_t* __restrict__ colors = j.colors;
  uint8_t* __restrict__ out_colors = j.out_colors;
  const uint64_t capacity = j.capacity;
  const uint32_t npx = j.npx, width = j.width, span = j.chunks_per_tile * CLOUD_CHUNK;
  const uint32_t px_end = min(npx, t * span + span);
  DivBy dfx{}, dfy{};
  bool focal_ok = false;
  if (depth16) dfx = div_prepare(j.bp_fx), dfy = div_prepare(j.bp_fy), focal_ok = div_den_ok(j.bp_fx) & div_den_ok(j.bp_fy);
  uint32_t base = s_base;  // kept pixels of the image before this chunk
  for (uint32_t px0 = t * span; px0 < px_end; px0 += CLOUD_CHUNK) {
    uint64_t ballot[CLOUD_ROUNDS];
    uint32_t depth[CLOUD_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CLOUD_ROUNDS; ++r) {
      const uint32_t p = px0 + r * CLOUD_THREADS + threadIdx.x;
      depth[r] = 0;
      bool keep = false;
      if (p < px_end) {
        if (depth16) depth[r] = depth16[p], keep = depth[r] != 0;  // mask == (depth16 != 0) on such images
        else keep = mask[p] != 0;
      }
      ballot[r] = __builtin_amdgcn_ballot_w64(keep);
    }
    if (lane == 0) {
#pragma unroll
      for (uint32_t r = 0; r < CLOUD_ROUNDS; ++r) s_wave[r][wave] = (uint32_t)__builtin_popcountll(ballot[r]);
    }
    __syncthreads();
    // exclusive offsets in pixel order: round-major, then wave, then lane
    uint32_t off[CLOUD_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CLOUD_ROUNDS; ++r)
      for (uint32_t w = 0; w < CLOUD_WAVES; ++w) {
        if (w == wave) off[r] = base;
        base += s_wave[r][w];
      }
    __syncthreads();  // (s_wave is rewritten by the next chunk)
#pragma unroll
    for (uint32_t r = 0; r < CLOUD_ROUNDS; ++r) {
      if (!((ballot[r] >> lane) & 1ull)) continue;
      const uint32_t p = px0 + r * CLOUD_THREADS + threadIdx.x;
      const uint64_t dst = (uint64_t)off[r] + lane_rank(ballot[r]);
      if (dst >= capacity) continue;  // (cannot happen: the image's total fits; kept as a bound on every store)
      f32x3 pt;
      if (depth16) {
        const uint32_t row = p / width, col = p - row * width;
        const V3 v = backproject_px(depth[r], (int)row, (int)col, j.bp_fx, j.bp_fy, j.bp_cx, j.bp_cy, j.depth_scale, dfx,
                                    dfy, focal_ok);
        pt = f32x3{v.x, v.y, v.z};
      } else {
        pt = *(const f32x3_u*)(points + 3 * (size_t)p);
      }
      *(f32x3_u*)(out_points + 3 * dst) = pt;
      if (out_normals) *(f32x3_u*)(out_normals + 3 * dst) = *(const f32x3_u*)(normals + 3 * (size_t)p);
      if (out_colors) store_color(out_colors, dst, load_color(colors, p));
    }
  }
}

}  // namespace

extern "C" {

a3d_status a3d_range_image_has_normals(const a3d_device_image* image, int32_t* out_has_normals) {
  A3D_REQUIRE(image && out_has_normals, A3D_INVALID_PARAMETER, "null argument");
  *out_has_normals = image->has_normals ? 1 : 0;
  return A3D_OK;
}

a3d_status a3d_range_image_has_colors(const a3d_device_image* image, int32_t* out_has_colors) {
  A3D_REQUIRE(image && out_has_colors, A3D_INVALID_PARAMETER, "null argument");
  *out_has_colors = image->colors ? 1 : 0;
  return A3D_OK;
}

a3d_status a3d_range_image_to_point_clouds_rgb(const a3d_device_image* const* images, uint64_t n, float* const* d_points,
                                               float* const* d_normals, uint8_t* const* d_colors,
                                               const uint64_t* capacities, uint64_t* out_lens) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(images && d_points && capacities && out_lens, A3D_INVALID_PARAMETER, "null argument");
  a3d_context* ctx = images[0] ? images[0]->ctx : nullptr;
  std::vector<CloudJob> jobs(n);
  uint64_t tiles = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_device_image* im = images[i];
    A3D_REQUIRE(im && d_points[i], A3D_INVALID_PARAMETER, "null image or output pointer");
    A3D_REQUIRE(im->ctx == ctx, A3D_INVALID_PARAMETER, "a3d_range_image_to_point_clouds: the images must share a context");
    float* out_normals = d_normals ? d_normals[i] : nullptr;
    A3D_REQUIRE(!out_normals || im->has_normals, A3D_MISSING_FIELD, "image has no normals");
    uint8_t* out_colors = d_colors ? d_colors[i] : nullptr;
    A3D_REQUIRE(!out_colors || im->colors, A3D_MISSING_FIELD, "image has no colours");
    CloudJob& j = jobs[i];
    j = CloudJob{};
    const uint64_t npx = (uint64_t)im->width * im->height;
    A3D_REQUIRE(npx > 0 && npx < (1ull << 31), A3D_INVALID_PARAMETER, "bad image size");
    j.points = im->points, j.mask = im->mask;
    j.normals = out_normals ? im->normals : nullptr;
    j.out_points = d_points[i], j.out_normals = out_normals;
    j.colors = out_colors ? im->colors : nullptr, j.out_colors = out_colors;
    j.capacity = capacities[i];
    j.npx = (uint32_t)npx, j.width = im->width;
    A3D_TRY(plan_tiles(npx, CLOUD_CHUNK, CLOUD_MAX_TILES, &tiles, &j.first_tile, &j.chunks_per_tile));
    j.n_tiles = (uint32_t)tiles - j.first_tile;
    if (im->points_from_depth && im->depth16) {  // (builder level 0: 2 bytes of depth instead of 1 + 12 of mask + point)
      j.depth16 = im->depth16;
      j.bp_fx = im->bp_fx, j.bp_fy = im->bp_fy, j.bp_cx = im->bp_cx, j.bp_cy = im->bp_cy, j.depth_scale = im->depth_scale;
    }
  }
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  BatchScratch scratch;  // the words: one length per image
  A3D_TRY(batch_scratch(ctx, n * sizeof(CloudJob), n, tiles, 0, &scratch));
  const CloudJob* d_jobs = (const CloudJob*)scratch.jobs;
  unsigned long long* d_lens = scratch.words;
  uint32_t* d_tile_counts = scratch.tile_counts;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  hipLaunchKernelGGL(cloud_count_kernel, dim3((uint32_t)tiles), dim3(CLOUD_THREADS), 0, s, d_jobs, (uint32_t)n, d_tile_counts,
                     d_lens);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cloud_write_kernel, dim3((uint32_t)tiles), dim3(CLOUD_THREADS), 0, s, d_jobs, (uint32_t)n,
                     (const uint32_t*)d_tile_counts, (const unsigned long long*)d_lens);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> lens(n);
  A3D_HIP_TRY(hipMemcpyAsync(lens.data(), d_lens, n * 8, hipMemcpyDeviceToHost, s));
  // host-synchronous: the work on the images is complete on return, so their arenas need no fence (a3d_range_image_free)
  A3D_HIP_TRY(hipStreamSynchronize(s));
  bool over = false;
  for (uint64_t i = 0; i < n; ++i) out_lens[i] = lens[i], over |= lens[i] > capacities[i];
  A3D_REQUIRE(!over, A3D_INVALID_PARAMETER,
              "a3d_range_image_to_point_clouds: a capacity is smaller than its image's point count (nothing was written)");
  return A3D_OK;
}

a3d_status a3d_range_image_to_point_clouds(const a3d_device_image* const* images, uint64_t n, float* const* d_points,
                                           float* const* d_normals, const uint64_t* capacities, uint64_t* out_lens) {
  return a3d_range_image_to_point_clouds_rgb(images, n, d_points, d_normals, nullptr, capacities, out_lens);
}

a3d_status a3d_range_image_to_point_cloud(const a3d_device_image* image, float* d_points, float* d_normals,
                                          uint64_t capacity, uint64_t* out_len) {
  A3D_REQUIRE(image && d_points && out_len, A3D_INVALID_PARAMETER, "null argument");
  return a3d_range_image_to_point_clouds(&image, 1, &d_points, &d_normals, &capacity, out_len);
}

}  // extern "C"
