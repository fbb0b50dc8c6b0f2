// RangeImage::pyramid (src/range_image/structure.rs:309-351) and compute_intensity / compute_intensity_map
// (structure.rs:266-297) for resident images from any source: uploaded, filtered or edited after upload, or level 0 of a
// builder pyramid.  The frame builder (frame.hip) runs the same stages on its own arenas; here level 0 is the caller's
// image and the coarser levels live in a new arena per image, so every kernel reads a table of per-image, per-level
// pointers (PyrLevel[n][levels], uploaded per call into the context's scratch region 4) instead of arena + offset.
// blockIdx.z is the image: one launch per stage for the whole batch.  The stage bodies are the builder's own
// (pyramid_ops.hpp): the same operations in the same order, the same bits.
//   levels 1, 2: pyr_level0_quad_kernel (sides multiples of 4, three levels or more) — level 0's points, mask and normals
//                read once in row order into LDS, each thread picks one level-1 pixel from its 2 x 2 quad, the patch's
//                level-1 picks meet in LDS for the level-2 picks;
//   otherwise:   pyr_pick_kernel per level (any size: the reference's `(dst as f32 * ratio) as usize` source index);
//   colours:     pyr_blur_halve[_words]_kernel per level (image 0.24.7 blur + 2x subsample, PARITY UNPINNED);
//   intensity:   pyr_luma_imap_kernel, one launch for every level of every image.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pyramid_ops.hpp"

namespace {

constexpr uint64_t PYR_MAX_LEVELS = 16;  // as the builder's MAX_LEVELS
constexpr uint32_t PYR_MAX_Z = 65535;    // images per launch (gridDim.z)
constexpr size_t COLOR_SLACK = 16;       // bytes readable past a colour array's end (the blur loads whole words)

// One level of one image as the kernels see it.  Null normals / colours / intensities: the level has none.
struct PyrLevel {
  float* points;
  uint8_t* mask;
  float* normals;
  uint8_t* colors;
  uint8_t* intensities;
  float* imap;
  uint32_t w, h;
};

// A table pointer read from memory is a generic (flat) pointer to the compiler; as_global() tells it the array is in
// global memory, so the bodies' loads and stores become global_* instructions (flat ones also count against the LDS
// counter and cannot use the scalar-base addressing of global_*).
template <typename T>
__device__ __forceinline__ T* as_global(T* p) {
  return (T*)(T __attribute__((address_space(1)))*)(uintptr_t)p;
}
__device__ __forceinline__ PyrLevel global_level(const PyrLevel& L) {
  return PyrLevel{as_global(L.points), as_global(L.mask), as_global(L.normals), as_global(L.colors),
                  as_global(L.intensities), as_global(L.imap), L.w, L.h};
}

// ---- levels 1 and 2 from level 0 in one pass (sides multiples of four) -----------------------------------------------
// A block owns an aligned 32 x 32 patch of level 0.  Its points, normals (three 12-byte loads per thread and array, row
// order: a wave's load instruction covers two whole patch rows) and masks (one word per thread) are staged in LDS; thread
// (ty, tx) then picks level-1 pixel (ty, tx) of the patch from its 2 x 2 quad, and the 16 x 16 level-1 picks of the patch
// meet in LDS for the 8 x 8 level-2 picks (128 threads: points and mask, then normals) — level0_quad_kernel's level-1/2
// stage (frame.hip) on loaded instead of back-projected points.
constexpr int PQ = 32, PQT = PQ / 2;
__global__ void __launch_bounds__(256)
    pyr_level0_quad_kernel(const PyrLevel* __restrict__ tab, uint32_t levels, uint32_t img0, bool l2_is_last) {
  __shared__ float sp[3][PQ][PQ + 1];  // points
  __shared__ float sn[3][PQ][PQ + 1];  // normals
  __shared__ __attribute__((aligned(4))) uint8_t sm[PQ][PQ];
  __shared__ float s1[2][3][PQT][PQT + 1];  // level-1 picks (0: points, 1: normals)
  __shared__ uint8_t s1m[PQT][PQT];         // level-1 masks
  const PyrLevel* lv = tab + (size_t)(img0 + blockIdx.z) * levels;
  const PyrLevel L0 = global_level(lv[0]), L1 = global_level(lv[1]), L2 = global_level(lv[2]);
  const bool with_normals = L0.normals != nullptr;  // (block-uniform)
  const uint32_t w = L0.w, h = L0.h;
  const int t = (int)threadIdx.x;
  const int r0 = (int)blockIdx.y * PQ, c0 = (int)blockIdx.x * PQ;
  // ---- staging: load k of thread t is pixel (t / 32 + 8 k, t % 32) of the patch; every load issued before the first
  // LDS write (a pixel outside the image loads pixel 0 and is never picked: the quads of a 4-aligned image are whole)
  {
    const int sx = t & (PQ - 1), sy0 = t >> 5;
    const bool col_in = c0 + sx < (int)w;
    V3 p[4], nr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = sy0 + 8 * k;
      const uint32_t idx = (col_in && r0 + y < (int)h) ? __umul24((uint32_t)(r0 + y), w) + (uint32_t)(c0 + sx) : 0u;
      p[k] = ld_v3g(L0.points, idx);
      nr[k] = with_normals ? ld_v3g(L0.normals, idx) : V3{0.f, 0.f, 0.f};
    }
    // the patch's masks: 32 rows x 32 bytes = one word per thread (the width is a multiple of four: rows start aligned)
    const int my = t >> 3, mx = 4 * (t & 7);
    const uint32_t mword = (r0 + my < (int)h && c0 + mx < (int)w)
                               ? *(const uint32_t*)(L0.mask + (__umul24((uint32_t)(r0 + my), w) + (uint32_t)(c0 + mx)))
                               : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = sy0 + 8 * k;
      sp[0][y][sx] = p[k].x, sp[1][y][sx] = p[k].y, sp[2][y][sx] = p[k].z;
      sn[0][y][sx] = nr[k].x, sn[1][y][sx] = nr[k].y, sn[2][y][sx] = nr[k].z;
    }
    *(uint32_t*)&sm[my][mx] = mword;
  }
  __syncthreads();
  // ---- level 1 (resize_range_points / _normals, resize.rs:42-104): the sides are even, so level-1 pixel (dv, du) is
  // source block (2 dv .. 2 dv + 1, 2 du .. 2 du + 1), candidates in block order 00, 01, 10, 11, source mask == 1
  const int tx = t & (PQT - 1), ty = t >> 4;
  const bool quad_in = r0 + 2 * ty < (int)h && c0 + 2 * tx < (int)w;
  V3 cand[4];
  bool ok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int y = 2 * ty + (q >> 1), x = 2 * tx + (q & 1);
    cand[q] = V3{sp[0][y][x], sp[1][y][x], sp[2][y][x]};
    ok[q] = sm[y][x] == 1;
  }
  int n_valid = 0;
  const V3 pk_p = pick_nearest_to_mean(cand, ok, &n_valid);
  V3 pk_n{0.f, 0.f, 0.f};
  if (with_normals) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int y = 2 * ty + (q >> 1), x = 2 * tx + (q & 1);
      cand[q] = V3{sn[0][y][x], sn[1][y][x], sn[2][y][x]};
    }
    int unused;
    pk_n = pick_nearest_to_mean(cand, ok, &unused);
  }
  if (quad_in) {  // (nothing in this call reads level 1 again: streaming stores)
    const uint32_t i1 = __umul24((uint32_t)((r0 >> 1) + ty), L1.w) + (uint32_t)((c0 >> 1) + tx);
    st_v3u_stream(L1.points, i1, pk_p);
    st_u8u_stream(L1.mask, i1, n_valid > 0 ? 1 : 0);
    if (with_normals) st_v3u_stream(L1.normals, i1, pk_n);
  }
  // ---- level 2 from the patch's 16 x 16 level-1 picks (the level-1 sides are even too: blocks are whole)
  s1[0][0][ty][tx] = pk_p.x, s1[0][1][ty][tx] = pk_p.y, s1[0][2][ty][tx] = pk_p.z;
  s1[1][0][ty][tx] = pk_n.x, s1[1][1][ty][tx] = pk_n.y, s1[1][2][ty][tx] = pk_n.z;
  s1m[ty][tx] = (quad_in && n_valid > 0) ? 1 : 0;
  __syncthreads();
  const int which = t >> 6;  // 0: points (and the mask), 1: normals; threads 128 .. 255 have no task
  if (which > 1 || (which == 1 && !with_normals)) return;
  const int ly = (t >> 3) & 7, lx = t & 7;
  const uint32_t r2 = ((uint32_t)r0 >> 2) + (uint32_t)ly, c2 = ((uint32_t)c0 >> 2) + (uint32_t)lx;
  if (r2 >= L2.h || c2 >= L2.w) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int y = 2 * ly + (q >> 1), x = 2 * lx + (q & 1);
    cand[q] = V3{s1[which][0][y][x], s1[which][1][y][x], s1[which][2][y][x]};
    ok[q] = s1m[y][x] == 1;
  }
  const V3 pk2 = pick_nearest_to_mean(cand, ok, &n_valid);
  const uint32_t i2 = __umul24(r2, L2.w) + c2;
  float* dst = which ? L2.normals : L2.points;
  if (l2_is_last) {
    st_v3u_stream(dst, i2, pk2);
    if (!which) st_u8u_stream(L2.mask, i2, n_valid > 0 ? 1 : 0);
  } else {  // (level 3 reads it next)
    st_v3u(dst, i2, pk2);
    if (!which) st_u8u(L2.mask, i2, n_valid > 0 ? 1 : 0);
  }
}

// Level l from level l - 1, any sizes: blockIdx.y = 0 the points and mask, 1 the normals (images without normals return).
__global__ void __launch_bounds__(256) pyr_pick_kernel(const PyrLevel* __restrict__ tab, uint32_t levels, uint32_t img0, uint32_t l) {
  const PyrLevel* lv = tab + (size_t)(img0 + blockIdx.z) * levels;
  const PyrLevel S = global_level(lv[l - 1]), D = global_level(lv[l]);
  const bool normals = blockIdx.y == 1;
  if (normals && !S.normals) return;  // (block-uniform)
  resize_pick_body(blockIdx.x * blockDim.x + threadIdx.x, S.w, S.h, D.w, D.h, normals, normals ? S.normals : S.points, S.mask,
                   normals ? D.normals : D.points, D.mask);
}

// Colours of level l from level l - 1 (images without colours return).
__global__ void __launch_bounds__(256)
    pyr_blur_halve_kernel(const PyrLevel* __restrict__ tab, uint32_t levels, uint32_t img0, uint32_t l,
                          const TapRow* __restrict__ taps_v, const TapRow* __restrict__ taps_h) {
  const PyrLevel* lv = tab + (size_t)(img0 + blockIdx.z) * levels;
  const PyrLevel S = global_level(lv[l - 1]), D = global_level(lv[l]);
  if (!S.colors) return;
  blur_halve_body(S.colors, S.w, D.w, D.h, taps_v, taps_h, D.colors);
}
__global__ void __launch_bounds__(256)
    pyr_blur_halve_words_kernel(const PyrLevel* __restrict__ tab, uint32_t levels, uint32_t img0, uint32_t l, float support,
                                const TapRow* __restrict__ taps_v, const TapRow* __restrict__ taps_h) {
  const PyrLevel* lv = tab + (size_t)(img0 + blockIdx.z) * levels;
  const PyrLevel S = global_level(lv[l - 1]), D = global_level(lv[l]);
  if (!S.colors) return;
  blur_halve_words_body(S.colors, S.w, S.h, D.w, D.h, support, taps_v, taps_h, D.colors);
}

// compute_intensity + compute_intensity_map of every level of every image: blockIdx.y = level, blockIdx.z = image; the
// grid covers the largest level (smaller ones return early).  QUADS: every width of the launch is a multiple of four.
template <bool QUADS>
__global__ void __launch_bounds__(256) pyr_luma_imap_kernel(const PyrLevel* __restrict__ tab, uint32_t levels, uint32_t img0) {
  const PyrLevel L = global_level(tab[(size_t)(img0 + blockIdx.z) * levels + blockIdx.y]);
  luma_imap_body<QUADS>(blockIdx.x * blockDim.x + threadIdx.x, L.w, L.h, L.colors, L.intensities, L.imap);
}

// The per-call table -> the context's scratch region 4 (stream-ordered behind the work of earlier calls that read it).  A
// copy from pageable memory has taken its bytes when the call returns, so the enqueue-only caller may drop `tab` then.
a3d_status upload_table(a3d_context* ctx, const std::vector<PyrLevel>& tab, const PyrLevel** out) {
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 4, tab.size() * sizeof(PyrLevel), &region));
  A3D_HIP_TRY(hipMemcpyAsync(region, tab.data(), tab.size() * sizeof(PyrLevel), hipMemcpyHostToDevice, ctx->stream));
  *out = (const PyrLevel*)region;
  return A3D_OK;
}

// The luma + intensity map launch over tab[n][levels] (every entry has colours, intensities and a map).
void launch_luma_imap(a3d_context* ctx, const PyrLevel* d_tab, const std::vector<PyrLevel>& tab, uint64_t n, uint32_t levels) {
  bool quads = true;
  for (const PyrLevel& L : tab) quads = quads && L.w % 4 == 0;
  uint64_t threads = 0;
  for (const PyrLevel& L : tab)
    threads = std::max<uint64_t>(threads, quads ? (uint64_t)L.h * (L.w / 4) + 2 * (L.w + 2) + 2 * L.h : (uint64_t)(L.w + 2) * (L.h + 2));
  const uint32_t bx = (uint32_t)((threads + 255) / 256);
  for (uint64_t i0 = 0; i0 < n; i0 += PYR_MAX_Z) {
    const uint32_t z = (uint32_t)std::min<uint64_t>(PYR_MAX_Z, n - i0);
    if (quads)
      hipLaunchKernelGGL(pyr_luma_imap_kernel<true>, dim3(bx, levels, z), dim3(256), 0, ctx->stream, d_tab, levels, (uint32_t)i0);
    else
      hipLaunchKernelGGL(pyr_luma_imap_kernel<false>, dim3(bx, levels, z), dim3(256), 0, ctx->stream, d_tab, levels, (uint32_t)i0);
  }
}

// Intensities and the map an image lacks, in allocations of their own (freed with the image); `made` collects them for an
// undo on failure.
a3d_status alloc_intensity(const a3d_device_image* im, uint8_t** inten, float** imap, std::vector<void*>& made) {
  const size_t n = (size_t)im->width * im->height;
  *inten = im->has_intensities ? im->intensities : nullptr;
  *imap = im->has_imap ? im->imap : nullptr;
  if (!*inten) {
    A3D_HIP_TRY(hipMalloc((void**)inten, n));
    made.push_back(*inten);
  }
  if (!*imap) {
    A3D_HIP_TRY(hipMalloc((void**)imap, (size_t)(im->width + 2) * (im->height + 2) * 4));
    made.push_back(*imap);
  }
  return A3D_OK;
}

// Hands the buffers alloc_intensity made over to the image.
void adopt_intensity(a3d_device_image* im, uint8_t* inten, float* imap) {
  if (!im->has_intensities) im->intensities = inten, im->has_intensities = true, im->own_intensities = true;
  if (!im->has_imap) im->imap = imap, im->has_imap = true, im->own_imap = true;
}

inline size_t padded(size_t bytes) { return pad256(std::max<size_t>(1, bytes)); }

}  // namespace

extern "C" {

a3d_status a3d_range_image_set_colors(a3d_device_image* image, const uint8_t* rgb) {
  A3D_REQUIRE(image && rgb, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(!image->colors, A3D_INVALID_PARAMETER, "a3d_range_image_set_colors: the image already has colours");
  A3D_HIP_TRY(hipSetDevice(image->ctx->device));
  const size_t bytes = (size_t)image->width * image->height * 3;
  uint8_t* d = nullptr;
  A3D_HIP_TRY(hipMalloc((void**)&d, bytes + COLOR_SLACK));  // (the blur reads whole words: slack behind the last row)
  if (hipMemcpyAsync(d, rgb, bytes, hipMemcpyHostToDevice, image->ctx->stream) != hipSuccess ||
      hipStreamSynchronize(image->ctx->stream) != hipSuccess) {
    set_error("a3d_range_image_set_colors: upload failed: %s", hipGetErrorString(hipGetLastError()));
    hipFree(d);
    return A3D_HIP_ERROR;
  }
  image->colors = d, image->own_colors = true;
  return A3D_OK;
}

a3d_status a3d_range_image_compute_intensity(a3d_device_image* const* images, uint64_t n) {
  A3D_REQUIRE(images || n == 0, A3D_INVALID_PARAMETER, "null argument");
  if (n == 0) return A3D_OK;
  for (uint64_t i = 0; i < n; ++i) {
    A3D_REQUIRE(images[i], A3D_INVALID_PARAMETER, "image is null");
    A3D_REQUIRE(images[i]->ctx == images[0]->ctx, A3D_INVALID_PARAMETER,
                "a3d_range_image_compute_intensity: the images must share a context");
  }
  for (uint64_t i = 0; i < n; ++i)
    A3D_REQUIRE(images[i]->colors, A3D_MISSING_FIELD, "a3d_range_image_compute_intensity: image has no colours");
  a3d_context* ctx = images[0]->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  std::vector<PyrLevel> tab(n);
  std::vector<void*> made;
  a3d_status st = A3D_OK;
  for (uint64_t i = 0; i < n && st == A3D_OK; ++i) {
    const a3d_device_image* im = images[i];
    tab[i] = PyrLevel{im->points, im->mask, nullptr, im->colors, nullptr, nullptr, im->width, im->height};
    st = alloc_intensity(im, &tab[i].intensities, &tab[i].imap, made);
  }
  const PyrLevel* d_tab = nullptr;
  if (st == A3D_OK) st = upload_table(ctx, tab, &d_tab);
  if (st == A3D_OK) {
    launch_luma_imap(ctx, d_tab, tab, n, 1);
    if (hipGetLastError() != hipSuccess) set_error("a3d_range_image_compute_intensity: launch failed"), st = A3D_HIP_ERROR;
  }
  if (st != A3D_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : made) hipFree(p);
    return st;
  }
  for (uint64_t i = 0; i < n; ++i) adopt_intensity(images[i], tab[i].intensities, tab[i].imap);
  fence_self_work(ctx, images, n);  // enqueue-only, like a3d_range_image_compute_normals_batch
  return A3D_OK;
}

a3d_status a3d_range_image_pyramids(const a3d_device_image* const* level0, uint64_t n, uint64_t levels, float blur_sigma,
                                    uint32_t with_intensity, a3d_device_image** out_levels) {
  A3D_REQUIRE((level0 && out_levels) || n == 0, A3D_INVALID_PARAMETER, "null argument");
  // the builder's checks (a3d_range_image_build_pyramids), for the same reasons
  A3D_REQUIRE(levels >= 1 && levels <= PYR_MAX_LEVELS, A3D_INVALID_PARAMETER, "bad pyramid levels");
  A3D_REQUIRE(std::isfinite(blur_sigma), A3D_INVALID_PARAMETER, "blur_sigma must be finite");
  A3D_REQUIRE(levels == 1 || blur_sigma <= 3.0f, A3D_INVALID_PARAMETER, "blur_sigma above 3 is not supported");
  if (n == 0) return A3D_OK;
  for (uint64_t i = 0; i < n; ++i) {
    A3D_REQUIRE(level0[i], A3D_INVALID_PARAMETER, "image is null");
    A3D_REQUIRE(level0[i]->ctx == level0[0]->ctx && level0[i]->width == level0[0]->width &&
                    level0[i]->height == level0[0]->height,
                A3D_INVALID_PARAMETER, "a3d_range_image_pyramids: the images must share a context and a size");
  }
  const uint32_t w = level0[0]->width, h = level0[0]->height, L = (uint32_t)levels;
  A3D_REQUIRE((w >> (L - 1)) >= 2 && (h >> (L - 1)) >= 2, A3D_INVALID_PARAMETER,
              "image too small for this many pyramid levels");
  if (with_intensity)
    for (uint64_t i = 0; i < n; ++i)
      A3D_REQUIRE(level0[i]->colors, A3D_MISSING_FIELD, "a3d_range_image_pyramids: with_intensity needs colours");
  a3d_context* ctx = level0[0]->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  float sigma = blur_sigma;
  if (sigma <= 0.0f) sigma = 1.0f;  // (as the builder)

  // ---- the coarser levels: one pooled arena per image, laid out level by level
  std::vector<a3d_device_image*> made_images;  // [n][L - 1]
  std::vector<void*> made_buffers;             // level-0 intensities / maps not yet handed over
  std::vector<PyrLevel> tab((size_t)n * L);
  auto fail = [&](a3d_status st) {
    (void)hipStreamSynchronize(ctx->stream);
    for (a3d_device_image* im : made_images) a3d_range_image_free(im);  // (an image's last level releases its arena)
    for (void* p : made_buffers) hipFree(p);
    return st;
  };
  bool any_colors = false;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_device_image* im0 = level0[i];
    const bool normals = im0->has_normals && im0->normals, colors = im0->colors != nullptr;
    any_colors |= colors;
    PyrLevel& T0 = tab[i * L];
    T0 = PyrLevel{im0->points, im0->mask, normals ? im0->normals : nullptr, im0->colors, nullptr, nullptr, w, h};
    if (with_intensity && alloc_intensity(im0, &T0.intensities, &T0.imap, made_buffers) != A3D_OK) return fail(A3D_HIP_ERROR);
    if (L == 1) continue;
    size_t bytes = 0;
    std::vector<size_t> off((size_t)L * 6, 0);
    auto take = [&](size_t b) {
      const size_t at = bytes;
      bytes += padded(b);
      return at;
    };
    for (uint32_t l = 1; l < L; ++l) {
      const size_t px = (size_t)(w >> l) * (h >> l);
      size_t* o = &off[l * 6];
      o[0] = colors ? take(px * 3 + COLOR_SLACK) : 0;
      o[1] = take(px * 12), o[2] = take(px);
      o[3] = normals ? take(px * 12) : 0;
      o[4] = with_intensity ? take(px) : 0;
      o[5] = with_intensity ? take((size_t)((w >> l) + 2) * ((h >> l) + 2) * 4) : 0;
    }
    DeviceArena* arena = new DeviceArena();
    if (ctx_arena_acquire(ctx, bytes, arena) != A3D_OK) {
      delete arena;
      set_error("a3d_range_image_pyramids: hipMalloc(%zu) failed", bytes);
      return fail(A3D_HIP_ERROR);
    }
    char* b = (char*)arena->base;
    const a3d_device_image* prev = im0;
    for (uint32_t l = 1; l < L; ++l) {
      const size_t* o = &off[l * 6];
      a3d_device_image* im = new a3d_device_image();
      im->ctx = ctx, im->arena = arena;
      ++arena->refs;
      im->width = w >> l, im->height = h >> l;
      // CameraIntrinsics::scale(0.5) per level (camera.rs:119-127)
      im->fx64 = prev->fx64 * 0.5, im->fy64 = prev->fy64 * 0.5, im->cx64 = prev->cx64 * 0.5, im->cy64 = prev->cy64 * 0.5;
      im->fx = (float)im->fx64, im->fy = (float)im->fy64, im->cx = (float)im->cx64, im->cy = (float)im->cy64;
      // a pick is (0, 0, 0) with mask 0 or a source point of mask 1: mask == (z != 0) carries over from level 0
      im->mask_is_z = im0->mask_is_z;
      im->points = (float*)(b + o[1]), im->mask = (uint8_t*)(b + o[2]);
      if (colors) im->colors = (uint8_t*)(b + o[0]);
      if (normals) im->normals = (float*)(b + o[3]), im->has_normals = true;
      if (with_intensity) {
        im->intensities = (uint8_t*)(b + o[4]), im->imap = (float*)(b + o[5]);
        im->has_intensities = im->has_imap = true;
      }
      made_images.push_back(im);
      tab[i * L + l] = PyrLevel{im->points, im->mask, im->normals, im->colors, im->intensities, im->imap, im->width, im->height};
      prev = im;
    }
  }

  // ---- the launches: picks, colours, intensities (all on the context's stream)
  hipStream_t s = ctx->stream;
  const PyrLevel* d_tab = nullptr;
  if (upload_table(ctx, tab, &d_tab) != A3D_OK) return fail(A3D_HIP_ERROR);
  const bool fused = L >= 3 && w % 4 == 0 && h % 4 == 0;
  for (uint64_t i0 = 0; i0 < n; i0 += PYR_MAX_Z) {
    const uint32_t z = (uint32_t)std::min<uint64_t>(PYR_MAX_Z, n - i0), img0 = (uint32_t)i0;
    if (fused)
      hipLaunchKernelGGL(pyr_level0_quad_kernel, dim3((w + PQ - 1) / PQ, (h + PQ - 1) / PQ, z), dim3(256), 0, s, d_tab, L, img0,
                         L == 3);
    for (uint32_t l = fused ? 3 : 1; l < L; ++l) {
      const uint32_t dpx = (w >> l) * (h >> l);
      hipLaunchKernelGGL(pyr_pick_kernel, dim3((dpx + 255) / 256, 2, z), dim3(256), 0, s, d_tab, L, img0, l);
    }
    if (!any_colors) continue;
    for (uint32_t l = 1; l < L; ++l) {
      const uint32_t sw = w >> (l - 1), sh = h >> (l - 1), dw = w >> l, dh = h >> l;
      TapRow *d_tv = nullptr, *d_th = nullptr;
      if (taps_for(ctx, sh, dh, sigma, &d_tv) != A3D_OK || taps_for(ctx, sw, dw, sigma, &d_th) != A3D_OK) return fail(A3D_HIP_ERROR);
      const dim3 grid((dw + BLUR_TILE - 1) / BLUR_TILE, (dh + BLUR_ROWS - 1) / BLUR_ROWS, z);
      if ((sw * 3) % 4 == 0 && (RAW_PITCH / 4) <= 128)
        hipLaunchKernelGGL(pyr_blur_halve_words_kernel, grid, dim3(256), 0, s, d_tab, L, img0, l, 2.0f * sigma, d_tv, d_th);
      else
        hipLaunchKernelGGL(pyr_blur_halve_kernel, grid, dim3(256), 0, s, d_tab, L, img0, l, d_tv, d_th);
    }
  }
  if (with_intensity) launch_luma_imap(ctx, d_tab, tab, n, L);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("a3d_range_image_pyramids: %s", hipGetErrorString(hipGetLastError()));
    return fail(A3D_HIP_ERROR);
  }
  // complete: level 0 takes its intensities, the caller the new levels
  if (with_intensity)
    for (uint64_t i = 0; i < n; ++i)
      adopt_intensity(const_cast<a3d_device_image*>(level0[i]), tab[i * L].intensities, tab[i * L].imap);
  for (size_t k = 0; k < made_images.size(); ++k) out_levels[k] = made_images[k];
  return A3D_OK;
}

}  // extern "C"
