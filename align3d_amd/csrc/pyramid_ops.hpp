// Device pieces of the pyramid stages, shared by the frame builder (frame.hip: one arena per frame, arrays at fixed
// offsets) and the pyramid of arbitrary resident images (pyramid.hip: a table of per-image, per-level pointers).  Each
// stage is a __device__ body on plain pointers; the kernels of both files are thin wrappers that find their pointers and
// call it, so both run the same operations in the same order and give the same bits.
//   resize_range_points / _normals   src/range_image/resize.rs:4-104          (pick_nearest_to_mean, resize_pick_body)
//   py_scale_down2                   src/range_image/structure.rs:38-47        (blur_halve[_words]_body, make_taps, taps_for)
//   compute_intensity / _map         src/range_image/structure.rs:266-297, src/image/luma.rs:81-83,
//                                    src/intensity_map.rs:37-92              (luma_imap_body)
// The RGB blur (image 0.24.7 imageops::blur) is restated from its published algorithm like the oracle's: PARITY UNPINNED.
#pragma once
#include <cmath>
#include <vector>

#include "bilateral.hpp"

using namespace a3d;

namespace {

// One Vector3<f32> as ONE 12-byte store (global_store_dwordx3): three dword stores at a 12-byte lane stride make the
// memory pipeline touch every line of the wave's span three times, each time partially.
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef f32x3 __attribute__((aligned(4))) f32x3_u;
__device__ __forceinline__ void st_v3(float* base, size_t idx, V3 v) { *(f32x3_u*)(base + 3 * idx) = f32x3{v.x, v.y, v.z}; }
// The same off a block-uniform base pointer with a 32-bit pixel index (images are below 2^28 pixels: idx * 12 fits):
// `global_store … v_off, s[base]` — no 64-bit address arithmetic in the VALU (v_mad_u64_u32 runs at a quarter rate).
__device__ __forceinline__ void st_v3u(void* base, uint32_t idx, V3 v) {
  *(f32x3_u __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 12u) = f32x3{v.x, v.y, v.z};
}
__device__ __forceinline__ void st_u8u(void* base, uint32_t idx, uint8_t v) {
  *(uint8_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx) = v;
}
// Streaming forms for arrays nothing reads back soon (level 0's points, mask and normals; intensities and their maps).
__device__ __forceinline__ void st_v3u_stream(void* base, uint32_t idx, V3 v) {
#ifdef A3D_BUILDER_NO_NT
  st_v3u(base, idx, v);
#else
  __builtin_nontemporal_store(f32x3{v.x, v.y, v.z}, (f32x3_u __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 12u));
#endif
}
__device__ __forceinline__ void st_u8u_stream(void* base, uint32_t idx, uint8_t v) {
#ifdef A3D_BUILDER_NO_NT
  st_u8u(base, idx, v);
#else
  __builtin_nontemporal_store(v, (uint8_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx));
#endif
}
__device__ __forceinline__ void st_u16u_stream(void* base, uint32_t idx, uint16_t v) {
#ifdef A3D_BUILDER_NO_NT
  *(uint16_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 2u) = v;
#else
  __builtin_nontemporal_store(v, (uint16_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 2u));
#endif
}
// two horizontally adjacent u16 (idx even: 4-byte aligned)
__device__ __forceinline__ void st_u16x2u_stream(void* base, uint32_t idx, uint32_t lo, uint32_t hi) {
#ifdef A3D_BUILDER_NO_NT
  *(uint32_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 2u) = lo | (hi << 16);
#else
  __builtin_nontemporal_store(lo | (hi << 16), (uint32_t __attribute__((address_space(1)))*)((a3d_gptr)base + idx * 2u));
#endif
}
__device__ __forceinline__ V3 ld_v3g(const float* base, size_t idx) {
  const f32x3 v = *(const f32x3_u*)(base + 3 * idx);
  return V3{v.x, v.y, v.z};
}

// get_neighborhood_mean_point (src/range_image/resize.rs:4-40) on the four candidates of a 2 x 2 block in block order
// (00, 01, 10, 11): among the entries whose SOURCE mask is 1, the one nearest to their mean (strict <, first wins);
// (0,0,0) when none is valid.  *n_valid = how many were.
__device__ __forceinline__ V3 pick_nearest_to_mean(const V3 (&cand)[4], const bool (&ok)[4], int* n_valid) {
  int n = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) n += ok[q] ? 1 : 0;
  *n_valid = n;
  V3 nearest{0.f, 0.f, 0.f};
  if (n > 0) {
    V3 sum{0.f, 0.f, 0.f};  // valid entries in block order, as the reference's `local` list
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (ok[q]) sum = sum + cand[q];
    // sum / n (resize.rs:22-25): n is 1, 2, 3 or 4 — a division by 1, 2 or 4 is a multiplication by an exact power of two,
    // only n == 3 needs a real (IEEE) quotient
    V3 mean = sum * (n == 1 ? 1.0f : (n == 2 ? 0.5f : 0.25f));
    if (__builtin_amdgcn_ballot_w64(n == 3) != 0ull)  // (rare: three of the four valid — only at the edge of a hole)
      if (n == 3) mean = sum / 3.0f;
    float min_dist = 3.402823466e+38f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = norm_squared(cand[q] - mean);
      if (ok[q] && d < min_dist) {  // strict <: the first minimum wins
        min_dist = d;
        nearest = cand[q];
      }
    }
  }
  return nearest;
}

// rgb_to_luma_u8 (src/image/luma.rs:81-83): (r*0.3 + g*0.59 + b*0.11) as u8 (saturating truncation)
__device__ __forceinline__ uint8_t luma_u8(const uint8_t* __restrict__ rgb, uint32_t i) {
  const float l = (float)rgb[3 * i] * 0.3f + (float)rgb[3 * i + 1] * 0.59f + (float)rgb[3 * i + 2] * 0.11f;
  return l >= 255.0f ? 255 : (l <= 0.0f ? 0 : (uint8_t)l);
}

// compute_intensity + compute_intensity_map (structure.rs:266-297) for every level of every frame in one launch:
// blockIdx.y = level, blockIdx.z = frame.
// IntensityMap::from_luma_image (src/intensity_map.rs:37-92) including the incomplete border: rows h, h+1 copy row
// h-1 for cols < w-1; cols w, w+1 copy col w-1 for rows < h-1; (h, w) and (h+1, w+1) take the last pixel; the other
// border cells stay 0.  The luma of a cell's pixel is computed from the level's colours on the fly; interior cells
// also store it as the level's `intensities`.
// QUADS (the width is a multiple of four): a thread takes four interior cells of a row — 12 colour bytes as three
// aligned words, four lumas as one word, four map cells — and the threads behind the interior take the border cells
// one each; otherwise one thread per cell of the (h+2) x (w+2) map.
__device__ __forceinline__ uint8_t luma_of(uint32_t r, uint32_t g, uint32_t b) {
  const float l = (float)r * 0.3f + (float)g * 0.59f + (float)b * 0.11f;
  return l >= 255.0f ? 255 : (l <= 0.0f ? 0 : (uint8_t)l);
}
__device__ __forceinline__ float imap_border_cell(const uint8_t* __restrict__ rgb, uint32_t w, uint32_t h, uint32_t r, uint32_t c) {
  if (r >= h && c + 1 < w) return (float)luma_u8(rgb, (h - 1) * w + c) / 255.0f;
  if (c >= w && r + 1 < h) return (float)luma_u8(rgb, r * w + (w - 1)) / 255.0f;
  if ((r == h && c == w) || (r == h + 1 && c == w + 1)) return (float)luma_u8(rgb, (h - 1) * w + (w - 1)) / 255.0f;
  return 0.0f;
}
template <bool QUADS>
__device__ __forceinline__ void luma_imap_body(uint32_t i, uint32_t w, uint32_t h, const uint8_t* __restrict__ rgb,
                                               uint8_t* intensities, float* __restrict__ imap) {
  const uint32_t mw = w + 2, mh = h + 2;
  if (QUADS) {
    const uint32_t qpr = w / 4, n_quads = h * qpr, n_border = 2 * mw + 2 * h;
    if (i < n_quads) {
      const uint32_t r = i / qpr, c = 4 * (i % qpr), px = r * w + c;
      const uint32_t* src = (const uint32_t*)(rgb + (size_t)px * 3);  // 12 bytes at a multiple of 12: word-aligned
      const uint32_t a = src[0], b = src[1], d = src[2];
      const uint8_t l0 = luma_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
      const uint8_t l1 = luma_of(a >> 24, b & 255u, (b >> 8) & 255u);
      const uint8_t l2 = luma_of((b >> 16) & 255u, b >> 24, d & 255u);
      const uint8_t l3 = luma_of((d >> 8) & 255u, (d >> 16) & 255u, d >> 24);
      const uint32_t packed4 = (uint32_t)l0 | ((uint32_t)l1 << 8) | ((uint32_t)l2 << 16) | ((uint32_t)l3 << 24);
      float* o = imap + (size_t)r * mw + c;
#ifdef A3D_BUILDER_NO_NT
      *(uint32_t*)(intensities + px) = packed4;
      o[0] = (float)l0 / 255.0f, o[1] = (float)l1 / 255.0f, o[2] = (float)l2 / 255.0f, o[3] = (float)l3 / 255.0f;
#else  // streaming stores: the alignment reads these, much later
      __builtin_nontemporal_store(packed4, (uint32_t*)(intensities + px));
      __builtin_nontemporal_store((float)l0 / 255.0f, o), __builtin_nontemporal_store((float)l1 / 255.0f, o + 1);
      __builtin_nontemporal_store((float)l2 / 255.0f, o + 2), __builtin_nontemporal_store((float)l3 / 255.0f, o + 3);
#endif
    } else if (i < n_quads + n_border) {
      const uint32_t j = i - n_quads;
      uint32_t r, c;
      if (j < 2 * mw) r = h + j / mw, c = j % mw;
      else r = (j - 2 * mw) / 2, c = w + ((j - 2 * mw) & 1u);
      imap[(size_t)r * mw + c] = imap_border_cell(rgb, w, h, r, c);
    }
    return;
  }
  if (i >= mw * mh) return;
  const uint32_t r = i / mw, c = i % mw;
  float v;
  if (r < h && c < w) {
    const uint8_t l = luma_u8(rgb, r * w + c);
    (intensities)[r * w + c] = l;
    v = (float)l / 255.0f;
  } else {
    v = imap_border_cell(rgb, w, h, r, c);
  }
  imap[i] = v;
}

// get_neighborhood_mean_point over every 2x2 block (src/range_image/resize.rs:4-40): among the entries
// whose SOURCE mask is 1, the one nearest to their mean (strict <, first wins).  Used for points
// (writes the destination mask) and for normals (mask output null).
// The four candidates stay in registers (no dynamically indexed private array).
// (normals: dst_mask is not written)
__device__ __forceinline__ void resize_pick_body(uint32_t i, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, bool normals,
                                                 const float* __restrict__ src, const uint8_t* __restrict__ src_mask,
                                                 float* __restrict__ dst, uint8_t* dst_mask) {
  if (i >= dw * dh) return;
  const uint32_t dv = i / dw, du = i % dw;
  const float hr = (float)sh / (float)dh, wr = (float)sw / (float)dw;
  const uint32_t sv = (uint32_t)((float)dv * hr), su = (uint32_t)((float)du * wr);
  V3 cand[4];
  bool ok[4];
#pragma unroll
  for (uint32_t a = 0; a < 2; ++a)
#pragma unroll
    for (uint32_t b = 0; b < 2; ++b) {
      const uint32_t r = sv + a, c = su + b, q = a * 2 + b;
      const bool in = r < sh && c < sw;
      const uint32_t k = in ? r * sw + c : 0u;
      ok[q] = in && src_mask[k] == 1;
      cand[q] = ld_v3g(src, k);
    }
  int n;
  const V3 nearest = pick_nearest_to_mean(cand, ok, &n);
  st_v3u_stream(dst, i, nearest);  // (the coarsest levels: read by the alignment, not by the builder)
  if (!normals) st_u8u_stream(dst_mask, i, n > 0 ? 1 : 0);
}

// One tap table entry per output row / column: first tap, tap count, normalised weights.
constexpr int MAX_TAPS = 14;  // ceil(in + 2 sigma) - floor(in - 2 sigma) <= 14  <=>  sigma <= 3
struct TapRow {
  int32_t left, count;
  float w[MAX_TAPS];
};
// First tap and tap count of output sample `o` (source coordinates) of image::imageops::blur's sampling filter: the same
// f32 operations on host (make_taps) and device, so a kernel can place its loads without waiting for the table.
__host__ __device__ __forceinline__ void tap_range(uint32_t o, float support, uint32_t size, int32_t* left, int32_t* count) {
  const float in = (float)o + 0.5f;
  int32_t l = (int32_t)floorf(in - support);
  l = l < 0 ? 0 : (l > (int32_t)size - 1 ? (int32_t)size - 1 : l);
  int32_t r = (int32_t)ceilf(in + support);
  r = r < l + 1 ? l + 1 : (r > (int32_t)size ? (int32_t)size : r);
  *left = l, *count = r - l < MAX_TAPS ? r - l : MAX_TAPS;
}

// imageops::blur + 2x subsample fused: the pyramid keeps only the even rows and columns of the blurred image,
// so the vertical pass is evaluated at even rows only and never leaves the chip.  One block = BLUR_ROWS output rows x
// BLUR_TILE output columns: the source bytes its taps touch are fetched once, as aligned 32-bit words, into LDS
// (consecutive output rows share all but two of their source rows); the vertical sums (u8 -> f32, the crate's f32
// intermediate) go to a second LDS array, then the horizontal pass, clamp and round-half-away (u8) read them back.
// Per output the additions run in tap order from 0.0f in both passes, as in the crate.
constexpr uint32_t BLUR_TILE = 64, BLUR_ROWS = 4;  // (2 / 4 / 8 rows per block measured 32 / 31 / 37 us per 16 frames)
constexpr uint32_t BLUR_SPAN = 3 * (2 * BLUR_TILE + MAX_TAPS + 2);   // bytes / vertical results a tile's row can need
constexpr uint32_t RAW_ROWS = 2 * (BLUR_ROWS - 1) + MAX_TAPS;        // source rows under BLUR_ROWS output rows
constexpr uint32_t RAW_PITCH = ((BLUR_SPAN + 3 + 3) / 4) * 4;        // bytes per staged source row (+ alignment slack)
__device__ __forceinline__ void blur_halve_body(const uint8_t* __restrict__ rgb, uint32_t w, uint32_t dw, uint32_t dh,
                                                const TapRow* __restrict__ taps_v, const TapRow* __restrict__ taps_h,
                                                uint8_t* __restrict__ out) {
  __shared__ uint32_t s_raw[RAW_ROWS * RAW_PITCH / 4];
  __shared__ float s_v[BLUR_ROWS * BLUR_SPAN];
  __shared__ uint32_t s_shift[RAW_ROWS];
  const uint32_t dy0 = blockIdx.y * BLUR_ROWS, rows = min(BLUR_ROWS, dh - dy0);
  const uint32_t dx0 = blockIdx.x * BLUR_TILE, dx1 = min(dx0 + BLUR_TILE, dw) - 1;
  // rows [vtop, vbot) and columns [cmin, cmax) of the source under this tile (tap tables: block-uniform reads)
  const int32_t vtop = taps_v[dy0].left, vbot = taps_v[dy0 + rows - 1].left + taps_v[dy0 + rows - 1].count;
  const int32_t cmin = taps_h[dx0].left, cmax = taps_h[dx1].left + taps_h[dx1].count;
  const uint32_t span = (uint32_t)(cmax - cmin) * 3u, nraw = (uint32_t)(vbot - vtop);
  // ---- the source bytes, whole aligned words per row (colour arrays are 4-byte aligned and at least 3 bytes may
  // be read past their end: the builder's colours are never the last array of an arena, pyramid.hip pads its own) --------------------
  const uint32_t words = (span + 3 + 3) / 4;  // a row starts 0..3 bytes into its first word
  for (uint32_t e = threadIdx.x; e < nraw * words; e += 256) {
    const uint32_t j = e / words, k = e % words;
    const size_t first = ((size_t)(vtop + (int32_t)j) * w + (size_t)cmin) * 3;
    s_raw[j * (RAW_PITCH / 4) + k] = *(const uint32_t*)(rgb + (first & ~(size_t)3) + 4 * (size_t)k);
  }
  if (threadIdx.x < nraw)  // where in its first word each staged row starts
    s_shift[threadIdx.x] = (uint32_t)((((size_t)(vtop + (int32_t)threadIdx.x) * w + (size_t)cmin) * 3) & 3);
  __syncthreads();
  // ---- vertical pass: rows x span sums (row and taps block-uniform, the bytes of a row across lanes) ----------
  const uint8_t* raw = (const uint8_t*)s_raw;
  for (uint32_t r = 0; r < rows; ++r) {
    const TapRow* tv = taps_v + dy0 + r;  // row 2 * (dy0 + r) of the source (table built with stride 2)
    const int32_t j0 = tv->left - vtop, vcount = tv->count;
    for (uint32_t x = threadIdx.x; x < span; x += 256) {
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < MAX_TAPS; ++k)
        if (k < vcount) {
          const uint32_t j = (uint32_t)(j0 + k);
          acc += (float)raw[j * RAW_PITCH + s_shift[j] + x] * tv->w[k];
        }
      s_v[r * BLUR_SPAN + x] = acc;
    }
  }
  __syncthreads();
  // ---- horizontal pass: a thread owns one (column, channel) of the tile for all its rows: taps read once ------
  const uint32_t o = threadIdx.x, dx = dx0 + o / 3, ch = o % 3;
  if (o >= BLUR_TILE * 3 || dx >= dw) return;
  const TapRow th = taps_h[dx];
  const uint32_t h0 = (uint32_t)(th.left - cmin) * 3u + ch;
  for (uint32_t r = 0; r < rows; ++r) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < MAX_TAPS; ++k)
      if (k < th.count) acc += s_v[r * BLUR_SPAN + h0 + 3u * (uint32_t)k] * th.w[k];
    acc = fminf(fmaxf(acc, 0.0f), 255.0f);
    *(uint8_t __attribute__((address_space(1)))*)((a3d_gptr)out + (((dy0 + r) * dw + dx) * 3u + ch)) = (uint8_t)roundf(acc);
  }
}

// The same kernel when a colour row is a multiple of four bytes (w * 3 % 4 == 0: every staged row then starts at the
// same offset `sh` inside its first word): the vertical pass works on whole 32-bit words — one LDS read, four
// v_cvt_f32_ubyteN, four multiply / add pairs per word and tap instead of a byte-wide LDS read per output and tap — and
// the staging loop has no integer division.  Same operations per output in the same order: same bits.
__device__ __forceinline__ void blur_halve_words_body(const uint8_t* __restrict__ rgb, uint32_t w, uint32_t h, uint32_t dw,
                                                      uint32_t dh, float support, const TapRow* __restrict__ taps_v,
                                                      const TapRow* __restrict__ taps_h, uint8_t* __restrict__ out) {
  constexpr uint32_t PITCH_W = RAW_PITCH / 4;                    // words per staged row
  __shared__ uint32_t s_raw[RAW_ROWS * PITCH_W];
  __shared__ __attribute__((aligned(16))) float s_v[BLUR_ROWS * PITCH_W * 4];  // vertical sums, indexed by RAW byte position
  __shared__ uint32_t s_tv[BLUR_ROWS][16];                       // the tile's rows of the vertical tap table
  static_assert(sizeof(TapRow) == 64, "a tap row is sixteen words");
  const uint32_t dy0 = blockIdx.y * BLUR_ROWS, rows = min(BLUR_ROWS, dh - dy0);
  const uint32_t dx0 = blockIdx.x * BLUR_TILE, dx1 = min(dx0 + BLUR_TILE, dw) - 1;
  // The source rows [vtop, vbot) and columns [cmin, cmax) under this tile, from tap_range (what the tables hold): a block
  // then has ONE round of global loads — source words, its rows of the vertical table (to LDS) and each thread's row of
  // the horizontal table (to registers) are all in flight together — instead of table -> addresses -> source -> table.
  int32_t vtop, vbot, cmin, cmax, cnt;
  tap_range(2 * dy0, support, h, &vtop, &cnt);
  tap_range(2 * (dy0 + rows - 1), support, h, &vbot, &cnt), vbot += cnt;
  tap_range(2 * dx0, support, w, &cmin, &cnt);
  tap_range(2 * dx1, support, w, &cmax, &cnt), cmax += cnt;
  const uint32_t span = (uint32_t)(cmax - cmin) * 3u, nraw = (uint32_t)(vbot - vtop);
  const uint32_t sh = ((uint32_t)cmin * 3u) & 3u;               // the same for every row: w * 3 is a multiple of four
  const uint32_t words = (span + sh + 3) / 4;
  const uint32_t o = threadIdx.x, dx = dx0 + o / 3, ch = o % 3;
  const bool owns_output = o < BLUR_TILE * 3 && dx < dw;
  uint4 th4[4] = {};  // taps_h[dx]
  if (owns_output) {
    const uint4* src = (const uint4*)(taps_h + dx);
#pragma unroll
    for (int i = 0; i < 4; ++i) th4[i] = src[i];
  }
  const bool stages_taps = threadIdx.x < rows * 16u;
  const uint32_t tv_word = stages_taps ? ((const uint32_t*)(taps_v + dy0))[threadIdx.x] : 0u;  // (parked behind the source loads)
  // ---- staging: thread = (row slot t / 128, word t % 128); a tile's row has at most 108 words ----
  {
    const uint32_t k = threadIdx.x & 127u, jj = threadIdx.x >> 7;
    // (32-bit byte offsets off the image's uniform colour pointer: an image is below 2^28 pixels)
    const uint32_t row_bytes = w * 3u;
    const uint32_t first = (((uint32_t)vtop * w + (uint32_t)cmin) * 3u & ~3u) + 4u * k;
    // (every load of the thread issued before the first is parked in LDS: a loop over j with a run-time trip count is
    // compiled into rounds of two loads, each round waiting for the previous one)
    uint32_t got[RAW_ROWS / 2];
#pragma unroll
    for (uint32_t i = 0; i < RAW_ROWS / 2; ++i) {
      const uint32_t j = jj + 2 * i;
      got[i] = (k < words && j < nraw) ? *(const uint32_t __attribute__((address_space(1)))*)((a3d_gptr_c)rgb + (first + j * row_bytes)) : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < RAW_ROWS / 2; ++i) {
      const uint32_t j = jj + 2 * i;
      if (k < words && j < nraw) s_raw[j * PITCH_W + k] = got[i];
    }
  }
  if (stages_taps) s_tv[threadIdx.x >> 4][threadIdx.x & 15u] = tv_word;
  __syncthreads();
  // ---- vertical pass, word-wise: item = (output row r, word q) ----
  for (uint32_t e = threadIdx.x; e < rows * 128u; e += 256) {
    const uint32_t r = e >> 7, q = e & 127u;
    if (q >= words) continue;
    // row 2 * (dy0 + r) of the source (table built with stride 2)
    // (r is the same for the 64 lanes of a wave — 128 items per row — so the tap count is a scalar: up to SHORT_TAPS
    // taps (sigma = 1 has five) run an unrolled body of that many predicated taps instead of fourteen)
    const int32_t j0 = (int32_t)s_tv[r][0] - vtop, vcount = __builtin_amdgcn_readfirstlane((int32_t)s_tv[r][1]);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    auto tap = [&](int k) {
      const uint32_t word = s_raw[(uint32_t)(j0 + k) * PITCH_W + q];
      const float wk = __uint_as_float(s_tv[r][2 + k]);
      a0 += (float)(word & 255u) * wk, a1 += (float)((word >> 8) & 255u) * wk;
      a2 += (float)((word >> 16) & 255u) * wk, a3 += (float)(word >> 24) * wk;
    };
    constexpr int SHORT_TAPS = 6;
    if (vcount <= SHORT_TAPS) {
#pragma unroll
      for (int k = 0; k < SHORT_TAPS; ++k)
        if (k < vcount) tap(k);
    } else {
#pragma unroll
      for (int k = 0; k < MAX_TAPS; ++k)
        if (k < vcount) tap(k);
    }
    *(float4*)(s_v + (r * PITCH_W + q) * 4) = make_float4(a0, a1, a2, a3);
  }
  __syncthreads();
  // ---- horizontal pass: a thread owns one (column, channel) of the tile for all its rows: taps read once ------
  if (!owns_output) return;
  const uint32_t tw[16] = {th4[0].x, th4[0].y, th4[0].z, th4[0].w, th4[1].x, th4[1].y, th4[1].z, th4[1].w,
                           th4[2].x, th4[2].y, th4[2].z, th4[2].w, th4[3].x, th4[3].y, th4[3].z, th4[3].w};
  const int32_t hcount = (int32_t)tw[1];
  const uint32_t h0 = (uint32_t)((int32_t)tw[0] - cmin) * 3u + ch + sh;
  // (the same short body when no lane of the wave has more than SHORT_TAPS taps)
  const bool short_taps = __builtin_amdgcn_ballot_w64(hcount > 6) == 0ull;
  for (uint32_t r = 0; r < rows; ++r) {
    float acc = 0.0f;
    if (short_taps) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < hcount) acc += s_v[r * PITCH_W * 4 + h0 + 3u * (uint32_t)k] * __uint_as_float(tw[2 + k]);
    } else {
#pragma unroll
      for (int k = 0; k < MAX_TAPS; ++k)
        if (k < hcount) acc += s_v[r * PITCH_W * 4 + h0 + 3u * (uint32_t)k] * __uint_as_float(tw[2 + k]);
    }
    acc = fminf(fmaxf(acc, 0.0f), 255.0f);
    *(uint8_t __attribute__((address_space(1)))*)((a3d_gptr)out + (((dy0 + r) * dw + dx) * 3u + ch)) = (uint8_t)roundf(acc);
  }
}

// Tap tables of image::imageops::blur's sampling filter (support 2 sigma, weights renormalised over the
// clamped range), computed on the host in f32 exactly as the oracle computes them.
std::vector<TapRow> make_taps(uint32_t size, float sigma, uint32_t stride, uint32_t count) {
  const float support = 2.0f * sigma;
  std::vector<TapRow> rows(count);
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t o = k * stride;
    const float in = (float)o + 0.5f;
    const float c = in - 0.5f;
    TapRow r{};
    tap_range(o, support, size, &r.left, &r.count);  // (callers reject sigma > 3: more than MAX_TAPS taps)
    const int64_t left = r.left;
    float sum = 0.0f, wv[MAX_TAPS];
    for (int i = 0; i < r.count; ++i) {
      const float x = (float)(left + i) - c;
      wv[i] = 1.0f / (std::sqrt(2.0f * 3.14159265358979323846f) * sigma) * std::exp(-(x * x) / (2.0f * sigma * sigma));
      sum += wv[i];
    }
    for (int i = 0; i < r.count; ++i) r.w[i] = wv[i] / sum;
    rows[k] = r;
  }
  return rows;
}

// The tap tables depend on (size, sigma) only: computed and uploaded once per context, then reused.
a3d_status taps_for(a3d_context* ctx, uint32_t size, uint32_t count, float sigma, TapRow** out) {
  uint32_t key[4] = {0x54415053u /* 'TAPS' */, size, count, 0};
  memcpy(&key[3], &sigma, 4);
  for (const auto& t : ctx->tables)
    if (!memcmp(t.key, key, sizeof(key))) {
      *out = (TapRow*)t.d;
      return A3D_OK;
    }
  const std::vector<TapRow> rows = make_taps(size, sigma, 2, count);
  return ctx_cached_table(ctx, key, rows.data(), rows.size() * sizeof(TapRow), (void**)out);
}

}  // namespace
