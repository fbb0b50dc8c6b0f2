// Plane segmentation of resident clouds (a3d_point_clouds_segment_plane_device): RANSAC with every candidate scored,
// the inliers of the best candidate flagged, the model refitted to them from integer moments.
//
// The rule of the plane call.  Every f32 and every f64 operation is rounded on its own, as the build's
// -ffp-contract=off already ensures.  Divide and sqrt are correctly rounded.
// Per call: a distance threshold t, f32, finite and > 0, and a number of refinement rounds R with 0 <= R <= 8.
// Per cloud i: H_i candidate triples (a, b, c) of row numbers, [H_i][3] u32 in HOST memory.  0 <= H_i <= 4096.  Every
// index is < len_i.
//  1. Candidate plane of a triple.  The three points are widened to f64.  u = p_b - p_a, v = p_c - p_a.  m = u x v, each
//     component as u_y*v_z - u_z*v_y.  L = (m_x*m_x + m_y*m_y) + m_z*m_z.  U = (u_x*u_x + u_y*u_y) + u_z*u_z, and V
//     likewise.  The candidate is DEGENERATE iff two of its indices are equal, or L is not finite, or not
//     L > (U*V) * 2^-20.  That covers a repeated row, a non-finite row, and three rows whose sine is below 2^-10.
//     Otherwise n = (float)(m / sqrt(L)) per component, and the plane's point is p_a, in f32 as stored.
//  2. Distance and inlier, in f32.  e_k = p_k - p_ak, d = (n_x*e_x + n_y*e_y) + n_z*e_z.  Row p is an inlier of the
//     candidate iff fabsf(d) <= t.  A row with a NaN or an infinity is never an inlier.  The form p - a is deliberate.
//     n.p + w saves three operations per test and cancels badly for clouds far from the origin.
//  3. Score.  count[h] is the number of inliers of candidate h over ALL rows of the cloud, and 0 for a degenerate
//     candidate.  The best candidate maximises count[h] << 32 | (0xFFFFFFFF - h): the most inliers, the lowest h on a
//     tie.  If every candidate is degenerate, or H_i == 0 or len_i == 0, there is no plane: flags all 0, plane four
//     zeros, best = 0xFFFFFFFF, status A3D_OK.
//  4. Flags.  flags[p] = 1 iff p is an inlier of the current plane (n, point), else 0.  After step 3 the current plane
//     is the best candidate's.
//  5. Refit moments over the rows with flag 1, all in integers.  s = 64.0f / t in f32.  q_k = (int) rintf(e_k * s), ties
//     to even, with e from step 2 against the current plane's point.  A flagged row takes part iff
//     fabsf(e_k * s) <= 1048576.0f for all three k.  N = sum 1, S_k = sum q_k, and for the six products P = q_k q_l, with
//     |P| <= 2^40: Lo_kl = sum (P & 0x7FFFFFFF), Hi_kl = sum (P >> 31), an arithmetic shift.  So
//     M_kl = Hi_kl * 2^31 + Lo_kl exactly.  With len < 2^32, N, S, Lo and Hi each fit 64 bits, so no order of summation
//     can matter.  The record is 16 u64 words: N, S[3], Lo[6], Hi[6] in the order xx, xy, xz, yy, yz, zz.
//  6. Plane from moments, on the HOST (a3d_plane_from_moments).  A_kl = N*M_kl - S_k*S_l, exact in 128-bit integers
//     (|A| < 2^105).  Each A_kl converted to f64, round to nearest even.  mx = max |A_kl|.  The refit is VALID iff N >= 3
//     and mx > 0.  Then steps 4 (scaling by frexp's exponent) to 6 (normal = column of the smallest diagonal entry,
//     normalised) of the rule of a3d_point_clouds_estimate_normals_device: six cyclic Jacobi sweeps in f32.  Centroid in
//     f64: c_k = (double)a_k + ((double)S_k / (double)N) / (double)s, with a the point that the moments were taken
//     against.  d = -((n_x*c_x + n_y*c_y) + n_z*c_z) in f64, with n widened.  The four numbers are negated iff d < 0.
//     This is the side the origin is on: the default viewpoint of the normals call.  If the refit is not valid, the
//     plane is the current plane itself: its f32 normal widened, and c = a; d and the sign follow in the same way.
//  7. Refinement, R times.  The current plane becomes the plane of step 6: normal (float)n, point (float)c.  Steps 4 and
//     5 are repeated against it, then step 6.  R = 0 is the inliers of the best candidate and the model refitted to them.
// Every count, flag and moment is an integer decided on f32 bits that no order can change: the same on every run.
//
// The launches, whatever the number of clouds: one upload (job table, triples, zeroed words), one fill (the counters),
// then candidates (a thread per candidate, f64), score, best (a block per job) and flag + moments; per refinement round
// one download of the round's records, step 6 on the host, one upload of the new planes and one flag + moments launch.
//
// The score kernel is the hot path: N * H point-plane tests.  A block owns a tile of one job's rows and a range of its
// candidates; it loads four rows per thread into registers once per chunk and then walks its candidates.  The eight
// plane words of a candidate sit at a block-uniform address and arrive by one scalar load, a candidate ahead; a wave
// counts its inliers with ballot + popcount on the scalar unit and adds one number per candidate into an LDS array of
// counters; at the end the block adds its non-zero counters to the job's global counters, one no-return atomic each.  A
// degenerate candidate is skipped uniformly.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cloud_batch.hpp"

namespace a3d {
namespace {

constexpr uint32_t PL_THREADS = 256;
constexpr uint32_t PL_CHUNK = 1024;      // rows of a chunk of the tile plan (flag + moments: four rows per thread)
constexpr uint32_t PL_MAX_TILES = 4096;  // per job
constexpr uint32_t PL_MAX_CAND = 4096;   // candidates per job: the LDS counters of a score block (16 KB)
constexpr uint32_t PL_MAX_REFINE = 8;
constexpr uint32_t PL_RECORD = 17;       // device record of a round: flagged rows, then the 16 words of step 5
constexpr uint32_t PL_PLANE = 8;         // a plane in 32-bit words: n[3], point[3], 1 iff there is a plane, 0
// The same words read through the constant address space: at a wave-uniform address that is a scalar load into SGPRs.
// The words were written by an earlier launch of the same call, never by the kernel that reads them this way.
typedef const uint32_t __attribute__((address_space(4))) * PlaneWords;
__device__ __forceinline__ PlaneWords plane_words(const float* planes, size_t index) {
  return (PlaneWords)(uintptr_t)(planes + PL_PLANE * index);
}

struct PlaneJob {
  const float* points;
  uint32_t* flags;
  uint32_t* out_counts;     // the caller's [n_cand] or null
  const uint32_t* triples;  // [n_cand][3], in the call's upload
  float* cand;              // [n_cand][PL_PLANE]: a zero normal and a zero seventh word for a degenerate candidate
  uint32_t* counts;         // [n_cand], zeroed by the call's fill
  uint32_t len, n_cand;
  uint32_t first_tile, chunks_per_tile;
};
static_assert(sizeof(PlaneJob) == 64, "PlaneJob layout");

// Step 1: a thread per candidate of every job; `per` blocks per job.
__global__ void __launch_bounds__(PL_THREADS)
    plane_candidates_kernel(const PlaneJob* __restrict__ jobs, uint32_t per) {
  const PlaneJob& j = jobs[blockIdx.x / per];
  const uint32_t h = (blockIdx.x % per) * PL_THREADS + threadIdx.x;
  if (h >= j.n_cand) return;
  const uint32_t ia = j.triples[3 * h], ib = j.triples[3 * h + 1], ic = j.triples[3 * h + 2];
  const f32x3 a = *(const f32x3_u*)(j.points + 3 * (size_t)ia);
  const f32x3 b = *(const f32x3_u*)(j.points + 3 * (size_t)ib);
  const f32x3 c = *(const f32x3_u*)(j.points + 3 * (size_t)ic);
  const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
  const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
  const double mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
  const double L = (mx * mx + my * my) + mz * mz;
  const double U = (ux * ux + uy * uy) + uz * uz, V = (vx * vx + vy * vy) + vz * vz;
  const bool good = ia != ib && ia != ic && ib != ic && L - L == 0.0 && L > (U * V) * 0x1p-20;
  f32x3 n = {0.f, 0.f, 0.f};
  if (good) {
    const double r = sqrt(L);
    n.x = (float)(mx / r), n.y = (float)(my / r), n.z = (float)(mz / r);
  }
  float* out = j.cand + PL_PLANE * (size_t)h;
  *(f32x3_u*)out = n;
  *(f32x3_u*)(out + 3) = a;
  ((uint32_t*)out)[6] = good ? 1u : 0u, ((uint32_t*)out)[7] = 0u;
}

// Steps 2 and 3, the counts.  Grid: (tiles of the batch, splits of the candidates).  ROWS rows per thread and chunk pass;
// LDS_COUNTERS false is the form that lost: a global atomic per wave and candidate (diagnostics).
template <uint32_t ROWS, bool LDS_COUNTERS>
__global__ void __launch_bounds__(PL_THREADS)
    plane_score_kernel(const PlaneJob* __restrict__ jobs, uint32_t n_jobs, float t) {
  __shared__ uint32_t s_count[LDS_COUNTERS ? PL_MAX_CAND : 1];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const PlaneJob& j = jobs[ji];
  const uint32_t n_cand = j.n_cand;
  const uint32_t h_per = (n_cand + gridDim.y - 1) / gridDim.y;
  const uint32_t h0 = min(n_cand, blockIdx.y * h_per), h1 = min(n_cand, h0 + h_per);
  if (h0 >= h1) return;  // block-uniform
  const float* __restrict__ points = j.points;
  const float* cand = j.cand;
  uint32_t* __restrict__ counts = j.counts;
  const uint64_t len = j.len, span = (uint64_t)j.chunks_per_tile * PL_CHUNK;
  const uint64_t p0 = (uint64_t)(tile - j.first_tile) * span, p_end = min(len, p0 + span);
  if (LDS_COUNTERS) {
    for (uint32_t h = h0 + threadIdx.x; h < h1; h += PL_THREADS) s_count[h] = 0;
    __syncthreads();
  }
  const bool lane0 = (threadIdx.x & 63u) == 0;
  for (uint64_t base = p0; base < p_end; base += ROWS * PL_THREADS) {  // block-uniform
    f32x3 p[ROWS];
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
      const uint64_t row = base + r * PL_THREADS + threadIdx.x;
      // a row past the end is a NaN row: never an inlier
      p[r] = row < p_end ? *(const f32x3_u*)(points + 3 * row) : f32x3{NAN, NAN, NAN};
    }
    // block-uniform: the eight plane words of a candidate are one scalar load, requested a candidate ahead
    uint32_t w[PL_PLANE], ahead[PL_PLANE];
#pragma unroll
    for (uint32_t k = 0; k < PL_PLANE; ++k) w[k] = plane_words(cand, h0)[k];
    for (uint32_t h = h0; h < h1; ++h) {
      const PlaneWords next = plane_words(cand, min(h + 1, h1 - 1));
#pragma unroll
      for (uint32_t k = 0; k < PL_PLANE; ++k) ahead[k] = next[k];
      // not degenerate (a degenerate candidate counts 0).  Word 7 is always 0; reading it keeps all eight registers of the
      // load ahead alive through the tests, so none of them is reused as a temporary that would have to wait for the load.
      if (w[6] != w[7]) {
        const float nx = __uint_as_float(w[0]), ny = __uint_as_float(w[1]), nz = __uint_as_float(w[2]);
        const float ax = __uint_as_float(w[3]), ay = __uint_as_float(w[4]), az = __uint_as_float(w[5]);
        uint32_t c = 0;
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
          const float ex = p[r].x - ax, ey = p[r].y - ay, ez = p[r].z - az;
          const float d = (nx * ex + ny * ey) + nz * ez;
          c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(fabsf(d) <= t));  // wave-uniform
        }
        if (c && lane0) {
          if (LDS_COUNTERS) atomicAdd(&s_count[h], c);
          else atomicAdd(&counts[h], c);
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < PL_PLANE; ++k) w[k] = ahead[k];
    }
  }
  if (LDS_COUNTERS) {
    __syncthreads();
    for (uint32_t h = h0 + threadIdx.x; h < h1; h += PL_THREADS) {
      const uint32_t c = s_count[h];
      if (c) atomicAdd(&counts[h], c);
    }
  }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// Step 3, the best candidate: a block per job.  best[job] = its index or 0xFFFFFFFF; planes[job] = the current plane.
__global__ void __launch_bounds__(PL_THREADS)
    plane_best_kernel(const PlaneJob* __restrict__ jobs, unsigned long long* __restrict__ best, float* __restrict__ planes) {
  __shared__ unsigned long long s_key[PL_THREADS / 64];
  const PlaneJob& j = jobs[blockIdx.x];
  unsigned long long key = 0;
  for (uint32_t h = threadIdx.x; h < j.n_cand; h += PL_THREADS) {
    const uint32_t c = j.counts[h];
    if (j.out_counts) j.out_counts[h] = c;
    const unsigned long long k = (unsigned long long)c << 32 | (0xFFFFFFFFu - h);
    key = k > key ? k : key;
  }
  key = wave_max_u64(key);
  if ((threadIdx.x & 63u) == 0) s_key[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 0; w < PL_THREADS / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
    // a candidate that is not degenerate counts at least its own first row, so no count above 0 means no plane
    const bool found = (key >> 32) != 0;
    const uint32_t h = 0xFFFFFFFFu - (uint32_t)key;
    best[blockIdx.x] = found ? h : 0xFFFFFFFFull;
    float* out = planes + PL_PLANE * (size_t)blockIdx.x;
    for (uint32_t k = 0; k < 6; ++k) out[k] = found ? j.cand[PL_PLANE * (size_t)h + k] : 0.f;
    ((uint32_t*)out)[6] = found ? 1u : 0u;
    ((uint32_t*)out)[7] = 0u;
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Steps 4 and 5: a thread per row writes the flag; a wave sums its 17 integers by shuffles before its no-return 64-bit
// atomics into the job's record of this round.  s = 64.0f / t.
__global__ void __launch_bounds__(PL_THREADS)
    plane_flag_kernel(const PlaneJob* __restrict__ jobs, uint32_t n_jobs, float t, float s, const float* __restrict__ planes,
                      unsigned long long* __restrict__ records) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const PlaneJob& j = jobs[ji];
  const float* __restrict__ points = j.points;
  uint32_t* __restrict__ flags = j.flags;
  const PlaneWords w = plane_words(planes, ji);
  const float nx = __uint_as_float(w[0]), ny = __uint_as_float(w[1]), nz = __uint_as_float(w[2]);
  const float ax = __uint_as_float(w[3]), ay = __uint_as_float(w[4]), az = __uint_as_float(w[5]);
  const bool has_plane = w[6] != 0;
  const uint64_t len = j.len, span = (uint64_t)j.chunks_per_tile * PL_CHUNK;
  const uint64_t p0 = (uint64_t)(tile - j.first_tile) * span, p_end = min(len, p0 + span);
  unsigned long long acc[PL_RECORD];
#pragma unroll
  for (uint32_t k = 0; k < PL_RECORD; ++k) acc[k] = 0;
  for (uint64_t base = p0; base < p_end; base += PL_THREADS) {  // block-uniform
    const uint64_t row = base + threadIdx.x;
    if (row >= p_end) continue;
    const f32x3 p = *(const f32x3_u*)(points + 3 * row);
    const float ex = p.x - ax, ey = p.y - ay, ez = p.z - az;
    const float d = (nx * ex + ny * ey) + nz * ez;
    const bool inlier = has_plane && fabsf(d) <= t;
    flags[row] = inlier ? 1u : 0u;
    const float fx = ex * s, fy = ey * s, fz = ez * s;
    if (inlier) acc[0] += 1;
    if (inlier && fabsf(fx) <= 1048576.0f && fabsf(fy) <= 1048576.0f && fabsf(fz) <= 1048576.0f) {
      const long long qx = (long long)(int)rintf(fx), qy = (long long)(int)rintf(fy), qz = (long long)(int)rintf(fz);
      const long long pr[6] = {qx * qx, qx * qy, qx * qz, qy * qy, qy * qz, qz * qz};
      acc[1] += 1;
      acc[2] += (unsigned long long)qx, acc[3] += (unsigned long long)qy, acc[4] += (unsigned long long)qz;
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) {
        acc[5 + k] += (unsigned long long)(pr[k] & 0x7FFFFFFFll);
        acc[11 + k] += (unsigned long long)(pr[k] >> 31);
      }
    }
  }
  const unsigned long long flagged = wave_sum_u64(acc[0]);
  if (flagged == 0) return;  // wave-uniform: nothing to add
  unsigned long long* __restrict__ rec = records + PL_RECORD * (size_t)ji;
  const bool lane0 = (threadIdx.x & 63u) == 0;
  if (lane0) atomicAdd(&rec[0], flagged);
#pragma unroll
  for (uint32_t k = 1; k < PL_RECORD; ++k) {
    const unsigned long long v = wave_sum_u64(acc[k]);
    if (lane0 && v) atomicAdd(&rec[k], v);
  }
}

// ---- step 6 on the host ----------------------------------------------------------------------------------------------

void jacobi_rotate_host(float& app, float& aqq, float& apq, float& aop, float& aoq, float* vp, float* vq) {
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  const float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
  const float h = t * apq;
  app = app - h, aqq = aqq + h, apq = 0.f;
  const float op = aop, oq = aoq;
  aop = c * op - s * oq, aoq = s * op + c * oq;
  for (int k = 0; k < 3; ++k) {
    const float a = vp[k], b = vq[k];
    vp[k] = c * a - s * b, vq[k] = s * a + c * b;
  }
}

// What no call can have produced is refused; everything else cannot overflow 128 bits.
bool moments_in_range(const uint64_t m[16]) {
  const uint64_t N = m[0];
  if (N >= (1ull << 32)) return false;
  for (int k = 0; k < 3; ++k) {
    const int64_t S = (int64_t)m[1 + k];
    if ((S < 0 ? -(unsigned __int128)S : (unsigned __int128)S) > ((unsigned __int128)N << 20)) return false;
  }
  for (int k = 0; k < 6; ++k) {
    const int64_t hi = (int64_t)m[10 + k];
    if ((unsigned __int128)m[4 + k] > (unsigned __int128)N * 0x7FFFFFFFull) return false;
    if ((hi < 0 ? -(unsigned __int128)hi : (unsigned __int128)hi) > ((unsigned __int128)N << 9)) return false;
  }
  return true;
}

// Step 6.  plane[4]; centroid[3] = c, the point of the next round's plane; returns whether the refit was valid.
bool plane_from_moments(const uint64_t m[16], const float a[3], float t, const float fallback[3], double plane[4],
                        double centroid[3]) {
  typedef __int128 i128;
  const float s = 64.0f / t;
  const uint64_t N = m[0];
  i128 S[3], M[6];
  for (int k = 0; k < 3; ++k) S[k] = (i128)(int64_t)m[1 + k];
  for (int k = 0; k < 6; ++k) M[k] = (i128)(int64_t)m[10 + k] * ((i128)1 << 31) + (i128)m[4 + k];
  static const int KL[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  double A[6], mx = 0.0;
  for (int k = 0; k < 6; ++k) {
    A[k] = (double)((i128)N * M[k] - S[KL[k][0]] * S[KL[k][1]]);
    mx = std::fmax(mx, std::fabs(A[k]));
  }
  const bool valid = N >= 3 && mx > 0.0;
  double n[3] = {(double)fallback[0], (double)fallback[1], (double)fallback[2]};
  double c[3] = {(double)a[0], (double)a[1], (double)a[2]};
  if (valid) {
    int e;
    (void)std::frexp(mx, &e);
    float a00 = (float)std::ldexp(A[0], -e), a01 = (float)std::ldexp(A[1], -e), a02 = (float)std::ldexp(A[2], -e),
          a11 = (float)std::ldexp(A[3], -e), a12 = (float)std::ldexp(A[4], -e), a22 = (float)std::ldexp(A[5], -e);
    float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};  // the columns of V
    for (int sweep = 0; sweep < 6; ++sweep) {
      jacobi_rotate_host(a00, a11, a01, a02, a12, v0, v1);  // (0,1), o = 2
      jacobi_rotate_host(a00, a22, a02, a01, a12, v0, v2);  // (0,2), o = 1
      jacobi_rotate_host(a11, a22, a12, a01, a02, v1, v2);  // (1,2), o = 0
    }
    float lam = a00;
    const float* col = v0;
    if (a11 < lam) lam = a11, col = v1;
    if (a22 < lam) lam = a22, col = v2;
    const float norm = sqrtf((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]);
    for (int k = 0; k < 3; ++k) {
      n[k] = (double)(col[k] / norm);
      c[k] = (double)a[k] + ((double)(int64_t)m[1 + k] / (double)N) / (double)s;
    }
  }
  double d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]);
  if (d < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2], d = -d;
  plane[0] = n[0], plane[1] = n[1], plane[2] = n[2], plane[3] = d;
  centroid[0] = c[0], centroid[1] = c[1], centroid[2] = c[2];
  return valid;
}

}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" {

a3d_status a3d_point_clouds_segment_plane_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n, float t,
                                                 uint32_t refine, const uint32_t* const* triples, const uint32_t* n_triples,
                                                 uint32_t* const* d_out_flags, uint32_t* const* d_out_counts,
                                                 double* out_planes, uint64_t* out_best, uint64_t* out_inliers,
                                                 uint64_t* out_refit_rows) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(ctx && d_clouds && triples && n_triples && d_out_flags && out_planes, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(std::isfinite(t) && t > 0.f, A3D_INVALID_PARAMETER,
              "a3d_point_clouds_segment_plane_device: the distance threshold must be finite and positive");
  const float s = 64.0f / t;
  A3D_REQUIRE(std::isfinite(s), A3D_INVALID_PARAMETER,
              "a3d_point_clouds_segment_plane_device: a distance threshold so small that 64 / t is not finite in f32");
  A3D_REQUIRE(refine <= PL_MAX_REFINE, A3D_INVALID_PARAMETER,
              "a3d_point_clouds_segment_plane_device: at most 8 refinement rounds");
  std::vector<PlaneJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  std::vector<size_t> cand_at;  // per job: the candidates of the jobs before it
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), cand_at.reserve(n), ranges.reserve(4 * n);
  uint64_t tiles = 0;
  size_t cand_total = 0;
  uint32_t cand_max = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    const uint32_t H = n_triples[i];
    A3D_REQUIRE(c.len < (1ull << 32), A3D_INVALID_PARAMETER, "a cloud of 2^32 points or more");
    A3D_REQUIRE(H <= PL_MAX_CAND, A3D_INVALID_PARAMETER,
                "a3d_point_clouds_segment_plane_device: at most 4096 candidates per cloud");
    A3D_REQUIRE(H == 0 || triples[i], A3D_INVALID_PARAMETER, "null triples pointer");
    for (size_t k = 0; k < 3 * (size_t)H; ++k)
      A3D_REQUIRE(triples[i][k] < c.len, A3D_INVALID_PARAMETER,
                  "a3d_point_clouds_segment_plane_device: a triple names a row past the end of its cloud");
    if (c.len == 0) continue;  // no plane; its pointers may be null
    A3D_REQUIRE(c.points && d_out_flags[i], A3D_INVALID_PARAMETER, "null points or flags pointer");
    PlaneJob j{};
    j.points = c.points, j.flags = d_out_flags[i];
    j.out_counts = d_out_counts && H ? d_out_counts[i] : nullptr;
    j.len = (uint32_t)c.len, j.n_cand = H;
    cand_at.push_back(cand_total);
    cand_total += H, cand_max = std::max(cand_max, H);
    A3D_TRY(plan_tiles(c.len, PL_CHUNK, PL_MAX_TILES, &tiles, &j.first_tile, &j.chunks_per_tile));
    jobs.push_back(j), cloud_of_job.push_back(i);
    ranges.in(c.points, c.len * 12), ranges.in(c.normals, c.len * 12);
    ranges.out(j.flags, c.len * 4), ranges.out(j.out_counts, (uint64_t)H * 4);
  }
  A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
              "a3d_point_clouds_segment_plane_device: an output overlaps an input or another output");
  for (uint64_t i = 0; i < n; ++i) {
    for (int k = 0; k < 4; ++k) out_planes[4 * i + k] = 0.0;
    if (out_best) out_best[i] = 0xFFFFFFFFull;
    if (out_inliers) out_inliers[i] = 0;
    if (out_refit_rows) out_refit_rows[i] = 0;
  }
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size(), rounds = (size_t)refine + 1;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // the table: the jobs, then every job's triples; the words: best per job | current plane per job (4 words each) | the
  // records, round by round; the tail: counters (zeroed by the one fill) | candidate planes
  const size_t jobs_bytes = pad256(n_jobs * sizeof(PlaneJob)), triples_bytes = cand_total * 12;
  const size_t counts_bytes = pad256(cand_total * 4);
  std::vector<char> table(jobs_bytes + triples_bytes);
  BatchScratch scratch;
  A3D_TRY(batch_scratch(ctx, table.size(), n_jobs * (1 + PL_PLANE / 2 + rounds * PL_RECORD), 0,
                        counts_bytes + pad256(cand_total * PL_PLANE * 4), &scratch));
  uint32_t* d_counts = (uint32_t*)scratch.tail;
  float* d_cand = (float*)(scratch.tail + counts_bytes);
  const uint32_t* d_triples = (const uint32_t*)((const char*)scratch.jobs + jobs_bytes);
  for (size_t q = 0; q < n_jobs; ++q) {
    PlaneJob& j = jobs[q];
    const size_t at = cand_at[q];
    if (j.n_cand) memcpy(table.data() + jobs_bytes + at * 12, triples[cloud_of_job[q]], (size_t)j.n_cand * 12);
    j.triples = d_triples + 3 * at, j.counts = d_counts + at, j.cand = d_cand + PL_PLANE * at;
  }
  memcpy(table.data(), jobs.data(), n_jobs * sizeof(PlaneJob));
  const PlaneJob* d_jobs = (const PlaneJob*)scratch.jobs;
  unsigned long long* d_best = scratch.words;
  float* d_planes = (float*)(d_best + n_jobs);
  unsigned long long* d_records = d_best + n_jobs * (1 + PL_PLANE / 2);
  hipStream_t st = ctx->stream;
  A3D_TRY(batch_upload(scratch, table.data(), st));
  const uint32_t nj = (uint32_t)n_jobs;
  const dim3 block(PL_THREADS);
  if (cand_total) {
    A3D_HIP_TRY(hipMemsetAsync(d_counts, 0, cand_total * 4, st));
    const uint32_t per = (cand_max + PL_THREADS - 1) / PL_THREADS;
    hipLaunchKernelGGL(plane_candidates_kernel, dim3(nj * per), block, 0, st, d_jobs, per);
    A3D_HIP_TRY(hipGetLastError());
    // Few tiles (one frame is 264) leave most of the chip idle: the candidates are split over blocks as well, which costs
    // no atomics (a block flushes only its own range of counters) and a reload of the tile's rows per split.
    uint32_t rows = 4, split = 1;
    while (split < 8 && tiles * split < 2048 && cand_max / (2 * split) >= 64) split *= 2;
    bool lds = true;
#ifdef A3D_DIAGNOSTICS  // the forms that lose (scripts/cloud_plane_probe.py)
    if (const char* e = getenv("A3D_PLANE_ROWS")) rows = (uint32_t)atoi(e);
    if (const char* e = getenv("A3D_PLANE_SPLIT")) split = std::min(64u, std::max(1u, (uint32_t)atoi(e)));
    if (const char* e = getenv("A3D_PLANE_COUNTERS")) lds = strcmp(e, "global") != 0;
#endif
    const dim3 score_grid((uint32_t)tiles, split);
#define PL_SCORE(ROWS, LDS) hipLaunchKernelGGL((plane_score_kernel<ROWS, LDS>), score_grid, block, 0, st, d_jobs, nj, t)
    if (!lds) PL_SCORE(4, false);
    else if (rows == 1) PL_SCORE(1, true);
    else if (rows == 2) PL_SCORE(2, true);
    else if (rows == 8) PL_SCORE(8, true);
    else PL_SCORE(4, true);
#undef PL_SCORE
    A3D_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(plane_best_kernel, dim3(nj), block, 0, st, d_jobs, d_best, d_planes);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> head(n_jobs * (1 + PL_PLANE / 2)), records(n_jobs * PL_RECORD);
  std::vector<float> next(n_jobs * PL_PLANE);  // the planes of a round: read from the device at first, uploaded afterwards
  std::vector<double> planes(4 * n_jobs);
  for (size_t r = 0; r < rounds; ++r) {
    unsigned long long* d_round = d_records + r * n_jobs * PL_RECORD;
    hipLaunchKernelGGL(plane_flag_kernel, dim3((uint32_t)tiles), block, 0, st, d_jobs, nj, t, s, (const float*)d_planes,
                       d_round);
    A3D_HIP_TRY(hipGetLastError());
    if (r == 0) A3D_HIP_TRY(hipMemcpyAsync(head.data(), d_best, head.size() * 8, hipMemcpyDeviceToHost, st));
    A3D_HIP_TRY(hipMemcpyAsync(records.data(), d_round, records.size() * 8, hipMemcpyDeviceToHost, st));
    // host-synchronous: the caller may free inputs and outputs right after
    A3D_HIP_TRY(hipStreamSynchronize(st));
    if (r == 0) memcpy(next.data(), head.data() + n_jobs, next.size() * 4);
    for (size_t q = 0; q < n_jobs; ++q) {
      float* cur = next.data() + PL_PLANE * q;
      uint32_t has_plane;
      memcpy(&has_plane, cur + 6, 4);
      if (!has_plane) continue;
      const uint64_t* rec = (const uint64_t*)records.data() + PL_RECORD * q;
      double centroid[3];
      plane_from_moments(rec + 1, cur + 3, t, cur, planes.data() + 4 * q, centroid);
      for (int k = 0; k < 3; ++k) cur[k] = (float)planes[4 * q + k], cur[3 + k] = (float)centroid[k];
    }
    if (r + 1 < rounds) A3D_HIP_TRY(hipMemcpyAsync(d_planes, next.data(), next.size() * 4, hipMemcpyHostToDevice, st));
  }
  for (size_t q = 0; q < n_jobs; ++q) {
    const uint64_t i = cloud_of_job[q];
    if (head[q] == 0xFFFFFFFFull) continue;  // no plane: the zeros written above
    for (int k = 0; k < 4; ++k) out_planes[4 * i + k] = planes[4 * q + k];
    if (out_best) out_best[i] = head[q];
    if (out_inliers) out_inliers[i] = records[PL_RECORD * q];
    if (out_refit_rows) out_refit_rows[i] = records[PL_RECORD * q + 1];
  }
  return A3D_OK;
}

a3d_status a3d_plane_hypotheses(uint64_t seed, uint64_t len, uint64_t H, uint32_t* out_triples) {
  if (H == 0) return A3D_OK;
  A3D_REQUIRE(out_triples, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(len > 0 && len < (1ull << 32), A3D_INVALID_PARAMETER,
              "a3d_plane_hypotheses: candidates need a cloud of at least one row and fewer than 2^32");
  A3D_REQUIRE(H <= PL_MAX_CAND, A3D_INVALID_PARAMETER, "a3d_plane_hypotheses: at most 4096 candidates");
  for (uint64_t w = 0; w < 3 * H; ++w) {
    uint64_t z = seed + (w + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27, z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    out_triples[w] = (uint32_t)(((z >> 32) * len) >> 32);
  }
  return A3D_OK;
}

a3d_status a3d_plane_from_moments(const uint64_t moments[16], const float point[3], float t, const float fallback_normal[3],
                                  double out_plane[4], uint32_t* out_valid) {
  A3D_REQUIRE(moments && point && fallback_normal && out_plane, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(std::isfinite(t) && t > 0.f && std::isfinite(64.0f / t), A3D_INVALID_PARAMETER,
              "a3d_plane_from_moments: the distance threshold must be finite and positive");
  A3D_REQUIRE(moments_in_range(moments), A3D_INVALID_PARAMETER, "a3d_plane_from_moments: moments that no call can have produced");
  double centroid[3];
  const bool valid = plane_from_moments(moments, point, t, fallback_normal, out_plane, centroid);
  if (out_valid) *out_valid = valid ? 1u : 0u;
  return A3D_OK;
}

}  // extern "C"
