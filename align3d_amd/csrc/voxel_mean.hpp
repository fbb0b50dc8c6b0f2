// The arithmetic of the cell-mean rule (steps 2 to 5 of the header comment of voxel_mean.hip) and the wave's run
// combining, shared by the batch call (voxel_mean.hip) and the persistent map in mean mode (voxel_map.hip): one
// definition, so that a map of means gives the bits of the batch call.  Every f32 and f64 operation is rounded on its own
// (-ffp-contract=off), so where a function is inlined changes nothing.
#pragma once
#include "voxel_grid.hpp"

namespace a3d {

struct MeanParams {  // host constants in f32 (voxel_mean_params)
  float s, u;        // 32768 / v and v / 32768
};
inline MeanParams voxel_mean_params(float v) { return MeanParams{32768.0f / v, v / 32768.0f}; }

#ifdef __HIPCC__
// A run is a maximal stretch of lanes of one wave with the same key.  first: this lane starts one.
__device__ __forceinline__ uint64_t run_heads(unsigned long long key, uint32_t lane, bool* first) {
  const unsigned long long prev = __shfl_up(key, 1, 64);
  *first = lane == 0 || prev != key;
  return __builtin_amdgcn_ballot_w64(*first);
}
__device__ __forceinline__ uint32_t run_first_lane(uint64_t heads, uint32_t lane) {  // (lane 0 always starts a run)
  return 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
}
__device__ __forceinline__ uint32_t run_end_lane(uint64_t heads, uint32_t lane) {  // one past the run's last lane
  const uint64_t above = lane == 63u ? 0ull : heads >> (lane + 1u);
  return above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u;
}

// The sums of a cell, or of the part of one that a wave holds.
struct VmSums {
  uint32_t n;
  long long s[3];
  int t[3];  // (a wave's 64 rows of |r| <= 2^21 fit; what is kept beyond a wave is 64-bit)
  uint32_t c[3];
};

// Step 2: the lattice offsets of a kept point, ctr and d exactly as voxel_key computes them.
__device__ __forceinline__ void vmean_offsets(const f32x3 pt, const VoxelGrid grid, float s, long long* q) {
  const float cx = floorf((pt.x - grid.ox) / grid.v), cy = floorf((pt.y - grid.oy) / grid.v),
              cz = floorf((pt.z - grid.oz) / grid.v);
  const float dx = pt.x - ((cx + 0.5f) * grid.v + grid.ox), dy = pt.y - ((cy + 0.5f) * grid.v + grid.oy),
              dz = pt.z - ((cz + 0.5f) * grid.v + grid.oz);
  q[0] = (int)rintf(dx * s), q[1] = (int)rintf(dy * s), q[2] = (int)rintf(dz * s);
}

// Step 4, per row: the rounded normal, left as it is (zeros) for a row that is not counted.
__device__ __forceinline__ void vmean_round_normal(const f32x3 nr, int* t) {
  // (a NaN fails every comparison)
  if (fabsf(nr.x) <= 2.f && fabsf(nr.y) <= 2.f && fabsf(nr.z) <= 2.f)
    t[0] = (int)rintf(nr.x * 1048576.0f), t[1] = (int)rintf(nr.y * 1048576.0f), t[2] = (int)rintf(nr.z * 1048576.0f);
}

// The inclusive scan of a wave's sums inside every run: a run's last lane ends with the run's sums.  Every lane of the
// wave calls it.
__device__ __forceinline__ void vmean_scan_runs(VmSums& a, uint32_t lane, uint32_t first_lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t un = __shfl_up(a.n, o, 64);
    const long long us0 = __shfl_up(a.s[0], o, 64), us1 = __shfl_up(a.s[1], o, 64), us2 = __shfl_up(a.s[2], o, 64);
    const int ut0 = __shfl_up(a.t[0], o, 64), ut1 = __shfl_up(a.t[1], o, 64), ut2 = __shfl_up(a.t[2], o, 64);
    const uint32_t uc0 = __shfl_up(a.c[0], o, 64), uc1 = __shfl_up(a.c[1], o, 64), uc2 = __shfl_up(a.c[2], o, 64);
    if (lane >= first_lane + (uint32_t)o) {
      a.n += un;
      a.s[0] += us0, a.s[1] += us1, a.s[2] += us2;
      a.t[0] += ut0, a.t[1] += ut1, a.t[2] += ut2;
      a.c[0] += uc0, a.c[1] += uc1, a.c[2] += uc2;
    }
  }
}

// Step 3 for a cell of n > 1 rows whose cell numbers are (cx, cy, cz), integers held in f32 as floorf gives them.
__device__ __forceinline__ f32x3 vmean_point(float cx, float cy, float cz, const VoxelGrid grid, float u,
                                             unsigned long long n, const long long* s) {
  const double dn = (double)n;
  const float mx = (float)((double)s[0] / dn), my = (float)((double)s[1] / dn), mz = (float)((double)s[2] / dn);
  f32x3 out;
  out.x = ((cx + 0.5f) * grid.v + grid.ox) + mx * u;
  out.y = ((cy + 0.5f) * grid.v + grid.oy) + my * u;
  out.z = ((cz + 0.5f) * grid.v + grid.oz) + mz * u;
  return out;
}

// Step 4 for a cell of n > 1 rows.
__device__ __forceinline__ f32x3 vmean_normal(const long long* t) {
  const double tx = (double)t[0], ty = (double)t[1], tz = (double)t[2];
  const double l = sqrt((tx * tx + ty * ty) + tz * tz);
  f32x3 nrm = {0.f, 0.f, 0.f};
  if (l > 0.0) nrm.x = (float)(tx / l), nrm.y = (float)(ty / l), nrm.z = (float)(tz / l);
  return nrm;
}

// Step 5 for a cell of n > 1 rows: r | g << 8 | b << 16.
__device__ __forceinline__ uint32_t vmean_color(unsigned long long n, const unsigned long long* c) {
  const uint32_t r = (uint32_t)((2 * c[0] + n) / (2 * n)), g = (uint32_t)((2 * c[1] + n) / (2 * n)),
                 b = (uint32_t)((2 * c[2] + n) / (2 * n));
  return r | g << 8 | b << 16;
}
#endif  // __HIPCC__

}  // namespace a3d
