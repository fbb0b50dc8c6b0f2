// What the TSDF translation units share (tsdf.hip: integrate, raycast; tsdf_surface.hip: surface extraction; tsdf_icp.hip:
// the per-point field query and the point-to-SDF ICP): the volume handle, the grid the kernels take by value, and the
// raycast rule's trilinear sample and clamped rounding, which the surface rule uses unchanged for its normals and colours
// and the field query for its distance and direction.
#pragma once
#include "cloud_batch.hpp"
#include "solo_icp.hpp"

struct a3d_tsdf_volume {
  a3d_context* ctx = nullptr;
  uint32_t nx = 0, ny = 0, nz = 0, max_weight = 0;
  float v = 0.f, tau = 0.f, ox = 0.f, oy = 0.f, oz = 0.f;
  bool with_colors = false;
  void* block = nullptr;  // records | colours, one block of the context's
  size_t block_bytes = 0, used_bytes = 0;
  float2* records = nullptr;   // [nz][ny][nx] {D, W}
  uint32_t* colors = nullptr;  // [nz][ny][nx] r | g << 8 | b << 16, or null
  // the working state of the point-to-SDF ICP (tsdf_icp.hip): taken by the first align or accumulate and released with
  // the volume (solo_icp_release)
  a3d::SoloIcp icp;
};

namespace a3d {

constexpr uint64_t TS_MAX_WEIGHT = 1ull << 24;  // integers up to here are exact in f32

struct TsdfGrid {
  float2* records;
  uint32_t* colors;
  uint32_t nx, ny, nz, total;
  float v, tau, ox, oy, oz, max_weight;
};

inline TsdfGrid grid_of(const a3d_tsdf_volume* vol) {
  TsdfGrid g{};
  g.records = vol->records, g.colors = vol->colors;
  g.nx = vol->nx, g.ny = vol->ny, g.nz = vol->nz, g.total = vol->nx * vol->ny * vol->nz;
  g.v = vol->v, g.tau = vol->tau, g.ox = vol->ox, g.oy = vol->oy, g.oz = vol->oz, g.max_weight = (float)vol->max_weight;
  return g;
}

#ifdef __HIPCC__
__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// Step 3 of the raycast rule.  Every index it loads from is inside the volume: 0 <= i0 and i0 + 1 <= nx - 1 on each axis.
__device__ __forceinline__ bool tri(const TsdfGrid& g, V3 p, float* out) {
  const float fx0 = floorf(p.x), fy0 = floorf(p.y), fz0 = floorf(p.z);
  if (!(fx0 >= 0.0f && fx0 + 1.0f <= (float)(g.nx - 1) && fy0 >= 0.0f && fy0 + 1.0f <= (float)(g.ny - 1) && fz0 >= 0.0f &&
        fz0 + 1.0f <= (float)(g.nz - 1)))
    return false;  // (NaN and the infinities fail)
  const size_t sx = 1, sy = g.nx, sz = (size_t)g.nx * g.ny;
  const float2* c = g.records + ((size_t)(uint32_t)fz0 * sz + (size_t)(uint32_t)fy0 * sy + (uint32_t)fx0);
  const float2 c000 = c[0], c100 = c[sx], c010 = c[sy], c110 = c[sy + sx];
  const float2 c001 = c[sz], c101 = c[sz + sx], c011 = c[sz + sy], c111 = c[sz + sy + sx];
  if (!(c000.y > 0.0f && c100.y > 0.0f && c010.y > 0.0f && c110.y > 0.0f && c001.y > 0.0f && c101.y > 0.0f &&
        c011.y > 0.0f && c111.y > 0.0f))
    return false;
  const float tx = p.x - fx0, ty = p.y - fy0, tz = p.z - fz0;
  const float c00 = lerp(c000.x, c100.x, tx), c10 = lerp(c010.x, c110.x, tx);
  const float c01 = lerp(c001.x, c101.x, tx), c11 = lerp(c011.x, c111.x, tx);
  *out = lerp(lerp(c00, c10, ty), lerp(c01, c11, ty), tz);
  return true;
}

__device__ __forceinline__ uint32_t clamped_voxel(float coordinate, uint32_t n) {
  return (uint32_t)fminf(fmaxf(roundf(coordinate), 0.0f), (float)(n - 1));
}
#endif  // __HIPCC__

}  // namespace a3d
