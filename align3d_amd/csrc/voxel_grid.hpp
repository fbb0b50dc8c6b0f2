// The per-point arithmetic of the voxel grid and the slot of its hash tables, shared by the batch downsample
// (voxel_downsample.hip) and the persistent map (voxel_map.hip): one definition, so the two cannot drift apart.
// Per point, all in f32, every operation rounded on its own (-ffp-contract=off, correctly rounded divide):
//   c_k   = floorf((p_k - o_k) / v)            dropped unless every c_k is finite and in [-2^20, 2^20)
//   key   = (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20)
//   ctr_k = (c_k + 0.5f) * v + o_k,  d_k = p_k - ctr_k,  dist = (d_x * d_x + d_y * d_y) + d_z * d_z   (never NaN, may be +inf)
// The host's checks of a grid's parameters and the size of a table are here too, once for every entry point.
#pragma once
#include <cmath>

#include "cloud_batch.hpp"

namespace a3d {

constexpr unsigned long long VX_EMPTY = ~0ull;  // no key has bit 63 set
constexpr float VX_CELL_LIMIT = 1048576.0f;     // 2^20

struct VoxelSlot {
  unsigned long long key;   // VX_EMPTY or the 63-bit cell key
  unsigned long long best;  // min over the key's points of bits(dist) << 32 | index
};
static_assert(sizeof(VoxelSlot) == 16, "VoxelSlot layout");

struct VoxelGrid {
  float v, ox, oy, oz;
};

// The grid of pitch `voxel_size` anchored at `origin` (null: the zero point), as the entry point `name` accepts it.
inline a3d_status voxel_grid_from(const char* name, float voxel_size, const float origin[3], VoxelGrid* grid) {
  if (!(std::isfinite(voxel_size) && voxel_size > 0.f))
    return refuse(A3D_INVALID_PARAMETER, name, "the voxel size must be finite and positive");
  *grid = VoxelGrid{voxel_size, 0.f, 0.f, 0.f};
  if (origin) {
    if (!(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
      return refuse(A3D_INVALID_PARAMETER, name, "the origin must be finite");
    grid->ox = origin[0], grid->oy = origin[1], grid->oz = origin[2];
  }
  return A3D_OK;
}

// The neighbour grid of pitch `radius` at the zero point, with r2 = radius^2 and s = 32768 / radius (the distance
// lattice; `s` may be null), as the entry point `name` accepts it.
inline a3d_status radius_grid_from(const char* name, float radius, VoxelGrid* grid, float* r2, float* s) {
  if (!(std::isfinite(radius) && radius > 0.f))
    return refuse(A3D_INVALID_PARAMETER, name, "the radius must be finite and positive");
  const float lattice = 32768.0f / radius;
  *r2 = radius * radius;
  if (!(*r2 > 0.f && std::isfinite(lattice)))
    return refuse(A3D_INVALID_PARAMETER, name, "a radius whose square is 0 in f32 (below about 1e-19)");
  if (s) *s = lattice;
  *grid = VoxelGrid{radius, 0.f, 0.f, 0.f};
  return A3D_OK;
}

// Slots of a hash table that holds up to `len` keys: the power of two that is at least 2 * len, and at least `least`.
inline uint64_t table_slots(uint64_t len, uint64_t least = 2) {
  uint64_t slots = least;
  while (slots < 2 * len) slots <<= 1;
  return slots;
}

#ifdef __HIPCC__
// The cell key of a point and (with_dist) its squared distance to the cell centre; false = the point is dropped.
__device__ __forceinline__ bool voxel_key(const f32x3 p, const VoxelGrid g, unsigned long long* key, float* dist) {
  const float cx = floorf((p.x - g.ox) / g.v), cy = floorf((p.y - g.oy) / g.v), cz = floorf((p.z - g.oz) / g.v);
  // (a NaN fails every comparison, an infinity the range)
  const bool ok = cx >= -VX_CELL_LIMIT && cx < VX_CELL_LIMIT && cy >= -VX_CELL_LIMIT && cy < VX_CELL_LIMIT &&
                  cz >= -VX_CELL_LIMIT && cz < VX_CELL_LIMIT;
  if (!ok) return false;
  const unsigned long long kx = (unsigned long long)((int)cx + (1 << 20)), ky = (unsigned long long)((int)cy + (1 << 20)),
                           kz = (unsigned long long)((int)cz + (1 << 20));
  *key = kx << 42 | ky << 21 | kz;
  if (dist) {
    const float dx = p.x - ((cx + 0.5f) * g.v + g.ox), dy = p.y - ((cy + 0.5f) * g.v + g.oy),
                dz = p.z - ((cz + 0.5f) * g.v + g.oz);
    *dist = (dx * dx + dy * dy) + dz * dz;
  }
  return true;
}

__device__ __forceinline__ unsigned long long slot_hash(unsigned long long k) {  // the 64-bit finaliser of MurmurHash3
  k ^= k >> 33, k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33, k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ k >> 33;
}

#define VX_LOAD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif  // __HIPCC__

}  // namespace a3d
