// The surface of a TSDF volume as vertices on crossing edges and, in the mesh form, marching-tetrahedra triangles on the
// Kuhn split of every cell.  The rule is stated in align3d_hip.h (a3d_tsdf_volume_extract_surface); all of it is f32,
// every operation rounded on its own.  Nothing is summed or appended across threads: a vertex's index is its rank in
// (voxel number, class) order, a triangle's its rank in (cell, tetrahedron, triangle) order, both from prefix sums, so the
// result depends neither on launch geometry nor on scheduling, on what scratch held or on how often the call runs.
//
// Scratch (region 3 of the context; the call is host-synchronous): per voxel ONE mask byte (bit c - 1: the owned edge of
// class c crosses; bit 7: the cell gives triangles) and two u16, the voxel's first vertex and first triangle counted from
// its block's: 5 bytes a voxel; per block of 256 voxels its packed counts and its two 32-bit bases; two 64-bit totals.  The
// u16 are stored only where the mask has their bits, and read only there.
//
//  * surface_count_kernel: one thread per voxel reads its record and the up to seven records at +1 offsets (the cell's
//    corners: the same eight serve the edges and the cell), and the block scans its packed counts.
//  * surface_scan_kernel: ONE block walks the block counts in tiles of 4096 with a running base: the launch count does not
//    depend on the volume's size.
//  The host reads the two totals here; a count-only call, or one whose capacities are short, ends without another launch.
//  * surface_vertices_kernel / surface_faces_kernel: one thread per voxel again; a thread whose mask byte has none of its
//    bits leaves after that one byte, so all but the surface's waves cost one coalesced 64-byte read.
#include <cmath>
#include <vector>

#include "tsdf.hpp"

using namespace a3d;

namespace {

constexpr uint32_t SF_THREADS = 256, SF_WAVES = SF_THREADS / 64;
constexpr uint32_t SF_SCAN_THREADS = 1024, SF_SCAN_WAVES = SF_SCAN_THREADS / 64;
constexpr uint32_t SF_SCAN_ITEMS = 4, SF_SCAN_TILE = SF_SCAN_THREADS * SF_SCAN_ITEMS;  // 4096 blocks, 2^20 voxels, a tile
constexpr uint32_t SF_MESH_CLASSES = 0x7F, SF_CLOUD_CLASSES = 0x0B;  // bit c - 1 per class; the cloud keeps 1, 2 and 4
constexpr uint32_t SF_CELL_BIT = 0x80;
constexpr uint64_t SF_MAX_COUNT = 0xFFFFFFFFull;  // counts of 2^32 - 1 or more are refused
// Local vertices 1 and 2 of tetrahedron t (permutations xyz, xzy, yxz, yzx, zxy, zyx) as corner numbers x | y << 1 | z << 2,
// one nibble per t; vertex 0 is corner 0 and vertex 3 corner 7.
constexpr uint32_t SF_TET_V1 = 0x442211u, SF_TET_V2 = 0x656353u;

// Rule 5's table, derived by tests/tsdf_surface_restatement.py from the rule's paragraph (test_tsdf_surface_cpu.py derives
// it again and compares).  TS_TET_TABLE[t][s], bit n of s = local vertex n is inside: the triangle count in bits 0-1, then
// corner c of triangle m in the 6 bits from 2 + 18 m + 6 c: the owner's corner number low, the edge class high.
__device__ const uint64_t TS_TET_TABLE[6][16] = {
    {0x0000000000ull, 0x00000E1821ull, 0x0000047121ull, 0x11C58C7862ull, 0x000008D161ull, 0x23448E2322ull, 0x188C88F122ull, 0x000008F1E1ull, 0x00000C63E1ull, 0x318C88D822ull, 0x23E0846322ull, 0x0000046361ull, 0x38C58C5162ull, 0x00000C5121ull, 0x0000063821ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000A3821ull, 0x00000C6121ull, 0x31868E31A2ull, 0x00000855A1ull, 0x2154857822ull, 0x15A08C5522ull, 0x00000C55E1ull, 0x00000571E1ull, 0x15C48A1522ull, 0x3854856122ull, 0x00000561A1ull, 0x31E28871A2ull, 0x0000087121ull, 0x00000E2821ull, 0x0000000000ull},
    {0x0000000000ull, 0x0000063841ull, 0x00000A8A41ull, 0x2A298E2A62ull, 0x000002A361ull, 0x0A8D08F842ull, 0x23610AA342ull, 0x00000AA3E1ull, 0x000008EAE1ull, 0x23A9062342ull, 0x388D08CA42ull, 0x000008CA61ull, 0x2AE182AA62ull, 0x000002AA41ull, 0x00000E1841ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000E3041ull, 0x000008AA41ull, 0x22AB0AB8C2ull, 0x000003A2C1ull, 0x0E890E0E42ull, 0x303903AA42ull, 0x000003AAE1ull, 0x00000A8EE1ull, 0x2A3903B042ull, 0x0EE1088E42ull, 0x0000088EC1ull, 0x38AB0AA2C2ull, 0x00000AA241ull, 0x00000C3841ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000E2881ull, 0x0000031C81ull, 0x0C728738A2ull, 0x0000054CA1ull, 0x15320E1582ull, 0x2856055C82ull, 0x0000055CE1ull, 0x00000715E1ull, 0x1C56056882ull, 0x15E2031582ull, 0x00000315A1ull, 0x3872870CA2ull, 0x0000070C81ull, 0x00000A3881ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000C3881ull, 0x0000071481ull, 0x1C530E1CC2ull, 0x0000050EC1ull, 0x143A03B882ull, 0x0EC2070E82ull, 0x0000070EE1ull, 0x0000039CE1ull, 0x0E720C0E82ull, 0x383A039482ull, 0x00000394C1ull, 0x1CE3051CC2ull, 0x0000051C81ull, 0x00000E3081ull, 0x0000000000ull},
};

struct SurfScratch {
  uint8_t* mask;           // [total]
  uint16_t* vlocal;        // [total]
  uint16_t* flocal;        // [total]
  uint32_t* block_counts;  // [blocks] vertices | triangles << 16
  uint32_t* vbase;         // [blocks]
  uint32_t* fbase;         // [blocks]
  unsigned long long* totals;  // vertices, triangles
};

// The pattern of tetrahedron t: bit n = local vertex n is inside, from the cell's eight corner bits.
__device__ __forceinline__ uint32_t tet_pattern(uint32_t inside, uint32_t t) {
  const uint32_t v1 = (SF_TET_V1 >> (4 * t)) & 7u, v2 = (SF_TET_V2 >> (4 * t)) & 7u;
  return (inside & 1u) | ((inside >> v1) & 1u) << 1 | ((inside >> v2) & 1u) << 2 | ((inside >> 7) & 1u) << 3;
}

// Rules 1, 2 and the counts of rule 5.  `FACES`: the mesh form (seven classes, triangles); else classes 1, 2 and 4.
template <bool FACES>
__global__ void __launch_bounds__(SF_THREADS) surface_count_kernel(const TsdfGrid g, float min_weight, SurfScratch s) {
  __shared__ uint32_t wave_sums[SF_WAVES];
  const uint32_t idx = blockIdx.x * SF_THREADS + threadIdx.x;  // (total <= 2^30: no wrap)
  uint32_t mask = 0, triangles = 0;
  if (idx < g.total) {
    const uint32_t i = idx % g.nx, line = idx / g.nx, j = line % g.ny, k = line / g.ny;
    const bool px = i + 1 < g.nx, py = j + 1 < g.ny, pz = k + 1 < g.nz;
    const size_t sy = g.nx, sz = (size_t)g.nx * g.ny;
    uint32_t valid = 0, inside = 0;  // bit c: corner a + e_c (a corner outside the volume has neither)
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
      if (((c & 1u) && !px) || ((c & 2u) && !py) || ((c & 4u) && !pz)) continue;
      const float2 r = g.records[(size_t)idx + (c & 1u) + (c >> 1 & 1u) * sy + (c >> 2 & 1u) * sz];  // (inside the volume)
      const bool ok = r.y >= min_weight && fabsf(r.x) < INFINITY;  // (a NaN fails both)
      valid |= (uint32_t)ok << c;
      inside |= (uint32_t)(ok && r.x <= 0.0f) << c;  // (-0 is inside)
    }
    if (valid & 1u) {
      const uint32_t other_side = (inside & 1u) ? ~inside : inside;
      mask = ((valid & other_side) >> 1) & (FACES ? SF_MESH_CLASSES : SF_CLOUD_CLASSES);
    }
    if (FACES && valid == 0xFFu) {  // (all eight corners exist and are valid: a cell)
#pragma unroll
      for (uint32_t t = 0; t < 6; ++t) {
        const uint32_t n = __popc(tet_pattern(inside, t));
        triangles += min(n, 4u - n);  // 0, 1, 2, 1, 0: the table's counts
      }
      if (triangles) mask |= SF_CELL_BIT;
    }
  }
  const uint32_t mine = (uint32_t)__popc(mask & SF_MESH_CLASSES) | triangles << 16;  // (a block's sums stay below 2^16 each)
  uint32_t incl = mine;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= (uint32_t)o) incl += up;
  }
  if (lane == 63u) wave_sums[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < SF_WAVES; ++w) {
    if (w < wave) before += wave_sums[w];
    all += wave_sums[w];
  }
  const uint32_t excl = before + incl - mine;
  if (idx < g.total) {
    s.mask[idx] = (uint8_t)mask;
    if (mask & SF_MESH_CLASSES) s.vlocal[idx] = (uint16_t)(excl & 0xFFFFu);
    if (mask & SF_CELL_BIT) s.flocal[idx] = (uint16_t)(excl >> 16);
  }
  if (threadIdx.x == 0) s.block_counts[blockIdx.x] = all;
}

// Exclusive sums of the block counts, by one block: tiles of SF_SCAN_TILE counts (SF_SCAN_ITEMS consecutive ones per
// thread) with a running 64-bit base.  The 32-bit bases may wrap when a total does not fit: the host refuses such a call
// before anything reads them.
__global__ void __launch_bounds__(SF_SCAN_THREADS) surface_scan_kernel(SurfScratch s, uint32_t blocks) {
  __shared__ unsigned long long wave_sums[SF_SCAN_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long base_v = 0, base_f = 0;
  for (uint32_t first = 0; first < blocks; first += SF_SCAN_TILE) {  // (uniform over the block)
    const uint32_t b0 = first + threadIdx.x * SF_SCAN_ITEMS;
    uint32_t packed[SF_SCAN_ITEMS];
    unsigned long long mine = 0;  // vertices low, triangles high (a tile's sums stay below 2^32 each)
#pragma unroll
    for (uint32_t k = 0; k < SF_SCAN_ITEMS; ++k) {
      packed[k] = b0 + k < blocks ? s.block_counts[b0 + k] : 0u;
      mine += (unsigned long long)(packed[k] & 0xFFFFu) | (unsigned long long)(packed[k] >> 16) << 32;
    }
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63u) wave_sums[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SF_SCAN_WAVES; ++w) {
      if (w < wave) before += wave_sums[w];
      all += wave_sums[w];
    }
    unsigned long long excl = before + incl - mine;
#pragma unroll
    for (uint32_t k = 0; k < SF_SCAN_ITEMS; ++k) {
      if (b0 + k < blocks) {
        s.vbase[b0 + k] = (uint32_t)(base_v + (excl & 0xFFFFFFFFull));
        s.fbase[b0 + k] = (uint32_t)(base_f + (excl >> 32));
      }
      excl += (unsigned long long)(packed[k] & 0xFFFFu) | (unsigned long long)(packed[k] >> 16) << 32;
    }
    base_v += all & 0xFFFFFFFFull, base_f += all >> 32;
    __syncthreads();  // (the sums are read before the next tile's are stored)
  }
  if (threadIdx.x == 0) s.totals[0] = base_v, s.totals[1] = base_f;
}

// Rule 3 for every crossing edge the voxel owns, in class order from the voxel's first vertex.
__global__ void __launch_bounds__(SF_THREADS)
    surface_vertices_kernel(const TsdfGrid g, const SurfScratch s, float* __restrict__ out_points,
                            float* __restrict__ out_normals, uint8_t* __restrict__ out_colors, unsigned long long capacity) {
  const uint32_t idx = blockIdx.x * SF_THREADS + threadIdx.x;
  if (idx >= g.total) return;
  const uint32_t mask = s.mask[idx] & SF_MESH_CLASSES;
  if (!mask) return;
  const uint32_t i = idx % g.nx, line = idx / g.nx, j = line % g.ny, k = line / g.ny;
  const size_t sy = g.nx, sz = (size_t)g.nx * g.ny;
  unsigned long long dst = (unsigned long long)s.vbase[blockIdx.x] + s.vlocal[idx];
  const float Da = g.records[idx].x;
  for (uint32_t c = 1; c < 8; ++c) {
    if (!((mask >> (c - 1)) & 1u)) continue;
    const uint32_t ex = c & 1u, ey = c >> 1 & 1u, ez = c >> 2 & 1u;
    const float Db = g.records[(size_t)idx + ex + ey * sy + ez * sz].x;  // (the edge crosses: b is in the volume)
    const float t = Da / (Da - Db);
    const V3 gs{(float)i + t * (float)ex, (float)j + t * (float)ey, (float)k + t * (float)ez};
    const f32x3 p{g.ox + gs.x * g.v, g.oy + gs.y * g.v, g.oz + gs.z * g.v};
    f32x3 n{0.f, 0.f, 0.f};
    if (out_normals) {  // step 6 of the raycast rule at g*, no pose
      float xp, xm, yp, ym, zp, zm;
      // (bitwise on purpose: all six samples are taken, as the rule states them)
      const bool all = tri(g, V3{gs.x + 1.0f, gs.y, gs.z}, &xp) & tri(g, V3{gs.x - 1.0f, gs.y, gs.z}, &xm) &
                       tri(g, V3{gs.x, gs.y + 1.0f, gs.z}, &yp) & tri(g, V3{gs.x, gs.y - 1.0f, gs.z}, &ym) &
                       tri(g, V3{gs.x, gs.y, gs.z + 1.0f}, &zp) & tri(g, V3{gs.x, gs.y, gs.z - 1.0f}, &zm);
      if (all) {
        const V3 G{xp - xm, yp - ym, zp - zm};
        const float len = sqrtf(G.x * G.x + G.y * G.y + G.z * G.z);
        if (len > 0.0f && len < INFINITY) {
          const V3 u = G / len;
          n = f32x3{u.x, u.y, u.z};
        }
      }
    }
    if (dst < capacity) {  // (always: the host launches only when the total fits; a bound on every store)
      *(f32x3_u*)(out_points + 3 * dst) = p;
      if (out_normals) *(f32x3_u*)(out_normals + 3 * dst) = n;
      if (out_colors)
        store_color(out_colors, dst,
                    g.colors[((size_t)clamped_voxel(gs.z, g.nz) * g.ny + clamped_voxel(gs.y, g.ny)) * g.nx + clamped_voxel(gs.x, g.nx)]);
    }
    ++dst;
  }
}

// Rule 5 for every cell that gives triangles, in (tetrahedron, triangle) order from the cell's first triangle.
__global__ void __launch_bounds__(SF_THREADS)
    surface_faces_kernel(const TsdfGrid g, const SurfScratch s, uint32_t* __restrict__ out_faces, unsigned long long capacity) {
  const uint32_t idx = blockIdx.x * SF_THREADS + threadIdx.x;
  if (idx >= g.total) return;
  if (!(s.mask[idx] & SF_CELL_BIT)) return;
  const size_t sy = g.nx, sz = (size_t)g.nx * g.ny;
  uint32_t inside = 0;  // (the bit says all eight corners exist and are valid)
#pragma unroll
  for (uint32_t c = 0; c < 8; ++c)
    inside |= (uint32_t)(g.records[(size_t)idx + (c & 1u) + (c >> 1 & 1u) * sy + (c >> 2 & 1u) * sz].x <= 0.0f) << c;
  unsigned long long dst = (unsigned long long)s.fbase[blockIdx.x] + s.flocal[idx];
  for (uint32_t t = 0; t < 6; ++t) {
    const uint64_t word = TS_TET_TABLE[t][tet_pattern(inside, t)];
    const uint32_t count = (uint32_t)(word & 3u);
    for (uint32_t m = 0; m < count; ++m) {
      uint32_t corner[3];
#pragma unroll
      for (uint32_t c = 0; c < 3; ++c) {
        const uint32_t code = (uint32_t)(word >> (2 + 18 * m + 6 * c)) & 63u, cls = code >> 3;
        // the edge's owner: a corner of this cell, so inside the volume; the edge crosses, so the owner's mask has its bit
        // and its first vertex was stored
        const size_t owner = (size_t)idx + (code & 1u) + (code >> 1 & 1u) * sy + (code >> 2 & 1u) * sz;
        corner[c] = s.vbase[owner / SF_THREADS] + s.vlocal[owner] + (uint32_t)__popc(s.mask[owner] & ((1u << (cls - 1)) - 1u));
      }
      if (dst < capacity) {  // (always, as above)
        uint32_t* f = out_faces + 3 * dst;
        f[0] = corner[0], f[1] = corner[1], f[2] = corner[2];
      }
      ++dst;
    }
  }
}

}  // namespace

extern "C" {

a3d_status a3d_tsdf_volume_extract_surface(a3d_tsdf_volume* volume, uint64_t min_weight, int want_faces, float* d_out_points,
                                           float* d_out_normals, uint8_t* d_out_colors, uint64_t vertex_capacity,
                                           uint32_t* d_out_faces, uint64_t face_capacity, uint64_t* out_vertices,
                                           uint64_t* out_faces) {
  A3D_REQUIRE(volume && out_vertices && out_faces, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(min_weight >= 1 && min_weight <= TS_MAX_WEIGHT, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_extract_surface: min_weight lies in [1, 2^24]");
  const bool faces = want_faces != 0;
  if (!faces) d_out_faces = nullptr, face_capacity = 0;  // (ignored in the point-cloud form)
  A3D_REQUIRE(d_out_points || (vertex_capacity == 0 && !d_out_normals && !d_out_colors), A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_extract_surface: without d_out_points the vertex capacity is 0 and no other vertex output is given");
  A3D_REQUIRE(d_out_faces || face_capacity == 0, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_extract_surface: without d_out_faces the face capacity is 0");
  A3D_REQUIRE(!d_out_colors || volume->with_colors, A3D_MISSING_FIELD, "a3d_tsdf_volume_extract_surface: the volume has no colours");
  const bool count_only = !d_out_points && !d_out_faces;
  {
    // what the call may write: the first min(capacity, 2^32 - 2) elements of each output
    const uint64_t vcap = std::min<uint64_t>(vertex_capacity, SF_MAX_COUNT - 1);
    const uint64_t fcap = std::min<uint64_t>(face_capacity, SF_MAX_COUNT - 1);
    RangeRecorder ranges;
    ranges.in(volume->block, volume->used_bytes);
    ranges.out(d_out_points, vcap * 12), ranges.out(d_out_normals, vcap * 12), ranges.out(d_out_colors, vcap * 3);
    ranges.out(d_out_faces, fcap * 12);
    A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
                "a3d_tsdf_volume_extract_surface: an output overlaps the volume or another output");
  }
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  const TsdfGrid g = grid_of(volume);
  const size_t total = g.total;
  const uint32_t blocks = (uint32_t)((total + SF_THREADS - 1) / SF_THREADS);
  const size_t mask_bytes = pad256(total), local_bytes = pad256(total * 2), block_bytes = pad256((size_t)blocks * 4);
  void* region = nullptr;  // scratch region 3: mask | vlocal | flocal | block counts | vertex bases | face bases | totals
  A3D_TRY(ctx_scratch(ctx, 3, mask_bytes + 2 * local_bytes + 3 * block_bytes + 256, &region));
  char* base = (char*)region;
  SurfScratch s{};
  s.mask = (uint8_t*)base;
  s.vlocal = (uint16_t*)(base + mask_bytes);
  s.flocal = (uint16_t*)(base + mask_bytes + local_bytes);
  s.block_counts = (uint32_t*)(base + mask_bytes + 2 * local_bytes);
  s.vbase = (uint32_t*)(base + mask_bytes + 2 * local_bytes + block_bytes);
  s.fbase = (uint32_t*)(base + mask_bytes + 2 * local_bytes + 2 * block_bytes);
  s.totals = (unsigned long long*)(base + mask_bytes + 2 * local_bytes + 3 * block_bytes);
  hipStream_t st = ctx->stream;
  const dim3 grid(blocks), block(SF_THREADS);
  if (faces)
    hipLaunchKernelGGL(surface_count_kernel<true>, grid, block, 0, st, g, (float)min_weight, s);
  else
    hipLaunchKernelGGL(surface_count_kernel<false>, grid, block, 0, st, g, (float)min_weight, s);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(surface_scan_kernel, dim3(1), dim3(SF_SCAN_THREADS), 0, st, s, blocks);
  A3D_HIP_TRY(hipGetLastError());
  unsigned long long totals[2] = {0, 0};
  A3D_HIP_TRY(hipMemcpyAsync(totals, s.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
  A3D_HIP_TRY(hipStreamSynchronize(st));
  *out_vertices = totals[0], *out_faces = totals[1];
  A3D_REQUIRE(totals[0] < SF_MAX_COUNT && totals[1] < SF_MAX_COUNT, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_extract_surface: 2^32 - 1 vertices or triangles, or more (nothing was written)");
  if (count_only) return A3D_OK;
  A3D_REQUIRE(totals[0] <= vertex_capacity && totals[1] <= face_capacity, A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_extract_surface: a capacity is smaller than its count (nothing was written)");
  if (totals[0] && d_out_points) {
    hipLaunchKernelGGL(surface_vertices_kernel, grid, block, 0, st, g, s, d_out_points, d_out_normals, d_out_colors,
                       (unsigned long long)vertex_capacity);
    A3D_HIP_TRY(hipGetLastError());
  }
  if (totals[1] && d_out_faces) {
    hipLaunchKernelGGL(surface_faces_kernel, grid, block, 0, st, g, s, d_out_faces, (unsigned long long)face_capacity);
    A3D_HIP_TRY(hipGetLastError());
  }
  // host-synchronous: the outputs are complete on return
  A3D_HIP_TRY(hipStreamSynchronize(st));
  return A3D_OK;
}

}  // extern "C"
