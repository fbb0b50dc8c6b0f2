// Reading the persistent voxel map (voxel_map.hip) as a spatial index: a3d_voxel_map_nearest_device and the
// frame-to-map point-to-plane ICP a3d_voxel_map_icp_align_device.  The table is only read here, with plain loads; every
// call is host-synchronous, so inserts and retains may follow.
//
// The association (include/align3d_hip.h states it; tests/voxel_map_icp_restatement.py restates it): a query q, after
// its pose, lies in cell c = floorf((q - o) / v) as voxel_key computes it; the candidates are the stored rows of the
// occupied cells c + d, d in {-1, 0, 1}^3, a neighbour whose coordinate leaves [-2^20, 2^20) on an axis being skipped
// before the key is packed; the winner minimises bits(d2) << 32 | seq with d = q - r, d2 = (dx dx + dy dy) + dz dz in
// f32.  A minimum over a set: slot order, table size and growth history play no part.
//
// A thread serves one query and walks its 27 cells alone, a plane of nine at a time: the keys of the nine home slots are
// loaded together, every probe then runs on to its key or to the first empty slot (the table is at most half full), the
// nine rows and sequence numbers are loaded together (lanes that found no cell all read slot 0: one address per wave),
// and the compares follow.  Six dependent rounds of loads per query where no chain is longer than a slot; the nine probes
// of a plane still run one after the other, so a fuller table costs rounds.  Slot indices are held
// in 32 bits and the winner's row is fetched again behind the walk: the ICP kernel then fits the 128 registers of a
// 1024-thread block but for a dozen spilled words.
//
// The ICP's iteration kernel is solo_icp_head_kernel (pcl_icp.hpp) over MapTarget, whose match() is that walk and the
// gather of the winner's row; the working buffers and the launch sequence of a call are SoloIcp's (solo_icp.hpp).  What
// is left here: the refusals, the empty map, and the launch of one pass.  Launch geometry follows the source length and
// the device alone, so an iteration's sums depend on the map's contents and never on its slot count.
#include <cmath>
#include <vector>

#include "pcl_icp.hpp"
#include "voxel_map.hpp"

using namespace a3d;

namespace {

constexpr uint32_t VQ_THREADS = 256;       // nearest: a thread per query, grid-stride
constexpr uint32_t VQ_BLOCKS_PER_CU = 8;
constexpr int VI_BLOCK = 1024;             // ICP: few, fat blocks as Icp's (every block of the next launch sums all partials)
constexpr uint32_t VM_ABSENT = ~0u;  // probe_slot: no slot holds the key (a table has at most 2^32 slots, its mask apart)
constexpr unsigned long long VM_NONE_WORD = 0x7F800000FFFFFFFFull;  // bits(+inf) << 32 | 0xFFFFFFFF: no correspondence
constexpr int VX_CELL_LIMIT_I = 1 << 20;

struct MapView {
  const VoxelSlot* table;
  const float* points;   // [slots][3]
  const float* normals;  // [slots][3] or null
  uint32_t mask;  // slots - 1 (the entries refuse a table of more than 2^32 slots: slot indices are 32-bit here)
};

// The slot that holds `key`, or VM_ABSENT.  `first` is the key of slot `s`, the key's home slot, as already loaded.
// Stops at the first empty slot; bounded by tries <= mask like claim_slot.  Plain loads: nobody writes the table.
__device__ __forceinline__ uint32_t probe_slot(const VoxelSlot* __restrict__ table, uint32_t mask, unsigned long long key,
                                               uint32_t s, unsigned long long first) {
  unsigned long long k = first;
  for (unsigned long long tries = 0; tries <= mask; ++tries) {
    if (k == key) return s;
    if (k == VX_EMPTY) break;
    s = (s + 1) & mask;
    k = table[s].key;
  }
  return VM_ABSENT;
}

struct VmMatch {
  unsigned long long word;  // bits(d2) << 32 | seq, VM_NONE_WORD: none
  uint32_t slot;            // of the winner (0 if none)
};

// The association of the header for one query.
__device__ __forceinline__ VmMatch vm_associate(const MapView& m, const VoxelGrid g, const V3 q) {
  VmMatch win{VM_NONE_WORD, 0u};
  const float cx = floorf((q.x - g.ox) / g.v), cy = floorf((q.y - g.oy) / g.v), cz = floorf((q.z - g.oz) / g.v);
  const bool ok = cx >= -VX_CELL_LIMIT && cx < VX_CELL_LIMIT && cy >= -VX_CELL_LIMIT && cy < VX_CELL_LIMIT &&
                  cz >= -VX_CELL_LIMIT && cz < VX_CELL_LIMIT;  // voxel_key's drop rule
  if (!ok) return win;
  const int ix = (int)cx, iy = (int)cy, iz = (int)cz;
#pragma unroll 1
  for (int dx = -1; dx <= 1; ++dx) {
    const int nx = ix + dx;
    if (nx < -VX_CELL_LIMIT_I || nx >= VX_CELL_LIMIT_I) continue;  // per axis, before the key is packed
    unsigned long long key[9], first[9];
    uint32_t home[9];
    bool live[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const int ny = iy + (c / 3 - 1), nz = iz + (c % 3 - 1);
      live[c] = ny >= -VX_CELL_LIMIT_I && ny < VX_CELL_LIMIT_I && nz >= -VX_CELL_LIMIT_I && nz < VX_CELL_LIMIT_I;
      const unsigned long long k = (unsigned long long)(nx + VX_CELL_LIMIT_I) << 42 |
                                   (unsigned long long)(ny + VX_CELL_LIMIT_I) << 21 |
                                   (unsigned long long)(nz + VX_CELL_LIMIT_I);
      key[c] = live[c] ? k : 0ull;  // (a skipped neighbour probes for key 0 and its answer is dropped)
      home[c] = (uint32_t)slot_hash(key[c]) & m.mask;
      first[c] = m.table[home[c]].key;
    }
    uint32_t slot[9];
    bool hit[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const uint32_t s = probe_slot(m.table, m.mask, key[c], home[c], first[c]);
      hit[c] = live[c] && s != VM_ABSENT;
      slot[c] = hit[c] ? s : 0u;  // (the loads below stay unconditional and in one round; the lanes without a cell all ask
                                  // for slot 0, one address per wave instead of one per lane)
    }
    f32x3 row[9];
    uint32_t seq[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      row[c] = *(const f32x3_u*)(m.points + 3 * (size_t)slot[c]);
      seq[c] = (uint32_t)m.table[slot[c]].best;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const float ex = q.x - row[c].x, ey = q.y - row[c].y, ez = q.z - row[c].z;
      const float d2 = (ex * ex + ey * ey) + ez * ez;
      const unsigned long long word = (unsigned long long)__float_as_uint(d2) << 32 | seq[c];
      if (hit[c] && word < win.word) win = VmMatch{word, slot[c]};
    }
  }
  return win;
}

__global__ void __launch_bounds__(VQ_THREADS)
    voxel_map_nearest_kernel(MapView map, VoxelGrid grid, const float* __restrict__ queries, uint32_t m, Pose pose,
                             uint32_t has_pose, uint32_t* __restrict__ out_seq, float* __restrict__ out_dist2) {
  const uint32_t stride = gridDim.x * VQ_THREADS;  // (m < 2^31, stride <= 2^19: the index cannot wrap)
  for (uint32_t i = blockIdx.x * VQ_THREADS + threadIdx.x; i < m; i += stride) {
    const f32x3 qv = *(const f32x3_u*)(queries + 3 * (size_t)i);
    V3 q{qv.x, qv.y, qv.z};
    if (has_pose) q = transform_vector(pose, q);
    const VmMatch win = vm_associate(map, grid, q);
    out_seq[i] = (uint32_t)win.word;
    out_dist2[i] = __uint_as_float((uint32_t)(win.word >> 32));
  }
}

// The map as solo_icp_head_kernel's target (pcl_icp.hpp): the map in place of the tree.
struct MapTarget {
  MapView map;
  VoxelGrid grid;
  __device__ __forceinline__ PointMatch match(const V3& p) const {
    const VmMatch win = vm_associate(map, grid, p);
    // the winner's row and its normal: one 12-byte gather each (slot 0 when nothing was found)
    const f32x3 tp = *(const f32x3_u*)(map.points + 3 * (size_t)win.slot), tn = *(const f32x3_u*)(map.normals + 3 * (size_t)win.slot);
    return PointMatch{win.word != VM_NONE_WORD, V3{tp.x, tp.y, tp.z}, V3{tn.x, tn.y, tn.z},
                      __uint_as_float((uint32_t)(win.word >> 32))};
  }
};

// Slot indices are 32-bit in these kernels (registers): a table of more than 2^32 slots, over 120 GiB, is refused.
a3d_status check_slots(const a3d_voxel_map* m) {
  A3D_REQUIRE(m->slots <= (1ull << 32), A3D_INVALID_PARAMETER, "a3d_voxel_map: a table of more than 2^32 slots cannot be queried");
  return A3D_OK;
}

MapView view_of(const a3d_voxel_map* m) {
  return MapView{m->table, m->points, m->normals, (uint32_t)(m->slots - 1)};
}

// Blocks of an iteration launch: the source length and the device alone decide (never the table).
uint32_t icp_grid(const a3d_voxel_map* map, uint32_t m) {
  return std::max(1u, std::min((m + VI_BLOCK - 1) / VI_BLOCK, map->icp.capacity));
}

// The map's working buffers, taken by its first align or accumulate: room for a block partial per CU.
a3d_status icp_reserve(a3d_voxel_map* map) {
  A3D_HIP_TRY(hipSetDevice(map->ctx->device));
  return solo_icp_reserve(map->ctx, &map->icp, (uint32_t)std::max(1, map->ctx->num_cus));
}

// One pass of the iteration kernel over `src`.
SoloLaunch pass_launcher(const a3d_voxel_map* map, const a3d_icp_params* params, const a3d_point_cloud_view* src) {
  const PclGates g = pcl_gates(*params);
  return [map, src, g](const SoloPass& p) -> a3d_status {
    const uint32_t m = (uint32_t)src->len;
    hipLaunchKernelGGL((solo_icp_head_kernel<VI_BLOCK, MapTarget>), dim3(icp_grid(map, m)), dim3(VI_BLOCK), 0,
                       map->ctx->stream, MapTarget{view_of(map), map->grid}, src->points, src->normals, m, p.state_in,
                       p.state_out, g, p.partials_in, p.partials_out, p.head);
    A3D_HIP_TRY(hipGetLastError());
    return A3D_OK;
  };
}

// The refusals of align and accumulate, decided before the context is touched.
a3d_status check_icp_call(const a3d_voxel_map* map, const a3d_icp_params* params, const a3d_point_cloud_view* src,
                          const void* out) {
  A3D_REQUIRE(map && params && src && out && src->points, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(src->len > 0 && src->len < (1ull << 31), A3D_INVALID_PARAMETER,
              "a3d_voxel_map_icp: the source needs 1 <= len < 2^31 points");
  A3D_REQUIRE(map->with_normals, A3D_MISSING_FIELD, "a3d_voxel_map_icp: the map keeps no normals");
  A3D_REQUIRE(src->normals, A3D_MISSING_FIELD, "Please, the source point cloud should have normals.");
  return check_slots(map);
}

}  // namespace

extern "C" {

a3d_status a3d_voxel_map_nearest_device(a3d_voxel_map* map, const float* d_queries, uint64_t m, const a3d_pose* pose_host,
                                        uint32_t* d_out_seq, float* d_out_dist2) {
  A3D_REQUIRE(map, A3D_INVALID_PARAMETER, "null argument");
  if (m == 0) return A3D_OK;
  A3D_REQUIRE(d_queries && d_out_seq && d_out_dist2, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(m < (1ull << 31), A3D_INVALID_PARAMETER, "a3d_voxel_map_nearest_device: 2^31 queries or more");
  {
    RangeRecorder ranges;
    ranges.in(d_queries, m * 12), ranges.out(d_out_seq, m * 4), ranges.out(d_out_dist2, m * 4);
    A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
                "a3d_voxel_map_nearest_device: the outputs overlap each other or the queries");
  }
  A3D_TRY(check_slots(map));
  a3d_context* ctx = map->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!map->block) {  // no table yet: every answer is "none"
    A3D_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_out_seq, (int)0xFFFFFFFFu, m, s));
    A3D_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_out_dist2, 0x7F800000, m, s));
  } else {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((m + VQ_THREADS - 1) / VQ_THREADS,
                                                         (uint64_t)std::max(1, ctx->num_cus) * VQ_BLOCKS_PER_CU);
    hipLaunchKernelGGL(voxel_map_nearest_kernel, dim3(blocks), dim3(VQ_THREADS), 0, s, view_of(map), map->grid, d_queries,
                       (uint32_t)m, pose_host ? pose_from_c(pose_host) : pose_eye(), pose_host ? 1u : 0u, d_out_seq,
                       d_out_dist2);
    A3D_HIP_TRY(hipGetLastError());
  }
  // host-synchronous: the caller may read or free the outputs right after
  A3D_HIP_TRY(hipStreamSynchronize(s));
  return A3D_OK;
}

a3d_status a3d_voxel_map_icp_align_device(a3d_voxel_map* map, const a3d_icp_params* params,
                                          const a3d_point_cloud_view* d_source, const a3d_pose* initial_host,
                                          a3d_pose* out_pose) {
  A3D_TRY(check_icp_call(map, params, d_source, out_pose));
  const Pose start = initial_host ? pose_from_c(initial_host) : pose_eye();
  if (!map->block) {  // no table yet: no point finds a row, as on a cleared map; the pose stays where it started
    pose_to_c(start, out_pose);
    map->icp.last_device_ms = 0.f;
    if (params->max_iterations == 0) return A3D_OK;
    set_error("GaussNewton::solve() returned None (count == 0 or Cholesky failed)");
    return A3D_SOLVE_FAILED;
  }
  A3D_TRY(icp_reserve(map));
  return solo_icp_align(map->ctx, &map->icp, *params, &start, icp_grid(map, (uint32_t)d_source->len),
                        "a3d_voxel_map_icp_align_device", pass_launcher(map, params, d_source), out_pose);
}

a3d_status a3d_voxel_map_icp_accumulate_device(a3d_voxel_map* map, const a3d_icp_params* params,
                                               const a3d_point_cloud_view* d_source, const a3d_pose* pose,
                                               a3d_gn_state* out_state) {
  A3D_TRY(check_icp_call(map, params, d_source, out_state));
  if (!map->block) {  // no table yet: nothing is accumulated
    const double sums[GN_PARTIAL] = {};
    gn_states_from_sums(sums, out_state, nullptr);
    return A3D_OK;
  }
  A3D_TRY(icp_reserve(map));
  return solo_icp_accumulate(map->ctx, &map->icp, pose ? pose_from_c(pose) : pose_eye(),
                             icp_grid(map, (uint32_t)d_source->len), "a3d_voxel_map_icp_accumulate_device",
                             pass_launcher(map, params, d_source), out_state);
}

a3d_status a3d_voxel_map_icp_last_device_ms(a3d_voxel_map* map, float* out_ms) {
  A3D_REQUIRE(map && out_ms, A3D_INVALID_PARAMETER, "null argument");
  *out_ms = map->icp.last_device_ms;
  return A3D_OK;
}

}  // extern "C"
