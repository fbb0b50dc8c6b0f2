// The per-point body of Icp::align (src/icp/pcl_icp.rs:68-92), shared by the one-pair kernel (kdtree.hip) and the
// batch kernel (pcl_icp_batch.hip) so that both compute the same bits per point.  Its tail behind the association,
// pcl_point_tail, also ends the loop of solo_icp_head_kernel below: the iteration kernel of the targets a lane queries
// alone, the voxel map (voxel_map_icp.hip) and the TSDF volume (tsdf_icp.hip).
#pragma once
#include "icp_engine.hpp"
#include "kdtree.hpp"

namespace a3d {

struct PclGates {
  float max_distance_sqr;
  float dot_reject_max;  // reject iff -1 <= sn.tn <= dot_reject_max  (== acos(sn.tn).abs() > max_normal_angle)
};

// The gates of Icp::align (pcl_icp.rs:76-83), both strict: every point-cloud ICP builds them here.
inline PclGates pcl_gates(const a3d_icp_params& params) {
  PclGates g;
  g.max_distance_sqr = params.max_distance * params.max_distance;
  g.dot_reject_max = acos_gate_threshold(params.max_normal_angle, /*strict=*/true);
  return g;
}

// What follows the association (src/icp/pcl_icp.rs:74-91): the two gates, the residual and the Jacobian of the
// point-to-plane cost, one Gauss-Newton step.  `live`: the thread holds a source point and it found a row.  p, sn: the
// source point and normal under the pose; tp, tn: the associated row and its normal; d2: their squared distance as the
// association computed it.  One definition for the kd-tree loop and solo_icp_head_kernel below.
__device__ __forceinline__ void pcl_point_tail(bool live, const V3& p, const V3& sn, const V3& tp, const V3& tn, float d2,
                                               const PclGates& gates, float (&acc)[GN_ACC]) {
  const float c = dot(sn, tn);
  const bool keep = live && !(d2 > gates.max_distance_sqr) && !(c >= -1.0f && c <= gates.dot_reject_max);
  if (keep) {
    const float rr = dot(tp - p, tn);
    const V3 tw = cross(p, tn);
    const float J[6] = {tn.x, tn.y, tn.z, tw.x, tw.y, tw.z};
    gn_step(acc, rr, J);
  }
}

// The body of Icp::align's point loop (src/icp/pcl_icp.rs:68-92); grid-stride.
template <int BLOCK>
__device__ __forceinline__ void pcl_point_loop(const KdSplits& sp, const float4* __restrict__ leaves,
                                               const float4* __restrict__ leaf_normals, uint32_t n, uint32_t max_depth,
                                               const float* __restrict__ src_points, const float* __restrict__ src_normals,
                                               uint32_t m, const Pose& T, const PclGates& gates, float (&acc)[GN_ACC]) {
  typedef float f32x3 __attribute__((ext_vector_type(3)));
  typedef f32x3 __attribute__((aligned(4))) f32x3_u;
  // every lane stays in the loop: the cooperative leaf scan needs the whole wave
  const uint32_t rounds = (m + gridDim.x * BLOCK - 1) / (gridDim.x * BLOCK);
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t i = (r * gridDim.x + blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t ii = i < m ? i : m - 1;
    const f32x3 pv = *(const f32x3_u*)(src_points + 3 * (size_t)ii), nv = *(const f32x3_u*)(src_normals + 3 * (size_t)ii);
    const V3 p = transform_vector(T, V3{pv.x, pv.y, pv.z});
    const uint32_t base = kdtree_descend(sp, n, max_depth, p);
    uint32_t slot;
    float d2;
    kdtree_scan_leaves_coop(leaves, base, p, &slot, &d2);
    // the winner's record and its normal: one 16-byte gather each (the point's line was just scanned)
    const float4 win = leaves[slot], tn4 = leaf_normals[slot];
    const V3 sn = transform_normal(T, V3{nv.x, nv.y, nv.z});
    pcl_point_tail(i < m, p, sn, V3{win.x, win.y, win.z}, V3{tn4.x, tn4.y, tn4.z}, d2, gates, acc);
  }
}

// What a target answers for one source point p under the pose: whether it has a partner at all, the partner and its
// normal, and their squared distance.
struct PointMatch {
  bool live;
  V3 tp, tn;
  float d2;
};

// One iteration of a single-job ICP against a target that every lane queries alone: pcl_icp_head_kernel's shape
// (kdtree.hip) without a split table to stage.  head_advance finishes the previous iteration, the point loop runs under
// the pose it leaves, and the block stores one partial.  Target: passed by value, with
// `__device__ __forceinline__ PointMatch match(const V3& p) const`.
template <int BLOCK, typename Target>
__global__ void __launch_bounds__(BLOCK)
    solo_icp_head_kernel(Target target, const float* __restrict__ src_points, const float* __restrict__ src_normals,
                         uint32_t m, const JobState* __restrict__ state_in, JobState* __restrict__ state_out, PclGates gates,
                         const float* __restrict__ partials_in, float* __restrict__ partials_out, HeadArgs head) {
  typedef float f32x3 __attribute__((ext_vector_type(3)));
  typedef f32x3 __attribute__((aligned(4))) f32x3_u;
  __shared__ uint32_t s_state[JOB_WORDS];
  head_advance<BLOCK>(state_in, blockIdx.x == 0 ? state_out : nullptr, partials_in, head, 0, s_state, blockIdx.x == 0);
  float acc[GN_ACC];
#pragma unroll
  for (int k = 0; k < GN_ACC; ++k) acc[k] = 0.0f;
  if ((int)s_state[15] == A3D_OK) {  // a failed job stays frozen
    const float* f = (const float*)s_state;
    const Pose T{{f[0], f[1], f[2]}, {f[3], f[4], f[5], f[6]}};
    const uint32_t stride = gridDim.x * BLOCK;  // (m < 2^31, stride = blocks <= CUs times 1024: the index cannot wrap)
#pragma unroll 1
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < m; i += stride) {
      const f32x3 pv = *(const f32x3_u*)(src_points + 3 * (size_t)i), nv = *(const f32x3_u*)(src_normals + 3 * (size_t)i);
      const V3 p = transform_vector(T, V3{pv.x, pv.y, pv.z});
      const PointMatch w = target.match(p);
      const V3 sn = transform_normal(T, V3{nv.x, nv.y, nv.z});
      pcl_point_tail(w.live, p, sn, w.tp, w.tn, w.d2, gates, acc);
    }
  }
  float* out = partials_out + (size_t)blockIdx.x * GN_PARTIAL;
  block_reduce_store<GN_ACC, false, BLOCK / 64>(acc, out);
  if (threadIdx.x >= GN_ACC && threadIdx.x < GN_PARTIAL) out[threadIdx.x] = 0.0f;  // no colour term
}

}  // namespace a3d
