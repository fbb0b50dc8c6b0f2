// Reading the dense TSDF volume (tsdf.hip) as an alignment target: the per-point field query
// a3d_tsdf_volume_sample_device and the point-to-SDF ICP a3d_tsdf_volume_icp_align_device.  The volume is only read
// here, with plain loads; every call is host-synchronous, so clear, upload and integrate may follow.
//
// The rule (include/align3d_hip.h states it; tests/tsdf_icp_restatement.py restates it): a point q, after its pose, has
// the voxel coordinate g = (q - origin) / v; D = tri(g) is the raycast rule's trilinear sample (tsdf.hpp), the gradient
// its six-sample central difference at unit voxel offsets, n = G / len in the world frame, d = D * tau, and the
// associated point is q - d * n.  There is no association step: no tree, no table, no search.
//
// Loads.  The lookup is seven tri() calls, 56 eight-byte loads per point, and it is written as those seven calls.  The
// offset samples do NOT share g's cell in f32: g + 1 is rounded, so floor(g + 1) may be floor(g) + 2 (g = 2 - 2^-23
// gives 3) and (g + 1) - floor(g + 1) carries fewer fraction bits than g - floor(g); every bit of the rule is therefore
// taken from tri() itself, on the rounded sum.  The 32 distinct voxels of the 4 x 4 x 4 neighbourhood are each asked for
// up to three times, the repeats hit the line the first load brought in: a lane's x-run of four records is one 32-byte
// stretch, and the lanes of a wave, neighbouring pixels of a frame cloud, overlap in x.  The six gradient samples are
// taken only where the centre has a value with |D| < 1: away from the surface a point costs eight loads.
//
// The ICP's iteration kernel is solo_icp_head_kernel (pcl_icp.hpp) over SdfTarget, whose match() is that lookup; the
// working buffers and the launch sequence of a call are SoloIcp's (solo_icp.hpp), as for the voxel map and Icp.  What is
// left here: the refusals and the launch of one pass.  Launch geometry follows the source length and the device alone,
// never the volume's size.  Registers: DESIGN.md, section 4.
#include <cmath>
#include <vector>

#include "pcl_icp.hpp"
#include "tsdf.hpp"

using namespace a3d;

namespace {

constexpr uint32_t TQ_THREADS = 256;  // sample: a thread per query, grid-stride
constexpr uint32_t TQ_BLOCKS_PER_CU = 8;
constexpr int TI_BLOCK = 1024;  // ICP: few, fat blocks as Icp's (every block of the next launch sums all partials)
constexpr uint32_t TQ_NAN_BITS = 0x7FC00000u;  // no value

struct SdfSample {
  bool value;      // step 2: the centre sample is valid
  bool direction;  // steps 3 and 4: |D| < 1 and a finite, non-zero gradient
  float d;         // D * tau (TQ_NAN_BITS without a value, and for any NaN)
  V3 n;            // G / len in the world frame (+0 without a direction)
};

// Steps 1-5 of the header's rule for one point in the world frame.
__device__ __forceinline__ SdfSample sdf_sample(const TsdfGrid& g, const V3 q) {
  SdfSample s{false, false, __uint_as_float(TQ_NAN_BITS), V3{0.0f, 0.0f, 0.0f}};
  const V3 gc{(q.x - g.ox) / g.v, (q.y - g.oy) / g.v, (q.z - g.oz) / g.v};
  float D;
  if (!tri(g, gc, &D)) return s;
  s.value = true;
  const float d = D * g.tau;
  if (d == d) s.d = d;  // (a NaN keeps the one bit pattern)
  if (!(fabsf(D) < 1.0f)) return s;  // clamped at the truncation: no direction (a NaN fails)
  float xp, xm, yp, ym, zp, zm;
  // (bitwise on purpose: all six samples are taken, as the rule states them)
  const bool all = tri(g, V3{gc.x + 1.0f, gc.y, gc.z}, &xp) & tri(g, V3{gc.x - 1.0f, gc.y, gc.z}, &xm) &
                   tri(g, V3{gc.x, gc.y + 1.0f, gc.z}, &yp) & tri(g, V3{gc.x, gc.y - 1.0f, gc.z}, &ym) &
                   tri(g, V3{gc.x, gc.y, gc.z + 1.0f}, &zp) & tri(g, V3{gc.x, gc.y, gc.z - 1.0f}, &zm);
  if (!all) return s;
  const V3 G{xp - xm, yp - ym, zp - zm};
  const float len = sqrtf(G.x * G.x + G.y * G.y + G.z * G.z);
  if (!(len > 0.0f && len < INFINITY)) return s;
  s.direction = true;
  s.n = G / len;
  return s;
}

__global__ void __launch_bounds__(TQ_THREADS)
    tsdf_sample_kernel(TsdfGrid grid, const float* __restrict__ queries, uint32_t m, Pose pose, uint32_t has_pose,
                       float* __restrict__ out_distance, float* __restrict__ out_normals) {
  const uint32_t stride = gridDim.x * TQ_THREADS;  // (m < 2^31, stride <= 2^19: the index cannot wrap)
  for (uint32_t i = blockIdx.x * TQ_THREADS + threadIdx.x; i < m; i += stride) {
    const f32x3 qv = *(const f32x3_u*)(queries + 3 * (size_t)i);
    V3 q{qv.x, qv.y, qv.z};
    if (has_pose) q = transform_vector(pose, q);
    const SdfSample s = sdf_sample(grid, q);
    out_distance[i] = s.d;
    *(f32x3_u*)(out_normals + 3 * (size_t)i) = f32x3{s.n.x, s.n.y, s.n.z};
  }
}

// The field as solo_icp_head_kernel's target (pcl_icp.hpp): the lookup in place of a search.
struct SdfTarget {
  TsdfGrid grid;
  __device__ __forceinline__ PointMatch match(const V3& p) const {
    const SdfSample s = sdf_sample(grid, p);
    const V3 tp{p.x - s.d * s.n.x, p.y - s.d * s.n.y, p.z - s.d * s.n.z};
    return PointMatch{s.direction, tp, s.n, s.d * s.d};
  }
};

// Blocks of an iteration launch: the source length and the device alone decide (never the volume).
uint32_t icp_grid(const a3d_tsdf_volume* vol, uint32_t m) {
  return std::max(1u, std::min((m + TI_BLOCK - 1) / TI_BLOCK, vol->icp.capacity));
}

// The volume's working buffers, taken by its first align or accumulate: room for a block partial per CU.
a3d_status icp_reserve(a3d_tsdf_volume* vol) {
  A3D_HIP_TRY(hipSetDevice(vol->ctx->device));
  return solo_icp_reserve(vol->ctx, &vol->icp, (uint32_t)std::max(1, vol->ctx->num_cus));
}

// One pass of the iteration kernel over `src`.
SoloLaunch pass_launcher(const a3d_tsdf_volume* vol, const a3d_icp_params* params, const a3d_point_cloud_view* src) {
  const PclGates g = pcl_gates(*params);
  return [vol, src, g](const SoloPass& p) -> a3d_status {
    const uint32_t m = (uint32_t)src->len;
    hipLaunchKernelGGL((solo_icp_head_kernel<TI_BLOCK, SdfTarget>), dim3(icp_grid(vol, m)), dim3(TI_BLOCK), 0,
                       vol->ctx->stream, SdfTarget{grid_of(vol)}, src->points, src->normals, m, p.state_in, p.state_out, g,
                       p.partials_in, p.partials_out, p.head);
    A3D_HIP_TRY(hipGetLastError());
    return A3D_OK;
  };
}

// The refusals of align and accumulate, decided before the volume or the context is touched.
a3d_status check_icp_call(const a3d_tsdf_volume* vol, const a3d_icp_params* params, const a3d_point_cloud_view* src,
                          const void* out) {
  A3D_REQUIRE(vol && params && src && out && src->points, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(src->len > 0 && src->len < (1ull << 31), A3D_INVALID_PARAMETER,
              "a3d_tsdf_volume_icp: the source needs 1 <= len < 2^31 points");
  A3D_REQUIRE(src->normals, A3D_MISSING_FIELD, "Please, the source point cloud should have normals.");
  return A3D_OK;
}

}  // namespace

extern "C" {

a3d_status a3d_tsdf_volume_sample_device(a3d_tsdf_volume* volume, const float* d_queries, uint64_t m,
                                         const a3d_pose* pose_host, float* d_out_distance, float* d_out_normals) {
  A3D_REQUIRE(volume, A3D_INVALID_PARAMETER, "null argument");
  if (m == 0) return A3D_OK;
  A3D_REQUIRE(d_queries && d_out_distance && d_out_normals, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(m < (1ull << 31), A3D_INVALID_PARAMETER, "a3d_tsdf_volume_sample_device: 2^31 queries or more");
  {
    RangeRecorder ranges;
    ranges.in(d_queries, m * 12), ranges.out(d_out_distance, m * 4), ranges.out(d_out_normals, m * 12);
    A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER,
                "a3d_tsdf_volume_sample_device: the outputs overlap each other or the queries");
  }
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((m + TQ_THREADS - 1) / TQ_THREADS,
                                                       (uint64_t)std::max(1, ctx->num_cus) * TQ_BLOCKS_PER_CU);
  hipLaunchKernelGGL(tsdf_sample_kernel, dim3(blocks), dim3(TQ_THREADS), 0, s, grid_of(volume), d_queries, (uint32_t)m,
                     pose_host ? pose_from_c(pose_host) : pose_eye(), pose_host ? 1u : 0u, d_out_distance, d_out_normals);
  A3D_HIP_TRY(hipGetLastError());
  // host-synchronous: the caller may read or free the outputs right after
  A3D_HIP_TRY(hipStreamSynchronize(s));
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_icp_align_device(a3d_tsdf_volume* volume, const a3d_icp_params* params,
                                            const a3d_point_cloud_view* d_source, const a3d_pose* initial_host,
                                            a3d_pose* out_pose) {
  A3D_TRY(check_icp_call(volume, params, d_source, out_pose));
  const Pose start = initial_host ? pose_from_c(initial_host) : pose_eye();
  A3D_TRY(icp_reserve(volume));
  return solo_icp_align(volume->ctx, &volume->icp, *params, &start, icp_grid(volume, (uint32_t)d_source->len),
                        "a3d_tsdf_volume_icp_align_device", pass_launcher(volume, params, d_source), out_pose);
}

a3d_status a3d_tsdf_volume_icp_accumulate_device(a3d_tsdf_volume* volume, const a3d_icp_params* params,
                                                 const a3d_point_cloud_view* d_source, const a3d_pose* pose,
                                                 a3d_gn_state* out_state) {
  A3D_TRY(check_icp_call(volume, params, d_source, out_state));
  A3D_TRY(icp_reserve(volume));
  return solo_icp_accumulate(volume->ctx, &volume->icp, pose ? pose_from_c(pose) : pose_eye(),
                             icp_grid(volume, (uint32_t)d_source->len), "a3d_tsdf_volume_icp_accumulate_device",
                             pass_launcher(volume, params, d_source), out_state);
}

a3d_status a3d_tsdf_volume_icp_last_device_ms(a3d_tsdf_volume* volume, float* out_ms) {
  A3D_REQUIRE(volume && out_ms, A3D_INVALID_PARAMETER, "null argument");
  *out_ms = volume->icp.last_device_ms;
  return A3D_OK;
}

}  // extern "C"
