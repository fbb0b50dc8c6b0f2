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
// tsdf_icp_head_kernel is voxel_map_icp_head_kernel (voxel_map_icp.hip) with that lookup in place of the hash-grid walk:
// head_advance finishes the previous iteration, the point loop runs under the pose it leaves, and the block stores one
// partial.  The tail of the point loop is pcl_point_tail (pcl_icp.hpp), the very function the kd-tree loops call.  Launch
// geometry follows the source length and the device alone, never the volume's size.  Registers: DESIGN.md, section 4.
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

// One iteration of the point-to-SDF ICP: voxel_map_icp_head_kernel's shape, the field in place of the map.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    tsdf_icp_head_kernel(TsdfGrid grid, const float* __restrict__ src_points, const float* __restrict__ src_normals, uint32_t m,
                         const JobState* __restrict__ state_in, JobState* __restrict__ state_out, PclGates gates,
                         const float* __restrict__ partials_in, float* __restrict__ partials_out, HeadArgs head) {
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
      const SdfSample s = sdf_sample(grid, p);
      const V3 sn = transform_normal(T, V3{nv.x, nv.y, nv.z});
      const V3 tp{p.x - s.d * s.n.x, p.y - s.d * s.n.y, p.z - s.d * s.n.z};
      pcl_point_tail(s.direction, p, sn, tp, s.n, s.d * s.d, gates, acc);
    }
  }
  float* out = partials_out + (size_t)blockIdx.x * GN_PARTIAL;
  block_reduce_store<GN_ACC, false, BLOCK / 64>(acc, out);
  if (threadIdx.x >= GN_ACC && threadIdx.x < GN_PARTIAL) out[threadIdx.x] = 0.0f;  // no colour term
}

// The volume's ICP working buffers inside its one block: two states | two partial sets | out pose (status 128 bytes
// behind it) | the f64 readback | the pose an align starts from.
struct IcpBuffers {
  JobState* state;
  float* partials;  // [2][blocks][GN_PARTIAL]
  Pose* out_pose;
  int32_t* out_status;
  double* readback;
  Pose* start_pose;
};

a3d_status icp_buffers(a3d_tsdf_volume* vol, IcpBuffers* out) {
  const uint32_t blocks = (uint32_t)std::max(1, vol->ctx->num_cus);
  const size_t state_b = pad256(2 * sizeof(JobState)), part_b = pad256(2 * (size_t)blocks * GN_PARTIAL * sizeof(float)),
               pose_b = 256, read_b = pad256(GN_PARTIAL * sizeof(double));
  if (!vol->icp_block) {
    A3D_TRY(ctx_block_alloc(vol->ctx, state_b + part_b + pose_b + read_b + pose_b, &vol->icp_block, &vol->icp_block_bytes));
    vol->icp_blocks = blocks;
  }
  char* blk = (char*)vol->icp_block;
  out->state = (JobState*)blk;
  out->partials = (float*)(blk + state_b);
  out->out_pose = (Pose*)(blk + state_b + part_b);
  out->out_status = (int32_t*)(blk + state_b + part_b + 128);
  out->readback = (double*)(blk + state_b + part_b + pose_b);
  out->start_pose = (Pose*)(blk + state_b + part_b + pose_b + read_b);
  return A3D_OK;
}

// Blocks of an iteration launch: the source length and the device alone decide (never the volume).
uint32_t icp_grid(const a3d_tsdf_volume* vol, uint32_t m) {
  return std::max(1u, std::min((m + TI_BLOCK - 1) / TI_BLOCK, vol->icp_blocks));
}

PclGates gates_of(const a3d_icp_params* params) {
  PclGates g;
  g.max_distance_sqr = params->max_distance * params->max_distance;
  g.dot_reject_max = acos_gate_threshold(params->max_normal_angle, /*strict=*/true);
  return g;
}

a3d_status launch_head_pass(const a3d_tsdf_volume* vol, const IcpBuffers& b, const PclGates& g, const a3d_point_cloud_view* src,
                            uint32_t seq, const HeadArgs& head) {
  const uint32_t m = (uint32_t)src->len, blocks = icp_grid(vol, m);
  const size_t half = (size_t)vol->icp_blocks * GN_PARTIAL;
  const JobState* st_in = b.state + (seq & 1u);
  JobState* st_out = b.state + ((seq + 1u) & 1u);
  const float* part_in = b.partials + (size_t)((seq + 1u) & 1u) * half;  // written by launch seq - 1
  float* part_out = b.partials + (size_t)(seq & 1u) * half;
  hipLaunchKernelGGL(tsdf_icp_head_kernel<TI_BLOCK>, dim3(blocks), dim3(TI_BLOCK), 0, vol->ctx->stream, grid_of(vol),
                     src->points, src->normals, m, st_in, st_out, g, part_in, part_out, head);
  A3D_HIP_TRY(hipGetLastError());
  return A3D_OK;
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

namespace a3d {
void tsdf_icp_release(a3d_tsdf_volume* vol) {
  if (vol->icp_block) ctx_block_release(vol->ctx, vol->icp_block, vol->icp_block_bytes);
  if (vol->icp_ev0) hipEventDestroy(vol->icp_ev0);
  if (vol->icp_ev1) hipEventDestroy(vol->icp_ev1);
  vol->icp_block = nullptr, vol->icp_ev0 = vol->icp_ev1 = nullptr;
}
}  // namespace a3d

extern "C" {

a3d_status a3d_tsdf_volume_sample_device(a3d_tsdf_volume* volume, const float* d_queries, uint64_t m,
                                         const a3d_pose* pose_host, float* d_out_distance, float* d_out_normals) {
  A3D_REQUIRE(volume, A3D_INVALID_PARAMETER, "null argument");
  if (m == 0) return A3D_OK;
  A3D_REQUIRE(d_queries && d_out_distance && d_out_normals, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(m < (1ull << 31), A3D_INVALID_PARAMETER, "a3d_tsdf_volume_sample_device: 2^31 queries or more");
  {
    std::vector<ByteRange> ranges{{(uintptr_t)d_queries, (uintptr_t)d_queries + (uintptr_t)m * 12, false},
                                  {(uintptr_t)d_out_distance, (uintptr_t)d_out_distance + (uintptr_t)m * 4, true},
                                  {(uintptr_t)d_out_normals, (uintptr_t)d_out_normals + (uintptr_t)m * 12, true}};
    A3D_REQUIRE(!outputs_overlap(ranges), A3D_INVALID_PARAMETER,
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
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  IcpBuffers b;
  A3D_TRY(icp_buffers(volume, &b));
  if (!volume->icp_ev1) {  // (both or neither: ev0 alone is a failed attempt that is taken up again)
    if (!volume->icp_ev0) A3D_HIP_TRY(hipEventCreate(&volume->icp_ev0));
    A3D_HIP_TRY(hipEventCreate(&volume->icp_ev1));
  }
  hipStream_t s = ctx->stream;
  const PclGates g = gates_of(params);
  a3d_status st = A3D_OK;
  if (hipMemcpyAsync(b.start_pose, &start, sizeof(Pose), hipMemcpyHostToDevice, s) != hipSuccess) st = A3D_HIP_ERROR;
  if (st == A3D_OK) hipEventRecord(volume->icp_ev0, s);
  if (st == A3D_OK) st = launch_job_init(s, b.state, b.start_pose, 1);
  // Icp::align's loop (pcl_icp.rs:59-106) in the head-solve form: launch k finishes iteration k - 1
  HeadArgs prev{};
  prev.mode = SOLVE_NONE;
  uint32_t seq = 0;
  const uint32_t blocks = icp_grid(volume, (uint32_t)d_source->len);
  for (uint64_t it = 0; st == A3D_OK && it < params->max_iterations; ++it, ++seq) {
    st = launch_head_pass(volume, b, g, d_source, seq, prev);
    prev.weight = params->weight, prev.color_weight = 0.0f, prev.mode = SOLVE_PCL_ICP;
    prev.tiles = blocks;
    prev.first_in_level = it == 0, prev.last_in_level = it + 1 == params->max_iterations;
  }
  if (st == A3D_OK)  // the last iteration is still pending: the finish kernel applies it
    st = launch_job_finish_head(s, b.state + (seq & 1u),
                                b.partials + (size_t)((seq + 1u) & 1u) * volume->icp_blocks * GN_PARTIAL, 0, prev, b.out_pose,
                                b.out_status, nullptr, 1);
  if (st == A3D_OK) hipEventRecord(volume->icp_ev1, s);
  Pose h_pose{};
  int32_t h_status = A3D_OK;
  if (st == A3D_OK && (hipMemcpyAsync(&h_pose, b.out_pose, sizeof(Pose), hipMemcpyDeviceToHost, s) != hipSuccess ||
                       hipMemcpyAsync(&h_status, b.out_status, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess))
    st = A3D_HIP_ERROR;
  // host-synchronous, the one wait of the call
  if (hipStreamSynchronize(s) != hipSuccess && st == A3D_OK) st = A3D_HIP_ERROR;
  if (st == A3D_OK) hipEventElapsedTime(&volume->icp_last_device_ms, volume->icp_ev0, volume->icp_ev1);
  if (st == A3D_HIP_ERROR)
    set_error("a3d_tsdf_volume_icp_align_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
  if (st != A3D_OK) return st;
  pose_to_c(h_pose, out_pose);
  if (h_status == A3D_SOLVE_FAILED) set_error("GaussNewton::solve() returned None (count == 0 or Cholesky failed)");
  return (a3d_status)h_status;
}

a3d_status a3d_tsdf_volume_icp_accumulate_device(a3d_tsdf_volume* volume, const a3d_icp_params* params,
                                                 const a3d_point_cloud_view* d_source, const a3d_pose* pose,
                                                 a3d_gn_state* out_state) {
  A3D_TRY(check_icp_call(volume, params, d_source, out_state));
  double sums[GN_PARTIAL] = {};
  a3d_context* ctx = volume->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  IcpBuffers b;
  A3D_TRY(icp_buffers(volume, &b));
  hipStream_t s = ctx->stream;
  const Pose h_pose = pose ? pose_from_c(pose) : pose_eye();
  a3d_status st = A3D_OK;
  if (hipMemcpyAsync(b.start_pose, &h_pose, sizeof(Pose), hipMemcpyHostToDevice, s) != hipSuccess) st = A3D_HIP_ERROR;
  if (st == A3D_OK) st = launch_job_init(s, b.state, b.start_pose, 1);
  HeadArgs none{};  // the per-iteration launch with nothing to finish at its head: partials in buffer 0
  none.mode = SOLVE_NONE;
  if (st == A3D_OK) st = launch_head_pass(volume, b, gates_of(params), d_source, 0, none);
  if (st == A3D_OK) st = launch_gn_readback(s, b.partials, (int)icp_grid(volume, (uint32_t)d_source->len), b.readback);
  if (st == A3D_OK && hipMemcpyAsync(sums, b.readback, sizeof(sums), hipMemcpyDeviceToHost, s) != hipSuccess)
    st = A3D_HIP_ERROR;
  if (hipStreamSynchronize(s) != hipSuccess && st == A3D_OK) st = A3D_HIP_ERROR;
  if (st == A3D_HIP_ERROR)
    set_error("a3d_tsdf_volume_icp_accumulate_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
  if (st != A3D_OK) return st;
  gn_states_from_sums(sums, out_state, nullptr);
  return A3D_OK;
}

a3d_status a3d_tsdf_volume_icp_last_device_ms(a3d_tsdf_volume* volume, float* out_ms) {
  A3D_REQUIRE(volume && out_ms, A3D_INVALID_PARAMETER, "null argument");
  *out_ms = volume->icp_last_device_ms;
  return A3D_OK;
}

}  // extern "C"
