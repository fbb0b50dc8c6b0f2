// The working buffers and the two launch sequences of the single-job point-cloud ICPs (solo_icp.hpp).
#include "solo_icp.hpp"

namespace a3d {

a3d_status solo_icp_reserve(a3d_context* ctx, SoloIcp* s, uint32_t capacity) {
  if (s->block) return A3D_OK;
  const size_t state_b = pad256(2 * sizeof(JobState)), part_b = pad256(2 * (size_t)capacity * GN_PARTIAL * sizeof(float)),
               slot_b = 256, read_b = pad256(GN_PARTIAL * sizeof(double));
  A3D_TRY(ctx_block_alloc(ctx, state_b + part_b + slot_b + read_b + 2 * slot_b, &s->block, &s->block_bytes));
  s->capacity = capacity;
  char* at = (char*)s->block;
  s->state = (JobState*)at, at += state_b;
  s->partials = (float*)at, at += part_b;
  s->out_pose = (Pose*)at, s->out_status = (int32_t*)(at + 128), at += slot_b;
  s->readback = (double*)at, at += read_b;
  s->start_pose = (Pose*)at, at += slot_b;
  s->counter = (unsigned*)at;
  return A3D_OK;
}

void solo_icp_release(a3d_context* ctx, SoloIcp* s) {
  if (s->block) ctx_block_release(ctx, s->block, s->block_bytes);
  if (s->ev0) hipEventDestroy(s->ev0);
  if (s->ev1) hipEventDestroy(s->ev1);
  s->block = nullptr, s->ev0 = s->ev1 = nullptr;
}

namespace {

// Launch `seq` of a job: state and partials ping-pong, so that the blocks of a launch may still read what the launch
// before it left while one of them writes the new state.
SoloPass pass_of(const SoloIcp& s, uint32_t seq, const HeadArgs& head) {
  const size_t half = (size_t)s.capacity * GN_PARTIAL;
  return SoloPass{s.state + (seq & 1u), s.state + ((seq + 1u) & 1u), s.partials + (size_t)((seq + 1u) & 1u) * half,
                  s.partials + (size_t)(seq & 1u) * half, head};
}

}  // namespace

a3d_status solo_icp_align(a3d_context* ctx, SoloIcp* s, const a3d_icp_params& params, const Pose* start, uint32_t blocks,
                          const char* entry_name, const SoloLaunch& launch_pass, a3d_pose* out) {
  if (!s->ev1) {  // (both or neither: ev0 alone is a failed attempt that is taken up again)
    if (!s->ev0) A3D_HIP_TRY(hipEventCreate(&s->ev0));
    A3D_HIP_TRY(hipEventCreate(&s->ev1));
  }
  hipStream_t stream = ctx->stream;
  a3d_status st = A3D_OK;
  if (start && hipMemcpyAsync(s->start_pose, start, sizeof(Pose), hipMemcpyHostToDevice, stream) != hipSuccess)
    st = A3D_HIP_ERROR;
  if (st == A3D_OK) hipEventRecord(s->ev0, stream);
  if (st == A3D_OK) st = launch_job_init(stream, s->state, start ? s->start_pose : nullptr, 1);
  // the head-solve form: launch k finishes iteration k - 1
  HeadArgs prev{};
  prev.mode = SOLVE_NONE;
  uint32_t seq = 0;
  for (uint64_t it = 0; st == A3D_OK && it < params.max_iterations; ++it, ++seq) {
    st = launch_pass(pass_of(*s, seq, prev));
    prev.weight = params.weight, prev.color_weight = 0.0f, prev.mode = SOLVE_PCL_ICP;
    prev.tiles = blocks;
    prev.first_in_level = it == 0, prev.last_in_level = it + 1 == params.max_iterations;
  }
  if (st == A3D_OK) {  // the last iteration is still pending: the finish kernel applies it
    const SoloPass last = pass_of(*s, seq, prev);
    st = launch_job_finish_head(stream, last.state_in, last.partials_in, 0, prev, s->out_pose, s->out_status, nullptr, 1);
  }
  if (st == A3D_OK) hipEventRecord(s->ev1, stream);
  Pose h_pose{};
  int32_t h_status = A3D_OK;
  if (st == A3D_OK && (hipMemcpyAsync(&h_pose, s->out_pose, sizeof(Pose), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                       hipMemcpyAsync(&h_status, s->out_status, sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess))
    st = A3D_HIP_ERROR;
  // host-synchronous, the one wait of the call
  if (hipStreamSynchronize(stream) != hipSuccess && st == A3D_OK) st = A3D_HIP_ERROR;
  if (st == A3D_OK) hipEventElapsedTime(&s->last_device_ms, s->ev0, s->ev1);
  if (st == A3D_HIP_ERROR) set_error("%s: HIP failure: %s", entry_name, hipGetErrorString(hipGetLastError()));
  if (st != A3D_OK) return st;
  pose_to_c(h_pose, out);
  if (h_status == A3D_SOLVE_FAILED) set_error("GaussNewton::solve() returned None (count == 0 or Cholesky failed)");
  return (a3d_status)h_status;
}

a3d_status solo_icp_accumulate(a3d_context* ctx, SoloIcp* s, const Pose& pose, uint32_t blocks, const char* entry_name,
                               const SoloLaunch& launch_pass, a3d_gn_state* out) {
  hipStream_t stream = ctx->stream;
  double sums[GN_PARTIAL] = {};
  a3d_status st = A3D_OK;
  if (hipMemcpyAsync(s->start_pose, &pose, sizeof(Pose), hipMemcpyHostToDevice, stream) != hipSuccess) st = A3D_HIP_ERROR;
  if (st == A3D_OK) st = launch_job_init(stream, s->state, s->start_pose, 1);
  HeadArgs none{};  // the per-iteration launch with nothing to finish at its head: partials in buffer 0
  none.mode = SOLVE_NONE;
  if (st == A3D_OK) st = launch_pass(pass_of(*s, 0, none));
  if (st == A3D_OK) st = launch_gn_readback(stream, s->partials, (int)blocks, s->readback);
  if (st == A3D_OK && hipMemcpyAsync(sums, s->readback, sizeof(sums), hipMemcpyDeviceToHost, stream) != hipSuccess)
    st = A3D_HIP_ERROR;
  if (hipStreamSynchronize(stream) != hipSuccess && st == A3D_OK) st = A3D_HIP_ERROR;
  if (st == A3D_HIP_ERROR) set_error("%s: HIP failure: %s", entry_name, hipGetErrorString(hipGetLastError()));
  if (st != A3D_OK) return st;
  gn_states_from_sums(sums, out, nullptr);
  return A3D_OK;
}

}  // namespace a3d
