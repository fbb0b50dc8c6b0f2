// The host side of a point-to-plane ICP that aligns ONE resident cloud against one target in the head-solve form
// (icp_engine.hpp): its working buffers and the two launch sequences.  Icp (kdtree.hip), DeviceVoxelMap.align
// (voxel_map_icp.hip) and DeviceTsdfVolume.align (tsdf_icp.hip) each hold one SoloIcp and hand the drivers a callable
// that launches their iteration kernel for one pass; everything else about a call is decided here, once.
#pragma once
#include <functional>

#include "icp_engine.hpp"

namespace a3d {

// One block of the context's (ctx_block_alloc), laid out by solo_icp_reserve:
//   two JobState | two sets of `capacity` block partials | out pose, its status 128 bytes behind it | the f64 readback |
//   the pose a call starts from | the ticket counter of Icp's diagnostics form (256 bytes each from the out pose on).
struct SoloIcp {
  void* block = nullptr;
  size_t block_bytes = 0;
  uint32_t capacity = 0;  // partial rows per half: the most blocks a pass may launch
  JobState* state = nullptr;    // [2]: launch seq reads seq & 1 and writes the other
  float* partials = nullptr;    // [2][capacity][GN_PARTIAL]: launch seq writes half seq & 1 and sums the other
  Pose* out_pose = nullptr;     // what job_finish_head leaves for the host
  int32_t* out_status = nullptr;
  double* readback = nullptr;   // [GN_PARTIAL], accumulate
  Pose* start_pose = nullptr;
  unsigned* counter = nullptr;  // zeroed by the owner that uses it (pcl_icp_new_impl); the drivers never touch it
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket the iteration launches of the last align
  float last_device_ms = 0.f;
};

// What one launch of an owner's iteration kernel is given.
struct SoloPass {
  const JobState* state_in;
  JobState* state_out;
  const float* partials_in;  // written by the launch before
  float* partials_out;
  HeadArgs head;
};
using SoloLaunch = std::function<a3d_status(const SoloPass&)>;

// Takes the block on first use (room for `capacity` partials per half); later calls change nothing.
a3d_status solo_icp_reserve(a3d_context* ctx, SoloIcp* s, uint32_t capacity);
void solo_icp_release(a3d_context* ctx, SoloIcp* s);

// Icp::align's loop (pcl_icp.rs:59-106) on ctx->stream, host-synchronous.  `start`: the pose the job starts from, null
// for the identity (then nothing is copied to the device).  `blocks`: what launch_pass launches, every pass alike.
// `entry_name`: the entry point, for the message of a HIP failure.
a3d_status solo_icp_align(a3d_context* ctx, SoloIcp* s, const a3d_icp_params& params, const Pose* start, uint32_t blocks,
                          const char* entry_name, const SoloLaunch& launch_pass, a3d_pose* out);
// Test hook: the sums of one pass at `pose`, nothing solved.
a3d_status solo_icp_accumulate(a3d_context* ctx, SoloIcp* s, const Pose& pose, uint32_t blocks, const char* entry_name,
                               const SoloLaunch& launch_pass, a3d_gn_state* out);

}  // namespace a3d
