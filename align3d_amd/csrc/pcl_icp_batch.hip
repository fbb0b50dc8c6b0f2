// P independent Icp::new(params, &target_p).align(&source_p) (src/icp/pcl_icp.rs:31-107) over clouds that are resident
// in device memory, as one launch sequence: the kd-trees are built back to back behind ONE host wait, and every
// iteration is one launch for all pairs (grid = blocks per pair x pairs, job = blockIdx.y) in the head-solve form of
// the one-pair kernel (kdtree.hip: pcl_icp_head_kernel).  The per-point arithmetic is pcl_point_loop's (pcl_icp.hpp).
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "pcl_icp.hpp"

using namespace a3d;

namespace {

// What a block needs to know about its pair: read through blockIdx.y (wave-uniform loads).  Trees of one batch differ
// in depth and size, sources in length.
struct PclPairDesc {
  const float* split;
  const float4* leaves;
  const float4* leaf_normals;
  const float* src_points;
  const float* src_normals;
  uint32_t n, max_depth, m, pad;
  uint64_t pad2;
};
static_assert(sizeof(PclPairDesc) == 64, "one descriptor per 64-byte line");

// One iteration of every pair.  Launch k first finishes iteration k - 1 of its pair from the previous launch's
// partials (head_advance: every block of the pair sums them in the same order and solves; block 0 stores the new
// state into the other state buffer), then takes the point loop and stores its partial with plain stores.
// partials: [pairs][gridDim.x][GN_PARTIAL] per buffer; a pair with few points still has gridDim.x blocks (a block
// without a point stores a zero partial).
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    pcl_icp_batch_head_kernel(const PclPairDesc* __restrict__ descs, uint32_t lds_levels_cap,
                              const JobState* __restrict__ state_in, JobState* __restrict__ state_out, PclGates gates,
                              const float* __restrict__ partials_in, float* __restrict__ partials_out, HeadArgs head) {
  // head_advance picks the solving wave as (blockIdx.x + blockIdx.y) & 3 (A3D_HEAD_ROTATE) and sums the partials with
  // the block's first 256 threads
  extern __shared__ __attribute__((aligned(16))) float kd_lds[];
  __shared__ uint32_t s_state[JOB_WORDS];
  const uint32_t job = blockIdx.y;
  const PclPairDesc d = descs[job];
  const uint32_t n_split = (1u << d.max_depth) - 1u;
  const uint32_t lds_levels = d.max_depth < lds_levels_cap ? d.max_depth : lds_levels_cap;  // deeper levels do not exist
  kd_stage_splits(d.split, n_split, lds_levels, kd_lds);
  const KdSplits sp{d.split, kd_lds, lds_levels};
  const size_t job_stride = (size_t)gridDim.x * GN_PARTIAL;
  head_advance<BLOCK>(state_in + job, blockIdx.x == 0 ? state_out + job : nullptr, partials_in + job * job_stride, head,
               (int)job, s_state, blockIdx.x == 0);
  float acc[GN_ACC];
#pragma unroll
  for (int k = 0; k < GN_ACC; ++k) acc[k] = 0.0f;
  if ((int)s_state[15] == A3D_OK) {  // a failed pair stays frozen; the others do not see it
    const float* f = (const float*)s_state;
    const Pose T{{f[0], f[1], f[2]}, {f[3], f[4], f[5], f[6]}};
    pcl_point_loop<BLOCK>(sp, d.leaves, d.leaf_normals, d.n, d.max_depth, d.src_points, d.src_normals, d.m, T, gates, acc);
  }
  float* out = partials_out + job * job_stride + (size_t)blockIdx.x * GN_PARTIAL;
  block_reduce_store<GN_ACC, false, BLOCK / 64>(acc, out);
  if (threadIdx.x >= GN_ACC && threadIdx.x < GN_PARTIAL) out[threadIdx.x] = 0.0f;  // no colour term
}

struct PairTree {
  float* split;
  float4* leaves;
  float4* leaf_normals;
  uint32_t n, max_depth;
};

}  // namespace

struct a3d_pcl_icp_batch {
  a3d_context* ctx = nullptr;
  a3d_icp_params params;
  uint32_t n_pairs = 0;
  std::vector<PairTree> trees;
  // Launch geometry ("IcpBatch"): `block` threads, at most `lds_levels` heap levels of a pair's split
  // table in LDS, at most `bpp_cap` blocks per pair (the partials are sized for it; a pass uses fewer when its largest
  // source has fewer points than that many blocks hold).
  uint32_t block = 1024, lds_levels = 15, bpp_cap = 1;
  uint32_t max_tree_depth = 0;
  void* d_block = nullptr;  // ONE device block (ctx_block_alloc): every tree's arrays and leaf normals, then the arrays below
  size_t block_bytes = 0;
  JobState* d_state = nullptr;  // [2][n_pairs]
  float* d_partials = nullptr;  // [2][n_pairs][bpp_cap][GN_PARTIAL]
  PclPairDesc* d_descs = nullptr;
  Pose* d_out_pose = nullptr;
  int32_t* d_out_status = nullptr;
  void* h_pinned = nullptr;  // page-locked: descriptor table, the builds' flag words, the results of the last pass
  PclPairDesc* h_descs = nullptr;
  uint32_t* h_flags = nullptr;
  Pose* h_pose = nullptr;
  int32_t* h_status = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;  // round the iteration launches; behind the result copies
  bool pass_recorded = false;
};

namespace {

void batch_destroy(a3d_pcl_icp_batch* b) {
  if (!b) return;
  if (b->ctx) {
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    ctx_block_release(b->ctx, b->d_block, b->block_bytes);
  }
  if (b->h_pinned) hipHostFree(b->h_pinned);
  if (b->ev0) hipEventDestroy(b->ev0);
  if (b->ev1) hipEventDestroy(b->ev1);
  if (b->ev_done) hipEventDestroy(b->ev_done);
  delete b;
}

struct BatchDeleter {
  void operator()(a3d_pcl_icp_batch* b) const { batch_destroy(b); }
};

// The geometry rule.  Product: 1024-thread blocks with up to 15 heap levels in LDS (128 KiB: one block per CU, the
// one-pair kernel's geometry) and one block per CU over the whole batch, i.e. num_cus / P blocks per pair.
// Diagnostics build: A3D_PCLB_BLOCK / _LDS_LEVELS / _BLOCKS_PER_CU (scripts/pcl_icp_batch_probe.py measures them).
void batch_geometry(a3d_pcl_icp_batch* b) {
  uint32_t block = 1024, levels = 15, per_cu = 1;
  if (const char* v = A3D_DIAG_ENV("A3D_PCLB_BLOCK")) block = (uint32_t)atoi(v);
  if (const char* v = A3D_DIAG_ENV("A3D_PCLB_LDS_LEVELS")) levels = (uint32_t)atoi(v);
  if (const char* v = A3D_DIAG_ENV("A3D_PCLB_BLOCKS_PER_CU")) per_cu = (uint32_t)atoi(v);
  if (block != 256 && block != 512 && block != 1024) block = 1024;
  b->block = block;
  b->lds_levels = std::min<uint32_t>(std::min<uint32_t>(levels, 15u), b->max_tree_depth);
  const uint64_t budget = (uint64_t)std::max(1, b->ctx->num_cus) * std::max<uint32_t>(1, std::min<uint32_t>(per_cu, 8u));
  b->bpp_cap = (uint32_t)std::max<uint64_t>(1, budget / std::max<uint32_t>(1, b->n_pairs));
}

template <int BLOCK>
a3d_status launch_iteration(a3d_pcl_icp_batch* b, uint32_t bpp, size_t lds_bytes, const PclGates& g, uint32_t seq,
                            const HeadArgs& head) {
  const uint32_t P = b->n_pairs;
  const size_t half = (size_t)P * b->bpp_cap * GN_PARTIAL;
  const JobState* st_in = b->d_state + (size_t)(seq & 1u) * P;
  JobState* st_out = b->d_state + (size_t)((seq + 1u) & 1u) * P;
  const float* part_in = b->d_partials + (size_t)((seq + 1u) & 1u) * half;  // written by launch seq - 1
  float* part_out = b->d_partials + (size_t)(seq & 1u) * half;
  hipLaunchKernelGGL(pcl_icp_batch_head_kernel<BLOCK>, dim3(bpp, P), dim3(BLOCK), lds_bytes, b->ctx->stream, b->d_descs,
                     b->lds_levels, st_in, st_out, g, part_in, part_out, head);
  A3D_HIP_TRY(hipGetLastError());
  return A3D_OK;
}

template <int BLOCK>
a3d_status allow_lds(size_t lds_bytes) {
  if (lds_bytes > 48 * 1024)
    A3D_HIP_TRY(hipFuncSetAttribute((const void*)pcl_icp_batch_head_kernel<BLOCK>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  return A3D_OK;
}

a3d_status batch_read_results(a3d_pcl_icp_batch* b, a3d_pose* out_poses_host, int32_t* out_status_host) {
  A3D_HIP_TRY(hipEventSynchronize(b->ev_done));
  for (uint32_t p = 0; p < b->n_pairs; ++p) {
    if (out_poses_host) pose_to_c(b->h_pose[p], out_poses_host + p);
    if (out_status_host) out_status_host[p] = b->h_status[p];
  }
  return A3D_OK;
}

}  // namespace

extern "C" {

a3d_status a3d_pcl_icp_batch_free(a3d_pcl_icp_batch* batch) {
  batch_destroy(batch);
  return A3D_OK;
}

a3d_status a3d_pcl_icp_batch_new_device(a3d_context* ctx, const a3d_icp_params* params, uint64_t n_pairs,
                                        const a3d_point_cloud_view* d_targets, a3d_pcl_icp_batch** out) {
  A3D_REQUIRE(ctx && params && out && (n_pairs == 0 || d_targets), A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(n_pairs <= 65535, A3D_INVALID_PARAMETER, "a3d_pcl_icp_batch_new_device: at most 65535 pairs (grid y)");
  std::unique_ptr<a3d_pcl_icp_batch, BatchDeleter> b(new a3d_pcl_icp_batch());
  b->params = *params;
  b->n_pairs = (uint32_t)n_pairs;
  const uint32_t P = b->n_pairs;
  if (P == 0) {  // an empty batch: its align is a no-op
    *out = b.release();
    return A3D_OK;
  }
  // every check before the first launch
  std::vector<size_t> arrays_b(P), normals_b(P);
  b->trees.resize(P);
  size_t scratch_b = 0, trees_b = 0;
  for (uint32_t p = 0; p < P; ++p) {
    const a3d_point_cloud_view& t = d_targets[p];
    if (!t.points || t.len == 0 || t.len >= (1ull << 31)) {
      set_error("a3d_pcl_icp_batch_new_device: pair %u: kd-tree needs 1 <= n < 2^31 points (the reference indexes an empty leaf and panics)", p);
      return A3D_INVALID_PARAMETER;
    }
    if (!t.normals) {  // the reference `expect`s at align time (pcl_icp.rs:50-53); a batch says so before it builds
      set_error("Please, the target point cloud should have normals. (pair %u)", p);
      return A3D_MISSING_FIELD;
    }
    uint64_t n_leaves, n_internal;
    uint32_t depth;
    kdtree_shape((uint32_t)t.len, &depth, &n_leaves, &n_internal);
    if (depth > 23) {
      set_error("a3d_pcl_icp_batch_new_device: pair %u: point cloud too large for the implicit kd-tree layout (leaf byte offsets are 32-bit)", p);
      return A3D_INVALID_PARAMETER;
    }
    b->trees[p].n = (uint32_t)t.len, b->trees[p].max_depth = depth;
    b->max_tree_depth = std::max(b->max_tree_depth, depth);
    arrays_b[p] = pad256(kdtree_arrays_bytes((uint32_t)t.len, depth));
    normals_b[p] = pad256((((size_t)1 << depth) * 16) * sizeof(float4));
    trees_b += arrays_b[p] + normals_b[p];
    scratch_b = std::max(scratch_b, kdtree_build_scratch_bytes((uint32_t)t.len, depth, ctx->stream));
  }
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  b->ctx = ctx;
  batch_geometry(b.get());
  for (hipEvent_t* e : {&b->ev0, &b->ev1, &b->ev_done}) A3D_HIP_TRY(hipEventCreate(e));
  // page-locked side: descriptor table | flag words of the builds | results
  const size_t h_desc_b = pad256((size_t)P * sizeof(PclPairDesc)), h_flag_b = pad256((size_t)P * 2 * sizeof(uint32_t)),
               h_pose_b = pad256((size_t)P * sizeof(Pose)), h_stat_b = pad256((size_t)P * sizeof(int32_t));
  A3D_HIP_TRY(hipHostMalloc(&b->h_pinned, h_desc_b + h_flag_b + h_pose_b + h_stat_b, hipHostMallocDefault));
  b->h_descs = (PclPairDesc*)b->h_pinned;
  b->h_flags = (uint32_t*)((char*)b->h_pinned + h_desc_b);
  b->h_pose = (Pose*)((char*)b->h_pinned + h_desc_b + h_flag_b);
  b->h_status = (int32_t*)((char*)b->h_pinned + h_desc_b + h_flag_b + h_pose_b);
  // device side: one block for all trees and the batch's own arrays (one allocation, not 2 P)
  const size_t state_b = pad256(2 * (size_t)P * sizeof(JobState)),
               part_b = pad256(2 * (size_t)P * b->bpp_cap * GN_PARTIAL * sizeof(float)), desc_b = h_desc_b,
               pose_b = h_pose_b, stat_b = h_stat_b;
  char* blk = nullptr;
  A3D_TRY(ctx_block_alloc(ctx, trees_b + state_b + part_b + desc_b + pose_b + stat_b, (void**)&blk, &b->block_bytes));
  b->d_block = blk;
  char* tail = blk + trees_b;
  b->d_state = (JobState*)tail;
  b->d_partials = (float*)(tail + state_b);
  b->d_descs = (PclPairDesc*)(tail + state_b + part_b);
  b->d_out_pose = (Pose*)(tail + state_b + part_b + desc_b);
  b->d_out_status = (int32_t*)(tail + state_b + part_b + desc_b + pose_b);
  // the builds share the context's kd-tree scratch region in stream order: grown once, for the largest tree, before
  // the first launch (growing it waits for the stream)
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 2, scratch_b, &region));
  a3d_status st = A3D_OK;
  char* cur = blk;
  for (uint32_t p = 0; p < P && st == A3D_OK; ++p) {
    a3d_kdtree t;  // (borrows the batch's memory: never handed to a3d_kdtree_free)
    t.ctx = ctx;
    t.n = b->trees[p].n, t.max_depth = b->trees[p].max_depth;
    t.n_split = (uint32_t)((1ull << t.max_depth) - 1);
    t.n_leaf_slots = (1ull << t.max_depth) * 16;
    st = kdtree_build_device(&t, d_targets[p].points, cur, b->h_flags + 2 * p);
    if (st == A3D_OK) st = kdtree_scatter_normals_device(&t, d_targets[p].normals, cur + arrays_b[p]);
    b->trees[p].split = t.d_split, b->trees[p].leaves = t.d_leaves, b->trees[p].leaf_normals = t.d_leaf_normals;
    cur += arrays_b[p] + normals_b[p];
  }
  // ONE wait for all trees; the NaN flags of all builds are read behind it
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == A3D_OK) {
    set_error("a3d_pcl_icp_batch_new_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
    st = A3D_HIP_ERROR;
  }
  if (st != A3D_OK) return st;
  for (uint32_t p = 0; p < P; ++p)
    if (kdtree_build_deferred_check(ctx, b->h_flags + 2 * p) != A3D_OK) {
      set_error("a3d_pcl_icp_batch_new_device: pair %u: NaN coordinate in kd-tree input (the reference panics in partial_cmp().unwrap())", p);
      return A3D_NAN_IN_INPUT;
    }
  *out = b.release();
  return A3D_OK;
}

a3d_status a3d_pcl_icp_batch_align_device(a3d_pcl_icp_batch* b, const a3d_point_cloud_view* d_sources,
                                          a3d_pose* out_poses_host, int32_t* out_status_host) {
  A3D_REQUIRE(b && (b->n_pairs == 0 || d_sources), A3D_INVALID_PARAMETER, "null argument");
  const uint32_t P = b->n_pairs;
  if (P == 0) return A3D_OK;
  uint64_t max_m = 0;
  for (uint32_t p = 0; p < P; ++p) {  // every check before the first launch
    const a3d_point_cloud_view& s = d_sources[p];
    if (s.len == 0 || s.len >= (1ull << 31)) {
      set_error("a3d_pcl_icp_batch_align_device: pair %u: bad source cloud (needs 1 <= len < 2^31 points)", p);
      return A3D_INVALID_PARAMETER;
    }
    if (!s.normals) {  // pcl_icp.rs:54-58
      set_error("Please, the source point cloud should have normals. (pair %u)", p);
      return A3D_MISSING_FIELD;
    }
    if (!s.points) {
      set_error("a3d_pcl_icp_batch_align_device: pair %u: bad source cloud (null points)", p);
      return A3D_INVALID_PARAMETER;
    }
    max_m = std::max<uint64_t>(max_m, s.len);
  }
  A3D_HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t s = b->ctx->stream;
  // the page-locked table and result slots belong to the previous pass until it is complete
  if (b->pass_recorded) A3D_HIP_TRY(hipEventSynchronize(b->ev_done));
  for (uint32_t p = 0; p < P; ++p) {
    PclPairDesc& d = b->h_descs[p];
    const PairTree& t = b->trees[p];
    d.split = t.split, d.leaves = t.leaves, d.leaf_normals = t.leaf_normals;
    d.src_points = d_sources[p].points, d.src_normals = d_sources[p].normals;
    d.n = t.n, d.max_depth = t.max_depth, d.m = (uint32_t)d_sources[p].len, d.pad = 0, d.pad2 = 0;
  }
  const uint32_t bpp = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b->bpp_cap, (max_m + b->block - 1) / b->block));
  const size_t lds_bytes = (size_t)std::min<uint64_t>((1ull << b->lds_levels) - 1, (1ull << b->max_tree_depth) - 1) * sizeof(float);
  const PclGates g = pcl_gates(b->params);
  if (b->block == 256) A3D_TRY(allow_lds<256>(lds_bytes));
  else if (b->block == 512) A3D_TRY(allow_lds<512>(lds_bytes));
  else A3D_TRY(allow_lds<1024>(lds_bytes));
  a3d_status st = A3D_OK;
  if (hipMemcpyAsync(b->d_descs, b->h_descs, (size_t)P * sizeof(PclPairDesc), hipMemcpyHostToDevice, s) != hipSuccess)
    st = A3D_HIP_ERROR;
  if (st == A3D_OK && hipEventRecord(b->ev0, s) != hipSuccess) st = A3D_HIP_ERROR;
  // every pair starts from Transform::eye(): initial_transform is ignored (pcl_icp.rs:59)
  if (st == A3D_OK) st = launch_job_init(s, b->d_state, nullptr, (int)P);
  HeadArgs prev{};
  prev.mode = SOLVE_NONE;
  uint32_t seq = 0;
  for (uint64_t it = 0; st == A3D_OK && it < b->params.max_iterations; ++it, ++seq) {
    if (b->block == 256) st = launch_iteration<256>(b, bpp, lds_bytes, g, seq, prev);
    else if (b->block == 512) st = launch_iteration<512>(b, bpp, lds_bytes, g, seq, prev);
    else st = launch_iteration<1024>(b, bpp, lds_bytes, g, seq, prev);
    prev.weight = b->params.weight, prev.color_weight = 0.0f, prev.mode = SOLVE_PCL_ICP;
    prev.tiles = bpp;
    prev.first_in_level = it == 0, prev.last_in_level = it + 1 == b->params.max_iterations;
  }
  if (st == A3D_OK)  // the last iteration is still pending: the finish kernel applies it, one block per pair
    st = launch_job_finish_head(s, b->d_state + (size_t)(seq & 1u) * P,
                                b->d_partials + (size_t)((seq + 1u) & 1u) * P * b->bpp_cap * GN_PARTIAL, bpp * GN_PARTIAL,
                                prev, b->d_out_pose, b->d_out_status, nullptr, (int)P);
  if (st == A3D_OK && hipEventRecord(b->ev1, s) != hipSuccess) st = A3D_HIP_ERROR;
  if (st == A3D_OK &&
      (hipMemcpyAsync(b->h_pose, b->d_out_pose, (size_t)P * sizeof(Pose), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipMemcpyAsync(b->h_status, b->d_out_status, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipEventRecord(b->ev_done, s) != hipSuccess))
    st = A3D_HIP_ERROR;
  if (st != A3D_OK) {  // some launches may be running with no event behind them
    if (st == A3D_HIP_ERROR) set_error("a3d_pcl_icp_batch_align_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
    hipStreamSynchronize(s);
    b->pass_recorded = false;
    return st;
  }
  b->pass_recorded = true;
  if (!out_poses_host && !out_status_host) return A3D_OK;  // enqueue only
  return batch_read_results(b, out_poses_host, out_status_host);
}

a3d_status a3d_pcl_icp_batch_results(a3d_pcl_icp_batch* b, a3d_pose* out_poses_host, int32_t* out_status_host) {
  A3D_REQUIRE(b && (out_poses_host || out_status_host), A3D_INVALID_PARAMETER, "null argument");
  if (b->n_pairs == 0) return A3D_OK;
  A3D_REQUIRE(b->pass_recorded, A3D_INVALID_PARAMETER, "a3d_pcl_icp_batch_results: no pass has been enqueued on this batch");
  A3D_HIP_TRY(hipSetDevice(b->ctx->device));
  return batch_read_results(b, out_poses_host, out_status_host);
}

a3d_status a3d_pcl_icp_batch_last_device_ms(a3d_pcl_icp_batch* b, float* out_ms) {
  A3D_REQUIRE(b && out_ms, A3D_INVALID_PARAMETER, "null argument");
  if (b->n_pairs == 0 || !b->pass_recorded) {
    *out_ms = 0.0f;
    return A3D_OK;
  }
  A3D_HIP_TRY(hipSetDevice(b->ctx->device));
  A3D_HIP_TRY(hipEventSynchronize(b->ev1));
  A3D_HIP_TRY(hipEventElapsedTime(out_ms, b->ev0, b->ev1));
  return A3D_OK;
}

}  // extern "C"
