// What the batched operations over resident clouds share (pointcloud.hip, cloud_transform.hip, voxel_downsample.hip).
// A call turns its clouds into a table of jobs in the context's scratch region 3 and launches over every tile of every
// job at once: a block finds its job with a block-uniform search over first_tile, and no block waits on another block.
// An operation that compacts runs a count pass (per tile and per job) and a write pass whose blocks sum their job's
// earlier tile counts for their offset and write nothing if any job of the batch overflows its capacity.  The end of
// the count pass and the start of the write pass stay in the kernels (cloud_count_kernel / voxel_flag_kernel,
// cloud_write_kernel / voxel_compact_kernel; keep each pair alike): as functions of this header they were inlined
// into slightly different code.
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"

namespace a3d {

#ifdef __HIPCC__
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef f32x3 __attribute__((aligned(4))) f32x3_u;  // one 12-byte load / store at a point's 4-byte alignment

// The job whose tiles hold `tile` (jobs are in tile order and none is empty; the search is uniform over the block).
template <class Job>
__device__ __forceinline__ uint32_t find_job(const Job* __restrict__ jobs, uint32_t n_jobs, uint32_t tile) {
  uint32_t lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_tile <= tile) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t ballot) {  // set lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// A colour row of a cloud: [3] u8 at byte 3 * index of a buffer that may itself start at any byte (the merge puts a
// cloud's first colour wherever the clouds before it end), so a row has no alignment at all.  It moves as three byte
// loads and three byte stores: right for every residue of the address mod 4, and the last store of a buffer ends on the
// buffer's last byte (a dword store over a row would write one byte past it).  r | g << 8 | b << 16 is the packed form
// the voxel map keeps by slot.
__device__ __forceinline__ uint32_t load_color(const uint8_t* colors, size_t index) {
  const uint8_t* c = colors + 3 * index;
  return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
}
__device__ __forceinline__ void store_color(uint8_t* colors, size_t index, uint32_t rgb) {
  uint8_t* c = colors + 3 * index;
  c[0] = (uint8_t)rgb, c[1] = (uint8_t)(rgb >> 8), c[2] = (uint8_t)(rgb >> 16);
}
#endif  // __HIPCC__

struct ByteRange {
  uintptr_t begin, end;
  bool output;
};

// Whether any output range overlaps any other range (inputs may overlap inputs).
inline bool outputs_overlap(std::vector<ByteRange>& ranges) {
  std::sort(ranges.begin(), ranges.end(), [](const ByteRange& a, const ByteRange& b) { return a.begin < b.begin; });
  uintptr_t end_any = 0, end_out = 0;  // furthest end among the ranges / the output ranges seen so far
  for (const ByteRange& r : ranges) {
    if (r.begin < (r.output ? end_any : end_out)) return true;
    end_any = std::max(end_any, r.end);
    if (r.output) end_out = std::max(end_out, r.end);
  }
  return false;
}

// A job's `len` elements as tiles of one or more chunks of `chunk` elements: at most `max_tiles` tiles, so the offset sum
// of a write-pass block stays short whatever the length.  *tiles: the batch's running total, advanced past this job
// (its tiles are *first_tile ... *tiles - 1).
inline a3d_status plan_tiles(uint64_t len, uint32_t chunk, uint32_t max_tiles, uint64_t* tiles, uint32_t* first_tile,
                             uint32_t* chunks_per_tile) {
  const uint64_t chunks = (len + chunk - 1) / chunk;
  *chunks_per_tile = (uint32_t)((chunks + max_tiles - 1) / max_tiles);
  *first_tile = (uint32_t)*tiles;
  *tiles += (chunks + *chunks_per_tile - 1) / *chunks_per_tile;
  A3D_REQUIRE(*tiles < (1ull << 31), A3D_INVALID_PARAMETER, "batch too large");
  return A3D_OK;
}

// A call's part of scratch region 3: job table | n_words 64-bit words, zeroed by the same upload as the table | one
// 32-bit count per tile | `extra_bytes` the operation lays out itself; every part 256-byte aligned.
struct BatchScratch {
  void* jobs = nullptr;
  unsigned long long* words = nullptr;
  uint32_t* tile_counts = nullptr;
  char* tail = nullptr;
  size_t table_bytes = 0;
  std::vector<char> staging;  // the upload's source: lives until the caller has waited for the stream
};
// The layout first (a job may hold addresses inside the tail) ...
inline a3d_status batch_scratch(a3d_context* ctx, size_t table_bytes, size_t n_words, uint64_t tiles, size_t extra_bytes,
                                BatchScratch* out) {
  const size_t jobs_bytes = pad256(table_bytes), words_bytes = pad256(n_words * 8), counts_bytes = pad256(tiles * 4);
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 3, jobs_bytes + words_bytes + counts_bytes + extra_bytes, &region));
  char* base = (char*)region;
  out->jobs = base;
  out->words = (unsigned long long*)(base + jobs_bytes);
  out->tile_counts = (uint32_t*)(base + jobs_bytes + words_bytes);
  out->tail = base + jobs_bytes + words_bytes + counts_bytes;
  out->table_bytes = table_bytes;
  out->staging.assign(jobs_bytes + words_bytes, 0);
  return A3D_OK;
}
// ... then the one upload of the table and the zeroed words.
inline a3d_status batch_upload(BatchScratch& b, const void* jobs, hipStream_t s) {
  memcpy(b.staging.data(), jobs, b.table_bytes);
  A3D_HIP_TRY(hipMemcpyAsync(b.jobs, b.staging.data(), b.staging.size(), hipMemcpyHostToDevice, s));
  return A3D_OK;
}

}  // namespace a3d
