// What the batched operations over resident clouds share: the conversion from range images (pointcloud.hip), transform
// and merge (cloud_transform.hip), the voxel downsamples (voxel_downsample.hip, voxel_mean.hip), select, knn distances
// and clustering (cloud_outliers.hip), normals (cloud_normals.hip), plane segmentation (cloud_plane.hip), the voxel map's
// insert and extract (voxel_map.hip) and the renders (cloud_render.hip).
// A call turns its clouds into a table of jobs in the context's scratch region 3 and launches over every tile of every
// job at once: a block finds its job with a block-uniform search over first_tile, and no block waits on another block.
// An operation that compacts runs a count pass (per tile and per job) and a write pass whose blocks sum their job's
// earlier tile counts for their offset and write nothing if any job of the batch overflows its capacity.  The end of
// the count pass and the start of the write pass stay in the kernels (cloud_count_kernel / voxel_flag_kernel,
// cloud_write_kernel / voxel_compact_kernel; keep each pair alike): as functions of this header they were inlined
// into slightly different code.
// The host front of those calls is here once, in plain C++17 (tests/cpp/cloud_batch_host_test.cpp runs it on made-up
// addresses): refuse() for a refusal in an entry point's name, RangeRecorder for "no output overlaps anything",
// plan_tiles / plan_job_tiles, compact_front / compact_finish for the calls that compact (select, voxel downsample,
// voxel mean), TailPart for the per-job arrays in the scratch tail (an offset until the region is allocated, an address
// afterwards), and download_words / zero_results / scatter_words for the end of a call.  A job struct is filled by field
// name, so every job keeps its own layout.
#pragma once
#include <algorithm>
#include <initializer_list>
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

// The refusal `what` of the entry point `name`, as the thread's error text.
inline a3d_status refuse(a3d_status status, const char* name, const char* what) {
  set_error("%s: %s", name, what);
  return status;
}

// The byte ranges a call reads (in) and writes (out).  A null pointer or zero bytes record nothing.
class RangeRecorder {
 public:
  void reserve(size_t n) { ranges_.reserve(n); }
  void in(const void* p, uint64_t bytes) { add(p, bytes, false); }
  void out(const void* p, uint64_t bytes) { add(p, bytes, true); }
  // Whether any output range overlaps any other range (inputs may overlap inputs; ranges that touch do not overlap).
  bool overlap() {
    std::sort(ranges_.begin(), ranges_.end(), [](const Range& a, const Range& b) { return a.begin < b.begin; });
    uintptr_t end_any = 0, end_out = 0;  // furthest end among the ranges / the output ranges seen so far
    for (const Range& r : ranges_) {
      if (r.begin < (r.output ? end_any : end_out)) return true;
      end_any = std::max(end_any, r.end);
      if (r.output) end_out = std::max(end_out, r.end);
    }
    return false;
  }
  size_t size() const { return ranges_.size(); }

 private:
  struct Range {
    uintptr_t begin, end;
    bool output;
  };
  void add(const void* p, uint64_t bytes, bool output) {
    if (p && bytes) ranges_.push_back({(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes, output});
  }
  std::vector<Range> ranges_;
};

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

// plan_tiles into the job's own fields, with its len; refuses a cloud so long that the kernels' 32-bit point positions,
// which run up to one tile span past len, would wrap.
template <class Job>
inline a3d_status plan_job_tiles(const char* name, uint64_t len, uint32_t chunk, uint32_t max_tiles, uint64_t* tiles, Job* j) {
  j->len = (uint32_t)len;
  A3D_TRY(plan_tiles(len, chunk, max_tiles, tiles, &j->first_tile, &j->chunks_per_tile));
  if (len + (uint64_t)j->chunks_per_tile * chunk >= (1ull << 32))
    return refuse(A3D_INVALID_PARAMETER, name, "a cloud within one tile of 2^32 points");
  return A3D_OK;
}

// The per-cloud arrays of a call that compacts (select, voxel downsample, voxel mean), as its entry point received them.
// colors, out_normals, out_colors and out_index may be null, and so may their entries.
struct CompactArgs {
  const a3d_point_cloud_view* clouds;
  const uint8_t* const* colors;
  float* const* out_points;
  float* const* out_normals;
  uint8_t* const* out_colors;
  uint32_t* const* out_index;
  const uint64_t* capacities;
};

// The front of such a call for its non-empty cloud i: what it requires of the cloud (`others_given`: the entry point's
// further arrays of this cloud are there; `nulls`: its text for a null one), the job's points ... out_colors, out_index,
// capacity, len and tiles, and the ranges: every input whole, of each output the first min(len, capacity) elements,
// which is all the call may write.
template <class Job>
inline a3d_status compact_front(const char* name, const CompactArgs& a, uint64_t i, bool others_given, const char* nulls,
                                uint32_t chunk, uint32_t max_tiles, uint64_t* tiles, RangeRecorder* ranges, Job* j) {
  const a3d_point_cloud_view& c = a.clouds[i];
  if (!(c.points && a.out_points[i] && others_given)) return refuse(A3D_INVALID_PARAMETER, name, nulls);
  float* out_normals = a.out_normals ? a.out_normals[i] : nullptr;
  if (out_normals && !c.normals) return refuse(A3D_MISSING_FIELD, name, "cloud has no normals");
  uint8_t* out_colors = a.out_colors ? a.out_colors[i] : nullptr;
  const uint8_t* colors = out_colors && a.colors ? a.colors[i] : nullptr;
  if (out_colors && !colors) return refuse(A3D_MISSING_FIELD, name, "cloud has no colours");
  j->points = c.points, j->normals = out_normals ? c.normals : nullptr, j->colors = colors;
  j->out_points = a.out_points[i], j->out_normals = out_normals, j->out_colors = out_colors;
  j->out_index = a.out_index ? a.out_index[i] : nullptr;
  j->capacity = a.capacities[i];
  A3D_TRY(plan_job_tiles(name, c.len, chunk, max_tiles, tiles, j));
  const uint64_t kept = std::min<uint64_t>(c.len, j->capacity);
  ranges->in(j->points, c.len * 12), ranges->in(j->normals, c.len * 12), ranges->in(j->colors, c.len * 3);
  ranges->out(j->out_points, kept * 12), ranges->out(out_normals, kept * 12), ranges->out(j->out_index, kept * 4);
  ranges->out(out_colors, kept * 3);
  return A3D_OK;
}

// A part of the scratch tail that holds one array per job.  While the clouds are walked a job's field holds the offset
// of its array inside the part; once the region is there, place_parts says where each part starts and rebase turns the
// offset into the address.
struct TailPart {
  size_t bytes = 0;      // of the arrays taken so far
  char* base = nullptr;  // set by place_parts
  template <class T>
  void take(T** field, size_t array_bytes) {
    *field = (T*)bytes;
    bytes += array_bytes;
  }
  template <class T>
  void rebase(T** field) const {
    *field = (T*)(base + (size_t)*field);
  }
};
// The parts back to back from `at` (BatchScratch::tail), in the order given.
inline void place_parts(char* at, std::initializer_list<TailPart*> parts) {
  for (TailPart* p : parts) p->base = at, at += p->bytes;
}

// A per-cloud result array zeroed, if the caller gave one (`per` words per cloud).
inline void zero_results(uint64_t* out, uint64_t n, size_t per = 1) {
  if (out) std::fill_n(out, per * n, (uint64_t)0);
}
// A run of `per` words per job to the per-cloud array `out`, if the caller gave one.
inline void scatter_words(const unsigned long long* words, const std::vector<uint64_t>& cloud_of_job, uint64_t* out,
                          size_t per = 1) {
  if (!out) return;
  for (size_t q = 0; q < cloud_of_job.size(); ++q)
    for (size_t w = 0; w < per; ++w) out[per * cloud_of_job[q] + w] = words[per * q + w];
}

// The end of a call that compacts: words = lens per job, then dropped per job (read only if out_dropped is given).  A
// capacity below its cloud's count (`rows`: what the entry point calls them) is refused after the counts are out.
template <class Job>
inline a3d_status compact_finish(const char* name, const char* rows, const std::vector<Job>& jobs,
                                 const std::vector<uint64_t>& cloud_of_job, const unsigned long long* words,
                                 uint64_t* out_lens, uint64_t* out_dropped) {
  scatter_words(words, cloud_of_job, out_lens);
  scatter_words(words + jobs.size(), cloud_of_job, out_dropped);
  for (size_t k = 0; k < jobs.size(); ++k)
    if (words[k] > jobs[k].capacity) {
      set_error("%s: a capacity is smaller than its cloud's %s (nothing was written)", name, rows);
      return A3D_INVALID_PARAMETER;
    }
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

// The end of a call: its n words to the host and the call's one wait.  Host-synchronous: the caller may free inputs and
// outputs right after.
inline a3d_status download_words(const unsigned long long* d_words, size_t n, hipStream_t s,
                                 std::vector<unsigned long long>* words) {
  words->resize(n);
  A3D_HIP_TRY(hipMemcpyAsync(words->data(), d_words, n * 8, hipMemcpyDeviceToHost, s));
  A3D_HIP_TRY(hipStreamSynchronize(s));
  return A3D_OK;
}

}  // namespace a3d
