// The neighbour graph of a resident cloud, shared by the entries that walk it (cloud_normals.hip: normals;
// cloud_outliers.hip: knn distances and clustering): a hash grid of pitch r that keeps ALL points of a cell, a counting
// sort of the kept points by cell (three launches over the job table of cloud_batch.hpp), and the walk over the 27 cells
// around a record.  One definition, so the entries cannot drift apart.  voxel_mean.hip sorts by cell with passes of its own
// (runs combined per wave, a representative per cell) and takes the record, find_slot and f32x4 from here.
//
// A job struct of a caller (NormalsJob, KnnJob) is read by field name, as find_job does: points, table, sorted, slot_mask,
// len, first_tile, chunks_per_tile, n_tiles; and it says what a dropped row gets with a __device__ member drop_row(p).
// Every walk takes cell_run.  normals_estimate_kernel and the count pass of cluster_walk_kernel take consume_run as well.
// Three loops stay written out in their kernels: the link pass of cluster_walk_kernel (its own software-pipelined trips),
// the LDS form of normals_estimate_kernel (its staging), and knn_distance_kernel, the hottest of the walks: through the
// helper the compiler emits other code for it (11 to 15 instructions fewer, the count-only form on 38 VGPRs for 36), and
// the timing gate's spread between runs of one build (+-0.5 %) is too coarse to show that this costs nothing; written
// out, every form of it is the parent's code instruction for instruction.  The figures of every kernel before and after
// are in profiles/cell_sort_isa_stats.txt: the same occupancy everywhere, no scratch.
#pragma once
#include "voxel_grid.hpp"  // VoxelGrid, voxel_key, slot_hash, VoxelSlot

namespace a3d {

constexpr uint32_t CELL_THREADS = 256;
constexpr uint32_t CELL_CHUNK = 4 * CELL_THREADS;  // points per chunk: a multiple of 64, so a ballot word never straddles tiles
constexpr uint32_t CELL_MAX_TILES = 4096;          // tiles per cloud at most
constexpr uint32_t CELL_AHEAD = 4;                 // candidates whose loads a walk issues together

struct CellRecord {  // a kept point in cell order
  float x, y, z;
  uint32_t index;
};
static_assert(sizeof(CellRecord) == 16, "CellRecord layout");

#ifdef __HIPCC__
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The slot that holds `tag` (key + 1), or ~0 if the table has none (the walk stops at the first empty slot).
__device__ __forceinline__ unsigned long long find_slot(const VoxelSlot* __restrict__ table, unsigned long long mask,
                                                        unsigned long long tag) {
  unsigned long long s = slot_hash(tag - 1) & mask;
  for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
    const unsigned long long k = table[s].key;
    if (k == tag) return s;
    if (k == 0) break;
  }
  return ~0ull;
}

// Pass 1: a thread per point claims the slot of its key (load, then 64-bit atomicCAS: the table has at least two slots per
// point; the key word holds key + 1, so that one fill with zeros empties keys and counts alike) and adds 1 to the slot's
// count.  dropped[job] += dropped points; *fault is set if a table were ever full (it cannot be).
template <class Job>
__global__ void __launch_bounds__(CELL_THREADS)
    cell_count_kernel(const Job* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, unsigned long long* __restrict__ dropped,
                      unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const Job& j = jobs[ji];
  const float* __restrict__ points = j.points;
  VoxelSlot* table = j.table;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (len < 2^32 - span: checked by the host)
  uint32_t n_dropped = 0;
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += CELL_THREADS) {
    const f32x3 pt = *(const f32x3_u*)(points + 3 * (size_t)p);
    unsigned long long key;
    if (!voxel_key(pt, grid, &key, nullptr)) {
      ++n_dropped;
      continue;
    }
    const unsigned long long tag = key + 1;
    unsigned long long s = slot_hash(key) & mask;
    bool placed = false;
    for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
      unsigned long long k = VX_LOAD_AGENT(&table[s].key);
      if (k == 0) k = atomicCAS(&table[s].key, 0ull, tag);
      if (k == 0 || k == tag) {
        placed = true;
        break;
      }
    }
    if (!placed) {
      atomicMax(fault, 1ull);
      continue;
    }
    atomicAdd(&table[s].best, 1ull);
  }
  n_dropped = wave_sum(n_dropped);
  if ((threadIdx.x & 63u) == 0 && n_dropped) atomicAdd(&dropped[ji], (unsigned long long)n_dropped);
}

// Pass 2: a thread per slot; every occupied slot's second word = start << 32 | count, the starts handed out from
// cursor[job] (zeroed by the upload; it ends as the job's kept count): a wave sums its occupied slots' counts and takes its
// run of the cursor with one atomicAdd.  The order of the cells in memory is free.  Tile t of a job takes slots
// [t * per, (t + 1) * per), per = ceil(slots / tiles).
template <class Job>
__global__ void __launch_bounds__(CELL_THREADS)
    cell_place_kernel(const Job* __restrict__ jobs, uint32_t n_jobs, unsigned long long* __restrict__ cursor) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const Job& j = jobs[ji];
  VoxelSlot* table = j.table;
  const unsigned long long slots = j.slot_mask + 1, per = (slots + j.n_tiles - 1) / j.n_tiles;
  const unsigned long long s0 = (unsigned long long)(tile - j.first_tile) * per, s_end = min(slots, s0 + per);
  const uint32_t lane = threadIdx.x & 63u;
  for (unsigned long long base = s0 + (threadIdx.x & ~63u); base < s_end; base += CELL_THREADS) {  // wave-uniform
    const unsigned long long s = base + lane;
    const bool occupied = s < s_end && table[s].key != 0;
    const uint32_t cnt = occupied ? (uint32_t)table[s].best : 0u;
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    if (total == 0) continue;  // wave-uniform
    unsigned long long start = 0;
    if (lane == 0) start = atomicAdd(&cursor[ji], (unsigned long long)total);
    start = __shfl(start, 0, 64);
    if (occupied) table[s].best = (start + (incl - cnt)) << 32 | cnt;
  }
}

// Pass 3: each kept point takes the next position of its cell's run (atomicAdd on the slot's high half) and writes x, y, z
// and its index as one 16-byte record; each dropped point gets what its job's drop_row writes.
template <class Job>
__global__ void __launch_bounds__(CELL_THREADS)
    cell_scatter_kernel(const Job* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const Job& j = jobs[ji];
  const float* __restrict__ points = j.points;
  VoxelSlot* table = j.table;
  CellRecord* sorted = j.sorted;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += CELL_THREADS) {
    const f32x3 pt = *(const f32x3_u*)(points + 3 * (size_t)p);
    unsigned long long key;
    if (!voxel_key(pt, grid, &key, nullptr)) {
      j.drop_row(p);
      continue;
    }
    const unsigned long long s = find_slot(table, mask, key + 1);
    if (s == ~0ull) {  // (cannot happen: pass 1 placed every kept point)
      atomicMax(fault, 2ull);
      continue;
    }
    const unsigned long long pos = atomicAdd(&table[s].best, 1ull << 32) >> 32;
    if (pos >= len) {  // (cannot happen: the runs partition the kept points; a bound on every store)
      atomicMax(fault, 3ull);
      continue;
    }
    const f32x4 rec = {pt.x, pt.y, pt.z, __uint_as_float(p)};
    *(f32x4*)(sorted + pos) = rec;
  }
}

// The run [*begin, *end) of the records of neighbour cell c (0 ... 26) of cell (kx, ky, kz); empty if the cell lies outside
// the grid or holds nothing.  After pass 3 a slot's second word is run end << 32 | count; the run is clamped to `kept`.
__device__ __forceinline__ void cell_run(const VoxelSlot* __restrict__ table, unsigned long long mask, uint32_t kept, int kx,
                                         int ky, int kz, int c, uint32_t* begin, uint32_t* end) {
  const int nx = kx + c / 9 - 1, ny = ky + c / 3 % 3 - 1, nz = kz + c % 3 - 1;
  *begin = 0, *end = 0;
  if ((unsigned)nx < (1u << 21) && (unsigned)ny < (1u << 21) && (unsigned)nz < (1u << 21)) {
    const unsigned long long nkey = (unsigned long long)nx << 42 | (unsigned long long)ny << 21 | (unsigned long long)nz;
    const unsigned long long s = find_slot(table, mask, nkey + 1);
    if (s != ~0ull) {
      const unsigned long long word = table[s].best;
      const uint32_t cnt = (uint32_t)word;
      *end = min((uint32_t)(word >> 32), kept);
      *begin = *end >= cnt ? *end - cnt : 0u;
    }
  }
}

// consume(record) for every record of a run, AHEAD candidates a trip: their loads are issued together (the index is
// clamped into the run, only the candidates that exist are consumed), so a thread waits for memory once per AHEAD
// candidates instead of once per candidate.
template <uint32_t AHEAD, class Consume>
__device__ __forceinline__ void consume_run(const CellRecord* __restrict__ sorted, uint32_t begin, uint32_t end,
                                            Consume&& consume) {
  for (uint32_t q = begin; q < end; q += AHEAD) {
    f32x4 rec[AHEAD];
#pragma unroll
    for (uint32_t u = 0; u < AHEAD; ++u) rec[u] = *(const f32x4*)(sorted + min(q + u, end - 1));
#pragma unroll
    for (uint32_t u = 0; u < AHEAD; ++u)
      if (q + u < end) consume(rec[u]);
  }
}
#endif  // __HIPCC__

// A batch's sort as the host plans it: the tiles so far, and the two parts of the scratch tail that hold every job's hash
// table and every job's records.
struct CellSortPlan {
  uint64_t tiles = 0;
  TailPart tables, sorted;
};

// Adds a cloud of `len` points (0 < len < 2^32) of the entry point `name` to the plan and fills the job's len, tiles,
// slot mask and, as offsets inside their parts for now, table and sorted.
template <class Job>
inline a3d_status cell_sort_plan(CellSortPlan* plan, const char* name, uint64_t len, Job* j) {
  A3D_TRY(plan_job_tiles(name, len, CELL_CHUNK, CELL_MAX_TILES, &plan->tiles, j));
  j->n_tiles = (uint32_t)plan->tiles - j->first_tile;
  const uint64_t slots = table_slots(len);
  j->slot_mask = slots - 1;
  plan->tables.take(&j->table, slots * sizeof(VoxelSlot)), plan->sorted.take(&j->sorted, pad256(len * sizeof(CellRecord)));
  return A3D_OK;
}

// The job's two offsets onto the parts of the scratch tail (after place_parts).
template <class Job>
inline void cell_sort_rebase(const CellSortPlan& plan, Job* j) {
  plan.tables.rebase(&j->table), plan.sorted.rebase(&j->sorted);
}

#ifdef __HIPCC__
// The three launches, over tables that the caller has zeroed.  cursor[job] ends as the job's kept count.
template <class Job>
inline a3d_status cell_sort_launch(const Job* d_jobs, uint32_t n_jobs, uint64_t tiles, VoxelGrid grid,
                                   unsigned long long* d_cursor, unsigned long long* d_dropped, unsigned long long* d_fault,
                                   hipStream_t s) {
  const dim3 grid_dim((uint32_t)tiles), block(CELL_THREADS);
  hipLaunchKernelGGL(cell_count_kernel<Job>, grid_dim, block, 0, s, d_jobs, n_jobs, grid, d_dropped, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cell_place_kernel<Job>, grid_dim, block, 0, s, d_jobs, n_jobs, d_cursor);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cell_scatter_kernel<Job>, grid_dim, block, 0, s, d_jobs, n_jobs, grid, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  return A3D_OK;
}
#endif  // __HIPCC__

}  // namespace a3d
