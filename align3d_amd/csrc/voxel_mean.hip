// Voxel-grid downsampling of resident clouds by cell MEAN: per occupied cell of a grid of pitch v anchored at o, the
// centroid of the cell's points, the mean of their normals and the mean of their colours.  The sibling
// (voxel_downsample.hip) keeps one real sample per cell because an f32 mean depends on the summation order; here the
// offsets are rounded to a lattice and summed in int64 (the answer of cloud_normals.hip), so the mean is a rule stated in
// arithmetic: the same bits as its numpy restatement and the same bits under any permutation of the rows.
//
// The rule.  All f32 operations are rounded on their own (-ffp-contract=off, correctly rounded / and sqrt); f64
// operations likewise.  Per call: v finite and > 0, a finite origin o (default 0).  Host constants in f32:
// s = 32768.0f / v and u = v / 32768.0f.
//  1. Cell.  voxel_key of voxel_grid.hpp, unchanged.  A point it refuses is dropped and counted.
//  2. Offsets.  ctr_k = (c_k + 0.5f) * v + o_k and d_k = p_k - ctr_k, as voxel_key computes them.
//     q_k = (int) rintf(d_k * s), ties to even.  Per cell, in int64: N = sum 1 and S_k = sum q_k.  |q_k| stays near 2^14,
//     so with len < 2^32 nothing can overflow.
//  3. Mean point.  If N == 1 the cell's only row is copied bit for bit: point, normal and colour.  Otherwise
//     m_k = (float)((double)S_k / (double)N) and out_k = ctr_k + m_k * u, with ctr taken from the cell's representative
//     (step 6).
//  4. Mean normal (only when normals are written, N > 1).  A row's normal is counted iff its three components are finite
//     and |n_k| <= 2.  r_k = (int) rintf(n_k * 1048576.0f), T_k = sum r_k in int64 over the counted rows (each sum stays
//     <= 2^53: exact in f64).  L = sqrt((T_x*T_x + T_y*T_y) + T_z*T_z) in f64, out_n_k = L > 0 ? (float)((double)T_k / L)
//     : 0.  A zero normal stays in the cloud: every aligner's angle gate rejects it, as after estimate_normals.
//  5. Mean colour (only when colours are written, N > 1).  Per channel C = sum c in u64 and out_c = (2 C + N) / (2 N) in
//     integer division, which rounds half up.
//  6. Order, index, count.  A cell's representative is its lowest input index.  Output rows are in ascending order of
//     representative (first-occurrence order), out_index[row] is that index, out_counts[row] = N as u32.
//
// The kernels: a counting sort by cell (the shape of cloud_normals.hip) and a reduction of each cell's contiguous run, so
// no sum is contended and the scratch beyond the sibling's is 20 bytes per input point (a 16-byte record and a 4-byte row
// number) plus 96 bytes per 64 points, not ten words per hash slot.  One upload, one fill and six launches over every tile
// of every cloud of a batch, whatever the batch size (the job table of cloud_batch.hpp); no block waits on another block,
// and the host waits once, at the end.
//  1. vmean_count_kernel: a wave combines each run of lanes with the same key (a frame cloud is row-major: neighbouring
//     lanes often share a cell); the run's first lane claims the slot of the key (load, then 64-bit atomicCAS on key + 1;
//     the fill is zeros) and adds the run's length to the slot's count (the low half of its second word) and atomicMaxes
//     ~index into the high half: the complement of the cell's lowest index, so that zero is "none yet".
//  2. vmean_flag_kernel: a point is its cell's representative iff the slot's high half is ~its index; ballots, tile
//     counts and row totals exactly as the sibling's pass 2.
//  3. vmean_place_kernel: a thread per slot; the slot's high half becomes the start of the cell's run in the sorted
//     records (a block takes its slots' total from the job's cursor with one atomicAdd), the low half stays the count.
//  4. vmean_scatter_kernel: in input order with the sibling's pass-3 ranking.  A representative writes its record
//     (x, y, z, index) at the START of its cell's run and its output row number beside it; the others take the positions
//     start + count - 1 down to start + 1 (one atomicSub per run of lanes with the same key).
//  5. vmean_reduce_kernel: a thread per record in cell order.  A wave's segmented scan sums the lattice offsets, the
//     rounded normals and the colours of each run of equal keys.  A cell that lies inside the wave is finished there and
//     written to its row.  A cell that crosses a wave boundary adds its partial sums to the spill accumulator of the
//     64-record group in which it starts: at most one cell starts in a group and leaves it, so 12 words per 64 records
//     are enough, and a cell of N rows adds to them N / 64 times, not N times.
//  6. vmean_spill_kernel: a thread per accumulator finishes the cells that crossed.
// Passes 5 and 6 write nothing if any cloud of the batch has more rows than its capacity, and bound every store by it.
#include <cmath>
#include <vector>

#include "cell_sort.hpp"   // CellRecord, f32x4, find_slot: shared with the neighbour walks (its sort passes are not: see there)
#include "voxel_mean.hpp"  // the rule's arithmetic and the run combining: shared with voxel_map.hip (a map of means)

using namespace a3d;

namespace {

constexpr uint32_t VM_THREADS = 256;
constexpr uint32_t VM_WAVES = VM_THREADS / 64;
constexpr uint32_t VM_ROUNDS = 4;
constexpr uint32_t VM_CHUNK = VM_ROUNDS * VM_THREADS;  // points per chunk: a multiple of 64
constexpr uint32_t VM_GROUPS = VM_CHUNK / 64;          // ballot words per chunk
constexpr uint32_t VM_MAX_TILES = 4096;
static_assert(VM_GROUPS <= 64, "a wave's lanes hold the chunk's ballot words");

struct VmSpill {  // the sums of the one cell that starts in a group of 64 records and crosses its end (zero-filled)
  unsigned long long n;
  long long s[3], t[3];
  unsigned long long c[3];
  unsigned long long head;  // the position of the cell's first record + 1; 0 = no such cell
  unsigned long long pad;
};
static_assert(sizeof(VmSpill) == 96, "VmSpill layout");

// One non-empty cloud of a batch as the kernels see it (uploaded per call).
struct MeanJob {
  const float* points;
  const float* normals;   // read only when out_normals is set
  const uint8_t* colors;  // read only when out_colors is set
  float* out_points;
  float* out_normals;    // null: no normals are written
  uint8_t* out_colors;   // null: no colours are written
  uint32_t* out_index;   // null: no indices are written
  uint32_t* out_counts;  // null: no counts are written
  VoxelSlot* table;      // slot_mask + 1 slots, zeroed before the count: key word 0 = empty, else key + 1
  unsigned long long* flags;  // (len + 63) / 64 ballot words
  CellRecord* sorted;         // len records, the first `kept` of them written; a run's first record is its representative
  uint32_t* row_at;           // len row numbers, written at the first position of every run
  VmSpill* spill;             // (len + 63) / 64 accumulators, zeroed
  unsigned long long slot_mask;
  unsigned long long capacity;
  uint32_t len, first_tile, chunks_per_tile, n_tiles;
};
static_assert(sizeof(MeanJob) == 136, "MeanJob layout");

// The halves of a slot's second word (little-endian: [0] the count, [1] ~lowest index, later the run's start).
__device__ __forceinline__ uint32_t* slot_half(VoxelSlot* slot, int h) { return (uint32_t*)&slot->best + h; }

// Pass 1.  dropped[job] += dropped points (zeroed by the host upload); *fault is set if a table were ever full (it cannot
// be: it has at least two slots per point).
__global__ void __launch_bounds__(VM_THREADS)
    vmean_count_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid,
                       unsigned long long* __restrict__ dropped, unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MeanJob& j = jobs[ji];
  const float* __restrict__ points = j.points;
  VoxelSlot* table = j.table;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (len < 2^32 - span: checked by the host)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t n_dropped = 0;
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VM_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    unsigned long long key = VX_EMPTY;  // no key: a lane past the end or a dropped point
    if (p < p_end && !voxel_key(*(const f32x3_u*)(points + 3 * (size_t)p), grid, &key, nullptr)) key = VX_EMPTY, ++n_dropped;
    bool first;
    const uint64_t heads = run_heads(key, lane, &first);
    if (first && key != VX_EMPTY) {  // (no lane leaves the trip early: the next one shuffles again)
      const uint32_t run = run_end_lane(heads, lane) - lane;
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
      if (placed) {
        atomicAdd(slot_half(&table[s], 0), run);
        // (a stale value can only be smaller than the true one, so the test never skips a needed update)
        if (VX_LOAD_AGENT(slot_half(&table[s], 1)) < ~p) atomicMax(slot_half(&table[s], 1), ~p);
      } else {
        atomicMax(fault, 1ull);
      }
    }
  }
  n_dropped = wave_sum(n_dropped);
  if (lane == 0 && n_dropped) atomicAdd(&dropped[ji], (unsigned long long)n_dropped);
}

// Pass 2: flags[p / 64] bit p % 64 = point p is its cell's representative; tile_counts[tile] = representatives of the
// tile; lens[job] += the same (zeroed by the host upload).
__global__ void __launch_bounds__(VM_THREADS)
    vmean_flag_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, uint32_t* __restrict__ tile_counts,
                      unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_wave[VM_WAVES];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MeanJob& j = jobs[ji];
  const float* __restrict__ points = j.points;
  const VoxelSlot* __restrict__ table = j.table;
  unsigned long long* __restrict__ flags = j.flags;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t c = 0;  // wave-uniform
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VM_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    bool win = false;
    unsigned long long key;
    if (p < p_end && voxel_key(*(const f32x3_u*)(points + 3 * (size_t)p), grid, &key, nullptr)) {
      const unsigned long long s = find_slot(table, mask, key + 1);
      win = s != ~0ull && (uint32_t)(table[s].best >> 32) == ~p;
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(win);
    if (lane == 0) flags[base >> 6] = ballot;
    c += (uint32_t)__builtin_popcountll(ballot);
  }
  if (lane == 0) s_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (uint32_t w = 0; w < VM_WAVES; ++w) total += s_wave[w];
    tile_counts[tile] = total;
    if (total) atomicAdd(&lens[ji], (unsigned long long)total);
  }
}

// Pass 3: every occupied slot's second word = start << 32 | count, the starts handed out from cursor[job] (zeroed by the
// upload; it ends as the job's kept count).  Tile t of a job takes slots [t * per, (t + 1) * per), per = ceil(slots / tiles).
// A block walks its slots twice: first every wave sums the counts of its share, then the block takes its run of the
// cursor with ONE atomicAdd and the waves hand out the starts on the second walk (the slots are in L2 by then).  The
// cursors of a batch's jobs are neighbours in one or a few cache lines: an atomicAdd per wave and trip, as in
// cloud_normals.hip, made this pass two thirds of a call on 64 clouds.
__global__ void __launch_bounds__(VM_THREADS)
    vmean_place_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, unsigned long long* __restrict__ cursor) {
  __shared__ unsigned long long s_wave[VM_WAVES];
  __shared__ unsigned long long s_start;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MeanJob& j = jobs[ji];
  VoxelSlot* table = j.table;
  const unsigned long long slots = j.slot_mask + 1, per = (slots + j.n_tiles - 1) / j.n_tiles;
  const unsigned long long s0 = (unsigned long long)(tile - j.first_tile) * per, s_end = min(slots, s0 + per);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long mine = 0;  // the counts of this wave's slots (per lane, then summed)
  for (unsigned long long s = s0 + threadIdx.x; s < s_end; s += VM_THREADS)
    if (table[s].key != 0) mine += (uint32_t)table[s].best;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (uint32_t w = 0; w < VM_WAVES; ++w) total += s_wave[w];
    s_start = total ? atomicAdd(&cursor[ji], total) : 0ull;
  }
  __syncthreads();
  unsigned long long start = s_start;  // of this wave's first cell
  for (uint32_t w = 0; w < wave; ++w) start += s_wave[w];
  if (mine == 0) return;  // wave-uniform; no barrier follows
  for (unsigned long long base = s0 + (threadIdx.x & ~63u); base < s_end; base += VM_THREADS) {  // wave-uniform
    const unsigned long long s = base + lane;
    const bool occupied = s < s_end && table[s].key != 0;
    const uint32_t cnt = occupied ? (uint32_t)table[s].best : 0u;
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    if (occupied) table[s].best = (start + (incl - cnt)) << 32 | cnt;
    start += __shfl(incl, 63, 64);
  }
}

// Pass 4: kept points into their cells' runs, the representative first, and its row number beside it.
__global__ void __launch_bounds__(VM_THREADS)
    vmean_scatter_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid,
                         const uint32_t* __restrict__ tile_counts, unsigned long long* __restrict__ fault) {
  __shared__ uint32_t s_base;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MeanJob& j = jobs[ji];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t = tile - j.first_tile;
  if (wave == 0) {
    uint32_t s = 0;
    for (uint32_t k = lane; k < t; k += 64) s += tile_counts[j.first_tile + k];
    s = wave_sum(s);
    if (lane == 0) s_base = s;
  }
  __syncthreads();
  const float* __restrict__ points = j.points;
  const unsigned long long* __restrict__ flags = j.flags;
  VoxelSlot* table = j.table;
  CellRecord* sorted = j.sorted;
  uint32_t* row_at = j.row_at;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK, n_groups = (len + 63u) >> 6;
  const uint32_t p0 = t * span, p_end = min(len, p0 + span);
  uint32_t base = s_base;  // representatives of the cloud before this chunk
  for (uint32_t px0 = p0; px0 < p_end; px0 += VM_CHUNK) {  // block-uniform
    // lane g < VM_GROUPS of every wave holds the ballot word of the chunk's group g; their exclusive prefix gives every
    // group's offset (voxel_compact_kernel's form)
    const uint32_t g = (px0 >> 6) + lane;
    const uint64_t word = lane < VM_GROUPS && g < n_groups ? flags[g] : 0ull;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < (int)VM_GROUPS; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    const uint32_t excl = incl - cnt;
    uint64_t ballots[VM_ROUNDS];
    uint32_t offs[VM_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < VM_ROUNDS; ++r) {
      const int src = (int)(r * VM_WAVES + wave);
      ballots[r] = (uint64_t)__shfl((unsigned long long)word, src, 64);
      offs[r] = base + __shfl(excl, src, 64);
    }
    base += __shfl(incl, (int)VM_GROUPS - 1, 64);
#pragma unroll
    for (uint32_t r = 0; r < VM_ROUNDS; ++r) {  // (every lane of the wave goes through every round: the shuffles below)
      const uint64_t ballot = ballots[r];
      const uint32_t p = px0 + r * VM_THREADS + threadIdx.x;
      const bool rep = (ballot >> lane) & 1ull;
      f32x3 pt = {0.f, 0.f, 0.f};
      unsigned long long key = VX_EMPTY;
      if (p < p_end) {
        pt = *(const f32x3_u*)(points + 3 * (size_t)p);
        if (!voxel_key(pt, grid, &key, nullptr)) key = VX_EMPTY;
      }
      bool first;
      const uint64_t heads = run_heads(key, lane, &first);
      const uint32_t first_lane = run_first_lane(heads, lane), end_lane = run_end_lane(heads, lane);
      // the lanes of this run that are not the representative, and how many of them are below this lane
      const uint64_t run_mask = (end_lane == 64u ? ~0ull : (1ull << end_lane) - 1ull) & (~0ull << first_lane);
      const uint64_t others = run_mask & ~ballot;
      const uint32_t n_others = (uint32_t)__builtin_popcountll(others);
      const uint32_t below = (uint32_t)__builtin_popcountll(others & ((1ull << lane) - 1ull));
      uint32_t start = 0, old = 0;
      if (first && key != VX_EMPTY) {
        const unsigned long long s = find_slot(table, mask, key + 1);
        if (s == ~0ull) {  // (cannot happen: pass 1 placed every kept point)
          atomicMax(fault, 2ull);
          start = ~0u;
        } else {
          start = (uint32_t)(table[s].best >> 32);  // (nothing writes the high half in this pass)
          if (n_others) old = atomicSub(slot_half(&table[s], 0), n_others);
        }
      }
      start = __shfl(start, (int)first_lane, 64), old = __shfl(old, (int)first_lane, 64);
      if (key != VX_EMPTY && start != ~0u) {
        // the representative at the run's start; the others at start + count - 1 ... start + 1, in any order
        const unsigned long long pos = rep ? (unsigned long long)start : (unsigned long long)start + old - 1u - below;
        if (pos >= len || (!rep && old < n_others + 1u)) {  // (cannot happen: the runs partition the kept points; a bound on every store)
          atomicMax(fault, 3ull);
        } else {
          const f32x4 rec = {pt.x, pt.y, pt.z, __uint_as_float(p)};
          *(f32x4*)(sorted + pos) = rec;
          if (rep) row_at[pos] = offs[r] + lane_rank(ballot);
        }
      }
    }
  }
}

// Steps 3 to 6 for one cell: `rec` is its representative, the sums are the whole cell's.
__device__ __forceinline__ void vmean_finish(const MeanJob& j, VoxelGrid grid, float u, unsigned long long row, f32x4 rec,
                                             unsigned long long n, const long long* s, const long long* t,
                                             const unsigned long long* c) {
  if (row >= j.capacity) return;  // (cannot happen: the rows are fewer than lens <= capacity; a bound on every store)
  const uint32_t index = __float_as_uint(rec.w);
  f32x3 out = {rec.x, rec.y, rec.z};
  if (n == 1) {
    *(f32x3_u*)(j.out_points + 3 * row) = out;
    if (j.out_normals) *(f32x3_u*)(j.out_normals + 3 * row) = *(const f32x3_u*)(j.normals + 3 * (size_t)index);
    if (j.out_colors) store_color(j.out_colors, row, load_color(j.colors, index));
  } else {
    const float cx = floorf((rec.x - grid.ox) / grid.v), cy = floorf((rec.y - grid.oy) / grid.v),
                cz = floorf((rec.z - grid.oz) / grid.v);
    *(f32x3_u*)(j.out_points + 3 * row) = vmean_point(cx, cy, cz, grid, u, n, s);
    if (j.out_normals) *(f32x3_u*)(j.out_normals + 3 * row) = vmean_normal(t);
    if (j.out_colors) store_color(j.out_colors, row, vmean_color(n, c));
  }
  if (j.out_index) j.out_index[row] = index;
  if (j.out_counts) j.out_counts[row] = (uint32_t)n;
}

// Whether any cloud of the batch has more rows than its capacity (then nothing is written anywhere); wave 0 decides.
__device__ __forceinline__ bool vmean_any_over(const MeanJob* __restrict__ jobs, uint32_t n_jobs,
                                               const unsigned long long* __restrict__ lens, uint32_t* s_over) {
  if (threadIdx.x < 64u) {
    bool over = false;
    for (uint32_t k = threadIdx.x; k < n_jobs; k += 64) over |= lens[k] > jobs[k].capacity;
    const bool any_over = __builtin_amdgcn_ballot_w64(over) != 0ull;
    if (threadIdx.x == 0) *s_over = any_over ? 1u : 0u;
  }
  __syncthreads();
  return *s_over != 0u;
}

// Pass 5.
__global__ void __launch_bounds__(VM_THREADS)
    vmean_reduce_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, MeanParams prm,
                        const unsigned long long* __restrict__ cursor, const unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_over;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  if (vmean_any_over(jobs, n_jobs, lens, &s_over)) return;
  const MeanJob& j = jobs[ji];
  const CellRecord* __restrict__ sorted = j.sorted;
  const float* __restrict__ normals = j.out_normals ? j.normals : nullptr;
  const uint8_t* __restrict__ colors = j.out_colors ? j.colors : nullptr;
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t kept = (uint32_t)min(cursor[ji], (unsigned long long)len);
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(kept, p0 + span);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VM_THREADS) {  // wave-uniform; base is a multiple of 64
    const uint32_t pos = base + lane;
    const bool live = pos < p_end;
    f32x4 rec = {0.f, 0.f, 0.f, 0.f};
    unsigned long long key = VX_EMPTY;
    VmSums a{};
    if (live) {
      rec = *(const f32x4*)(sorted + pos);
      const f32x3 pt = {rec.x, rec.y, rec.z};
      if (!voxel_key(pt, grid, &key, nullptr)) key = VX_EMPTY;  // (a record is a kept point: never refused)
      a.n = 1;
      vmean_offsets(pt, grid, prm.s, a.s);
      const uint32_t index = __float_as_uint(rec.w);
      if (normals) vmean_round_normal(*(const f32x3_u*)(normals + 3 * (size_t)index), a.t);
      if (colors) {
        const uint32_t rgb = load_color(colors, index);
        a.c[0] = rgb & 255u, a.c[1] = (rgb >> 8) & 255u, a.c[2] = (rgb >> 16) & 255u;
      }
    }
    // whether the cell of lane 0 starts before this wave, and whether the cell of lane 63 goes on after it
    bool open_left = false, open_right = false;
    if (lane == 0 && pos > 0) {
      const f32x4 before = *(const f32x4*)(sorted + (pos - 1));
      const f32x3 pb = {before.x, before.y, before.z};
      unsigned long long kb = VX_EMPTY;
      voxel_key(pb, grid, &kb, nullptr);
      open_left = kb == key;
    }
    if (lane == 63 && live && pos + 1u < kept) {
      const f32x4 after = *(const f32x4*)(sorted + (pos + 1));
      const f32x3 pa = {after.x, after.y, after.z};
      unsigned long long ka = VX_EMPTY;
      voxel_key(pa, grid, &ka, nullptr);
      open_right = ka == key;
    }
    open_left = __builtin_amdgcn_ballot_w64(open_left) != 0ull;
    bool first;
    const uint64_t heads = run_heads(key, lane, &first);
    const uint32_t first_lane = run_first_lane(heads, lane), end_lane = run_end_lane(heads, lane);
    vmean_scan_runs(a, lane, first_lane);  // a run's last lane ends with the run's sums
    // the run's first record, for its last lane
    f32x4 head;
    head.x = __shfl(rec.x, (int)first_lane, 64), head.y = __shfl(rec.y, (int)first_lane, 64);
    head.z = __shfl(rec.z, (int)first_lane, 64), head.w = __shfl(rec.w, (int)first_lane, 64);
    if (live && end_lane == lane + 1u) {  // the run's last lane (no lane leaves the trip early: the next one shuffles again)
      const long long s64[3] = {a.s[0], a.s[1], a.s[2]}, t64[3] = {a.t[0], a.t[1], a.t[2]};
      const unsigned long long c64[3] = {a.c[0], a.c[1], a.c[2]};
      const bool from_before = first_lane == 0 && open_left;
      if (!from_before && !open_right) {  // (open_right is lane 63's alone)
        vmean_finish(j, grid, prm.u, j.row_at[base + first_lane], head, a.n, s64, t64, c64);
      } else {
        const unsigned long long slot = find_slot(j.table, j.slot_mask, key + 1);
        // (a missing slot or a start past the end cannot happen; a bound on the accumulator's index)
        const uint32_t start = slot == ~0ull ? len : (uint32_t)(j.table[slot].best >> 32);
        if (start < len) {
          VmSpill* acc = j.spill + (start >> 6);
          atomicAdd(&acc->n, (unsigned long long)a.n);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (s64[k]) atomicAdd((unsigned long long*)&acc->s[k], (unsigned long long)s64[k]);
            if (t64[k]) atomicAdd((unsigned long long*)&acc->t[k], (unsigned long long)t64[k]);
            if (c64[k]) atomicAdd(&acc->c[k], c64[k]);
          }
          if (!from_before) acc->head = (unsigned long long)start + 1ull;  // the part that holds the cell's first record
        }
      }
    }
  }
}

// Pass 6: a thread per accumulator.
__global__ void __launch_bounds__(VM_THREADS)
    vmean_spill_kernel(const MeanJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, MeanParams prm,
                       const unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_over;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  if (vmean_any_over(jobs, n_jobs, lens, &s_over)) return;
  const MeanJob& j = jobs[ji];
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK, n_groups = (len + 63u) >> 6;
  const uint32_t g0 = (tile - j.first_tile) * (span >> 6), g_end = min(n_groups, g0 + (span >> 6));
  for (uint32_t g = g0 + threadIdx.x; g < g_end; g += VM_THREADS) {
    const VmSpill acc = j.spill[g];
    if (acc.head == 0 || acc.head > len) continue;
    const unsigned long long pos = acc.head - 1;
    vmean_finish(j, grid, prm.u, j.row_at[pos], *(const f32x4*)(j.sorted + pos), acc.n, acc.s, acc.t, acc.c);
  }
}

}  // namespace

extern "C" {

a3d_status a3d_point_clouds_voxel_mean_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                              const uint8_t* const* d_colors, uint64_t n, float voxel_size,
                                              const float origin[3], float* const* d_out_points,
                                              float* const* d_out_normals, uint8_t* const* d_out_colors,
                                              uint32_t* const* d_out_index, uint32_t* const* d_out_counts,
                                              const uint64_t* capacities, uint64_t* out_lens, uint64_t* out_dropped) {
  if (n == 0) return A3D_OK;
  static const char NAME[] = "a3d_point_clouds_voxel_mean_device";
  if (!(ctx && d_clouds && d_out_points && capacities && out_lens)) return refuse(A3D_INVALID_PARAMETER, NAME, "null argument");
  VoxelGrid grid;
  A3D_TRY(voxel_grid_from(NAME, voxel_size, origin, &grid));
  const MeanParams prm = voxel_mean_params(voxel_size);
  const CompactArgs args{d_clouds, d_colors, d_out_points, d_out_normals, d_out_colors, d_out_index, capacities};
  std::vector<MeanJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(8 * n);
  uint64_t tiles = 0;
  TailPart flags, rows, sorted, tables, spill;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = d_clouds[i].len;
    if (len >= (1ull << 32)) return refuse(A3D_INVALID_PARAMETER, NAME, "a cloud of 2^32 points or more");
    if (len == 0) continue;  // yields no points; its pointers may be null
    MeanJob j{};
    A3D_TRY(compact_front(NAME, args, i, true, "null points or output pointer", VM_CHUNK, VM_MAX_TILES, &tiles, &ranges, &j));
    j.n_tiles = (uint32_t)tiles - j.first_tile;
    j.out_counts = d_out_counts ? d_out_counts[i] : nullptr;
    ranges.out(j.out_counts, std::min<uint64_t>(len, j.capacity) * 4);
    const uint64_t slots = table_slots(len);
    j.slot_mask = slots - 1;
    const size_t groups = (len + 63) / 64;
    flags.take(&j.flags, pad256(groups * 8)), rows.take(&j.row_at, pad256(len * 4));
    sorted.take(&j.sorted, pad256(len * sizeof(CellRecord))), tables.take(&j.table, slots * sizeof(VoxelSlot));
    spill.take(&j.spill, pad256(groups * sizeof(VmSpill)));
    jobs.push_back(j), cloud_of_job.push_back(i);
  }
  if (ranges.overlap())
    return refuse(A3D_INVALID_PARAMETER, NAME, "an output overlaps an input or another output (there is no in-place form)");
  zero_results(out_lens, n), zero_results(out_dropped, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // the words: lens, dropped, cursor, fault; the tail: ballot words | row numbers | records | hash tables | accumulators
  BatchScratch scratch;
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(MeanJob), 3 * n_jobs + 1, tiles,
                        flags.bytes + rows.bytes + sorted.bytes + tables.bytes + spill.bytes, &scratch));
  place_parts(scratch.tail, {&flags, &rows, &sorted, &tables, &spill});
  for (MeanJob& j : jobs) {
    flags.rebase(&j.flags), rows.rebase(&j.row_at), sorted.rebase(&j.sorted);
    tables.rebase(&j.table), spill.rebase(&j.spill);
  }
  const MeanJob* d_jobs = (const MeanJob*)scratch.jobs;
  unsigned long long* d_lens = scratch.words;
  unsigned long long* d_dropped = d_lens + n_jobs;
  unsigned long long* d_cursor = d_lens + 2 * n_jobs;
  unsigned long long* d_fault = d_lens + 3 * n_jobs;
  uint32_t* d_tile_counts = scratch.tile_counts;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  A3D_HIP_TRY(hipMemsetAsync(tables.base, 0, tables.bytes + spill.bytes, s));  // every slot empty, every accumulator zero
  const dim3 grid_dim((uint32_t)tiles), block(VM_THREADS);
  hipLaunchKernelGGL(vmean_count_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, d_dropped, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vmean_flag_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, d_tile_counts, d_lens);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vmean_place_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, d_cursor);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vmean_scatter_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid,
                     (const uint32_t*)d_tile_counts, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vmean_reduce_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, prm,
                     (const unsigned long long*)d_cursor, (const unsigned long long*)d_lens);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vmean_spill_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, prm,
                     (const unsigned long long*)d_lens);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_lens, 3 * n_jobs + 1, s, &words));
  A3D_REQUIRE(words[3 * n_jobs] == 0, A3D_HIP_ERROR, "a3d_point_clouds_voxel_mean_device: a hash table filled up");
  return compact_finish(NAME, "rows", jobs, cloud_of_job, words.data(), out_lens, out_dropped);
}

}  // extern "C"
