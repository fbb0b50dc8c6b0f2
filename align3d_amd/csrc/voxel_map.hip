// A persistent voxel map: the hash table of the voxel-grid downsample (voxel_downsample.hip) kept between calls, so that
// resident clouds go in frame by frame.  After any sequence of inserts the map's contents equal merge(all inserted clouds
// under their poses, in insertion order) followed by voxel_downsample(v, origin): points, normals, order and winner
// indices, however the inserts were grouped into calls and whatever the table's size history was.  The downsample's rule
// is a pure minimum per key of bits(dist) << 32 | index (voxel_grid.hpp), and a minimum over a union is the minimum of
// the minima as long as `index` is the point's position in the merged cloud: point i of cloud j of a call gets
// seq = total + sum(len[0..j)) + i, where total counts every point ever offered, dropped ones included.
//
// State (one device block per table size, from the context's block pool): slots x VoxelSlot {key, best} | slots x 3 f32
// points | slots x 3 f32 normals (maps with normals) | slots x u32 colours (maps with colours) | one 64-bit count of
// occupied slots.  The payload is held BY SLOT in arrays of its own: a probe touches 16-byte slots only, and a winner's
// row has a fixed home that a later, better point simply overwrites, so there is no free list and nothing to compact
// between calls.  A colour is a payload like the normal: it never enters a key, a distance or a pose.  By slot it is
// packed r | g << 8 | b << 16 into one aligned dword (a winner's colour is one 4-byte store, a move of the table one
// 4-byte copy); a cloud's rows are [3] u8 without alignment, so the commit pass packs and the extract's last pass unpacks.
//
// Insert, two launches over every tile of every cloud of the call (the job table of cloud_batch.hpp), no block waits on
// another block, no LDS:
//  A. voxel_map_insert_kernel: a thread per point transforms it in registers (transform_vector of devmath.hpp, what
//     cloud_transform.hip calls), computes voxel_key, claims the key's slot (load before CAS) and atomicMins its word into
//     `best` (load before min), exactly as voxel_insert_kernel.  The threads whose CAS claimed an empty slot add themselves
//     to the cell count (one atomicAdd per wave).
//  B. voxel_map_commit_kernel: each kept point finds its slot again; iff the slot's low 32 bits of `best` are its seq it
//     is the final winner (unique per slot) and writes its transformed point and normal into the slot's row.  It cannot
//     be part of A: a thread whose atomicMin succeeded is not yet the final winner.
// The table never fills: before launching, the host makes sure slots >= 2 * (cells + L), L the points of the call, growing
// to the next sufficient power of two with one rehash launch over the old slots (keys are unique: only the claim is
// contended).  The `fault` word of the downsample stays as a guard.
//
// Extract writes the occupied slots' rows in ascending seq, the order voxel_downsample gives on the merged cloud (slot
// order depends on which colliding key claimed first, i.e. on timing): a bitmap of `total` bits in scratch, set per
// occupied slot (32-bit atomicOr), counted per tile, turned into one exclusive prefix per 64-bit word, and a last pass over
// the slots writes each row to prefix(word of seq) + popcount(lower bits of the word).
//
// Retain rebuilds the table from the cells that pass a rule (seq >= min_seq, row inside a box) and numbers the survivors
// 0 ... k-1 in their old order; afterwards the map is a new map into which the surviving rows went as one cloud without
// a pose.  That holds because a slot's row is the very f32 point its key and bits(dist) were computed from: the key and
// the distance half of `best` are kept, and only the seq half is replaced by the survivor's rank.  (Reading the map as a
// spatial index — nearest row, frame-to-map ICP — lives in voxel_map_icp.hip; the map's struct in voxel_map.hpp.)  Five launches,
// whatever the sizes: the extract's mark pass with the rule, its count and prefix passes unchanged, a thread per mark
// (callers' sequence numbers translated to the new numbering; `total` is translated too, which gives k), and a pass
// over the old slots that claims every survivor's key in a NEW table (the growth rehash with a renumbered `best`).  The
// new table's slot count follows from k, which the host learns only at the call's one wait: the block is sized for
// every old cell, the rebuild derives slots and the arrays' places from k on the device, and the host derives the same
// after the wait.  The old table is only read, so a failure of any kind leaves the map as it was.
//
// A map of MEANS (a3d_voxel_map_new_mean) keeps the cell-mean rule of voxel_mean.hip as running sums: per slot, in
// planes of their own behind the colours, a 64-bit count N, the three int64 sums of the lattice offsets, the three int64
// sums of the rounded normals (maps with normals), the three u64 sums of the colours (maps with colours) and a 32-bit
// epoch word.  Every term is an integer, so the atomic adds of any grouping of the inserts end in the same sums, and the
// finish arithmetic (voxel_mean.hpp, shared with the batch call) gives the batch call's bits.  `best` holds the cell's
// lowest seq with a distance half of zero.  The insert is again two launches over every tile of every cloud:
//  A. voxel_map_sum_kernel: a wave combines each run of lanes with the same key (segmented scan, vmean_scan_runs); the
//     run's last lane claims the slot, atomicMins the run's first seq into `best` and adds the run's sums to the slot's
//     with no-return 64-bit atomics (a term that is zero is not sent).
//  B. voxel_map_finish_kernel: the first lane of every run finds its slot and atomicMaxes the call's number into the
//     slot's epoch word; the one thread per cell that raises it reads the final sums and writes the cell's row: its own
//     raw row if N == 1, else steps 3 to 5 with ctr from the key's cell numbers.  So the row planes hold the rule's
//     output for every touched cell when the call's work is done, the readers (extract, nearest, align, render, retain)
//     read them as before, and the cost follows the call's points, never the slot count.
// Growth and retain move N and the sums with the row (the epoch words of a new table are zero: every call's number is
// above).  A retain of a map of means is six launches: one more, ahead of the rebuild, zeroes the sum planes of the new
// table, whose place follows from k.  The nearest-point kernels are the same code as before: the mode is a template
// parameter of the bodies they share with the mean forms.
#include <cmath>
#include <vector>

#include "voxel_map.hpp"
#include "voxel_mean.hpp"

using namespace a3d;

namespace {

constexpr uint32_t VM_THREADS = 256;
constexpr uint32_t VM_WAVES = VM_THREADS / 64;
constexpr uint32_t VM_CHUNK = 4 * VM_THREADS;  // points per chunk of an insert tile, as the downsample's
constexpr uint32_t VM_MAX_TILES = 4096;        // tiles per cloud (insert) / per bitmap (extract) at most
constexpr uint64_t VM_SEQ_MARGIN = 1ull << 21;  // above any tile span (a cloud has < 2^32 points: <= 1024 chunks per tile)
constexpr uint32_t VM_MAX_SLOT_BLOCKS = 1u << 20;  // grid of the passes over the slots (grid-stride beyond)
constexpr uint32_t VM_NO_SLOT = ~0u;

// One non-empty cloud of a call as the kernels see it (uploaded per call).
struct MapJob {
  const float* points;
  const float* normals;  // read only by maps with normals
  uint32_t len, first_tile, chunks_per_tile, has_pose;
  uint32_t seq0;  // sequence number of the cloud's point 0
  Pose pose;
  const uint8_t* colors;  // [len][3] u8, read only by maps with colours
};
static_assert(sizeof(MapJob) == 72, "MapJob layout");

struct MapTable {
  VoxelSlot* table;
  float* points;   // [slots][3]
  float* normals;  // [slots][3] or null
  uint32_t* colors;  // [slots] packed, or null
  unsigned long long mask;  // slots - 1
  unsigned long long* cell_count;
};

__device__ __forceinline__ f32x3 world_point(const MapJob& j, uint32_t p) {
  const f32x3 pt = *(const f32x3_u*)(j.points + 3 * (size_t)p);
  if (!j.has_pose) return pt;  // verbatim, as the merge without poses
  const V3 v = transform_vector(j.pose, V3{pt.x, pt.y, pt.z});
  return f32x3{v.x, v.y, v.z};
}

__device__ __forceinline__ f32x3 world_normal(const MapJob& j, uint32_t p) {
  const f32x3 nv = *(const f32x3_u*)(j.normals + 3 * (size_t)p);
  if (!j.has_pose) return nv;
  const V3 w = transform_normal(j.pose, V3{nv.x, nv.y, nv.z});
  return f32x3{w.x, w.y, w.z};
}

// The planes a map of means keeps beside MapTable's (all null in a nearest-point map).
struct MeanPlanes {
  unsigned long long* n;  // [slots] points of the cell
  long long* s;           // [slots][3] lattice sums
  long long* t;           // [slots][3] sums of the rounded normals, or null
  unsigned long long* c;  // [slots][3] colour sums, or null
  uint32_t* epoch;        // [slots] the number of the last insert call that finished the cell's row
};

// The slot that holds `key`, or ~0 (the walk stops at the first empty slot).
__device__ __forceinline__ unsigned long long find_key(const VoxelSlot* __restrict__ table, unsigned long long mask,
                                                       unsigned long long key) {
  unsigned long long s = slot_hash(key) & mask;
  for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
    const unsigned long long k = table[s].key;
    if (k == key) return s;
    if (k == VX_EMPTY) break;
  }
  return ~0ull;
}

// The slot that holds `key`, claimed if no slot does yet (*claimed); false = the table is full (it cannot be).
__device__ __forceinline__ bool claim_slot(VoxelSlot* table, unsigned long long mask, unsigned long long key,
                                           unsigned long long* slot, bool* claimed) {
  unsigned long long s = slot_hash(key) & mask;
  for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
    unsigned long long k = VX_LOAD_AGENT(&table[s].key);
    if (k == VX_EMPTY) {
      k = atomicCAS(&table[s].key, VX_EMPTY, key);
      if (k == VX_EMPTY) *claimed = true;
    }
    if (k == VX_EMPTY || k == key) {
      *slot = s;
      return true;
    }
  }
  return false;
}

// Pass A.  dropped[job] += dropped points (zeroed by the host upload); *fault is set if the table were ever full.
// STORE_SLOT (diagnostics build): slot_of[seq - seq_base] = the point's slot, VM_NO_SLOT for a dropped point.
template <bool STORE_SLOT>
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_insert_kernel(const MapJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, MapTable m,
                            unsigned long long* __restrict__ dropped, unsigned long long* __restrict__ fault,
                            uint32_t* __restrict__ slot_of, uint32_t seq_base) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MapJob& j = jobs[ji];
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (total + L < 2^32 - span: checked by the host)
  uint32_t n_dropped = 0, n_claimed = 0;
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += VM_THREADS) {
    const f32x3 pt = world_point(j, p);
    const uint32_t seq = j.seq0 + p;
    unsigned long long key, s;
    float dist;
    if (!voxel_key(pt, grid, &key, &dist)) {
      ++n_dropped;
      if (STORE_SLOT) slot_of[seq - seq_base] = VM_NO_SLOT;
      continue;
    }
    bool claimed = false;
    if (!claim_slot(m.table, m.mask, key, &s, &claimed)) {
      atomicMax(fault, 1ull);
      if (STORE_SLOT) slot_of[seq - seq_base] = VM_NO_SLOT;
      continue;
    }
    n_claimed += claimed ? 1u : 0u;
    const unsigned long long word = (unsigned long long)__float_as_uint(dist) << 32 | seq;
    if (VX_LOAD_AGENT(&m.table[s].best) > word) atomicMin(&m.table[s].best, word);
    if (STORE_SLOT) slot_of[seq - seq_base] = (uint32_t)s;
  }
  n_dropped = wave_sum(n_dropped), n_claimed = wave_sum(n_claimed);
  if ((threadIdx.x & 63u) == 0) {
    if (n_dropped) atomicAdd(&dropped[ji], (unsigned long long)n_dropped);
    if (n_claimed) atomicAdd(m.cell_count, (unsigned long long)n_claimed);
  }
}

// Pass B: the final winner of a slot writes the slot's row.
template <bool STORED_SLOT>
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_commit_kernel(const MapJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, MapTable m,
                            const uint32_t* __restrict__ slot_of, uint32_t seq_base) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MapJob& j = jobs[ji];
  const VoxelSlot* __restrict__ table = m.table;
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += VM_THREADS) {
    const uint32_t seq = j.seq0 + p;
    unsigned long long s = 0;
    bool found = false;
    f32x3 pt;
    if (STORED_SLOT) {
      const uint32_t stored = slot_of[seq - seq_base];
      if (stored == VM_NO_SLOT) continue;
      s = stored, found = true;
      pt = world_point(j, p);
    } else {
      pt = world_point(j, p);
      unsigned long long key;
      if (!voxel_key(pt, grid, &key, nullptr)) continue;
      s = slot_hash(key) & m.mask;
      for (unsigned long long tries = 0; tries <= m.mask; ++tries, s = (s + 1) & m.mask) {
        const unsigned long long k = table[s].key;
        if (k == key) {
          found = true;
          break;
        }
        if (k == VX_EMPTY) break;  // (cannot happen: pass A placed every kept point)
      }
    }
    if (!found || s > m.mask || (uint32_t)table[s].best != seq) continue;  // (a bound on every store)
    *(f32x3_u*)(m.points + 3 * (size_t)s) = pt;
    if (m.normals) {
      f32x3 nv = *(const f32x3_u*)(j.normals + 3 * (size_t)p);
      if (j.has_pose) {
        const V3 w = transform_normal(j.pose, V3{nv.x, nv.y, nv.z});
        nv = f32x3{w.x, w.y, w.z};
      }
      *(f32x3_u*)(m.normals + 3 * (size_t)s) = nv;
    }
    if (m.colors) m.colors[s] = load_color(j.colors, p);
  }
}

// Mean pass A.  COMBINE = false (diagnostics build): every lane is a run of its own, to show what combining buys.
template <bool COMBINE>
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_sum_kernel(const MapJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, float lattice, MapTable m,
                         MeanPlanes mp, unsigned long long* __restrict__ dropped, unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MapJob& j = jobs[ji];
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (total + L < 2^32 - span: checked by the host)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t n_dropped = 0, n_claimed = 0;
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VM_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    unsigned long long key = VX_EMPTY;  // no key: a lane past the end or a dropped point
    VmSums a{};
    if (p < p_end) {
      const f32x3 pt = world_point(j, p);
      if (voxel_key(pt, grid, &key, nullptr)) {
        a.n = 1;
        vmean_offsets(pt, grid, lattice, a.s);
        if (mp.t) vmean_round_normal(world_normal(j, p), a.t);
        if (mp.c) {
          const uint32_t rgb = load_color(j.colors, p);
          a.c[0] = rgb & 255u, a.c[1] = (rgb >> 8) & 255u, a.c[2] = (rgb >> 16) & 255u;
        }
      } else {
        key = VX_EMPTY, ++n_dropped;
      }
    }
    uint32_t first_lane = lane, end_lane = lane + 1u;
    if (COMBINE) {
      bool first;
      const uint64_t heads = run_heads(key, lane, &first);
      first_lane = run_first_lane(heads, lane), end_lane = run_end_lane(heads, lane);
      vmean_scan_runs(a, lane, first_lane);
    }
    if (key != VX_EMPTY && end_lane == lane + 1u) {  // the run's last lane (no lane leaves the trip early: the next one shuffles again)
      unsigned long long s;
      bool claimed = false;
      if (!claim_slot(m.table, m.mask, key, &s, &claimed)) {
        atomicMax(fault, 1ull);
      } else {
        n_claimed += claimed ? 1u : 0u;
        const unsigned long long word = j.seq0 + base + first_lane;  // the run's lowest seq; the distance half is zero
        if (VX_LOAD_AGENT(&m.table[s].best) > word) atomicMin(&m.table[s].best, word);
        atomicAdd(&mp.n[s], (unsigned long long)a.n);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (a.s[k]) atomicAdd((unsigned long long*)&mp.s[3 * s + k], (unsigned long long)a.s[k]);
          if (mp.t && a.t[k]) atomicAdd((unsigned long long*)&mp.t[3 * s + k], (unsigned long long)(long long)a.t[k]);
          if (mp.c && a.c[k]) atomicAdd(&mp.c[3 * s + k], (unsigned long long)a.c[k]);
        }
      }
    }
  }
  n_dropped = wave_sum(n_dropped), n_claimed = wave_sum(n_claimed);
  if (lane == 0) {
    if (n_dropped) atomicAdd(&dropped[ji], (unsigned long long)n_dropped);
    if (n_claimed) atomicAdd(m.cell_count, (unsigned long long)n_claimed);
  }
}

// Steps 3 to 5 for the cell of slot `s`, whose sums are final; `raw_*`: the only row of a cell with N == 1.
__device__ __forceinline__ void finish_slot(const MapTable& m, const MeanPlanes& mp, VoxelGrid grid, float u,
                                            unsigned long long s, unsigned long long key, f32x3 raw_point, f32x3 raw_normal,
                                            uint32_t raw_color) {
  const unsigned long long n = mp.n[s];
  f32x3 point = raw_point, normal = raw_normal;
  uint32_t color = raw_color;
  if (n != 1) {
    const float cx = (float)((int)(key >> 42) - (1 << 20)), cy = (float)((int)((key >> 21) & 0x1FFFFFull) - (1 << 20)),
                cz = (float)((int)(key & 0x1FFFFFull) - (1 << 20));  // the integers voxel_key's floorf gave
    const long long sum_s[3] = {mp.s[3 * s], mp.s[3 * s + 1], mp.s[3 * s + 2]};
    point = vmean_point(cx, cy, cz, grid, u, n, sum_s);
    if (mp.t) {
      const long long sum_t[3] = {mp.t[3 * s], mp.t[3 * s + 1], mp.t[3 * s + 2]};
      normal = vmean_normal(sum_t);
    }
    if (mp.c) {
      const unsigned long long sum_c[3] = {mp.c[3 * s], mp.c[3 * s + 1], mp.c[3 * s + 2]};
      color = vmean_color(n, sum_c);
    }
  }
  *(f32x3_u*)(m.points + 3 * (size_t)s) = point;
  if (m.normals) *(f32x3_u*)(m.normals + 3 * (size_t)s) = normal;
  if (m.colors) m.colors[s] = color;
}

// Mean pass B: one thread per touched cell, the one that raises the slot's epoch word to the call's number, writes the
// cell's row from the final sums.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_finish_kernel(const MapJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, float u, MapTable m,
                            MeanPlanes mp, uint32_t epoch_no) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const MapJob& j = jobs[ji];
  const uint32_t len = j.len, span = j.chunks_per_tile * VM_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VM_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    unsigned long long key = VX_EMPTY;
    f32x3 pt = {0.f, 0.f, 0.f};
    if (p < p_end) {
      pt = world_point(j, p);
      if (!voxel_key(pt, grid, &key, nullptr)) key = VX_EMPTY;
    }
    bool first;
    run_heads(key, lane, &first);
    if (first && key != VX_EMPTY) {  // (no lane leaves the trip early: the next one shuffles again)
      const unsigned long long s = find_key(m.table, m.mask, key);
      // (a missing slot cannot happen: pass A placed every kept point; a bound on every store)
      if (s <= m.mask && VX_LOAD_AGENT(&mp.epoch[s]) < epoch_no && atomicMax(&mp.epoch[s], epoch_no) < epoch_no) {
        // (a cell with N == 1 holds this very point: it is the cell's only one)
        const f32x3 zero = {0.f, 0.f, 0.f};
        finish_slot(m, mp, grid, u, s, key, pt, m.normals ? world_normal(j, p) : zero,
                    m.colors ? load_color(j.colors, p) : 0u);
      }
    }
  }
}

// N and the sums of slot `o` of one table into slot `s` of another (the epoch word stays zero).
__device__ __forceinline__ void move_sums(const MeanPlanes& mp, unsigned long long s, const MeanPlanes& old_mp,
                                          unsigned long long o) {
  mp.n[s] = old_mp.n[o];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mp.s[3 * s + k] = old_mp.s[3 * o + k];
    if (mp.t) mp.t[3 * s + k] = old_mp.t[3 * o + k];
    if (mp.c) mp.c[3 * s + k] = old_mp.c[3 * o + k];
  }
}

// The body of both growth passes.  MEAN: N and the sums move with the row.
template <bool MEAN>
__device__ __forceinline__ void rehash_slots(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                                             const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                                             unsigned long long old_slots, const MapTable& m, const MeanPlanes& old_mp,
                                             const MeanPlanes& mp, unsigned long long* __restrict__ fault) {
  uint32_t n_claimed = 0;
  for (unsigned long long o = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; o < old_slots;
       o += (unsigned long long)gridDim.x * VM_THREADS) {
    const unsigned long long key = old_table[o].key;
    if (key == VX_EMPTY) continue;
    unsigned long long s;
    bool claimed = false;
    if (!claim_slot(m.table, m.mask, key, &s, &claimed) || !claimed) {  // (keys are unique: the slot is always a fresh claim)
      atomicMax(fault, 1ull);
      continue;
    }
    ++n_claimed;
    m.table[s].best = old_table[o].best;
    *(f32x3_u*)(m.points + 3 * (size_t)s) = *(const f32x3_u*)(old_points + 3 * (size_t)o);
    if (m.normals) *(f32x3_u*)(m.normals + 3 * (size_t)s) = *(const f32x3_u*)(old_normals + 3 * (size_t)o);
    if (m.colors) m.colors[s] = old_colors[o];
    if (MEAN) move_sums(mp, s, old_mp, o);
  }
  n_claimed = wave_sum(n_claimed);
  if ((threadIdx.x & 63u) == 0 && n_claimed) atomicAdd(m.cell_count, (unsigned long long)n_claimed);
}

// Growth: every occupied slot of the old table into the new one (key, best, row); counts the new table's cells.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_rehash_kernel(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                            const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                            unsigned long long old_slots, MapTable m, unsigned long long* __restrict__ fault) {
  rehash_slots<false>(old_table, old_points, old_normals, old_colors, old_slots, m, MeanPlanes{}, MeanPlanes{}, fault);
}

// Growth of a map of means.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_rehash_mean_kernel(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                                 const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                                 unsigned long long old_slots, MapTable m, MeanPlanes old_mp, MeanPlanes mp,
                                 unsigned long long* __restrict__ fault) {
  rehash_slots<true>(old_table, old_points, old_normals, old_colors, old_slots, m, old_mp, mp, fault);
}

// The survival rule of a retain: seq >= min_seq and lo <= row <= hi per axis, plain f32 compares on the stored bits (no
// box: -inf / +inf, which every stored row passes: a kept point is finite).
struct RetainRule {
  uint32_t min_seq;  // min(min_seq, total)
  float lo[3], hi[3];
};

// The body of both mark passes.  RETAIN: only the slots that pass the rule.
template <bool RETAIN>
__device__ __forceinline__ void mark_slots(const VoxelSlot* __restrict__ table, const float* __restrict__ points,
                                           unsigned long long slots, uint32_t* __restrict__ bitmap32,
                                           unsigned long long total, const RetainRule& rule) {
  for (unsigned long long s = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; s < slots;
       s += (unsigned long long)gridDim.x * VM_THREADS) {
    if (table[s].key == VX_EMPTY) continue;
    const uint32_t seq = (uint32_t)table[s].best;
    if (RETAIN) {
      if (seq < rule.min_seq) continue;
      const f32x3 p = *(const f32x3_u*)(points + 3 * (size_t)s);
      if (!(p.x >= rule.lo[0] && p.x <= rule.hi[0] && p.y >= rule.lo[1] && p.y <= rule.hi[1] && p.z >= rule.lo[2] &&
            p.z <= rule.hi[2]))
        continue;
    }
    if (seq < total) atomicOr(&bitmap32[seq >> 5], 1u << (seq & 31u));
  }
}

// Extract 1: bit seq of the bitmap for every occupied slot (32-bit halves of the 64-bit words, little endian).
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_mark_kernel(const VoxelSlot* __restrict__ table, unsigned long long slots, uint32_t* __restrict__ bitmap32,
                          unsigned long long total) {
  mark_slots<false>(table, nullptr, slots, bitmap32, total, RetainRule{});
}

// Retain 1: bit seq of the bitmap for every occupied slot that survives.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_mark_retained_kernel(const VoxelSlot* __restrict__ table, const float* __restrict__ points,
                                   unsigned long long slots, uint32_t* __restrict__ bitmap32, unsigned long long total,
                                   RetainRule rule) {
  mark_slots<true>(table, points, slots, bitmap32, total, rule);
}

// Extract 2: tile_counts[tile] = set bits of the tile's words (a tile: chunks_per_tile * VM_THREADS 64-bit words).
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_count_kernel(const unsigned long long* __restrict__ bitmap, uint32_t n_words, uint32_t chunks_per_tile,
                           uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_wave[VM_WAVES];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t w0 = (uint64_t)tile * chunks_per_tile * VM_THREADS;
  const uint64_t w_end = min((uint64_t)n_words, w0 + (uint64_t)chunks_per_tile * VM_THREADS);
  uint32_t c = 0;
  for (uint64_t w = w0 + threadIdx.x; w < w_end; w += VM_THREADS) c += (uint32_t)__builtin_popcountll(bitmap[w]);
  c = wave_sum(c);
  if (lane == 0) s_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < VM_WAVES; ++w) sum += s_wave[w];
    tile_counts[tile] = sum;
  }
}

// Extract 3: word_prefix[w] = set bits of all words before w.  A block sums the earlier tiles' counts for its base
// (cloud_write_kernel's form: at most VM_MAX_TILES tiles) and scans its own words chunk by chunk.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_prefix_kernel(const unsigned long long* __restrict__ bitmap, uint32_t n_words, uint32_t chunks_per_tile,
                            const uint32_t* __restrict__ tile_counts, uint32_t* __restrict__ word_prefix) {
  __shared__ uint32_t s_base, s_wave[VM_WAVES];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave == 0) {
    uint32_t s = 0;
    for (uint32_t k = lane; k < tile; k += 64) s += tile_counts[k];
    s = wave_sum(s);
    if (lane == 0) s_base = s;
  }
  __syncthreads();
  uint32_t base = s_base;
  const uint64_t w0 = (uint64_t)tile * chunks_per_tile * VM_THREADS;
  const uint64_t w_end = min((uint64_t)n_words, w0 + (uint64_t)chunks_per_tile * VM_THREADS);
  for (uint64_t c0 = w0; c0 < w_end; c0 += VM_THREADS) {  // block-uniform
    const uint64_t w = c0 + threadIdx.x;
    const uint32_t cnt = w < w_end ? (uint32_t)__builtin_popcountll(bitmap[w]) : 0u;
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < VM_WAVES; ++k) {
      const uint32_t t = s_wave[k];
      before += k < wave ? t : 0u;
      all += t;
    }
    if (w < w_end) word_prefix[w] = base + before + incl - cnt;
    base += all;
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
}

// The body of both write passes.  COUNTS: out_counts[row] = the cell's N as u32, saturating.
template <bool COUNTS>
__device__ __forceinline__ void write_rows(const VoxelSlot* __restrict__ table, const float* __restrict__ points,
                                           const float* __restrict__ normals, const uint32_t* __restrict__ colors,
                                           unsigned long long slots, const unsigned long long* __restrict__ bitmap,
                                           const uint32_t* __restrict__ word_prefix, unsigned long long total,
                                           unsigned long long rows, float* __restrict__ out_points,
                                           float* __restrict__ out_normals, uint32_t* __restrict__ out_index,
                                           uint8_t* __restrict__ out_colors, const unsigned long long* __restrict__ sum_n,
                                           uint32_t* __restrict__ out_counts) {
  for (unsigned long long s = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; s < slots;
       s += (unsigned long long)gridDim.x * VM_THREADS) {
    if (table[s].key == VX_EMPTY) continue;
    const uint32_t seq = (uint32_t)table[s].best;
    if (seq >= total) continue;  // (cannot happen: every occupied slot holds the seq of an offered point)
    const uint32_t w = seq >> 6;
    const unsigned long long dst =
        (unsigned long long)word_prefix[w] + (unsigned long long)__builtin_popcountll(bitmap[w] & ((1ull << (seq & 63u)) - 1ull));
    if (dst >= rows) continue;  // (cannot happen: rows = the occupied slots; a bound on every store)
    *(f32x3_u*)(out_points + 3 * dst) = *(const f32x3_u*)(points + 3 * (size_t)s);
    if (out_normals) *(f32x3_u*)(out_normals + 3 * dst) = *(const f32x3_u*)(normals + 3 * (size_t)s);
    if (out_index) out_index[dst] = seq;
    if (out_colors) store_color(out_colors, dst, colors[s]);  // (dst < rows: the last byte written is 3 * rows - 1)
    if (COUNTS) out_counts[dst] = (uint32_t)min(sum_n[s], 0xFFFFFFFFull);
  }
}

// Extract 4: every occupied slot's row to its rank among the set bits: ascending seq.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_write_kernel(const VoxelSlot* __restrict__ table, const float* __restrict__ points,
                           const float* __restrict__ normals, const uint32_t* __restrict__ colors,
                           unsigned long long slots, const unsigned long long* __restrict__ bitmap,
                           const uint32_t* __restrict__ word_prefix, unsigned long long total, unsigned long long rows,
                           float* __restrict__ out_points, float* __restrict__ out_normals, uint32_t* __restrict__ out_index,
                           uint8_t* __restrict__ out_colors) {
  write_rows<false>(table, points, normals, colors, slots, bitmap, word_prefix, total, rows, out_points, out_normals,
                    out_index, out_colors, nullptr, nullptr);
}

// Extract 4 of a map of means with the cells' counts.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_write_counts_kernel(const VoxelSlot* __restrict__ table, const float* __restrict__ points,
                                  const float* __restrict__ normals, const uint32_t* __restrict__ colors,
                                  unsigned long long slots, const unsigned long long* __restrict__ bitmap,
                                  const uint32_t* __restrict__ word_prefix, unsigned long long total,
                                  unsigned long long rows, float* __restrict__ out_points, float* __restrict__ out_normals,
                                  uint32_t* __restrict__ out_index, uint8_t* __restrict__ out_colors,
                                  const unsigned long long* __restrict__ sum_n, uint32_t* __restrict__ out_counts) {
  write_rows<true>(table, points, normals, colors, slots, bitmap, word_prefix, total, rows, out_points, out_normals,
                   out_index, out_colors, sum_n, out_counts);
}

// The set bits below bit `m` of the bitmap, m <= total.  m = total with total a multiple of 64 names the word one past
// the last: it is answered from the last word.
__device__ __forceinline__ unsigned long long rank_below(const unsigned long long* __restrict__ bitmap,
                                                         const uint32_t* __restrict__ word_prefix, uint32_t n_words,
                                                         unsigned long long m) {
  const bool past = (m >> 6) >= n_words;
  const unsigned long long w = past ? n_words - 1 : m >> 6;
  const unsigned long long below = past ? ~0ull : (1ull << (m & 63u)) - 1ull;
  return (unsigned long long)word_prefix[w] + (unsigned long long)__builtin_popcountll(bitmap[w] & below);
}

// Retain 4: out[i] = survivors whose old seq is below marks[i], a thread per mark.  The host appends `total` as the last
// mark: its answer is k, the number of survivors, which retain 5 reads from out[n - 1].
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_marks_kernel(const unsigned long long* __restrict__ bitmap, const uint32_t* __restrict__ word_prefix,
                           uint32_t n_words, unsigned long long total, const unsigned long long* __restrict__ marks,
                           unsigned long long n, unsigned long long* __restrict__ out) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * VM_THREADS)
    out[i] = rank_below(bitmap, word_prefix, n_words, min(marks[i], total));
}

// A table of `slots` slots inside a block: slots | point rows | normal rows | packed colours, as ensure_slots lays them
// out (a plane the map does not keep takes no room: the next one starts where it would).
// A map of means goes on behind them: counts | lattice sums | normal sums | colour sums | epoch words (sums_at ... end,
// one stretch that is zero in an empty table).  In a nearest-point map sums_at == end and nothing is added.
struct TableLayout {
  size_t points_at, normals_at, colors_at, sums_at, s_at, t_at, c_at, epoch_at, end;
};
__host__ __device__ __forceinline__ TableLayout table_layout(unsigned long long slots, bool with_normals, bool with_colors,
                                                             bool mean) {
  const size_t table_bytes = ((size_t)slots * sizeof(VoxelSlot) + 255) & ~(size_t)255;
  const size_t row_bytes = ((size_t)slots * 12 + 255) & ~(size_t)255;
  const size_t color_bytes = ((size_t)slots * 4 + 255) & ~(size_t)255;
  const size_t colors_at = table_bytes + row_bytes * (with_normals ? 2 : 1);
  TableLayout lay{};
  lay.points_at = table_bytes, lay.normals_at = table_bytes + row_bytes, lay.colors_at = colors_at;
  lay.sums_at = colors_at + (with_colors ? color_bytes : 0);
  const size_t count_bytes = ((size_t)slots * 8 + 255) & ~(size_t)255, sum_bytes = ((size_t)slots * 24 + 255) & ~(size_t)255;
  lay.s_at = lay.sums_at + (mean ? count_bytes : 0);
  lay.t_at = lay.s_at + (mean ? sum_bytes : 0);
  lay.c_at = lay.t_at + (mean && with_normals ? sum_bytes : 0);
  lay.epoch_at = lay.c_at + (mean && with_colors ? sum_bytes : 0);
  lay.end = lay.epoch_at + (mean ? color_bytes : 0);
  return lay;
}
// The planes of a table of `slots` slots at `base`.
struct PlacedTable {
  MapTable m;
  MeanPlanes mp;
};
__host__ __device__ __forceinline__ PlacedTable place_table(char* base, unsigned long long slots, bool with_normals,
                                                            bool with_colors, bool mean, unsigned long long* cell_count) {
  const TableLayout lay = table_layout(slots, with_normals, with_colors, mean);
  PlacedTable t{};
  t.m = MapTable{(VoxelSlot*)base, (float*)(base + lay.points_at), with_normals ? (float*)(base + lay.normals_at) : nullptr,
                 with_colors ? (uint32_t*)(base + lay.colors_at) : nullptr, slots - 1, cell_count};
  if (mean)
    t.mp = MeanPlanes{(unsigned long long*)(base + lay.sums_at), (long long*)(base + lay.s_at),
                      with_normals ? (long long*)(base + lay.t_at) : nullptr,
                      with_colors ? (unsigned long long*)(base + lay.c_at) : nullptr, (uint32_t*)(base + lay.epoch_at)};
  return t;
}
// The slots of a map of k > 0 retained cells: the smallest power of two >= max(2 k, min_slots), min_slots the power of two
// of an empty map (max(2 * reserve_cells, 64)).  Host and device evaluate it alike.
__host__ __device__ __forceinline__ unsigned long long retained_slots(unsigned long long k, unsigned long long min_slots) {
  unsigned long long slots = min_slots;
  while (slots < 2 * k) slots <<= 1;
  return slots;
}

// Retain 5: every surviving slot of the old table (its bit is set: a seq belongs to one slot) into the new one under
// its rank among the survivors, the new seq; the distance half of `best` stays.  The new table's size follows from k,
// which only the device knows yet: the block has room for max_slots (the size for every old cell) and its first
// max_slots slots are VX_EMPTY.  Counts the new table's cells.
// MEAN: N and the sums move with the row (the new table's sum planes were zeroed by voxel_map_zero_sums_kernel).
template <bool MEAN>
__device__ __forceinline__ void rebuild_slots(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                                              const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                                              unsigned long long old_slots, const unsigned long long* __restrict__ bitmap,
                                              const uint32_t* __restrict__ word_prefix, unsigned long long total,
                                              const unsigned long long* __restrict__ k_word, char* new_base,
                                              unsigned long long min_slots, unsigned long long max_slots,
                                              uint32_t with_normals, uint32_t with_colors,
                                              unsigned long long* __restrict__ cell_count,
                                              unsigned long long* __restrict__ fault, const MeanPlanes& old_mp) {
  const unsigned long long k = *k_word;
  if (2 * k > max_slots) {  // (cannot happen: k <= the old cells; a bound on every store below)
    if (threadIdx.x == 0) atomicMax(fault, 1ull);
    return;
  }
  const unsigned long long slots = retained_slots(k, min_slots);  // <= max_slots
  const PlacedTable placed = place_table(new_base, slots, with_normals != 0, with_colors != 0, MEAN, cell_count);
  const MapTable& m = placed.m;
  uint32_t n_claimed = 0;
  for (unsigned long long o = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; o < old_slots;
       o += (unsigned long long)gridDim.x * VM_THREADS) {
    const unsigned long long key = old_table[o].key;
    if (key == VX_EMPTY) continue;
    const unsigned long long best = old_table[o].best;
    const uint32_t seq = (uint32_t)best;
    if (seq >= total) continue;  // (cannot happen, as in the extract)
    const unsigned long long bits = bitmap[seq >> 6];
    if (!(bits >> (seq & 63u) & 1ull)) continue;  // removed
    const unsigned long long new_seq =
        (unsigned long long)word_prefix[seq >> 6] + (unsigned long long)__builtin_popcountll(bits & ((1ull << (seq & 63u)) - 1ull));
    unsigned long long s;
    bool claimed = false;
    if (new_seq >= k || !claim_slot(m.table, m.mask, key, &s, &claimed) || !claimed) {  // (keys are unique: a fresh claim)
      atomicMax(fault, 1ull);
      continue;
    }
    ++n_claimed;
    m.table[s].best = (best & 0xFFFFFFFF00000000ull) | new_seq;
    *(f32x3_u*)(m.points + 3 * (size_t)s) = *(const f32x3_u*)(old_points + 3 * (size_t)o);
    if (m.normals) *(f32x3_u*)(m.normals + 3 * (size_t)s) = *(const f32x3_u*)(old_normals + 3 * (size_t)o);
    if (m.colors) m.colors[s] = old_colors[o];
    if (MEAN) move_sums(placed.mp, s, old_mp, o);
  }
  n_claimed = wave_sum(n_claimed);
  if ((threadIdx.x & 63u) == 0 && n_claimed) atomicAdd(m.cell_count, (unsigned long long)n_claimed);
}

__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_rebuild_kernel(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                             const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                             unsigned long long old_slots, const unsigned long long* __restrict__ bitmap,
                             const uint32_t* __restrict__ word_prefix, unsigned long long total,
                             const unsigned long long* __restrict__ k_word, char* new_base, unsigned long long min_slots,
                             unsigned long long max_slots, uint32_t with_normals, uint32_t with_colors,
                             unsigned long long* __restrict__ cell_count, unsigned long long* __restrict__ fault) {
  rebuild_slots<false>(old_table, old_points, old_normals, old_colors, old_slots, bitmap, word_prefix, total, k_word, new_base,
                       min_slots, max_slots, with_normals, with_colors, cell_count, fault, MeanPlanes{});
}

// Retain 5 of a map of means.
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_rebuild_mean_kernel(const VoxelSlot* __restrict__ old_table, const float* __restrict__ old_points,
                                  const float* __restrict__ old_normals, const uint32_t* __restrict__ old_colors,
                                  unsigned long long old_slots, const unsigned long long* __restrict__ bitmap,
                                  const uint32_t* __restrict__ word_prefix, unsigned long long total,
                                  const unsigned long long* __restrict__ k_word, char* new_base,
                                  unsigned long long min_slots, unsigned long long max_slots, uint32_t with_normals,
                                  uint32_t with_colors, unsigned long long* __restrict__ cell_count,
                                  unsigned long long* __restrict__ fault, MeanPlanes old_mp) {
  rebuild_slots<true>(old_table, old_points, old_normals, old_colors, old_slots, bitmap, word_prefix, total, k_word, new_base,
                      min_slots, max_slots, with_normals, with_colors, cell_count, fault, old_mp);
}

// Retain of a map of means, ahead of the rebuild: zeroes the sum planes of the new table, whose place follows from k
// (it may lie inside the stretch that the host filled with VX_EMPTY for max_slots slots).
__global__ void __launch_bounds__(VM_THREADS)
    voxel_map_zero_sums_kernel(const unsigned long long* __restrict__ k_word, char* new_base, unsigned long long min_slots,
                               unsigned long long max_slots, uint32_t with_normals, uint32_t with_colors) {
  const unsigned long long k = *k_word;
  if (2 * k > max_slots) return;  // (cannot happen; the rebuild reports it)
  const TableLayout lay = table_layout(retained_slots(k, min_slots), with_normals != 0, with_colors != 0, true);
  unsigned long long* words = (unsigned long long*)(new_base + lay.sums_at);
  const unsigned long long n_words = (lay.end - lay.sums_at) / 8;  // (every plane is a multiple of 256 bytes)
  for (unsigned long long w = (unsigned long long)blockIdx.x * VM_THREADS + threadIdx.x; w < n_words;
       w += (unsigned long long)gridDim.x * VM_THREADS)
    words[w] = 0ull;
}

uint32_t slot_blocks(uint64_t slots) {
  return (uint32_t)std::min<uint64_t>((slots + VM_THREADS - 1) / VM_THREADS, VM_MAX_SLOT_BLOCKS);
}

MapTable table_of(const a3d_voxel_map* m) {
  return MapTable{m->table, m->points, m->normals, m->colors, m->slots - 1, m->cell_count};
}
MeanPlanes planes_of(const a3d_voxel_map* m) { return MeanPlanes{m->sum_n, m->sum_s, m->sum_t, m->sum_c, m->epoch}; }

// The map's table is from now on the one of `slots` slots at the start of `block`.
void adopt_table(a3d_voxel_map* m, void* block, size_t block_bytes, uint64_t slots, unsigned long long* cell_count) {
  const PlacedTable t = place_table((char*)block, slots, m->with_normals, m->with_colors, m->mean, cell_count);
  m->block = block, m->block_bytes = block_bytes, m->slots = slots;
  m->table = t.m.table, m->points = t.m.points, m->normals = t.m.normals, m->colors = t.m.colors;
  m->cell_count = cell_count;
  m->sum_n = t.mp.n, m->sum_s = t.mp.s, m->sum_t = t.mp.t, m->sum_c = t.mp.c, m->epoch = t.mp.epoch;
}

// Makes sure the table has at least 2 * (cells + incoming) slots; `fault` is the call's guard word in scratch.
a3d_status ensure_slots(a3d_voxel_map* m, uint64_t incoming, unsigned long long* d_fault) {
  if (m->block && m->slots >= 2 * (m->cells + incoming)) return A3D_OK;
  const uint64_t slots = table_slots(std::max<uint64_t>(m->cells + incoming, m->reserve_cells), 64);
  a3d_context* ctx = m->ctx;
  const TableLayout lay = table_layout(slots, m->with_normals, m->with_colors, m->mean);
  const size_t bytes = lay.end + 256;
  void* block = nullptr;
  size_t block_bytes = 0;
  A3D_TRY(ctx_block_alloc(ctx, bytes, &block, &block_bytes));
  char* base = (char*)block;
  a3d_voxel_map old = *m;
  adopt_table(m, block, block_bytes, slots, (unsigned long long*)(base + bytes - 256));
  hipStream_t s = ctx->stream;
  hipError_t e = hipMemsetAsync(m->table, 0xFF, slots * sizeof(VoxelSlot), s);  // every key VX_EMPTY, every best word ~0
  if (e == hipSuccess) e = hipMemsetAsync(m->cell_count, 0, 8, s);
  if (e == hipSuccess && m->mean) e = hipMemsetAsync(base + lay.sums_at, 0, lay.end - lay.sums_at, s);
  if (e == hipSuccess && old.block && old.cells) {
    if (m->mean)
      hipLaunchKernelGGL(voxel_map_rehash_mean_kernel, dim3(slot_blocks(old.slots)), dim3(VM_THREADS), 0, s,
                         (const VoxelSlot*)old.table, (const float*)old.points, (const float*)old.normals,
                         (const uint32_t*)old.colors, (unsigned long long)old.slots, table_of(m), planes_of(&old),
                         planes_of(m), d_fault);
    else
      hipLaunchKernelGGL(voxel_map_rehash_kernel, dim3(slot_blocks(old.slots)), dim3(VM_THREADS), 0, s,
                         (const VoxelSlot*)old.table, (const float*)old.points, (const float*)old.normals,
                         (const uint32_t*)old.colors, (unsigned long long)old.slots, table_of(m), d_fault);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {  // the old table stays the map's
    (void)hipStreamSynchronize(s);
    ctx_block_release(ctx, block, block_bytes);
    *m = old;
    set_error("a3d_voxel_map_insert: growing the table failed: %s", hipGetErrorString(e));
    return A3D_HIP_ERROR;
  }
  if (old.block) {
    ++m->growths;
    ctx_block_release(ctx, old.block, old.block_bytes);  // reuse is ordered on the context's stream, behind the rehash
  }
  return A3D_OK;
}

bool no_combine_setting() {
  const char* env = A3D_DIAG_ENV("A3D_VOXEL_MAP_MEAN_NO_COMBINE");  // diagnostics build: mean pass A without run combining
  return env && *env == '1';
}

bool stored_slot_setting() {
  const char* env = A3D_DIAG_ENV("A3D_VOXEL_MAP_STORED_SLOT");  // diagnostics build: the pass-B form the probe times
  return env && *env == '1';
}

}  // namespace

extern "C" {

a3d_status a3d_voxel_map_new_rgb(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                                 int with_colors, uint64_t reserve_cells, a3d_voxel_map** out) {
  A3D_REQUIRE(ctx && out, A3D_INVALID_PARAMETER, "null argument");
  VoxelGrid grid;
  A3D_TRY(voxel_grid_from("a3d_voxel_map_new", voxel_size, origin, &grid));
  A3D_REQUIRE(reserve_cells < (1ull << 32), A3D_INVALID_PARAMETER, "a3d_voxel_map_new: a reservation of 2^32 cells or more");
  a3d_voxel_map* m = new a3d_voxel_map();
  m->ctx = ctx, m->grid = grid, m->with_normals = with_normals != 0, m->with_colors = with_colors != 0;
  m->reserve_cells = reserve_cells;
  *out = m;  // the table is allocated by the first insert that holds a point
  return A3D_OK;
}

a3d_status a3d_voxel_map_new(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                             uint64_t reserve_cells, a3d_voxel_map** out) {
  return a3d_voxel_map_new_rgb(ctx, voxel_size, origin, with_normals, 0, reserve_cells, out);
}

a3d_status a3d_voxel_map_new_mean(a3d_context* ctx, float voxel_size, const float origin[3], int with_normals,
                                  int with_colors, uint64_t reserve_cells, a3d_voxel_map** out) {
  A3D_TRY(a3d_voxel_map_new_rgb(ctx, voxel_size, origin, with_normals, with_colors, reserve_cells, out));
  (*out)->mean = true;
  return A3D_OK;
}

a3d_status a3d_voxel_map_insert_rgb(a3d_voxel_map* map, const a3d_point_cloud_view* d_clouds, const uint8_t* const* d_colors,
                                    const a3d_pose* poses_host, uint64_t n, uint64_t* out_dropped, uint64_t* out_cells) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(map && d_clouds, A3D_INVALID_PARAMETER, "null argument");
  std::vector<MapJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  jobs.reserve(n), cloud_of_job.reserve(n);
  uint64_t tiles = 0, incoming = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    A3D_REQUIRE(c.len < (1ull << 32), A3D_INVALID_PARAMETER, "a cloud of 2^32 points or more");
    if (c.len == 0) continue;  // offers no points; its pointers may be null
    A3D_REQUIRE(c.points, A3D_INVALID_PARAMETER, "null points pointer");
    A3D_REQUIRE(!map->with_normals || c.normals, A3D_MISSING_FIELD,
                "a3d_voxel_map_insert: the map has normals and a cloud has none (nothing was inserted)");
    const uint8_t* colors = map->with_colors && d_colors ? d_colors[i] : nullptr;
    A3D_REQUIRE(!map->with_colors || colors, A3D_MISSING_FIELD,
                "a3d_voxel_map_insert: the map has colours and a cloud has none (nothing was inserted)");
    // (a sum of < 2^32 terms below 2^32 cannot wrap 64 bits; the limit below bounds it)
    A3D_REQUIRE(map->total + incoming + c.len + VM_SEQ_MARGIN < (1ull << 32), A3D_INVALID_PARAMETER,
                "a3d_voxel_map_insert: the map would pass 2^32 - 2^21 offered points (a3d_voxel_map_retain renumbers it)");
    MapJob j{};
    j.points = c.points, j.normals = map->with_normals ? c.normals : nullptr;
    j.colors = colors;
    j.len = (uint32_t)c.len;
    j.seq0 = (uint32_t)(map->total + incoming);
    if (poses_host) j.has_pose = 1, j.pose = pose_from_c(&poses_host[i]);
    A3D_TRY(plan_tiles(c.len, VM_CHUNK, VM_MAX_TILES, &tiles, &j.first_tile, &j.chunks_per_tile));
    incoming += c.len;
    jobs.push_back(j), cloud_of_job.push_back(i);
  }
  zero_results(out_dropped, n);
  if (jobs.empty()) {
    if (out_cells) *out_cells = map->cells;
    return A3D_OK;
  }
  a3d_context* ctx = map->ctx;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  const bool want_stored = !map->mean && stored_slot_setting();
  BatchScratch scratch;  // the words: dropped per job, fault; the tail: the per-point slots of the stored-slot form
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(MapJob), n_jobs + 1, 0, want_stored ? incoming * 4 : 0, &scratch));
  const MapJob* d_jobs = (const MapJob*)scratch.jobs;
  unsigned long long* d_dropped = scratch.words;
  unsigned long long* d_fault = d_dropped + n_jobs;
  uint32_t* d_slot_of = (uint32_t*)scratch.tail;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));  // (before a rehash: it zeroes the fault word)
  A3D_TRY(ensure_slots(map, incoming, d_fault));
  const MapTable table = table_of(map);
  const bool stored = want_stored && map->slots <= (1ull << 31);  // (a slot fits the 32-bit word, VM_NO_SLOT apart)
  const dim3 grid_dim((uint32_t)tiles), block(VM_THREADS);
  const uint32_t seq_base = (uint32_t)map->total;
  if (map->mean) {
    if (++map->epoch_no == 0) {  // the call numbers wrapped: every epoch word starts again below them
      A3D_HIP_TRY(hipMemsetAsync(map->epoch, 0, map->slots * 4, s));
      map->epoch_no = 1;
    }
    const MeanParams prm = voxel_mean_params(map->grid.v);
    const MeanPlanes planes = planes_of(map);
#ifdef A3D_DIAGNOSTICS
    if (no_combine_setting())
      hipLaunchKernelGGL(voxel_map_sum_kernel<false>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, prm.s, table,
                         planes, d_dropped, d_fault);
    else
#endif
      hipLaunchKernelGGL(voxel_map_sum_kernel<true>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, prm.s, table,
                         planes, d_dropped, d_fault);
    A3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(voxel_map_finish_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, prm.u, table,
                       planes, map->epoch_no);
  } else
#ifdef A3D_DIAGNOSTICS  // (the product library holds the one form it launches)
  if (stored) {
    hipLaunchKernelGGL(voxel_map_insert_kernel<true>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, table,
                       d_dropped, d_fault, d_slot_of, seq_base);
    A3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(voxel_map_commit_kernel<true>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, table,
                       (const uint32_t*)d_slot_of, seq_base);
  } else
#endif
  {
    hipLaunchKernelGGL(voxel_map_insert_kernel<false>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, table,
                       d_dropped, d_fault, d_slot_of, seq_base);
    A3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(voxel_map_commit_kernel<false>, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, map->grid, table,
                       (const uint32_t*)d_slot_of, seq_base);
  }
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words(n_jobs + 1);
  unsigned long long cells = 0;
  A3D_HIP_TRY(hipMemcpyAsync(words.data(), d_dropped, words.size() * 8, hipMemcpyDeviceToHost, s));
  A3D_HIP_TRY(hipMemcpyAsync(&cells, map->cell_count, 8, hipMemcpyDeviceToHost, s));
  // host-synchronous, the one wait of the call: the caller may free the inputs right after
  A3D_HIP_TRY(hipStreamSynchronize(s));
  map->cells = cells, map->total += incoming;
  for (size_t k = 0; k < n_jobs; ++k) {
    map->dropped_total += words[k];
    if (out_dropped) out_dropped[cloud_of_job[k]] = words[k];
  }
  if (out_cells) *out_cells = map->cells;
  A3D_REQUIRE(words[n_jobs] == 0, A3D_HIP_ERROR, "a3d_voxel_map_insert: the hash table filled up");
  return A3D_OK;
}

a3d_status a3d_voxel_map_insert(a3d_voxel_map* map, const a3d_point_cloud_view* d_clouds, const a3d_pose* poses_host,
                                uint64_t n, uint64_t* out_dropped, uint64_t* out_cells) {
  return a3d_voxel_map_insert_rgb(map, d_clouds, nullptr, poses_host, n, out_dropped, out_cells);
}

a3d_status a3d_voxel_map_extract_mean(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                      uint32_t* d_out_index, uint32_t* d_out_counts, uint64_t capacity, uint64_t* out_len) {
  A3D_REQUIRE(map && d_out_points && out_len, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(!d_out_counts || map->mean, A3D_INVALID_PARAMETER,
              "a3d_voxel_map_extract_mean: a nearest-point map keeps no counts (a3d_voxel_map_new_mean makes a map of means)");
  A3D_REQUIRE(!d_out_normals || map->with_normals, A3D_MISSING_FIELD, "a3d_voxel_map_extract: the map has no normals");
  A3D_REQUIRE(!d_out_colors || map->with_colors, A3D_MISSING_FIELD, "a3d_voxel_map_extract: the map has no colours");
  {  // the outputs as the caller declared them: `capacity` rows each (no map has 2^32 cells)
    const uint64_t rows = std::min<uint64_t>(capacity, 1ull << 32);
    RangeRecorder ranges;
    ranges.out(d_out_points, rows * 12), ranges.out(d_out_normals, rows * 12), ranges.out(d_out_index, rows * 4);
    ranges.out(d_out_colors, rows * 3), ranges.out(d_out_counts, rows * 4);
    A3D_REQUIRE(!ranges.overlap(), A3D_INVALID_PARAMETER, "a3d_voxel_map_extract: the outputs overlap one another");
  }
  *out_len = map->cells;
  if (capacity < map->cells) {
    set_error("a3d_voxel_map_extract: capacity %llu is smaller than the map's %llu cells (nothing was written)",
              (unsigned long long)capacity, (unsigned long long)map->cells);
    return A3D_INVALID_PARAMETER;
  }
  if (map->cells == 0) return A3D_OK;
  a3d_context* ctx = map->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // scratch: one count per tile | the bitmap of `total` bits | one prefix per 64-bit word of it
  const uint64_t n_words = (map->total + 63) / 64;  // < 2^26
  uint64_t tiles = 0;
  uint32_t first_tile = 0, chunks_per_tile = 0;
  A3D_TRY(plan_tiles(n_words, VM_THREADS, VM_MAX_TILES, &tiles, &first_tile, &chunks_per_tile));
  const size_t counts_bytes = pad256(tiles * 4), bitmap_bytes = pad256(n_words * 8), prefix_bytes = pad256(n_words * 4);
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 3, counts_bytes + bitmap_bytes + prefix_bytes, &region));
  uint32_t* d_tile_counts = (uint32_t*)region;
  unsigned long long* d_bitmap = (unsigned long long*)((char*)region + counts_bytes);
  uint32_t* d_prefix = (uint32_t*)((char*)region + counts_bytes + bitmap_bytes);
  hipStream_t s = ctx->stream;
  A3D_HIP_TRY(hipMemsetAsync(d_bitmap, 0, bitmap_bytes, s));
  const dim3 over_slots(slot_blocks(map->slots)), over_words((uint32_t)tiles), block(VM_THREADS);
  hipLaunchKernelGGL(voxel_map_mark_kernel, over_slots, block, 0, s, (const VoxelSlot*)map->table,
                     (unsigned long long)map->slots, (uint32_t*)d_bitmap, (unsigned long long)map->total);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(voxel_map_count_kernel, over_words, block, 0, s, (const unsigned long long*)d_bitmap, (uint32_t)n_words,
                     chunks_per_tile, d_tile_counts);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(voxel_map_prefix_kernel, over_words, block, 0, s, (const unsigned long long*)d_bitmap, (uint32_t)n_words,
                     chunks_per_tile, (const uint32_t*)d_tile_counts, d_prefix);
  A3D_HIP_TRY(hipGetLastError());
  if (d_out_counts)
    hipLaunchKernelGGL(voxel_map_write_counts_kernel, over_slots, block, 0, s, (const VoxelSlot*)map->table,
                       (const float*)map->points, (const float*)map->normals, (const uint32_t*)map->colors,
                       (unsigned long long)map->slots, (const unsigned long long*)d_bitmap, (const uint32_t*)d_prefix,
                       (unsigned long long)map->total, (unsigned long long)map->cells, d_out_points, d_out_normals,
                       d_out_index, d_out_colors, (const unsigned long long*)map->sum_n, d_out_counts);
  else
    hipLaunchKernelGGL(voxel_map_write_kernel, over_slots, block, 0, s, (const VoxelSlot*)map->table, (const float*)map->points,
                       (const float*)map->normals, (const uint32_t*)map->colors, (unsigned long long)map->slots,
                       (const unsigned long long*)d_bitmap, (const uint32_t*)d_prefix, (unsigned long long)map->total,
                       (unsigned long long)map->cells, d_out_points, d_out_normals, d_out_index, d_out_colors);
  A3D_HIP_TRY(hipGetLastError());
  // host-synchronous: the caller may read or free the outputs right after
  A3D_HIP_TRY(hipStreamSynchronize(s));
  return A3D_OK;
}

a3d_status a3d_voxel_map_extract_rgb(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint8_t* d_out_colors,
                                     uint32_t* d_out_index, uint64_t capacity, uint64_t* out_len) {
  return a3d_voxel_map_extract_mean(map, d_out_points, d_out_normals, d_out_colors, d_out_index, nullptr, capacity, out_len);
}

a3d_status a3d_voxel_map_extract(a3d_voxel_map* map, float* d_out_points, float* d_out_normals, uint32_t* d_out_index,
                                 uint64_t capacity, uint64_t* out_len) {
  return a3d_voxel_map_extract_rgb(map, d_out_points, d_out_normals, nullptr, d_out_index, capacity, out_len);
}

a3d_status a3d_voxel_map_retain(a3d_voxel_map* map, const float box_min[3], const float box_max[3], uint64_t min_seq,
                                const uint64_t* marks, uint64_t n_marks, uint64_t* out_marks, uint64_t* out_removed) {
  A3D_REQUIRE(map, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE((box_min == nullptr) == (box_max == nullptr), A3D_INVALID_PARAMETER,
              "a3d_voxel_map_retain: box_min and box_max are both NULL or both given");
  A3D_REQUIRE(n_marks == 0 || (marks && out_marks), A3D_INVALID_PARAMETER, "a3d_voxel_map_retain: marks without an array");
  A3D_REQUIRE(n_marks < (1ull << 32), A3D_INVALID_PARAMETER, "a3d_voxel_map_retain: 2^32 marks or more");
  RetainRule rule{};
  for (int a = 0; a < 3; ++a) {
    rule.lo[a] = box_min ? box_min[a] : -INFINITY, rule.hi[a] = box_max ? box_max[a] : INFINITY;
    A3D_REQUIRE(!std::isnan(rule.lo[a]) && !std::isnan(rule.hi[a]), A3D_INVALID_PARAMETER,
                "a3d_voxel_map_retain: a bound of the box is NaN");
  }
  if (!map->block || map->cells == 0) {  // nothing to keep: the map is as new
    A3D_TRY(a3d_voxel_map_clear(map));
    for (uint64_t i = 0; i < n_marks; ++i) out_marks[i] = 0;
    if (out_removed) *out_removed = 0;
    return A3D_OK;
  }
  const uint64_t total = map->total;  // >= 1: a cell holds the seq of an offered point
  rule.min_seq = (uint32_t)std::min<uint64_t>(min_seq, total);
  a3d_context* ctx = map->ctx;
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // scratch, as the extract: one count per tile | the bitmap | one prefix per word; then the marks (with `total` appended:
  // its translation is k), their translations and the fault word
  const uint64_t n_words = (total + 63) / 64, n_all = n_marks + 1;
  uint64_t tiles = 0;
  uint32_t first_tile = 0, chunks_per_tile = 0;
  A3D_TRY(plan_tiles(n_words, VM_THREADS, VM_MAX_TILES, &tiles, &first_tile, &chunks_per_tile));
  const size_t counts_bytes = pad256(tiles * 4), bitmap_bytes = pad256(n_words * 8), prefix_bytes = pad256(n_words * 4);
  const size_t marks_bytes = pad256(n_all * 8), out_bytes = pad256((n_all + 1) * 8);
  void* region = nullptr;
  A3D_TRY(ctx_scratch(ctx, 3, counts_bytes + bitmap_bytes + prefix_bytes + marks_bytes + out_bytes, &region));
  uint32_t* d_tile_counts = (uint32_t*)region;
  unsigned long long* d_bitmap = (unsigned long long*)((char*)region + counts_bytes);
  uint32_t* d_prefix = (uint32_t*)((char*)region + counts_bytes + bitmap_bytes);
  unsigned long long* d_marks = (unsigned long long*)((char*)region + counts_bytes + bitmap_bytes + prefix_bytes);
  unsigned long long* d_out = (unsigned long long*)((char*)d_marks + marks_bytes);  // [n_all] translations, then the fault word
  unsigned long long* d_fault = d_out + n_all;
  // the new table: room for every old cell (k is known on the device only until the wait); its cell count at the end
  const uint64_t min_slots = table_slots(map->reserve_cells, 64);
  const uint64_t max_slots = retained_slots(map->cells, min_slots);
  const size_t bytes = table_layout(max_slots, map->with_normals, map->with_colors, map->mean).end + 256;
  void* block = nullptr;
  size_t block_bytes = 0;
  A3D_TRY(ctx_block_alloc(ctx, bytes, &block, &block_bytes));
  char* base = (char*)block;
  unsigned long long* d_cell_count = (unsigned long long*)(base + bytes - 256);
  std::vector<unsigned long long> h_marks(marks, marks + n_marks), h_out(n_all + 1);
  h_marks.push_back(total);
  hipStream_t s = ctx->stream;
  const dim3 over_slots(slot_blocks(map->slots)), over_words((uint32_t)tiles), block_dim(VM_THREADS);
  const dim3 over_marks((uint32_t)std::min<uint64_t>((n_all + VM_THREADS - 1) / VM_THREADS, VM_MAX_SLOT_BLOCKS));
  hipError_t e = hipMemsetAsync(d_bitmap, 0, bitmap_bytes, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_fault, 0, 8, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_marks, h_marks.data(), n_all * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(base, 0xFF, max_slots * sizeof(VoxelSlot), s);  // every key VX_EMPTY
  if (e == hipSuccess) e = hipMemsetAsync(d_cell_count, 0, 8, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(voxel_map_mark_retained_kernel, over_slots, block_dim, 0, s, (const VoxelSlot*)map->table,
                       (const float*)map->points, (unsigned long long)map->slots, (uint32_t*)d_bitmap,
                       (unsigned long long)total, rule);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(voxel_map_count_kernel, over_words, block_dim, 0, s, (const unsigned long long*)d_bitmap,
                       (uint32_t)n_words, chunks_per_tile, d_tile_counts);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(voxel_map_prefix_kernel, over_words, block_dim, 0, s, (const unsigned long long*)d_bitmap,
                       (uint32_t)n_words, chunks_per_tile, (const uint32_t*)d_tile_counts, d_prefix);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(voxel_map_marks_kernel, over_marks, block_dim, 0, s, (const unsigned long long*)d_bitmap,
                       (const uint32_t*)d_prefix, (uint32_t)n_words, (unsigned long long)total,
                       (const unsigned long long*)d_marks, (unsigned long long)n_all, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess && map->mean) {
    hipLaunchKernelGGL(voxel_map_zero_sums_kernel, dim3(slot_blocks(8 * max_slots)), block_dim, 0, s,
                       (const unsigned long long*)(d_out + n_marks), base, (unsigned long long)min_slots,
                       (unsigned long long)max_slots, map->with_normals ? 1u : 0u, map->with_colors ? 1u : 0u);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    if (map->mean)
      hipLaunchKernelGGL(voxel_map_rebuild_mean_kernel, over_slots, block_dim, 0, s, (const VoxelSlot*)map->table,
                         (const float*)map->points, (const float*)map->normals, (const uint32_t*)map->colors,
                         (unsigned long long)map->slots, (const unsigned long long*)d_bitmap, (const uint32_t*)d_prefix,
                         (unsigned long long)total, (const unsigned long long*)(d_out + n_marks), base,
                         (unsigned long long)min_slots, (unsigned long long)max_slots, map->with_normals ? 1u : 0u,
                         map->with_colors ? 1u : 0u, d_cell_count, d_fault, planes_of(map));
    else
      hipLaunchKernelGGL(voxel_map_rebuild_kernel, over_slots, block_dim, 0, s, (const VoxelSlot*)map->table,
                         (const float*)map->points, (const float*)map->normals, (const uint32_t*)map->colors,
                         (unsigned long long)map->slots, (const unsigned long long*)d_bitmap, (const uint32_t*)d_prefix,
                         (unsigned long long)total, (const unsigned long long*)(d_out + n_marks), base,
                         (unsigned long long)min_slots, (unsigned long long)max_slots, map->with_normals ? 1u : 0u,
                         map->with_colors ? 1u : 0u, d_cell_count, d_fault);
    e = hipGetLastError();
  }
  unsigned long long counted = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), d_out, (n_all + 1) * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&counted, d_cell_count, 8, hipMemcpyDeviceToHost, s);
  // host-synchronous, the one wait of the call
  const hipError_t waited = hipStreamSynchronize(s);
  if (e == hipSuccess) e = waited;
  const unsigned long long k = h_out[n_marks];
  if (e != hipSuccess || h_out[n_all] != 0 || counted != k || k > map->cells) {  // the old table, untouched, stays the map's
    ctx_block_release(ctx, block, block_bytes);
    if (e != hipSuccess)
      set_error("a3d_voxel_map_retain: rebuilding the table failed: %s", hipGetErrorString(e));
    else
      set_error("a3d_voxel_map_retain: the rebuilt table does not hold the survivors (the map is unchanged)");
    return A3D_HIP_ERROR;
  }
  const uint64_t removed = map->cells - k;
  if (k == 0) {  // as a3d_voxel_map_clear: the allocation and its slots stay
    ctx_block_release(ctx, block, block_bytes);
    A3D_TRY(a3d_voxel_map_clear(map));
  }
  for (uint64_t i = 0; i < n_marks; ++i) out_marks[i] = h_out[i];
  if (out_removed) *out_removed = removed;
  if (k == 0) return A3D_OK;
  ctx_block_release(ctx, map->block, map->block_bytes);  // (nothing enqueued reads it any more)
  adopt_table(map, block, block_bytes, retained_slots(k, min_slots), d_cell_count);
  map->cells = map->total = k, map->dropped_total = 0;
  return A3D_OK;
}

a3d_status a3d_voxel_map_get_stats(const a3d_voxel_map* map, a3d_voxel_map_stats* out) {
  A3D_REQUIRE(map && out, A3D_INVALID_PARAMETER, "null argument");
  out->cells = map->cells, out->slots = map->slots, out->total = map->total;
  out->dropped_total = map->dropped_total, out->growths = map->growths;
  return A3D_OK;
}

a3d_status a3d_voxel_map_clear(a3d_voxel_map* map) {
  A3D_REQUIRE(map, A3D_INVALID_PARAMETER, "null argument");
  if (map->block) {  // the allocation stays; ordered on the context's stream like every other use of the table
    A3D_HIP_TRY(hipSetDevice(map->ctx->device));
    A3D_HIP_TRY(hipMemsetAsync(map->table, 0xFF, map->slots * sizeof(VoxelSlot), map->ctx->stream));
    A3D_HIP_TRY(hipMemsetAsync(map->cell_count, 0, 8, map->ctx->stream));
    if (map->mean) {  // N, the sums and the epoch words: one stretch
      const TableLayout lay = table_layout(map->slots, map->with_normals, map->with_colors, true);
      A3D_HIP_TRY(hipMemsetAsync(map->sum_n, 0, lay.end - lay.sums_at, map->ctx->stream));
    }
  }
  map->cells = map->total = map->dropped_total = 0;
  return A3D_OK;
}

void a3d_voxel_map_free(a3d_voxel_map* map) {
  if (!map) return;
  if (map->block) ctx_block_release(map->ctx, map->block, map->block_bytes);
  solo_icp_release(map->ctx, &map->icp);
  delete map;
}

}  // extern "C"
