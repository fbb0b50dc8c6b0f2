// Outlier removal for resident clouds: a compaction by a per-row value (a3d_point_clouds_select_device), the per-row
// neighbour count and sum of the k nearest neighbour distances that the two classic filters decide by
// (a3d_point_clouds_knn_distance_device), and the statistical filter's threshold from that call's integer sums
// (a3d_knn_distance_threshold, host only).  The radius filter (PCL RadiusOutlierRemoval, Open3D remove_radius_outlier)
// is the k = 0 call followed by select(counts, lo = min_neighbors); the statistical filter (StatisticalOutlierRemoval,
// remove_statistical_outlier) is the knn call, the threshold, and select(qsum, 0, T).
//
// The rule of the knn call.  All f32 operations are rounded on their own (-ffp-contract=off, correctly rounded / and
// sqrtf).  Per call: radius r, finite and > 0; 0 <= k <= 32.  Host constants: r2 = r * r, s = 32768.0f / r.
//  1. Grid.  Pitch v = r, origin (0, 0, 0), cell and key by voxel_key.  A point whose key is refused (NaN, infinite,
//     outside +-2^20 cells) is DROPPED: it is nobody's neighbour, and it gets count 0 and qsum 0xFFFFFFFF.
//  2. Neighbours of point i.  Every kept point j of the same cloud, i itself included, such that each cell coordinate of
//     j differs from i's by at most 1, and with d_k = p_jk - p_ik, d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2.  These are
//     steps 1 and 2 of a3d_point_clouds_estimate_normals_device (cloud_normals.hip), word for word.
//  3. Counts.  counts[i] = N, the number of neighbours, the row itself included; 0 for a dropped row.  The same bits as
//     the d_out_counts of the normals entry at the same radius.
//  4. Lattice distance.  The OTHERS of row i are its neighbours with a different row index (a duplicate point is an
//     other at distance 0).  For each other, t = (uint32) rintf(sqrtf(d2) * s), ties to even.  t is non-decreasing in
//     d2, so the k smallest d2 give the k smallest t.
//  5. Distance sum.  qsum[i] = Q = the sum of the k smallest t; 0xFFFFFFFF if the row is dropped or has fewer than k
//     others.  The multiset of the k smallest values is unique, so Q does not depend on the order of the candidates.
//  6. Statistics.  Per cloud, over the m rows whose Q is not 0xFFFFFFFF: {m, sum Q, sum (Q*Q & 0xFFFFFFFF),
//     sum (Q*Q >> 32)}, u64 integer sums: the same bits on every run and under any permutation of the rows.  r2 is at most
//     twice r*r (a denormal product), so t <= 46342 < 2^16, Q < 2^21, Q*Q < 2^42; with len < 2^32 the four sums stay
//     below 2^32, 2^53, 2^64 and 2^42.
//  k == 0 is the count-only form: no distances, no qsum, statistics all zero.
//
// The knn call: one upload, one fill and four launches over every tile of every cloud of a batch, whatever the batch
// size (the job table of cloud_batch.hpp).  The first three are the counting sort by cell of cell_sort.hpp over a
// KnnJob table (cell_count_kernel, cell_place_kernel, cell_scatter_kernel), the one the normals entry runs.  The fourth,
// knn_distance_kernel, is the hot path: a thread per record in cell order, 27 slot lookups (cell_run), the candidates
// of a cell loaded four at a time as normals_estimate_kernel does.  The k smallest d2 (as bit patterns: d2 >= 0, so they order
// like the values) live in K registers as a sorted array, K in {8, 16, 32} chosen on the host from k; an insertion is an
// unrolled min / max chain that is skipped when the candidate is not below the current K-th; the lattice distance is
// computed for the k survivors only, after the walk.  No register array is indexed by a runtime value.  k == 0 has an
// instantiation without the array.  The diagnostics build keeps the forms that were considered and lose on paper
// (A3D_OUTLIERS_K=32: the widest array for every k; A3D_OUTLIERS_SELECT=t: the lattice distance of every candidate
// instead of its d2 bits), which scripts/cloud_outliers_probe.py measures against this one.
//
// The select call: one upload and two launches.  select_flag_kernel and select_compact_kernel are voxel_flag_kernel and
// voxel_compact_kernel of voxel_downsample.hip with the winner test replaced by lo <= value <= hi (KEEP EACH PAIR ALIKE,
// as cloud_batch.hpp says).
//
// Clustering (a3d_point_clouds_cluster_device): DBSCAN over the same neighbour graph, by a lock-free union-find.  PCL
// EuclideanClusterExtraction is min_points = 1; Open3D cluster_dbscan(eps, min_points) is the same two numbers.
//
// The rule of the cluster call.  All f32 operations are rounded on their own (-ffp-contract=off).  Per call: radius r,
// finite and > 0, r2 = r * r computed on the host in f32; min_points m >= 1.
//  1. Grid and neighbours.  Steps 1 and 2 of a3d_point_clouds_knn_distance_device, word for word: pitch r, origin 0,
//     voxel_key; refused rows are DROPPED and are nobody's neighbour; the neighbours of row i are the kept rows j of the
//     same cloud, i included, whose cell coordinates differ by at most 1 each and with
//     d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2.  d2 has the same bits seen from i and from j, so the relation is
//     symmetric.
//  2. Core.  N_i is the number of neighbours, the row itself counted: the same bits as that entry's counts.  Row i is a
//     CORE row iff it is kept and N_i >= m.  (Open3D counts the point itself too.)
//  3. Clusters.  Two core rows are linked iff they are neighbours.  A cluster is a connected component of the core rows
//     under that link.  Its ROOT is its lowest row index.
//  4. Border.  A kept row that is not core and has at least one core neighbour joins the cluster of one of them: the
//     core neighbour j that minimises bits(d2) << 32 | j, which is the nearest core row, the lower row on a tie (the
//     idiom of DeviceVoxelMap.nearest).  A border row never links two clusters.
//  5. Noise.  Every other row is noise: dropped rows, and non-core rows without a core neighbour.  Its label is
//     0xFFFFFFFF.
//  6. Labels.  Clusters are numbered 0 ... C-1 by ascending root.  labels[i] is the number of row i's cluster;
//     sizes[c] is the number of rows labelled c, border rows included; roots[c] is strictly increasing;
//     row_sizes[i] = sizes[labels[i]], and 0 for noise.
// Every output is integers decided on integers or on d2 bits: the same on every run.
//
// The cluster call: one upload, one fill and eight launches, whatever the batch size.  The first three are the same
// sort over a KnnJob table of the call's own; KnnJob::drop_row's "qsum of a dropped row = 0xFFFFFFFF" is pointed at
// parent[]: every dropped row a non-core row for free.  Then cluster_walk_kernel twice, the K = 0 shape of
// knn_distance_kernel: the count pass writes parent[row] = row
// for a core row and 0xFFFFFFFF otherwise; the link pass (a second walk: whether j is core is only known after the
// first) unions a core row with each core neighbour of LOWER row index (each edge is seen from both ends, half is
// enough), and keeps for a non-core row the minimum key of rule 4, stored as owner[row] = winner + 1 (0 from the fill =
// none; parent[] of a non-core row stays 0xFFFFFFFF through the pass, so "is j core" is one load that no other thread
// writes).  Union-find: find follows parent[] to a self-parent, every read a relaxed agent-scope atomic load (a plain
// load may be served from a stale L1 line); union hooks the HIGHER root under the lower with a 32-bit
// atomicCAS(&parent[hi], hi, lo) and retries from the value it saw on failure.  parent[x] <= x always and only a
// self-parent is ever CASed, so there are no cycles and a component's final root is its lowest row: rule 3.  Path
// halving stores a grandparent with a relaxed store.  A late halving store may put a HIGHER ancestor back over a lower
// one, so parent[x] does not only ever decrease; it stays an ancestor of x below x, which is all that find and union
// rely on.  Every loop has a trip bound of its own derived from len (find: a chain strictly decreases, <= len steps;
// union: a failed CAS strictly lowers the higher root, <= len retries, each with two finds, so the worst case of one
// union on paper is len retries times len steps; the probe chains are bounded by the table); exceeding one sets the
// call's fault word and the call returns A3D_HIP_ERROR instead of spinning.  cluster_flatten_kernel (row order): owner[p] = the row's root (find of itself, or of its winner) or
// 0xFFFFFFFF, size[root] += 1 (integer atomicAdd, order-free; a wave adds its rows of one root at once and carries the
// count of a run of rows across its trips, since one add per row queued a big cluster's rows up on one address: 4.4 ms
// a call instead of 3.3 ms on a frame of 270 k rows), and the roots' ballot words and per-tile counts exactly as
// select_flag_kernel makes them.  cluster_rank_kernel: select_compact_kernel's prefix machinery ranks the roots:
// labels[root] = rank, roots[rank], sizes[rank]; every row's row_sizes (size[] is final by then, so row_sizes needs no
// launch of its own) and the noise label.  cluster_label_kernel: labels[p] = labels[owner[p]] for the rest.  The
// diagnostics build keeps the forms that lose on paper: A3D_CLUSTER_LINK=all (union with every core neighbour, twice
// the finds) and A3D_CLUSTER_HALVING=0 (no path halving in the link pass), measured by scripts/cloud_cluster_probe.py.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cell_sort.hpp"  // the hash grid, the counting sort by cell, cell_run, consume_run

using namespace a3d;

namespace {

constexpr uint32_t CO_WAVES = CELL_THREADS / 64;
constexpr uint32_t CO_ROUNDS = CELL_CHUNK / CELL_THREADS;  // rounds of a block over a chunk
constexpr uint32_t CO_GROUPS = CELL_CHUNK / 64;            // ballot words per chunk
constexpr uint32_t CO_MAX_K = 32;
constexpr uint32_t CO_NONE = 0xFFFFFFFFu;  // the qsum of a row without k others
static_assert(CO_GROUPS <= 64, "a wave's lanes hold the chunk's ballot words");

// One non-empty cloud of a knn batch as the kernels see it (uploaded per call).
struct KnnJob {
  const float* points;
  uint32_t* out_counts;  // null: not written
  uint32_t* out_qsum;    // null: not written (k == 0)
  VoxelSlot* table;      // slot_mask + 1 slots, zeroed before the count: key word 0 = empty, else key + 1
  CellRecord* sorted;    // len records, the first `kept` of them written
  unsigned long long slot_mask;
  uint32_t len, first_tile, chunks_per_tile, n_tiles;

  __device__ void drop_row(uint32_t p) const {  // (cell_scatter_kernel) step 1's count 0 and qsum NONE
    if (out_counts) out_counts[p] = 0u;
    if (out_qsum) out_qsum[p] = CO_NONE;
  }
};
static_assert(sizeof(KnnJob) == 64, "KnnJob layout");

struct KnnParams {
  float r, r2, s;
  uint32_t k;
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Step 4 for one other: the lattice distance of a squared distance.
__device__ __forceinline__ uint32_t lattice_distance(float d2, float s) {
  return (uint32_t)__builtin_rintf(sqrtf(d2) * s);
}

// Pass 4.  K: the length of the sorted register array, >= the call's k; 0: counts only.  ON_T: the array holds lattice
// distances instead of d2 bits (diagnostics).  stats[4 * job ...] += the job's four sums.
template <uint32_t K, bool ON_T>
__global__ void __launch_bounds__(CELL_THREADS)
    knn_distance_kernel(const KnnJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, KnnParams prm,
                        const unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ stats) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const KnnJob& j = jobs[ji];
  const VoxelSlot* __restrict__ table = j.table;
  const CellRecord* __restrict__ sorted = j.sorted;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t kept = (uint32_t)min(cursor[ji], (unsigned long long)len);
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(kept, p0 + span);
  unsigned long long st_m = 0, st_q = 0, st_lo = 0, st_hi = 0;
  for (uint32_t base = p0; base < p_end; base += CELL_THREADS) {  // block-uniform
    const uint32_t t = base + threadIdx.x;
    f32x3 pi = {0.f, 0.f, 0.f};
    uint32_t row = t;
    unsigned long long key;
    bool live = t < p_end;
    if (live) {
      const f32x4 rec = *(const f32x4*)(sorted + t);
      pi.x = rec.x, pi.y = rec.y, pi.z = rec.z, row = __float_as_uint(rec.w);
      live = voxel_key(pi, grid, &key, nullptr) && row < len;  // (always: the record is a kept point's)
    }
    const int kx = live ? (int)(key >> 42) : 0, ky = live ? (int)(key >> 21 & 0x1FFFFF) : 0, kz = live ? (int)(key & 0x1FFFFF) : 0;
    uint32_t N = 0, others = 0;
    uint32_t a[K ? K : 1];  // the K smallest so far, ascending; ~0 = none yet (every d2 bit pattern and every t is below)
#pragma unroll
    for (uint32_t i = 0; i < (K ? K : 1); ++i) a[i] = CO_NONE;
    auto consume = [&](const f32x4 rec) {  // steps 2 to 4 for one candidate of a neighbouring cell
      const float dx = rec.x - pi.x, dy = rec.y - pi.y, dz = rec.z - pi.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (!(d2 <= prm.r2)) return;
      ++N;
      if constexpr (K > 0) {
        if (__float_as_uint(rec.w) == row) return;  // the row itself
        ++others;
        uint32_t x = ON_T ? lattice_distance(d2, prm.s) : __float_as_uint(d2);
        if (x < a[K - 1]) {
#pragma unroll
          for (uint32_t i = 0; i < K; ++i) {
            const uint32_t lo = min(a[i], x);
            x = max(a[i], x);
            a[i] = lo;
          }
        }
      }
    };
    for (int c = 0; c < 27; ++c) {
      if (!live) break;
      uint32_t begin, end;  // the run of the cell's records
      cell_run(table, mask, kept, kx, ky, kz, c, &begin, &end);
      // consume_run of cell_sort.hpp, written out (KEEP ALIKE): through the helper this kernel is compiled to other code
      // (K = 0: 38 VGPRs for 36), which the timing gate cannot tell from this one either way; the reasons are in the header
      for (uint32_t q = begin; q < end; q += CELL_AHEAD) {
        f32x4 rec[CELL_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < CELL_AHEAD; ++u) rec[u] = *(const f32x4*)(sorted + min(q + u, end - 1));
#pragma unroll
        for (uint32_t u = 0; u < CELL_AHEAD; ++u)
          if (q + u < end) consume(rec[u]);
      }
    }
    if (live) {
      if (j.out_counts) j.out_counts[row] = N;
      if constexpr (K > 0) {
        uint32_t Q = CO_NONE;
        if (others >= prm.k) {
          Q = 0;
          // k as the compiler cannot see through: it otherwise computes the K tests `i < k` once, ahead of the loop over
          // the rows, and keeps them as K lane masks in scalar registers (K = 32: 24 of them spilled to a VGPR's lanes)
          uint32_t k = prm.k;
          asm volatile("" : "+s"(k));
#pragma unroll
          for (uint32_t i = 0; i < K; ++i)
            if (i < k) Q += ON_T ? a[i] : lattice_distance(__uint_as_float(a[i]), prm.s);  // (uniform test)
          const unsigned long long sq = (unsigned long long)Q * Q;
          st_m += 1, st_q += Q, st_lo += sq & 0xFFFFFFFFull, st_hi += sq >> 32;
        }
        if (j.out_qsum) j.out_qsum[row] = Q;
      }
    }
  }
  if constexpr (K > 0) {
    st_m = wave_sum64(st_m), st_q = wave_sum64(st_q), st_lo = wave_sum64(st_lo), st_hi = wave_sum64(st_hi);
    if ((threadIdx.x & 63u) == 0 && st_m) {
      unsigned long long* w = stats + 4 * (size_t)ji;
      atomicAdd(w, st_m), atomicAdd(w + 1, st_q), atomicAdd(w + 2, st_lo), atomicAdd(w + 3, st_hi);
    }
  }
}

// One non-empty cloud of a select batch as the kernels see it (uploaded per call).
struct SelectJob {
  const float* points;
  const float* normals;  // read only when out_normals is set
  float* out_points;
  float* out_normals;         // null: no normals are written
  uint32_t* out_index;        // null: no indices are written
  const uint32_t* values;     // [len]
  unsigned long long* flags;  // (len + 63) / 64 ballot words
  unsigned long long capacity;
  uint32_t lo, hi;
  uint32_t len, first_tile, chunks_per_tile, pad;
  const uint8_t* colors;  // read only when out_colors is set
  uint8_t* out_colors;    // null: no colours are written
};
static_assert(sizeof(SelectJob) == 104, "SelectJob layout");

// Pass 1 (voxel_flag_kernel's twin): flags[p / 64] bit p % 64 = row p is kept; tile_counts[tile] = kept rows of the tile;
// lens[job] += the same (zeroed by the host upload).
__global__ void __launch_bounds__(CELL_THREADS)
    select_flag_kernel(const SelectJob* __restrict__ jobs, uint32_t n_jobs, uint32_t* __restrict__ tile_counts,
                       unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_wave[CO_WAVES];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const SelectJob& j = jobs[ji];
  const uint32_t* __restrict__ values = j.values;
  unsigned long long* __restrict__ flags = j.flags;
  const uint32_t lo = j.lo, hi = j.hi;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (len < 2^32 - span: checked by the host)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t c = 0;  // wave-uniform
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += CELL_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    bool win = false;
    if (p < p_end) {
      const uint32_t v = values[p];
      win = lo <= v && v <= hi;
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(win);
    if (lane == 0) flags[base >> 6] = ballot;
    c += (uint32_t)__builtin_popcountll(ballot);
  }
  if (lane == 0) s_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (uint32_t w = 0; w < CO_WAVES; ++w) total += s_wave[w];
    tile_counts[tile] = total;
    if (total) atomicAdd(&lens[ji], (unsigned long long)total);
  }
}

// Pass 2 (voxel_compact_kernel's twin): every kept row of the tile to out[offset + rank].  Nothing is written anywhere if
// any cloud of the batch keeps more rows than its capacity (the host then returns A3D_INVALID_PARAMETER).
__global__ void __launch_bounds__(CELL_THREADS)
    select_compact_kernel(const SelectJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ tile_counts,
                          const unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_base, s_over;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const SelectJob& j = jobs[ji];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t = tile - j.first_tile;
  if (wave == 0) {
    uint32_t s = 0;
    for (uint32_t k = lane; k < t; k += 64) s += tile_counts[j.first_tile + k];
    bool over = false;
    for (uint32_t k = lane; k < n_jobs; k += 64) over |= lens[k] > jobs[k].capacity;
    s = wave_sum(s);
    const bool any_over = __builtin_amdgcn_ballot_w64(over) != 0ull;
    if (lane == 0) s_base = s, s_over = any_over ? 1u : 0u;
  }
  __syncthreads();
  if (s_over) return;
  const float* __restrict__ points = j.points;
  const float* __restrict__ normals = j.normals;
  const unsigned long long* __restrict__ flags = j.flags;
  float* __restrict__ out_points = j.out_points;
  float* __restrict__ out_normals = j.out_normals;
  uint32_t* __restrict__ out_index = j.out_index;
  const uint8_t* __restrict__ colors = j.colors;
  uint8_t* __restrict__ out_colors = j.out_colors;
  const unsigned long long capacity = j.capacity;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK, n_groups = (len + 63u) >> 6;
  const uint32_t p0 = t * span, p_end = min(len, p0 + span);
  uint32_t base = s_base;  // kept rows of the cloud before this chunk
  for (uint32_t px0 = p0; px0 < p_end; px0 += CELL_CHUNK) {
    // lane g < CO_GROUPS of every wave holds the ballot word of the chunk's group g (rows px0 + 64 g ...), their
    // exclusive prefix gives every group's offset: no LDS, no block barrier
    const uint32_t g = (px0 >> 6) + lane;
    const uint64_t word = lane < CO_GROUPS && g < n_groups ? flags[g] : 0ull;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < (int)CO_GROUPS; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    const uint32_t excl = incl - cnt;
    uint64_t ballots[CO_ROUNDS];
    uint32_t offs[CO_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CO_ROUNDS; ++r) {  // (every lane takes part in the shuffles: no divergence yet)
      const int src = (int)(r * CO_WAVES + wave);  // the group of this wave's round r (round-major, then wave, then lane)
      ballots[r] = (uint64_t)__shfl((unsigned long long)word, src, 64);
      offs[r] = base + __shfl(excl, src, 64);
    }
    base += __shfl(incl, (int)CO_GROUPS - 1, 64);
#pragma unroll
    for (uint32_t r = 0; r < CO_ROUNDS; ++r) {
      const uint64_t ballot = ballots[r];
      if (!((ballot >> lane) & 1ull)) continue;
      const uint32_t p = px0 + r * CELL_THREADS + threadIdx.x;
      const unsigned long long dst = (unsigned long long)offs[r] + lane_rank(ballot);
      if (p >= p_end || dst >= capacity) continue;  // (cannot happen: the bit is a row's, the total fits; a bound on every store)
      *(f32x3_u*)(out_points + 3 * dst) = *(const f32x3_u*)(points + 3 * (size_t)p);
      if (out_normals) *(f32x3_u*)(out_normals + 3 * dst) = *(const f32x3_u*)(normals + 3 * (size_t)p);
      if (out_index) out_index[dst] = p;
      if (out_colors) store_color(out_colors, dst, load_color(colors, p));
    }
  }
}

// One non-empty cloud of a cluster batch as the cluster kernels see it (uploaded per call, behind the KnnJob table that the
// three sort kernels read; both tables have the same tiles).
struct ClusterJob {
  uint32_t* labels;
  uint32_t* row_sizes;        // null: not written
  uint32_t* sizes;            // null: not written
  uint32_t* roots;            // null: not written
  uint32_t* parent;           // [len] by row: the union-find; CO_NONE = not a core row
  uint32_t* owner;            // [len] by row, zeroed: winner + 1 of a border row; after the flatten: root or CO_NONE
  uint32_t* size;             // [len] by row, zeroed: rows of the cluster, at its root
  unsigned long long* flags;  // (len + 63) / 64 ballot words: row p is a root
  const VoxelSlot* table;
  const CellRecord* sorted;
  unsigned long long slot_mask;
  uint32_t len, first_tile, chunks_per_tile, pad;
};
static_assert(sizeof(ClusterJob) == 104, "ClusterJob layout");

// The self-parent above x.  parent[x] <= x for every core row and stays an ancestor of x (a late halving store may raise
// it again, never to x or above), so the chain strictly decreases and ends within len steps.
template <bool HALVE>
__device__ __forceinline__ uint32_t cluster_find(uint32_t* parent, uint32_t x, uint32_t len,
                                                 unsigned long long* __restrict__ fault) {
  for (uint32_t trips = 0; trips <= len; ++trips) {
    const uint32_t p = VX_LOAD_AGENT(&parent[x]);
    if (p == x) return x;
    if (p >= len) break;  // (cannot happen: x is a core row; a bound on every load)
    if constexpr (HALVE) {
      const uint32_t g = VX_LOAD_AGENT(&parent[p]);
      if (g < p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // an ancestor, below x
    }
    x = p;
  }
  atomicMax(fault, 4ull);
  return x;
}

// One set out of the sets of a and b (roots when they were read); returns the lower root.  A failed CAS saw a parent
// below hi, so the higher of the two roots strictly decreases: at most len retries of this loop (each retry runs two
// finds of at most len steps: the bound of the whole call is the product, the bound of each loop is len).
template <bool HALVE>
__device__ __forceinline__ uint32_t cluster_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t len,
                                                  unsigned long long* __restrict__ fault) {
  for (uint32_t trips = 0; trips <= len; ++trips) {
    if (a == b) return a;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return lo;
    if (old >= len) break;  // (cannot happen)
    a = cluster_find<HALVE>(parent, old, len, fault), b = cluster_find<HALVE>(parent, lo, len, fault);
  }
  atomicMax(fault, 5ull);
  return min(a, b);
}

// Passes 4 and 5: the walk of knn_distance_kernel<0>.  LINK false: parent[row] = row if N >= m, else
// CO_NONE.  LINK true: rule 3's unions for a core row (ALL: with every core neighbour, not only the lower rows) and
// rule 4's winner for the others.
template <bool LINK, bool ALL, bool HALVE>
__global__ void __launch_bounds__(CELL_THREADS)
    cluster_walk_kernel(const ClusterJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, float r2, uint32_t m,
                        const unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const ClusterJob& j = jobs[ji];
  const VoxelSlot* __restrict__ table = j.table;
  const CellRecord* __restrict__ sorted = j.sorted;
  uint32_t* parent = j.parent;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t kept = (uint32_t)min(cursor[ji], (unsigned long long)len);
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(kept, p0 + span);
  for (uint32_t base = p0; base < p_end; base += CELL_THREADS) {  // block-uniform
    const uint32_t t = base + threadIdx.x;
    f32x3 pi = {0.f, 0.f, 0.f};
    uint32_t row = t;
    unsigned long long key;
    bool live = t < p_end;
    if (live) {
      const f32x4 rec = *(const f32x4*)(sorted + t);
      pi.x = rec.x, pi.y = rec.y, pi.z = rec.z, row = __float_as_uint(rec.w);
      live = voxel_key(pi, grid, &key, nullptr) && row < len;  // (always: the record is a kept point's)
    }
    const int kx = live ? (int)(key >> 42) : 0, ky = live ? (int)(key >> 21 & 0x1FFFFF) : 0, kz = live ? (int)(key & 0x1FFFFF) : 0;
    uint32_t N = 0;
    uint32_t mine = row;              // LINK, core row: a root above this row as last seen
    unsigned long long best = ~0ull;  // LINK, non-core row: the minimum key of rule 4
    bool core = false;
    if constexpr (LINK) core = live && VX_LOAD_AGENT(&parent[row]) != CO_NONE;
    auto distance2 = [&](const f32x4 rec) {
      const float dx = rec.x - pi.x, dy = rec.y - pi.y, dz = rec.z - pi.z;
      return (dx * dx + dy * dy) + dz * dz;
    };
    // Rules 3 and 4 for one neighbour `other` of a different row.  above: a value parent[other] has held (whether `other`
    // is core never changes in this pass, and any value parent[other] has held is an ancestor of `other` for good, so a
    // value from this CU's cache serves both tests; it is not one of find's reads)
    auto link = [&](uint32_t other, float d2, uint32_t above) {
      if (above == CO_NONE) return;  // not a core row
      if (core) {
        if (above == mine) return;  // already under the root this row is under: the usual case in a dense cell
        const uint32_t theirs = cluster_find<HALVE>(parent, above < len ? above : other, len, fault);
        if (theirs != mine) mine = cluster_union<HALVE>(parent, mine, theirs, len, fault);
      } else {
        best = min(best, (unsigned long long)__float_as_uint(d2) << 32 | other);
      }
    };
    for (int c = 0; c < 27; ++c) {
      if (!live) break;
      uint32_t begin, end;  // the run of the cell's records
      cell_run(table, mask, kept, kx, ky, kz, c, &begin, &end);
      if constexpr (!LINK) {
        consume_run<CELL_AHEAD>(sorted, begin, end, [&](const f32x4 rec) {
          if (distance2(rec) <= r2) ++N;
        });
      } else if (begin < end) {
        // The same trips; a neighbour costs a second, dependent load (its parent), so the parents of a trip's neighbours
        // are requested together and behind the NEXT trip's records: a thread still waits for memory once per CELL_AHEAD
        // candidates.  (Measured: 270 k rows in one cell 743 -> 675 ms a call, a frame at r = 0.01 3.33 -> 3.28 ms; what is
        // left of this pass's 4 to 5 times the count pass is the finds, two or three dependent agent-scope loads each.)  A
        // candidate that is no neighbour, or a higher row that the other end of the edge will see, loads parent[row]
        // instead, a line the thread has.  The wavefront-scope atomic load is an ordinary cached load that the compiler
        // may not tear or invent.
        f32x4 rec[CELL_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < CELL_AHEAD; ++u) rec[u] = *(const f32x4*)(sorted + min(begin + u, end - 1));
        for (uint32_t q = begin; q < end; q += CELL_AHEAD) {
          f32x4 next[CELL_AHEAD];
          float d2[CELL_AHEAD];
          uint32_t other[CELL_AHEAD], above[CELL_AHEAD];
          bool need[CELL_AHEAD];
#pragma unroll
          for (uint32_t u = 0; u < CELL_AHEAD; ++u) next[u] = *(const f32x4*)(sorted + min(q + CELL_AHEAD + u, end - 1));
#pragma unroll
          for (uint32_t u = 0; u < CELL_AHEAD; ++u) {
            d2[u] = distance2(rec[u]), other[u] = __float_as_uint(rec[u].w);
            need[u] = q + u < end && d2[u] <= r2 && other[u] != row && other[u] < len && !(core && !ALL && other[u] > row);
            above[u] = __hip_atomic_load(&parent[need[u] ? other[u] : row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          }
#pragma unroll
          for (uint32_t u = 0; u < CELL_AHEAD; ++u)
            if (need[u]) link(other[u], d2[u], above[u]);
#pragma unroll
          for (uint32_t u = 0; u < CELL_AHEAD; ++u) rec[u] = next[u];
        }
      }
    }
    if (!live) continue;
    if constexpr (LINK) {
      if (!core && best != ~0ull) j.owner[row] = (uint32_t)best + 1u;
    } else {
      parent[row] = N >= m ? row : CO_NONE;
    }
  }
}

// Pass 6 (row order; its end is select_flag_kernel's: KEEP ALIKE): owner[p] = the root of row p's cluster or CO_NONE,
// size[root] += 1, flags bit p = row p is a root, tile_counts[tile] = roots of the tile; clusters[job] += the same,
// noise[job] += rows without a cluster.
__global__ void __launch_bounds__(CELL_THREADS)
    cluster_flatten_kernel(const ClusterJob* __restrict__ jobs, uint32_t n_jobs, uint32_t* __restrict__ tile_counts,
                           unsigned long long* __restrict__ clusters, unsigned long long* __restrict__ noise,
                           unsigned long long* __restrict__ fault) {
  __shared__ uint32_t s_wave[CO_WAVES], s_noise[CO_WAVES];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const ClusterJob& j = jobs[ji];
  uint32_t* parent = j.parent;
  uint32_t* __restrict__ owner = j.owner;
  uint32_t* __restrict__ size = j.size;
  unsigned long long* __restrict__ flags = j.flags;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (len < 2^32 - span: checked by the host)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t c = 0, lost = 0;                   // c: wave-uniform
  uint32_t run_root = CO_NONE, run_rows = 0;  // wave-uniform: rows of one root that size[] has not been given yet
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += CELL_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    uint32_t root = CO_NONE;
    bool is_root = false;
    if (p < p_end) {
      uint32_t from = CO_NONE;  // the core row whose root is this row's
      if (VX_LOAD_AGENT(&parent[p]) != CO_NONE) from = p;
      else if (owner[p] != 0u) from = owner[p] - 1u;
      if (from < len) root = cluster_find<true>(parent, from, len, fault);
      if (root >= len) root = CO_NONE, ++lost;
      owner[p] = root;
      is_root = root == p;
    }
    // size[root] += 1 per row.  The rows of a big cluster would queue up on one address, so a wave adds its rows of one
    // root at once and carries the last root's count into its next 64 rows (the rows of a cluster come in runs); at most
    // 64 distinct roots a trip
    uint64_t todo = __builtin_amdgcn_ballot_w64(root != CO_NONE);
    for (uint32_t trips = 0; todo != 0ull && trips < 64u; ++trips) {
      const uint32_t r = __shfl(root, __builtin_ctzll(todo), 64);
      const uint64_t same = __builtin_amdgcn_ballot_w64(root == r);
      if (r != run_root) {
        if (lane == 0 && run_rows) atomicAdd(&size[run_root], run_rows);
        run_root = r, run_rows = 0;
      }
      run_rows += (uint32_t)__builtin_popcountll(same);
      todo &= ~same;
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(is_root);
    if (lane == 0) flags[base >> 6] = ballot;
    c += (uint32_t)__builtin_popcountll(ballot);
  }
  if (lane == 0 && run_rows) atomicAdd(&size[run_root], run_rows);
  lost = wave_sum(lost);
  if (lane == 0) s_wave[wave] = c, s_noise[wave] = lost;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0, gone = 0;
    for (uint32_t w = 0; w < CO_WAVES; ++w) total += s_wave[w], gone += s_noise[w];
    tile_counts[tile] = total;
    if (total) atomicAdd(&clusters[ji], (unsigned long long)total);
    if (gone) atomicAdd(&noise[ji], (unsigned long long)gone);
  }
}

// Pass 7 (its start and its prefix are select_compact_kernel's: KEEP ALIKE): the roots of a cloud ranked in row order.
// labels[root] = rank, roots[rank] = root, sizes[rank] = size[root]; a noise row's label CO_NONE; every row's row_sizes.
__global__ void __launch_bounds__(CELL_THREADS)
    cluster_rank_kernel(const ClusterJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_base;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const ClusterJob& j = jobs[ji];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t = tile - j.first_tile;
  if (wave == 0) {
    uint32_t s = 0;
    for (uint32_t k = lane; k < t; k += 64) s += tile_counts[j.first_tile + k];
    s = wave_sum(s);
    if (lane == 0) s_base = s;
  }
  __syncthreads();
  const unsigned long long* __restrict__ flags = j.flags;
  const uint32_t* __restrict__ owner = j.owner;
  const uint32_t* __restrict__ size = j.size;
  uint32_t* __restrict__ labels = j.labels;
  uint32_t* __restrict__ row_sizes = j.row_sizes;
  uint32_t* __restrict__ sizes = j.sizes;
  uint32_t* __restrict__ roots = j.roots;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK, n_groups = (len + 63u) >> 6;
  const uint32_t p0 = t * span, p_end = min(len, p0 + span);
  uint32_t base = s_base;  // roots of the cloud before this chunk
  for (uint32_t px0 = p0; px0 < p_end; px0 += CELL_CHUNK) {
    const uint32_t g = (px0 >> 6) + lane;
    const uint64_t word = lane < CO_GROUPS && g < n_groups ? flags[g] : 0ull;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < (int)CO_GROUPS; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    const uint32_t excl = incl - cnt;
    uint64_t ballots[CO_ROUNDS];
    uint32_t offs[CO_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CO_ROUNDS; ++r) {  // (every lane takes part in the shuffles: no divergence yet)
      const int src = (int)(r * CO_WAVES + wave);
      ballots[r] = (uint64_t)__shfl((unsigned long long)word, src, 64);
      offs[r] = base + __shfl(excl, src, 64);
    }
    base += __shfl(incl, (int)CO_GROUPS - 1, 64);
#pragma unroll
    for (uint32_t r = 0; r < CO_ROUNDS; ++r) {
      const uint32_t p = px0 + r * CELL_THREADS + threadIdx.x;
      if (p >= p_end) continue;
      const uint32_t root = owner[p];
      if (root >= len) {  // noise
        labels[p] = CO_NONE;
        if (row_sizes) row_sizes[p] = 0u;
        continue;
      }
      const uint32_t rows = size[root];
      if (row_sizes) row_sizes[p] = rows;
      if (!((ballots[r] >> lane) & 1ull)) continue;
      const uint32_t rank = offs[r] + lane_rank(ballots[r]);
      if (rank >= len) continue;  // (cannot happen: there are at most len roots; a bound on every store)
      labels[p] = rank;
      if (roots) roots[rank] = p;
      if (sizes) sizes[rank] = rows;
    }
  }
}

// Pass 8: the label of every row that is in a cluster and is not its root (no root's label is written here).
__global__ void __launch_bounds__(CELL_THREADS) cluster_label_kernel(const ClusterJob* __restrict__ jobs, uint32_t n_jobs) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const ClusterJob& j = jobs[ji];
  const uint32_t* __restrict__ owner = j.owner;
  uint32_t* labels = j.labels;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += CELL_THREADS) {
    const uint32_t root = owner[p];
    if (root < len && root != p) labels[p] = labels[root];
  }
}

}  // namespace

extern "C" {

a3d_status a3d_point_clouds_select_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                          const uint8_t* const* d_colors, uint64_t n, const uint32_t* const* d_values,
                                          const uint32_t* lo, const uint32_t* hi, float* const* d_out_points,
                                          float* const* d_out_normals, uint8_t* const* d_out_colors,
                                          uint32_t* const* d_out_index, const uint64_t* capacities, uint64_t* out_lens) {
  if (n == 0) return A3D_OK;
  static const char NAME[] = "a3d_point_clouds_select_device";
  if (!(ctx && d_clouds && d_values && lo && hi && d_out_points && capacities && out_lens))
    return refuse(A3D_INVALID_PARAMETER, NAME, "null argument");
  const CompactArgs args{d_clouds, d_colors, d_out_points, d_out_normals, d_out_colors, d_out_index, capacities};
  std::vector<SelectJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(8 * n);
  uint64_t tiles = 0;
  TailPart flags;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = d_clouds[i].len;
    if (len >= (1ull << 32)) return refuse(A3D_INVALID_PARAMETER, NAME, "a cloud of 2^32 points or more");
    if (len == 0) continue;  // yields no rows; its pointers may be null
    SelectJob j{};
    // (the values are this call's own array: their null test rides in the shared one, which is why compact_front takes a
    // flag and the text: one refusal, at the place in the order where it has always stood)
    A3D_TRY(compact_front(NAME, args, i, d_values[i] != nullptr, "null points, values or output pointer", CELL_CHUNK,
                          CELL_MAX_TILES, &tiles, &ranges, &j));
    j.values = d_values[i], j.lo = lo[i], j.hi = hi[i];
    ranges.in(j.values, len * 4);
    flags.take(&j.flags, pad256((len + 63) / 64 * 8));
    jobs.push_back(j), cloud_of_job.push_back(i);
  }
  if (ranges.overlap())
    return refuse(A3D_INVALID_PARAMETER, NAME, "an output overlaps an input or another output (there is no in-place form)");
  zero_results(out_lens, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  BatchScratch scratch;  // the words: lens; the tail: ballot words
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(SelectJob), n_jobs, tiles, flags.bytes, &scratch));
  place_parts(scratch.tail, {&flags});
  for (SelectJob& j : jobs) flags.rebase(&j.flags);
  const SelectJob* d_jobs = (const SelectJob*)scratch.jobs;
  unsigned long long* d_lens = scratch.words;
  uint32_t* d_tile_counts = scratch.tile_counts;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  const dim3 grid_dim((uint32_t)tiles), block(CELL_THREADS);
  hipLaunchKernelGGL(select_flag_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, d_tile_counts, d_lens);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(select_compact_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, (const uint32_t*)d_tile_counts,
                     (const unsigned long long*)d_lens);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_lens, n_jobs, s, &words));
  return compact_finish(NAME, "kept rows", jobs, cloud_of_job, words.data(), out_lens, nullptr);
}

a3d_status a3d_point_clouds_knn_distance_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                float radius, uint32_t k, uint32_t* const* d_out_counts,
                                                uint32_t* const* d_out_qsum, uint64_t* out_stats, uint64_t* out_dropped) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(ctx && d_clouds, A3D_INVALID_PARAMETER, "null argument");
  static const char NAME[] = "a3d_point_clouds_knn_distance_device";
  VoxelGrid grid;
  KnnParams prm{radius, 0.f, 0.f, k};
  A3D_TRY(radius_grid_from(NAME, radius, &grid, &prm.r2, &prm.s));
  A3D_REQUIRE(k <= CO_MAX_K, A3D_INVALID_PARAMETER, "a3d_point_clouds_knn_distance_device: k must be at most 32");
  A3D_REQUIRE(k == 0 || d_out_qsum, A3D_INVALID_PARAMETER, "null argument");
  std::vector<KnnJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(3 * n);
  CellSortPlan plan;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    A3D_REQUIRE(c.len < (1ull << 32), A3D_INVALID_PARAMETER, "a cloud of 2^32 points or more");
    if (c.len == 0) continue;  // yields zeros; its pointers may be null
    A3D_REQUIRE(c.points && (k == 0 || d_out_qsum[i]), A3D_INVALID_PARAMETER, "null points or output pointer");
    KnnJob j{};
    j.points = c.points;
    j.out_counts = d_out_counts ? d_out_counts[i] : nullptr;
    j.out_qsum = k ? d_out_qsum[i] : nullptr;
    A3D_TRY(cell_sort_plan(&plan, NAME, c.len, &j));
    jobs.push_back(j), cloud_of_job.push_back(i);
    ranges.in(j.points, c.len * 12), ranges.out(j.out_counts, c.len * 4), ranges.out(j.out_qsum, c.len * 4);
  }
  if (ranges.overlap()) return refuse(A3D_INVALID_PARAMETER, NAME, "an output overlaps an input or another output");
  zero_results(out_stats, n, 4), zero_results(out_dropped, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  BatchScratch scratch;  // the words: cursors (kept counts), dropped, 4 sums per job, fault; the tail: hash tables | records
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(KnnJob), 6 * n_jobs + 1, 0, plan.tables.bytes + plan.sorted.bytes, &scratch));
  place_parts(scratch.tail, {&plan.tables, &plan.sorted});
  for (KnnJob& j : jobs) cell_sort_rebase(plan, &j);
  const KnnJob* d_jobs = (const KnnJob*)scratch.jobs;
  unsigned long long* d_cursor = scratch.words;
  unsigned long long* d_dropped = d_cursor + n_jobs;
  unsigned long long* d_stats = d_cursor + 2 * n_jobs;
  unsigned long long* d_fault = d_cursor + 6 * n_jobs;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  A3D_HIP_TRY(hipMemsetAsync(plan.tables.base, 0, plan.tables.bytes, s));  // every key word empty, every count 0
  const dim3 grid_dim((uint32_t)plan.tiles), block(CELL_THREADS);
  const uint32_t nj = (uint32_t)n_jobs;
  A3D_TRY(cell_sort_launch(d_jobs, nj, plan.tiles, grid, d_cursor, d_dropped, d_fault, s));
  const unsigned long long* d_kept = d_cursor;
#define CO_LAUNCH(K, ON_T) \
  hipLaunchKernelGGL((knn_distance_kernel<K, ON_T>), grid_dim, block, 0, s, d_jobs, nj, grid, prm, d_kept, d_stats)
  uint32_t width = k == 0 ? 0u : k <= 8 ? 8u : k <= 16 ? 16u : 32u;
  bool on_t = false;
#ifdef A3D_DIAGNOSTICS  // the forms that lose (scripts/cloud_outliers_probe.py)
  const char* widest = getenv("A3D_OUTLIERS_K");
  const char* select = getenv("A3D_OUTLIERS_SELECT");
  if (k && widest && !strcmp(widest, "32")) width = 32;
  on_t = k && select && !strcmp(select, "t");
  if (on_t) {
    if (width == 8) CO_LAUNCH(8, true);
    else if (width == 16) CO_LAUNCH(16, true);
    else CO_LAUNCH(32, true);
  }
#endif
  if (!on_t) {
    if (width == 0) CO_LAUNCH(0, false);
    else if (width == 8) CO_LAUNCH(8, false);
    else if (width == 16) CO_LAUNCH(16, false);
    else CO_LAUNCH(32, false);
  }
#undef CO_LAUNCH
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_cursor, 6 * n_jobs + 1, s, &words));
  A3D_REQUIRE(words[6 * n_jobs] == 0, A3D_HIP_ERROR, "a3d_point_clouds_knn_distance_device: a hash table filled up");
  scatter_words(&words[2 * n_jobs], cloud_of_job, out_stats, 4), scatter_words(&words[n_jobs], cloud_of_job, out_dropped);
  return A3D_OK;
}

a3d_status a3d_point_clouds_cluster_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n, float radius,
                                           uint32_t min_points, uint32_t* const* d_out_labels,
                                           uint32_t* const* d_out_row_sizes, uint32_t* const* d_out_sizes,
                                           uint32_t* const* d_out_roots, uint64_t* out_clusters, uint64_t* out_noise,
                                           uint64_t* out_dropped) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(ctx && d_clouds && d_out_labels, A3D_INVALID_PARAMETER, "null argument");
  static const char NAME[] = "a3d_point_clouds_cluster_device";
  VoxelGrid grid;
  float r2;
  A3D_TRY(radius_grid_from(NAME, radius, &grid, &r2, nullptr));
  A3D_REQUIRE(min_points >= 1, A3D_INVALID_PARAMETER, "a3d_point_clouds_cluster_device: min_points must be at least 1");
  std::vector<KnnJob> sort_jobs;
  std::vector<ClusterJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  sort_jobs.reserve(n), jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(6 * n);
  CellSortPlan plan;
  TailPart sizes, owners, parents, flags;  // (a job's size, owner and parent lie at one offset of their three parts)
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    A3D_REQUIRE(c.len < (1ull << 32), A3D_INVALID_PARAMETER, "a cloud of 2^32 points or more");
    if (c.len == 0) continue;  // yields zeros; its pointers may be null
    A3D_REQUIRE(c.points && d_out_labels[i], A3D_INVALID_PARAMETER, "null points or labels pointer");
    KnnJob k{};
    ClusterJob j{};
    k.points = c.points;
    A3D_TRY(cell_sort_plan(&plan, NAME, c.len, &k));
    j.len = k.len, j.first_tile = k.first_tile, j.chunks_per_tile = k.chunks_per_tile, j.slot_mask = k.slot_mask;
    const size_t row_bytes = pad256(c.len * 4);
    sizes.take(&j.size, row_bytes), owners.take(&j.owner, row_bytes), parents.take(&j.parent, row_bytes);
    flags.take(&j.flags, pad256((c.len + 63) / 64 * 8));
    j.labels = d_out_labels[i];
    j.row_sizes = d_out_row_sizes ? d_out_row_sizes[i] : nullptr;
    j.sizes = d_out_sizes ? d_out_sizes[i] : nullptr;
    j.roots = d_out_roots ? d_out_roots[i] : nullptr;
    sort_jobs.push_back(k), jobs.push_back(j), cloud_of_job.push_back(i);
    ranges.in(c.points, c.len * 12), ranges.in(c.normals, c.len * 12);
    for (uint32_t* out : {j.labels, j.row_sizes, j.sizes, j.roots}) ranges.out(out, c.len * 4);
  }
  if (ranges.overlap()) return refuse(A3D_INVALID_PARAMETER, NAME, "an output overlaps an input or another output");
  zero_results(out_clusters, n), zero_results(out_noise, n), zero_results(out_dropped, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  // the table: the sort's jobs, then the cluster jobs; the words: cursors (kept counts), dropped, clusters, noise per job,
  // fault; the tail: hash tables | size | owner (these three zeroed by the one fill) | parent | records | ballot words
  const size_t sort_table = n_jobs * sizeof(KnnJob), zeroed = plan.tables.bytes + sizes.bytes + owners.bytes;
  std::vector<char> both(sort_table + n_jobs * sizeof(ClusterJob));
  BatchScratch scratch;
  A3D_TRY(batch_scratch(ctx, both.size(), 4 * n_jobs + 1, plan.tiles, zeroed + parents.bytes + plan.sorted.bytes + flags.bytes,
                        &scratch));
  place_parts(scratch.tail, {&plan.tables, &sizes, &owners, &parents, &plan.sorted, &flags});
  for (size_t q = 0; q < n_jobs; ++q) {
    KnnJob& k = sort_jobs[q];
    ClusterJob& j = jobs[q];
    cell_sort_rebase(plan, &k);
    j.table = k.table, j.sorted = k.sorted;
    sizes.rebase(&j.size), owners.rebase(&j.owner), parents.rebase(&j.parent), flags.rebase(&j.flags);
    k.out_counts = nullptr, k.out_qsum = j.parent;  // the scatter's CO_NONE of a dropped row: not a core row
  }
  memcpy(both.data(), sort_jobs.data(), sort_table);
  memcpy(both.data() + sort_table, jobs.data(), n_jobs * sizeof(ClusterJob));
  const KnnJob* d_sort_jobs = (const KnnJob*)scratch.jobs;
  const ClusterJob* d_jobs = (const ClusterJob*)((const char*)scratch.jobs + sort_table);
  unsigned long long* d_cursor = scratch.words;
  unsigned long long* d_dropped = d_cursor + n_jobs;
  unsigned long long* d_clusters = d_cursor + 2 * n_jobs;
  unsigned long long* d_noise = d_cursor + 3 * n_jobs;
  unsigned long long* d_fault = d_cursor + 4 * n_jobs;
  uint32_t* d_tile_counts = scratch.tile_counts;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, both.data(), s));
  A3D_HIP_TRY(hipMemsetAsync(plan.tables.base, 0, zeroed, s));  // every key word empty, every count, size and owner 0
  const dim3 grid_dim((uint32_t)plan.tiles), block(CELL_THREADS);
  const uint32_t nj = (uint32_t)n_jobs;
  A3D_TRY(cell_sort_launch(d_sort_jobs, nj, plan.tiles, grid, d_cursor, d_dropped, d_fault, s));
  const unsigned long long* d_kept = d_cursor;
#define CL_LAUNCH(LINK, ALL, HALVE) \
  hipLaunchKernelGGL((cluster_walk_kernel<LINK, ALL, HALVE>), grid_dim, block, 0, s, d_jobs, nj, grid, r2, min_points, d_kept, d_fault)
  CL_LAUNCH(false, false, true);
  A3D_HIP_TRY(hipGetLastError());
  bool all = false, halve = true;
#ifdef A3D_DIAGNOSTICS  // the forms that lose (scripts/cloud_cluster_probe.py)
  const char* link = getenv("A3D_CLUSTER_LINK");
  const char* halving = getenv("A3D_CLUSTER_HALVING");
  all = link && !strcmp(link, "all");
  halve = !(halving && !strcmp(halving, "0"));
  if (all && halve) CL_LAUNCH(true, true, true);
  else if (all) CL_LAUNCH(true, true, false);
  else if (!halve) CL_LAUNCH(true, false, false);
#endif
  if (!all && halve) CL_LAUNCH(true, false, true);
#undef CL_LAUNCH
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cluster_flatten_kernel, grid_dim, block, 0, s, d_jobs, nj, d_tile_counts, d_clusters, d_noise, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cluster_rank_kernel, grid_dim, block, 0, s, d_jobs, nj, (const uint32_t*)d_tile_counts);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cluster_label_kernel, grid_dim, block, 0, s, d_jobs, nj);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_cursor, 4 * n_jobs + 1, s, &words));
  A3D_REQUIRE(words[4 * n_jobs] == 0, A3D_HIP_ERROR,
              "a3d_point_clouds_cluster_device: a hash table filled up or a union-find loop ran past its bound");
  scatter_words(&words[n_jobs], cloud_of_job, out_dropped), scatter_words(&words[2 * n_jobs], cloud_of_job, out_clusters);
  scatter_words(&words[3 * n_jobs], cloud_of_job, out_noise);
  return A3D_OK;
}

a3d_status a3d_knn_distance_threshold(const uint64_t stats[4], double std_ratio, uint32_t* out_hi) {
  A3D_REQUIRE(stats && out_hi, A3D_INVALID_PARAMETER, "null argument");
  A3D_REQUIRE(std::isfinite(std_ratio) && std_ratio >= 0.0, A3D_INVALID_PARAMETER,
              "a3d_knn_distance_threshold: std_ratio must be finite and not negative");
  const uint64_t m = stats[0], sum = stats[1];
  // what a cloud of fewer than 2^32 rows and k <= 32 can give (the header's bound): nothing below can overflow
  A3D_REQUIRE(m < (1ull << 32) && sum < (1ull << 53) && stats[3] < (1ull << 42), A3D_INVALID_PARAMETER,
              "a3d_knn_distance_threshold: statistics that no call can have produced");
  if (m == 0) {
    *out_hi = 0;
    return A3D_OK;
  }
  typedef unsigned __int128 u128;
  const u128 squares = (u128)stats[2] + ((u128)stats[3] << 32);
  const u128 left = (u128)m * squares, right = (u128)sum * sum;
  A3D_REQUIRE(left >= right, A3D_INVALID_PARAMETER,
              "a3d_knn_distance_threshold: statistics that no call can have produced");
  const u128 num = left - right;
  const double mean = (double)sum / (double)m;
  const double var = m < 2 ? 0.0 : (double)num / ((double)m * (double)(m - 1));
  const double t = std::floor(mean + std_ratio * std::sqrt(var));
  *out_hi = t >= 4294967294.0 ? 0xFFFFFFFEu : t > 0.0 ? (uint32_t)t : 0u;
  return A3D_OK;
}

}  // extern "C"
