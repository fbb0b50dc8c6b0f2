// Voxel-grid downsampling of resident clouds: of the points that share a cell of a grid of pitch v anchored at o, the one
// nearest to the cell's centre is kept (ties: the lowest index), and the kept points come out in input order, copied bit
// for bit.  It is the rule of the reference's only downsampler (src/range_image/resize.rs:4-40: one real sample per cell,
// never an average, so normals stay true normals) carried over to clouds, with the cell CENTRE in place of the cell mean:
// an f32 mean depends on the summation order, the centre does not, and the pick becomes one integer minimum.
//
// Per point i, all in f32, every operation rounded on its own (-ffp-contract=off, correctly rounded divide):
//   c_k   = floorf((p_k - o_k) / v)            dropped unless every c_k is finite and in [-2^20, 2^20)
//   key   = (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20)
//   ctr_k = (c_k + 0.5f) * v + o_k,  d_k = p_k - ctr_k,  dist = (d_x * d_x + d_y * d_y) + d_z * d_z   (never NaN, may be +inf)
//   the winner of a key minimises  bits(dist) << 32 | i   (dist >= 0: its bit pattern is monotone)
//
// Three launches over every tile of every cloud of a batch plus one fill of the hash tables, whatever the batch size (the
// job table of cloud_batch.hpp); no block waits on another block:
//  1. voxel_insert_kernel: a thread per point claims the slot of its key in the cloud's open-addressing table (linear
//     probing, 64-bit atomicCAS on the key word; at most half the slots can ever be taken) and atomicMins its word into
//     the slot's second word.  Both are preceded by a device-scope load of the word: a slot that already holds the key
//     needs no CAS, a slot that already holds a smaller word needs no atomicMin (a stale value can only be larger than
//     the true one, so the test never skips a needed update).  Dropped points only count themselves.
//  2. voxel_flag_kernel: each point finds its key's slot again; it is the winner iff the slot's low 32 bits are its
//     index.  A wave stores its 64-bit ballot (one bit per point: the whole flag array is len / 8 bytes) and the block
//     its tile's winner count.
//  3. voxel_compact_kernel: each block sums its cloud's earlier tile counts for its offset (cloud_write_kernel's form: at
//     most VX_MAX_TILES tiles per cloud), ranks its winners from the stored ballots and writes point, normal and index at
//     offset + rank: input order.  It writes nothing if any cloud of the batch has more winners than its capacity, so
//     the host needs one wait, after everything, to read the counts back.  A cloud's colours ([len][3] u8), when the
//     caller passes them, follow the winner in this pass: three bytes beside the point (store_color, cloud_batch.hpp).
//     They play no part in passes 1 and 2.
#include <cmath>
#include <vector>

#include "voxel_grid.hpp"  // VoxelGrid, voxel_key, slot_hash, VoxelSlot: shared with voxel_map.hip

using namespace a3d;

namespace {

constexpr uint32_t VX_THREADS = 256;
constexpr uint32_t VX_WAVES = VX_THREADS / 64;
constexpr uint32_t VX_ROUNDS = 4;
constexpr uint32_t VX_CHUNK = VX_ROUNDS * VX_THREADS;  // points per chunk: a multiple of 64, so a ballot word never straddles tiles
constexpr uint32_t VX_GROUPS = VX_CHUNK / 64;          // ballot words per chunk
constexpr uint32_t VX_MAX_TILES = 4096;                // tiles per cloud at most (the offset sum of a block stays short)
static_assert(VX_GROUPS <= 64, "a wave's lanes hold the chunk's ballot words");

// One non-empty cloud of a batch as the kernels see it (uploaded per call).
struct VoxelJob {
  const float* points;
  const float* normals;  // read only when out_normals is set
  float* out_points;
  float* out_normals;   // null: no normals are written
  uint32_t* out_index;  // null: no indices are written
  VoxelSlot* table;     // slot_mask + 1 slots, filled with VX_EMPTY / ~0 before the insert
  unsigned long long* flags;  // (len + 63) / 64 ballot words
  unsigned long long slot_mask;
  unsigned long long capacity;
  uint32_t len, first_tile, chunks_per_tile, pad;
  const uint8_t* colors;  // read only when out_colors is set
  uint8_t* out_colors;    // null: no colours are written
};
static_assert(sizeof(VoxelJob) == 104, "VoxelJob layout");

// Pass 1.  dropped[job] += dropped points (zeroed by the host upload); *fault is set if a table were ever full (it cannot
// be: it has at least two slots per point).
__global__ void __launch_bounds__(VX_THREADS)
    voxel_insert_kernel(const VoxelJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid,
                        unsigned long long* __restrict__ dropped, unsigned long long* __restrict__ fault) {
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const VoxelJob& j = jobs[ji];
  const float* __restrict__ points = j.points;
  VoxelSlot* table = j.table;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * VX_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);  // (len < 2^32 - span: checked by the host)
  uint32_t n_dropped = 0;
  for (uint32_t p = p0 + threadIdx.x; p < p_end; p += VX_THREADS) {
    const f32x3 pt = *(const f32x3_u*)(points + 3 * (size_t)p);
    unsigned long long key;
    float dist;
    if (!voxel_key(pt, grid, &key, &dist)) {
      ++n_dropped;
      continue;
    }
    const unsigned long long word = (unsigned long long)__float_as_uint(dist) << 32 | p;
    unsigned long long s = slot_hash(key) & mask;
    bool placed = false;
    for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
      unsigned long long k = VX_LOAD_AGENT(&table[s].key);
      if (k == VX_EMPTY) k = atomicCAS(&table[s].key, VX_EMPTY, key);
      if (k == VX_EMPTY || k == key) {
        placed = true;
        break;
      }
    }
    if (!placed) {
      atomicMax(fault, 1ull);
      continue;
    }
    if (VX_LOAD_AGENT(&table[s].best) > word) atomicMin(&table[s].best, word);
  }
  n_dropped = wave_sum(n_dropped);
  if ((threadIdx.x & 63u) == 0 && n_dropped) atomicAdd(&dropped[ji], (unsigned long long)n_dropped);
}

// Pass 2: flags[p / 64] bit p % 64 = point p is its voxel's winner; tile_counts[tile] = winners of the tile; lens[job] +=
// the same (zeroed by the host upload).
__global__ void __launch_bounds__(VX_THREADS)
    voxel_flag_kernel(const VoxelJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, uint32_t* __restrict__ tile_counts,
                      unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_wave[VX_WAVES];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const VoxelJob& j = jobs[ji];
  const float* __restrict__ points = j.points;
  const VoxelSlot* __restrict__ table = j.table;
  unsigned long long* __restrict__ flags = j.flags;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * VX_CHUNK;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(len, p0 + span);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t c = 0;  // wave-uniform
  for (uint32_t base = p0 + wave * 64u; base < p_end; base += VX_THREADS) {  // wave-uniform
    const uint32_t p = base + lane;
    bool win = false;
    unsigned long long key;
    if (p < p_end && voxel_key(*(const f32x3_u*)(points + 3 * (size_t)p), grid, &key, nullptr)) {
      unsigned long long s = slot_hash(key) & mask;
      for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
        const unsigned long long k = table[s].key;
        if (k == key) {
          win = (uint32_t)table[s].best == p;
          break;
        }
        if (k == VX_EMPTY) break;  // (cannot happen: pass 1 placed every kept point)
      }
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(win);
    if (lane == 0) flags[base >> 6] = ballot;
    c += (uint32_t)__builtin_popcountll(ballot);
  }
  if (lane == 0) s_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (uint32_t w = 0; w < VX_WAVES; ++w) total += s_wave[w];
    tile_counts[tile] = total;
    if (total) atomicAdd(&lens[ji], (unsigned long long)total);
  }
}

// Pass 3: every winner of the tile to out[offset + rank].  Nothing is written anywhere if any cloud of the batch has
// more winners than its capacity (the host then returns A3D_INVALID_PARAMETER).
__global__ void __launch_bounds__(VX_THREADS)
    voxel_compact_kernel(const VoxelJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ tile_counts,
                         const unsigned long long* __restrict__ lens) {
  __shared__ uint32_t s_base, s_over;
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const VoxelJob& j = jobs[ji];
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
  const uint32_t len = j.len, span = j.chunks_per_tile * VX_CHUNK, n_groups = (len + 63u) >> 6;
  const uint32_t p0 = t * span, p_end = min(len, p0 + span);
  uint32_t base = s_base;  // winners of the cloud before this chunk
  for (uint32_t px0 = p0; px0 < p_end; px0 += VX_CHUNK) {
    // lane g < VX_GROUPS of every wave holds the ballot word of the chunk's group g (points px0 + 64 g ...), their
    // exclusive prefix gives every group's offset: no LDS, no block barrier
    const uint32_t g = (px0 >> 6) + lane;
    const uint64_t word = lane < VX_GROUPS && g < n_groups ? flags[g] : 0ull;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < (int)VX_GROUPS; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= (uint32_t)o) incl += up;
    }
    const uint32_t excl = incl - cnt;
    uint64_t ballots[VX_ROUNDS];
    uint32_t offs[VX_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < VX_ROUNDS; ++r) {  // (every lane takes part in the shuffles: no divergence yet)
      const int src = (int)(r * VX_WAVES + wave);  // the group of this wave's round r (round-major, then wave, then lane)
      ballots[r] = (uint64_t)__shfl((unsigned long long)word, src, 64);
      offs[r] = base + __shfl(excl, src, 64);
    }
    base += __shfl(incl, (int)VX_GROUPS - 1, 64);
#pragma unroll
    for (uint32_t r = 0; r < VX_ROUNDS; ++r) {
      const uint64_t ballot = ballots[r];
      if (!((ballot >> lane) & 1ull)) continue;
      const uint32_t p = px0 + r * VX_THREADS + threadIdx.x;
      const unsigned long long dst = (unsigned long long)offs[r] + lane_rank(ballot);
      if (p >= p_end || dst >= capacity) continue;  // (cannot happen: the bit is a point's, the total fits; a bound on every store)
      *(f32x3_u*)(out_points + 3 * dst) = *(const f32x3_u*)(points + 3 * (size_t)p);
      if (out_normals) *(f32x3_u*)(out_normals + 3 * dst) = *(const f32x3_u*)(normals + 3 * (size_t)p);
      if (out_index) out_index[dst] = p;
      if (out_colors) store_color(out_colors, dst, load_color(colors, p));
    }
  }
}

}  // namespace

extern "C" {

a3d_status a3d_point_clouds_voxel_downsample_rgb_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds,
                                                        const uint8_t* const* d_colors, uint64_t n, float voxel_size,
                                                        const float origin[3], float* const* d_out_points,
                                                        float* const* d_out_normals, uint8_t* const* d_out_colors,
                                                        uint32_t* const* d_out_index, const uint64_t* capacities,
                                                        uint64_t* out_lens, uint64_t* out_dropped) {
  if (n == 0) return A3D_OK;
  // (the rgb form and the plain one are one call: both report under the plain one's name)
  static const char NAME[] = "a3d_point_clouds_voxel_downsample_device";
  if (!(ctx && d_clouds && d_out_points && capacities && out_lens)) return refuse(A3D_INVALID_PARAMETER, NAME, "null argument");
  VoxelGrid grid;
  A3D_TRY(voxel_grid_from(NAME, voxel_size, origin, &grid));
  const CompactArgs args{d_clouds, d_colors, d_out_points, d_out_normals, d_out_colors, d_out_index, capacities};
  std::vector<VoxelJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(7 * n);
  uint64_t tiles = 0;
  TailPart flags, tables;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = d_clouds[i].len;
    if (len >= (1ull << 32)) return refuse(A3D_INVALID_PARAMETER, NAME, "a cloud of 2^32 points or more");
    if (len == 0) continue;  // yields no points; its pointers may be null
    VoxelJob j{};
    A3D_TRY(compact_front(NAME, args, i, true, "null points or output pointer", VX_CHUNK, VX_MAX_TILES, &tiles, &ranges, &j));
    const uint64_t slots = table_slots(len);
    j.slot_mask = slots - 1;
    flags.take(&j.flags, pad256((len + 63) / 64 * 8)), tables.take(&j.table, slots * sizeof(VoxelSlot));
    jobs.push_back(j), cloud_of_job.push_back(i);
  }
  if (ranges.overlap())
    return refuse(A3D_INVALID_PARAMETER, NAME, "an output overlaps an input or another output (there is no in-place form)");
  zero_results(out_lens, n), zero_results(out_dropped, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  BatchScratch scratch;  // the words: lens, dropped, fault; the tail: ballot words | hash tables
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(VoxelJob), 2 * n_jobs + 1, tiles, flags.bytes + tables.bytes, &scratch));
  place_parts(scratch.tail, {&flags, &tables});
  for (VoxelJob& j : jobs) flags.rebase(&j.flags), tables.rebase(&j.table);
  const VoxelJob* d_jobs = (const VoxelJob*)scratch.jobs;
  unsigned long long* d_lens = scratch.words;
  unsigned long long* d_dropped = d_lens + n_jobs;
  unsigned long long* d_fault = d_lens + 2 * n_jobs;
  uint32_t* d_tile_counts = scratch.tile_counts;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  A3D_HIP_TRY(hipMemsetAsync(tables.base, 0xFF, tables.bytes, s));  // every key VX_EMPTY, every best word ~0
  const dim3 grid_dim((uint32_t)tiles), block(VX_THREADS);
  hipLaunchKernelGGL(voxel_insert_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, d_dropped, d_fault);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(voxel_flag_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, grid, d_tile_counts, d_lens);
  A3D_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(voxel_compact_kernel, grid_dim, block, 0, s, d_jobs, (uint32_t)n_jobs, (const uint32_t*)d_tile_counts,
                     (const unsigned long long*)d_lens);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_lens, 2 * n_jobs + 1, s, &words));
  A3D_REQUIRE(words[2 * n_jobs] == 0, A3D_HIP_ERROR, "a3d_point_clouds_voxel_downsample_device: a hash table filled up");
  return compact_finish(NAME, "kept points", jobs, cloud_of_job, words.data(), out_lens, out_dropped);
}

a3d_status a3d_point_clouds_voxel_downsample_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                    float voxel_size, const float origin[3], float* const* d_out_points,
                                                    float* const* d_out_normals, uint32_t* const* d_out_index,
                                                    const uint64_t* capacities, uint64_t* out_lens, uint64_t* out_dropped) {
  return a3d_point_clouds_voxel_downsample_rgb_device(ctx, d_clouds, nullptr, n, voxel_size, origin, d_out_points,
                                                      d_out_normals, nullptr, d_out_index, capacities, out_lens, out_dropped);
}

}  // extern "C"
