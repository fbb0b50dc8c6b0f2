// Normals of resident clouds from their own neighbourhoods: per point, the eigenvector of the smallest eigenvalue of the
// scatter matrix of the points within a radius, oriented towards a viewpoint (or along the normal the row already has).
// The image pipeline gets its normals from the pixel grid (compute_normals); this is the same step for a cloud that has
// no grid: a lidar scan, an uploaded cloud, the extract of a voxel map.  A row with a zero normal takes no part in any
// alignment (angle_between_normals of a zero normal is pi / 2, which dot_reject_max of pcl_icp.hpp rejects for every
// max_normal_angle < pi / 2), so nothing is compacted here.
//
// The rule.  All f32 operations are rounded on their own (-ffp-contract=off, correctly rounded / and sqrtf).
// Per call: radius r, finite and > 0; min_neighbors, at least 3.  Per cloud: a viewpoint e, three finite f32, default the
// origin.  Host constants: r2 = r * r, s = 32768.0f / r.
//  1. Grid.  Pitch v = r, origin (0, 0, 0), cell and key by voxel_key.  A point whose key is refused (NaN, infinite,
//     outside +-2^20 cells) is DROPPED: it is nobody's neighbour, and it gets normal (0, 0, 0), count 0, curvature 0.
//  2. Neighbours of point i.  Every kept point j of the same cloud, i itself included, such that each cell coordinate of
//     j differs from i's by at most 1, and with d_k = p_jk - p_ik, (d_x*d_x + d_y*d_y) + d_z*d_z <= r2.  This is the
//     definition, not an approximation of "within r": a point on the very edge of the ball whose quotient rounds into a
//     cell two away is, by this rule, not a neighbour.
//  3. Moments.  All in integers, hence independent of the order in which neighbours are met.
//     q_k = (int) rintf(d_k * s), ties to even, so |q_k| <= 32769.  N = sum 1, S_k = sum q_k, M_kl = sum q_k q_l (six of
//     them), all int64.  With len < 2^32 these cannot overflow.
//  4. Scatter matrix.  In f64, multiply and subtract only: A_kl = (double)N * (double)M_kl - (double)S_k * (double)S_l.
//     This is N times the covariance and has the same eigenvectors.  mx = max |A_kl|.  The row is VALID iff
//     N >= min_neighbors and mx > 0.  Otherwise normal 0, curvature 0, and the count is still reported.  Scale by an exact
//     power of two: frexp(mx) gives exponent e, and B_kl = (float) ldexp(A_kl, -e).
//  5. Eigenvectors.  Cyclic Jacobi in f32, exactly 6 sweeps over the pairs (0,1), (0,2), (1,2).  There is no convergence
//     test, so it is wave-uniform.  For a pair (p, q), with third index o:
//       skip the pair iff a_pq == 0
//       theta = (a_qq - a_pp) / (2 a_pq)
//       t = (theta < 0 ? -1 : 1) / (|theta| + sqrtf(theta*theta + 1))
//       c = 1 / sqrtf(t*t + 1),  s = t*c
//       a_pp -= t*a_pq,  a_qq += t*a_pq,  a_pq = 0
//       a_op' = c*a_op - s*a_oq,  a_oq' = s*a_op + c*a_oq, both from the old values
//       columns of V (identity at the start): V_kp' = c*V_kp - s*V_kq,  V_kq' = s*V_kp + c*V_kq
//     An infinite theta gives t = 0, c = 1.  No NaN can arise from finite input.
//  6. Normal.  Let m be the index of the smallest diagonal entry (ties: lowest index) and n column m of V.
//     n = n / sqrtf((n_x*n_x + n_y*n_y) + n_z*n_z).  curvature = lambda_m / ((lambda_0 + lambda_1) + lambda_2), or 0 if
//     that sum is not > 0.
//  7. Sign.  By default: w_k = e_k - p_ik, dot = (n_x*w_x + n_y*w_y) + n_z*w_z, and n is negated iff dot < 0.  With
//     orient_by_normals, w is the row's existing normal instead.  This form refreshes a map's normals without knowing
//     which camera saw each cell.
//
// One upload, one fill and four launches over every tile of every cloud of a batch, whatever the batch size (the job
// table of cloud_batch.hpp); no block waits on another block.  The grid is a hash table per cloud that, unlike the
// downsample's, keeps ALL points of a cell: a counting sort by cell.
//  1.-3. cell_count_kernel, cell_place_kernel, cell_scatter_kernel of cell_sort.hpp: the counting sort, shared with the
//     knn and cluster entries of cloud_outliers.hip.  The order of the cells in memory is free: the moments do not depend
//     on it.  Each dropped point gets its zeros in the scatter (NormalsJob::drop_row).
//  4. normals_estimate_kernel, the hot path: a thread per record IN CELL ORDER, so that a wave's 64 lanes belong to the
//     same or adjacent cells and the 27 slot lookups and the candidate loads are largely the same addresses across the
//     wave.  It sums the ten integers (one v_mad_i64_i32 per product term), does steps 4-7 in registers and stores to the
//     row of the record's index.  In place (out == the cloud's normals) a thread reads only its own row's old normal, and
//     before it writes.  The candidates of a cell are loaded four at a time, so that a thread waits for memory once per
//     four of them.  The diagnostics build keeps the forms that lose (A3D_NORMALS_ORDER=input: a thread per point of the
//     cloud, in input order; A3D_NORMALS_AHEAD=1: one candidate per trip; A3D_NORMALS_LDS=1: a wave stages the runs its
//     lanes share in LDS), which scripts/cloud_normals_probe.py measures against this one.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cell_sort.hpp"  // the hash grid, the counting sort by cell, cell_run, consume_run

using namespace a3d;

namespace {

constexpr int CN_SWEEPS = 6;

// One non-empty cloud of a batch as the kernels see it (uploaded per call).
struct NormalsJob {
  const float* points;
  const float* old_normals;  // orient_by_normals: the rows' existing normals (may be out_normals); else null
  float* out_normals;
  float* out_curvature;  // null: not written
  uint32_t* out_counts;  // null: not written
  VoxelSlot* table;      // slot_mask + 1 slots, zeroed before the count: key word 0 = empty, else key + 1
  CellRecord* sorted;    // len records, the first `kept` of them written
  unsigned long long slot_mask;
  uint32_t len, first_tile, chunks_per_tile, n_tiles;
  float ex, ey, ez;
  uint32_t pad;

  __device__ void drop_row(uint32_t p) const {  // (cell_scatter_kernel) step 1's zeros
    const f32x3 zero = {0.f, 0.f, 0.f};
    *(f32x3_u*)(out_normals + 3 * (size_t)p) = zero;
    if (out_curvature) out_curvature[p] = 0.f;
    if (out_counts) out_counts[p] = 0u;
  }
};
static_assert(sizeof(NormalsJob) == 96, "NormalsJob layout");

struct CnParams {
  float r, r2, s;
  uint32_t min_neighbors;
};

// One Jacobi rotation of step 5 on the pair (p, q) with third index o.
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& aop, float& aoq, float& v0p,
                                              float& v0q, float& v1p, float& v1q, float& v2p, float& v2q) {
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  const float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
  const float h = t * apq;
  app = app - h, aqq = aqq + h, apq = 0.f;
  const float op = aop, oq = aoq;
  aop = c * op - s * oq, aoq = s * op + c * oq;
  float a = v0p, b = v0q;
  v0p = c * a - s * b, v0q = s * a + c * b;
  a = v1p, b = v1q;
  v1p = c * a - s * b, v1q = s * a + c * b;
  a = v2p, b = v2q;
  v2p = c * a - s * b, v2q = s * a + c * b;
}

// Pass 4.  SORTED: a thread per record, in cell order; else a thread per point of the cloud, in input order (diagnostics).
// AHEAD: CELL_AHEAD; 1 is the plain candidate loop (diagnostics).  LDS: a wave stages the runs its lanes share in LDS
// (diagnostics).
// valid[job] += valid rows.
template <bool SORTED, uint32_t AHEAD, bool LDS>
__global__ void __launch_bounds__(CELL_THREADS)
    normals_estimate_kernel(const NormalsJob* __restrict__ jobs, uint32_t n_jobs, VoxelGrid grid, CnParams prm,
                            const unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ valid) {
  __shared__ f32x4 s_stage[LDS ? CELL_THREADS / 64 : 1][LDS ? 64 : 1];
  const uint32_t tile = blockIdx.x, ji = find_job(jobs, n_jobs, tile);
  const NormalsJob& j = jobs[ji];
  const VoxelSlot* __restrict__ table = j.table;
  const CellRecord* __restrict__ sorted = j.sorted;
  const unsigned long long mask = j.slot_mask;
  const uint32_t len = j.len, span = j.chunks_per_tile * CELL_CHUNK;
  const uint32_t kept = (uint32_t)min(cursor[ji], (unsigned long long)len);
  const uint32_t rows = SORTED ? kept : len;
  const uint32_t p0 = (tile - j.first_tile) * span, p_end = min(rows, p0 + span);
  uint32_t n_valid = 0;
  for (uint32_t base = p0; base < p_end; base += CELL_THREADS) {  // block-uniform
    const uint32_t t = base + threadIdx.x;
    bool is_valid = false;
    f32x3 pi = {0.f, 0.f, 0.f};
    uint32_t row = t;
    unsigned long long key;
    bool live = t < p_end;
    if (live) {
      if (SORTED) {
        const f32x4 rec = *(const f32x4*)(sorted + t);
        pi.x = rec.x, pi.y = rec.y, pi.z = rec.z, row = __float_as_uint(rec.w);
        live = voxel_key(pi, grid, &key, nullptr) && row < len;  // (always: the record is a kept point's)
      } else {
        pi = *(const f32x3_u*)(j.points + 3 * (size_t)t);
        live = voxel_key(pi, grid, &key, nullptr);  // dropped rows got their zeros in pass 3
      }
    }
    const int kx = live ? (int)(key >> 42) : 0, ky = live ? (int)(key >> 21 & 0x1FFFFF) : 0, kz = live ? (int)(key & 0x1FFFFF) : 0;
    uint32_t N = 0;
    long long sx = 0, sy = 0, sz = 0, mxx = 0, mxy = 0, mxz = 0, myy = 0, myz = 0, mzz = 0;
    auto consume = [&](const f32x4 rec) {  // steps 2 and 3 for one candidate of a neighbouring cell
      const float dx = rec.x - pi.x, dy = rec.y - pi.y, dz = rec.z - pi.z;
      if (!((dx * dx + dy * dy) + dz * dz <= prm.r2)) return;
      const int qx = (int)__builtin_rintf(dx * prm.s), qy = (int)__builtin_rintf(dy * prm.s),
                qz = (int)__builtin_rintf(dz * prm.s);
      ++N;
      sx += qx, sy += qy, sz += qz;
      mxx += (long long)qx * qx, mxy += (long long)qx * qy, mxz += (long long)qx * qz;
      myy += (long long)qy * qy, myz += (long long)qy * qz, mzz += (long long)qz * qz;
    };
    for (int c = 0; c < 27; ++c) {  // (LDS: every lane of the wave walks the 27 cells, a dead lane with an empty run)
      if (!LDS && !live) break;
      uint32_t begin = 0, end = 0;  // the run of the cell's records
      if (live) cell_run(table, mask, kept, kx, ky, kz, c, &begin, &end);
      if (LDS) {
        // The lanes of a wave that ask for the same run (in cell order: most of them) get it through LDS: the wave loads
        // 64 records of the run with one coalesced load, and the lanes whose run it is read them back one by one.
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint64_t pending = __builtin_amdgcn_ballot_w64(end > begin);
        while (pending) {  // wave-uniform
          const int leader = __builtin_ctzll(pending);
          const uint32_t lb = __shfl(begin, leader, 64), le = __shfl(end, leader, 64);
          const bool mine = end > begin && begin == lb && end == le;
          pending &= ~__builtin_amdgcn_ballot_w64(mine);
          for (uint32_t at = lb; at < le; at += 64) {  // wave-uniform
            if (at + lane < le) s_stage[wave][lane] = *(const f32x4*)(sorted + at + lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t held = min(64u, le - at);
            if (mine)
              for (uint32_t u = 0; u < held; ++u) consume(s_stage[wave][u]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (the next trip overwrites the stage)
          }
        }
      } else {
        consume_run<AHEAD>(sorted, begin, end, consume);
      }
    }
    if (live) {
      // step 4
      const double dn = (double)N, dsx = (double)sx, dsy = (double)sy, dsz = (double)sz;
      const double axx = dn * (double)mxx - dsx * dsx, ayy = dn * (double)myy - dsy * dsy,
                   azz = dn * (double)mzz - dsz * dsz, axy = dn * (double)mxy - dsx * dsy,
                   axz = dn * (double)mxz - dsx * dsz, ayz = dn * (double)myz - dsy * dsz;
      const double big = fmax(fmax(fmax(fabs(axx), fabs(ayy)), fmax(fabs(azz), fabs(axy))), fmax(fabs(axz), fabs(ayz)));
      f32x3 n = {0.f, 0.f, 0.f};
      float curvature = 0.f;
      if (N >= prm.min_neighbors && big > 0.0) {
        is_valid = true;
        int e;
        (void)frexp(big, &e);
        float a00 = (float)ldexp(axx, -e), a11 = (float)ldexp(ayy, -e), a22 = (float)ldexp(azz, -e),
              a01 = (float)ldexp(axy, -e), a02 = (float)ldexp(axz, -e), a12 = (float)ldexp(ayz, -e);
        float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
        for (int sweep = 0; sweep < CN_SWEEPS; ++sweep) {
          jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0,1), o = 2
          jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0,2), o = 1
          jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1,2), o = 0
        }
        // step 6
        float lam = a00;
        n.x = v00, n.y = v10, n.z = v20;
        if (a11 < lam) lam = a11, n.x = v01, n.y = v11, n.z = v21;
        if (a22 < lam) lam = a22, n.x = v02, n.y = v12, n.z = v22;
        const float norm = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
        n.x = n.x / norm, n.y = n.y / norm, n.z = n.z / norm;
        const float sum = (a00 + a11) + a22;
        curvature = sum > 0.f ? lam / sum : 0.f;
        // step 7
        f32x3 w;
        if (j.old_normals) w = *(const f32x3_u*)(j.old_normals + 3 * (size_t)row);
        else w.x = j.ex - pi.x, w.y = j.ey - pi.y, w.z = j.ez - pi.z;
        const float dot = (n.x * w.x + n.y * w.y) + n.z * w.z;
        if (dot < 0.f) n.x = -n.x, n.y = -n.y, n.z = -n.z;
      }
      *(f32x3_u*)(j.out_normals + 3 * (size_t)row) = n;
      if (j.out_curvature) j.out_curvature[row] = curvature;
      if (j.out_counts) j.out_counts[row] = N;
    }
    n_valid += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(is_valid));  // wave-uniform
  }
  if ((threadIdx.x & 63u) == 0 && n_valid) atomicAdd(&valid[ji], (unsigned long long)n_valid);
}

}  // namespace

extern "C" {

a3d_status a3d_point_clouds_estimate_normals_device(a3d_context* ctx, const a3d_point_cloud_view* d_clouds, uint64_t n,
                                                    float radius, uint32_t min_neighbors, const float* viewpoints_host,
                                                    int32_t orient_by_normals, float* const* d_out_normals,
                                                    float* const* d_out_curvature, uint32_t* const* d_out_counts,
                                                    uint64_t* out_valid, uint64_t* out_dropped) {
  if (n == 0) return A3D_OK;
  A3D_REQUIRE(ctx && d_clouds && d_out_normals && out_valid, A3D_INVALID_PARAMETER, "null argument");
  static const char NAME[] = "a3d_point_clouds_estimate_normals_device";
  VoxelGrid grid;
  CnParams prm{radius, 0.f, 0.f, min_neighbors};
  A3D_TRY(radius_grid_from(NAME, radius, &grid, &prm.r2, &prm.s));
  A3D_REQUIRE(min_neighbors >= 3, A3D_INVALID_PARAMETER,
              "a3d_point_clouds_estimate_normals_device: min_neighbors must be at least 3 (a plane needs three points)");
  if (viewpoints_host)
    for (uint64_t i = 0; i < 3 * n; ++i)
      A3D_REQUIRE(std::isfinite(viewpoints_host[i]), A3D_INVALID_PARAMETER,
                  "a3d_point_clouds_estimate_normals_device: the viewpoints must be finite");
  std::vector<NormalsJob> jobs;
  std::vector<uint64_t> cloud_of_job;
  RangeRecorder ranges;
  jobs.reserve(n), cloud_of_job.reserve(n), ranges.reserve(5 * n);
  CellSortPlan plan;
  for (uint64_t i = 0; i < n; ++i) {
    const a3d_point_cloud_view& c = d_clouds[i];
    A3D_REQUIRE(c.len < (1ull << 32), A3D_INVALID_PARAMETER, "a cloud of 2^32 points or more");
    if (c.len == 0) continue;  // yields zeros; its pointers may be null
    A3D_REQUIRE(c.points && d_out_normals[i], A3D_INVALID_PARAMETER, "null points or output pointer");
    A3D_REQUIRE(!orient_by_normals || c.normals, A3D_MISSING_FIELD,
                "a3d_point_clouds_estimate_normals_device: orient_by_normals on a cloud without normals");
    NormalsJob j{};
    j.points = c.points, j.old_normals = orient_by_normals ? c.normals : nullptr;
    j.out_normals = d_out_normals[i];
    j.out_curvature = d_out_curvature ? d_out_curvature[i] : nullptr;
    j.out_counts = d_out_counts ? d_out_counts[i] : nullptr;
    if (viewpoints_host) j.ex = viewpoints_host[3 * i], j.ey = viewpoints_host[3 * i + 1], j.ez = viewpoints_host[3 * i + 2];
    A3D_TRY(cell_sort_plan(&plan, NAME, c.len, &j));
    jobs.push_back(j), cloud_of_job.push_back(i);
    ranges.in(j.points, c.len * 12);
    // in place is the one allowed overlap: a thread reads its own row's old normal before it writes the new one
    if (j.old_normals != j.out_normals) ranges.in(j.old_normals, c.len * 12);
    ranges.out(j.out_normals, c.len * 12), ranges.out(j.out_curvature, c.len * 4), ranges.out(j.out_counts, c.len * 4);
  }
  if (ranges.overlap())
    return refuse(A3D_INVALID_PARAMETER, NAME,
                  "an output overlaps an input or another output (only the normals may be estimated in place)");
  zero_results(out_valid, n), zero_results(out_dropped, n);
  if (jobs.empty()) return A3D_OK;
  const size_t n_jobs = jobs.size();
  A3D_HIP_TRY(hipSetDevice(ctx->device));
  BatchScratch scratch;  // the words: cursors (kept counts), dropped, valid, fault; the tail: hash tables | records
  A3D_TRY(batch_scratch(ctx, n_jobs * sizeof(NormalsJob), 3 * n_jobs + 1, 0, plan.tables.bytes + plan.sorted.bytes, &scratch));
  place_parts(scratch.tail, {&plan.tables, &plan.sorted});
  for (NormalsJob& j : jobs) cell_sort_rebase(plan, &j);
  const NormalsJob* d_jobs = (const NormalsJob*)scratch.jobs;
  unsigned long long* d_cursor = scratch.words;
  unsigned long long* d_dropped = d_cursor + n_jobs;
  unsigned long long* d_valid = d_cursor + 2 * n_jobs;
  unsigned long long* d_fault = d_cursor + 3 * n_jobs;
  hipStream_t s = ctx->stream;
  A3D_TRY(batch_upload(scratch, jobs.data(), s));
  A3D_HIP_TRY(hipMemsetAsync(plan.tables.base, 0, plan.tables.bytes, s));  // every key word empty, every count 0
  const dim3 grid_dim((uint32_t)plan.tiles), block(CELL_THREADS);
  const uint32_t nj = (uint32_t)n_jobs;
  A3D_TRY(cell_sort_launch(d_jobs, nj, plan.tiles, grid, d_cursor, d_dropped, d_fault, s));
  const unsigned long long* d_kept = d_cursor;
#ifdef A3D_DIAGNOSTICS  // the forms that were measured slower (scripts/cloud_normals_probe.py)
  const char* order = getenv("A3D_NORMALS_ORDER");
  const char* ahead = getenv("A3D_NORMALS_AHEAD");
  const char* lds = getenv("A3D_NORMALS_LDS");
  if (order && !strcmp(order, "input"))
    hipLaunchKernelGGL((normals_estimate_kernel<false, CELL_AHEAD, false>), grid_dim, block, 0, s, d_jobs, nj, grid, prm, d_kept, d_valid);
  else if (lds && !strcmp(lds, "1"))
    hipLaunchKernelGGL((normals_estimate_kernel<true, 1, true>), grid_dim, block, 0, s, d_jobs, nj, grid, prm, d_kept, d_valid);
  else if (ahead && !strcmp(ahead, "1"))
    hipLaunchKernelGGL((normals_estimate_kernel<true, 1, false>), grid_dim, block, 0, s, d_jobs, nj, grid, prm, d_kept, d_valid);
  else
#endif
    hipLaunchKernelGGL((normals_estimate_kernel<true, CELL_AHEAD, false>), grid_dim, block, 0, s, d_jobs, nj, grid, prm, d_kept, d_valid);
  A3D_HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words;
  A3D_TRY(download_words(d_cursor, 3 * n_jobs + 1, s, &words));
  A3D_REQUIRE(words[3 * n_jobs] == 0, A3D_HIP_ERROR, "a3d_point_clouds_estimate_normals_device: a hash table filled up");
  scatter_words(&words[2 * n_jobs], cloud_of_job, out_valid), scatter_words(&words[n_jobs], cloud_of_job, out_dropped);
  return A3D_OK;
}

}  // extern "C"
