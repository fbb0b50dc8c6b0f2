"""The rules of a3d_point_clouds_knn_distance_device, a3d_knn_distance_threshold and a3d_point_clouds_select_device
(align3d_amd/csrc/cloud_outliers.hip) restated in numpy, brute force over pairs, chunked; the grid is
normals_restatement.cells, the threshold is Python integers and floats.  It is the expected value of every outlier test
and never the code under test.  numpy evaluates each f32 operation on its own (no fused multiply-add, IEEE divide and
sqrt), which is the arithmetic the library is compiled for; a Python float is an IEEE double.

The rule of the knn call.  All f32 operations are rounded on their own (-ffp-contract=off, correctly rounded / and
sqrtf).  Per call: radius r, finite and > 0; 0 <= k <= 32.  Host constants: r2 = r * r, s = 32768.0f / r.
 1. Grid.  Pitch v = r, origin (0, 0, 0), cell and key by voxel_key.  A point whose key is refused (NaN, infinite,
    outside +-2^20 cells) is DROPPED: it is nobody's neighbour, and it gets count 0 and qsum 0xFFFFFFFF.
 2. Neighbours of point i.  Every kept point j of the same cloud, i itself included, such that each cell coordinate of
    j differs from i's by at most 1, and with d_k = p_jk - p_ik, d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2.  These are
    steps 1 and 2 of a3d_point_clouds_estimate_normals_device (cloud_normals.hip), word for word.
 3. Counts.  counts[i] = N, the number of neighbours, the row itself included; 0 for a dropped row.  The same bits as
    the d_out_counts of the normals entry at the same radius.
 4. Lattice distance.  The OTHERS of row i are its neighbours with a different row index (a duplicate point is an
    other at distance 0).  For each other, t = (uint32) rintf(sqrtf(d2) * s), ties to even.  t is non-decreasing in
    d2, so the k smallest d2 give the k smallest t.
 5. Distance sum.  qsum[i] = Q = the sum of the k smallest t; 0xFFFFFFFF if the row is dropped or has fewer than k
    others.  The multiset of the k smallest values is unique, so Q does not depend on the order of the candidates.
 6. Statistics.  Per cloud, over the m rows whose Q is not 0xFFFFFFFF: {m, sum Q, sum (Q*Q & 0xFFFFFFFF),
    sum (Q*Q >> 32)}, u64 integer sums: the same bits on every run and under any permutation of the rows.  r2 is at most
    twice r*r (a denormal product), so t <= 46342 < 2^16, Q < 2^21, Q*Q < 2^42; with len < 2^32 the four sums stay
    below 2^32, 2^53, 2^64 and 2^42.
 k == 0 is the count-only form: no distances, no qsum, statistics all zero.

The threshold.  With {m, SQ, lo, hi} = stats and SQ2 = lo + hi * 2^32: mu = (double)SQ / (double)m; num = m * SQ2 - SQ * SQ
exactly; var = (double)num / ((double)m * (double)(m - 1)), 0 when m < 2; T = floor(mu + std_ratio * sqrt(var)) clamped to
[0, 0xFFFFFFFE]; m == 0 gives 0.

The select.  Row p is kept iff lo <= values[p] <= hi; kept rows keep their order.
"""
import math

import numpy as np

import normals_restatement as NR

F = np.float32
NONE = 0xFFFFFFFF
FAR = np.int64(1) << 40  # what a candidate that is no other counts as among the lattice distances


def knn_distance(points, radius, k, chunk=256, slab=True, rows=None, rint=np.rint):
    """(counts [n] uint32, qsum [n] uint32 or None when k == 0, stats (m, sum Q, sum Q^2 & 0xFFFFFFFF, sum Q^2 >> 32) as
    Python ints).  rows: compute only these rows (against every candidate, as always); the others come back as count 0 and
    qsum NONE and mean nothing, and the statistics are those of the computed rows.  slab: as normals_restatement.moments
    (only columns that step 2 refuses anyway are left out).  rint: the rounding of step 4 (the rule's is np.rint, ties to
    even; the edge-case tests pass another one to show that their inputs tell the two apart)."""
    assert 0 <= k <= 32
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(p)
    r = F(radius)
    r2, s = r * r, F(32768.0) / r
    assert r2.dtype == F and s.dtype == F
    kept, cell = NR.cells(p, r)
    counts = np.zeros(n, np.int64)
    qsum = np.full(n, NONE, np.int64)
    idx = np.flatnonzero(kept)
    idx = idx[np.argsort(cell[idx, 0], kind="stable")]
    cx = cell[idx, 0]
    wanted = idx if rows is None else idx[np.isin(idx, np.asarray(rows))]
    for a in range(0, len(wanted), chunk):
        these = wanted[a:a + chunk]
        if slab:
            lo, hi = np.searchsorted(cx, cell[these[0], 0] - 1, "left"), np.searchsorted(cx, cell[these[-1], 0] + 1, "right")
            cols = idx[lo:hi]
        else:
            cols = idx
        pr, pc, cr, cc = p[these], p[cols], cell[these].astype(np.int32), cell[cols].astype(np.int32)
        with np.errstate(all="ignore"):
            d = [pc[None, :, j] - pr[:, None, j] for j in range(3)]  # d_k = p_jk - p_ik, every pair of the chunk
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert d2.dtype == F
            nb = d2 <= r2
            for j in range(3):
                nb &= np.abs(cc[None, :, j] - cr[:, None, j]) <= 1
            counts[these] = nb.sum(axis=1)
            if k:
                other = nb & (cols[None, :] != these[:, None])
                lattice = rint(np.sqrt(np.where(other, d2, F(0))) * s)
                assert lattice.dtype == F
                t = np.where(other, lattice.astype(np.int64), FAR)
        if k:
            enough = other.sum(axis=1) >= k
            if t.shape[1] < k:
                t = np.concatenate([t, np.full((len(these), k - t.shape[1]), FAR)], axis=1)
            smallest = np.sort(t, axis=1)[:, :k].sum(axis=1)
            qsum[these] = np.where(enough, smallest, NONE)
    has = qsum != NONE
    q = [int(v) for v in qsum[has]] if k else []
    stats = (len(q), sum(q), sum(v * v & 0xFFFFFFFF for v in q), sum(v * v >> 32 for v in q))
    return counts.astype(np.uint32), (qsum.astype(np.uint32) if k else None), stats


def stats_of(qsum):
    """Step 6 from a qsum array of fewer than 2^31 rows (no u64 sum can wrap), as Python ints."""
    q = np.asarray(qsum).astype(np.uint64)
    assert len(q) < 1 << 31
    q = q[q != NONE]
    sq = q * q
    return (len(q), int(q.sum()), int((sq & np.uint64(0xFFFFFFFF)).sum()), int((sq >> np.uint64(32)).sum()))


def threshold(stats, std_ratio):
    """a3d_knn_distance_threshold: num in Python ints (exact), the rest in doubles, operation by operation."""
    m, total, low, high = (int(x) for x in stats)
    if m == 0:
        return 0
    squares = low + (high << 32)
    num = m * squares - total * total
    assert num >= 0
    mean = float(total) / float(m)
    var = 0.0 if m < 2 else float(num) / (float(m) * float(m - 1))  # (float(int) rounds to nearest even, as the cast does)
    t = math.floor(mean + float(std_ratio) * math.sqrt(var))
    return int(min(max(t, 0), 0xFFFFFFFE))


def select(values, lo, hi):
    """The input rows that a3d_point_clouds_select_device keeps, in order (uint32)."""
    v = np.asarray(values).astype(np.int64)
    return np.flatnonzero((v >= int(lo)) & (v <= int(hi))).astype(np.uint32)


def remove_radius_outliers(points, radius, min_neighbors):
    """The rows DevicePointCloud.remove_radius_outliers keeps."""
    counts, _, _ = knn_distance(points, radius, 0)
    return select(counts, min_neighbors, NONE)


def remove_statistical_outliers(points, radius, k, std_ratio):
    """(the rows DevicePointCloud.remove_statistical_outliers keeps, the threshold T)."""
    _, qsum, stats = knn_distance(points, radius, k)
    t = threshold(stats, std_ratio)
    return select(qsum, 0, t), t
