"""The rule of a3d_point_clouds_segment_plane_device (align3d_amd/csrc/cloud_plane.hip) restated in numpy: f64 arrays for
step 1, np.float32 arrays for steps 2 and 5, Python ints for step 6, brute force over rows x candidates.  It is the
expected value of every plane test and never the code under test.  numpy evaluates each operation on its own (no fused
multiply-add, IEEE divide and sqrt), which is the arithmetic the library is compiled for.

The rule of the plane call.  Every f32 and every f64 operation is rounded on its own, as the build's
-ffp-contract=off already ensures.  Divide and sqrt are correctly rounded.
Per call: a distance threshold t, f32, finite and > 0, and a number of refinement rounds R with 0 <= R <= 8.
Per cloud i: H_i candidate triples (a, b, c) of row numbers, [H_i][3] u32 in HOST memory.  0 <= H_i <= 4096.  Every
index is < len_i.
 1. Candidate plane of a triple.  The three points are widened to f64.  u = p_b - p_a, v = p_c - p_a.  m = u x v, each
    component as u_y*v_z - u_z*v_y.  L = (m_x*m_x + m_y*m_y) + m_z*m_z.  U = (u_x*u_x + u_y*u_y) + u_z*u_z, and V
    likewise.  The candidate is DEGENERATE iff two of its indices are equal, or L is not finite, or not
    L > (U*V) * 2^-20.  That covers a repeated row, a non-finite row, and three rows whose sine is below 2^-10.
    Otherwise n = (float)(m / sqrt(L)) per component, and the plane's point is p_a, in f32 as stored.
 2. Distance and inlier, in f32.  e_k = p_k - p_ak, d = (n_x*e_x + n_y*e_y) + n_z*e_z.  Row p is an inlier of the
    candidate iff fabsf(d) <= t.  A row with a NaN or an infinity is never an inlier.  The form p - a is deliberate.
    n.p + w saves three operations per test and cancels badly for clouds far from the origin.
 3. Score.  count[h] is the number of inliers of candidate h over ALL rows of the cloud, and 0 for a degenerate
    candidate.  The best candidate maximises count[h] << 32 | (0xFFFFFFFF - h): the most inliers, the lowest h on a
    tie.  If every candidate is degenerate, or H_i == 0 or len_i == 0, there is no plane: flags all 0, plane four
    zeros, best = 0xFFFFFFFF, status A3D_OK.
 4. Flags.  flags[p] = 1 iff p is an inlier of the current plane (n, point), else 0.  After step 3 the current plane
    is the best candidate's.
 5. Refit moments over the rows with flag 1, all in integers.  s = 64.0f / t in f32.  q_k = (int) rintf(e_k * s), ties
    to even, with e from step 2 against the current plane's point.  A flagged row takes part iff
    fabsf(e_k * s) <= 1048576.0f for all three k.  N = sum 1, S_k = sum q_k, and for the six products P = q_k q_l, with
    |P| <= 2^40: Lo_kl = sum (P & 0x7FFFFFFF), Hi_kl = sum (P >> 31), an arithmetic shift.  So
    M_kl = Hi_kl * 2^31 + Lo_kl exactly.  With len < 2^32, N, S, Lo and Hi each fit 64 bits, so no order of summation
    can matter.  The record is 16 u64 words: N, S[3], Lo[6], Hi[6] in the order xx, xy, xz, yy, yz, zz.
 6. Plane from moments, on the HOST (a3d_plane_from_moments).  A_kl = N*M_kl - S_k*S_l, exact in 128-bit integers
    (|A| < 2^105).  Each A_kl converted to f64, round to nearest even.  mx = max |A_kl|.  The refit is VALID iff N >= 3
    and mx > 0.  Then steps 4 (scaling by frexp's exponent) to 6 (normal = column of the smallest diagonal entry,
    normalised) of the rule of a3d_point_clouds_estimate_normals_device: six cyclic Jacobi sweeps in f32.  Centroid in
    f64: c_k = (double)a_k + ((double)S_k / (double)N) / (double)s, with a the point that the moments were taken
    against.  d = -((n_x*c_x + n_y*c_y) + n_z*c_z) in f64, with n widened.  The four numbers are negated iff d < 0.
    This is the side the origin is on: the default viewpoint of the normals call.  If the refit is not valid, the
    plane is the current plane itself: its f32 normal widened, and c = a; d and the sign follow in the same way.
 7. Refinement, R times.  The current plane becomes the plane of step 6: normal (float)n, point (float)c.  Steps 4 and
    5 are repeated against it, then step 6.  R = 0 is the inliers of the best candidate and the model refitted to them.
Every count, flag and moment is an integer decided on f32 bits that no order can change: the same on every run.
"""
from collections import namedtuple

import numpy as np

from normals_restatement import jacobi

F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
KL = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
MASK64 = (1 << 64) - 1

Segmentation = namedtuple("Segmentation", "counts best flags plane inliers refit_rows moments")


def hypotheses(seed, length, H):
    """a3d_plane_hypotheses: uint32 [H, 3]."""
    out = np.zeros((H, 3), np.uint32)
    for w in range(3 * H):
        z = (seed + (w + 1) * 0x9E3779B97F4A7C15) & MASK64
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & MASK64
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & MASK64
        z ^= z >> 31
        out[w // 3, w % 3] = ((z >> 32) * length) >> 32
    return out


def candidates(points, triples):
    """Step 1: (normals [H, 3] f32, zero where degenerate; points [H, 3] f32; good [H] bool)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    tr = np.asarray(triples, np.int64).reshape(-1, 3)
    a, b, c = (p[tr[:, k]].astype(D) for k in range(3))
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        L = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        U = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        V = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        distinct = (tr[:, 0] != tr[:, 1]) & (tr[:, 0] != tr[:, 2]) & (tr[:, 1] != tr[:, 2])
        good = distinct & np.isfinite(L) & (L > (U * V) * D(2.0 ** -20))
        n = (m / np.sqrt(L)[:, None]).astype(F)
    assert m.dtype == D and n.dtype == F
    return np.where(good[:, None], n, F(0)), p[tr[:, 0]], good


def inliers(points, normal, point, t):
    """Step 2 for one plane over every row: [len] bool."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, a, t = np.asarray(normal, F), np.asarray(point, F), F(t)
    with np.errstate(all="ignore"):
        e = p - a[None, :]
        d = (n[0] * e[:, 0] + n[1] * e[:, 1]) + n[2] * e[:, 2]
        assert d.dtype == F
        return np.abs(d) <= t


def counts(points, triples, t, chunk=64):
    """Steps 1 to 3: (count [H] uint32, best or NONE, (normals, points, good) of step 1)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, a, good = candidates(p, triples) if len(p) else (np.zeros((0, 3), F),) * 2 + (np.zeros(0, bool),)
    H = len(good)
    out = np.zeros(H, np.uint32)
    t = F(t)
    with np.errstate(all="ignore"):
        for h0 in range(0, H, chunk):
            nn, aa = n[h0:h0 + chunk], a[h0:h0 + chunk]
            e = [p[:, None, k] - aa[None, :, k] for k in range(3)]
            d = (nn[None, :, 0] * e[0] + nn[None, :, 1] * e[1]) + nn[None, :, 2] * e[2]
            assert d.dtype == F
            out[h0:h0 + chunk] = (np.abs(d) <= t).sum(axis=0)
    out[~good] = 0
    best = NONE
    if good.any():
        keys = [(int(out[h]) << 32) | (0xFFFFFFFF - h) for h in range(H) if good[h]]
        best = 0xFFFFFFFF - (max(keys) & 0xFFFFFFFF)
    return out, best, (n, a, good)


def moments(points, flags, point, t, rint=np.rint):
    """Step 5: the record as 16 Python ints (S and Hi signed).  rint: the rounding of q_k (the rule's is np.rint, ties to
    even; the edge-case tests pass another one to show that their inputs tell the two apart)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    a = np.asarray(point, F)
    s = F(64.0) / F(t)
    assert s.dtype == F
    with np.errstate(all="ignore"):
        f = (p - a[None, :]) * s
        assert f.dtype == F
        part = np.asarray(flags, bool) & (np.abs(f) <= F(1048576.0)).all(axis=1)
        q = rint(f[part]).astype(np.int64)
    rec = [int(part.sum())] + [int(q[:, k].sum()) for k in range(3)]
    prods = [q[:, k] * q[:, l] for k, l in KL]
    rec += [int((P & 0x7FFFFFFF).sum()) for P in prods]
    rec += [int((P >> 31).sum()) for P in prods]
    return rec


def plane_from_moments(rec, point, t, fallback):
    """Step 6: (plane [4] f64, valid, centroid [3] f64)."""
    N, S = rec[0], rec[1:4]
    M = {kl: rec[10 + i] * (1 << 31) + rec[4 + i] for i, kl in enumerate(KL)}
    A = np.zeros((3, 3), D)
    for k, l in KL:
        A[k, l] = A[l, k] = float(N * M[(k, l)] - S[k] * S[l])  # Python's int -> float rounds to nearest even
    mx = np.abs(A).max()
    a = np.asarray(point, F)
    s = F(64.0) / F(t)
    valid = bool(N >= 3 and mx > 0)
    n, c = np.asarray(fallback, F).astype(D), a.astype(D)
    if valid:
        _, e = np.frexp(mx)
        B = np.ldexp(A, -int(e)).astype(F)
        lam, V = jacobi(B[None])
        col = V[0][:, int(np.argmin(lam[0]))]  # the first of equal minima
        norm = np.sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2])
        nv = col / norm
        assert nv.dtype == F
        n = nv.astype(D)
        c = np.array([D(a[k]) + (D(S[k]) / D(N)) / D(s) for k in range(3)], D)
    d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
    plane = np.array([n[0], n[1], n[2], d], D)
    if d < 0:
        plane = -plane
    return plane, valid, c


def segment(points, triples, t, refine=0, rint=np.rint):
    """The whole rule for one cloud (rint: see moments)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    triples = np.asarray(triples, np.int64).reshape(-1, 3)
    count, best, (n, a, _) = counts(p, triples, t)
    if best == NONE:
        return Segmentation(count, NONE, np.zeros(len(p), np.uint32), np.zeros(4, D), 0, 0, [])
    cur_n, cur_a = n[best], a[best]
    records = []
    for _ in range(refine + 1):
        flags = inliers(p, cur_n, cur_a, t)
        rec = moments(p, flags, cur_a, t, rint)
        records.append(rec)
        plane, _, c = plane_from_moments(rec, cur_a, t, cur_n)
        cur_n, cur_a = plane[:3].astype(F), c.astype(F)
    return Segmentation(count, best, flags.astype(np.uint32), plane, int(flags.sum()), rec[0], records)
