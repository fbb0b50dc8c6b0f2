"""Seeded inputs that reach, by construction, the clauses of the three neighbourhood rules that random clouds, real frames
and the lattice at multiples of r never reach (no GPU needed to import):

  a3d_point_clouds_estimate_normals_device   normals_rint_ties, normals_degenerate, normals_orient_cases
  a3d_point_clouds_knn_distance_device       knn_rint_ties, knn_equal_kth, d2_witnesses   (and cluster, which shares the walk)
  a3d_point_clouds_segment_plane_device      plane_rint_ties, plane_threshold_witnesses, plane_degenerate_cut

Every builder returns a dict, or a list of dicts, with a name, [n, 3] f32 points, the call's parameters and the values
that are known by construction as Python integers or exact f32 values.  tests/test_neighbour_edge_cases_cpu.py proves, with
the restatements and with exact rationals, that each case is what it claims; tests/test_gpu_neighbour_edges.py runs them
on the device.  The expected value of a GPU test is the restatement, and the construction where there is one.

Ties.  With r a power of two, s = 32768 / r is one too, and an offset of (k + 0.5) / s from a row on exact coordinates is
an exact f32 whose product with s is exactly k + 0.5: rintf takes it to the even neighbour, roundf away from zero,
floorf(x + 0.5f) upwards.

Last bits.  The rule's d2 = (d_x*d_x + d_y*d_y) + d_z*d_z rounds five times, the fused form
fmaf(d_z, d_z, fmaf(d_x, d_x, d_y*d_y)) three times; they differ in the last bit often enough, and a seeded search over
d_z within three ulps of sqrt(r2 - d_x^2 - d_y^2) finds pairs whose membership they decide differently.  The search
classifies in f64 (a filter: it may miss a pair) and the pairs it keeps are classified again in exact rationals."""
from fractions import Fraction

import numpy as np

F = np.float32
D = np.float64

TIE_RADIUS = 0.0625  # 2^-4: s = 2^19
TIE_S = 1 << 19
CENTRE = (0.25, 0.5, 1.0)
TIE_KS = (0, 1, 2, 3, 6, 7, 100, 101, 16000, 16001, -1, -2, -3, -4, -7, -8, -101, -102, -16001, -16002)
EYE = (0.1, -0.3, 2.0)
WITNESS_RADII = (0.05, 0.0625, 0.1)
KINDS = ("unfused only", "fused only", "equal", "one ulp above")  # where d2 (or |d|) lies against r2 (or t)
KNN_KS = (1, 8, 9, 16, 17, 32)  # every width of the register array at its lower and upper edge
THIRD = 0x3EAAAAAB  # (float)(1 / 3), rounded up: the curvature of three equal eigenvalues


# ---- roundings ---------------------------------------------------------------------------------------------------------


def half_even(k):
    """rint(k + 0.5) for a Python int k: the even one of k and k + 1."""
    return k if k % 2 == 0 else k + 1


def half_away(x):
    """roundf on an f32 array: halves go away from zero."""
    x = np.asarray(x, F)
    return np.copysign(np.floor(np.abs(x) + F(0.5)), x)


def half_up(x):
    """floorf(x + 0.5f) on an f32 array: halves go up."""
    return np.floor(np.asarray(x, F) + F(0.5))


ALTERNATIVE_ROUNDINGS = {"half away from zero": half_away, "floor(x + 0.5)": half_up}


def round_f32(x, bits=24, least=-126):
    """A rational rounded to the nearest f32 (ties to even), as a rational; the normal range only.  (bits = 53,
    least = -1022: to the nearest f64.)"""
    x = Fraction(x)
    if x == 0:
        return x
    sign, x = (-1 if x < 0 else 1), abs(x)
    sh = x.numerator.bit_length() - x.denominator.bit_length() - bits
    while x / Fraction(2) ** sh >= 1 << bits:
        sh += 1
    while x / Fraction(2) ** sh < 1 << (bits - 1):
        sh -= 1
    assert sh + bits - 1 >= least
    q = x / Fraction(2) ** sh
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return sign * n * Fraction(2) ** sh


def frac(v):
    return Fraction(float(v))


def sum3_unfused(a, b):
    """(a_x*b_x + a_y*b_y) + a_z*b_z with every operation rounded to f32 on its own, in rationals."""
    a, b = [frac(v) for v in a], [frac(v) for v in b]
    return round_f32(round_f32(round_f32(a[0] * b[0]) + round_f32(a[1] * b[1])) + round_f32(a[2] * b[2]))


def sum3_fused(a, b):
    """fmaf(a_z, b_z, fmaf(a_x, b_x, a_y*b_y)): three roundings, in rationals."""
    a, b = [frac(v) for v in a], [frac(v) for v in b]
    return round_f32(a[2] * b[2] + round_f32(a[0] * b[0] + round_f32(a[1] * b[1])))


def _sum3_both(a, b):
    """The two sums for [..., 3] f32 arrays: (unfused as numpy computes it, fused emulated in f64).  The emulation rounds
    twice (to f64, then to f32), so it is a filter only."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        unfused = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        assert unfused.dtype == F
        a, b = a.astype(D), b.astype(D)
        inner = (a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1]).astype(F).astype(D)).astype(F).astype(D)
        fused = (a[..., 2] * b[..., 2] + inner).astype(F)
    return unfused, fused


def _step_ulps(x, steps):
    """x [m] f32 (no zeros) stepped by steps [k] ulps in magnitude: [m, k] f32."""
    bits = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)[:, None] + np.asarray(steps, np.int64)[None, :]
    return bits.astype(np.int32).view(F)


def _kind(unfused, fused, limit):
    """The index into KINDS of each sample, or -1: where the two forms of a sum lie against a limit."""
    above = np.nextafter(F(limit), F(np.inf))
    kind = np.full(unfused.shape, -1, np.int64)
    kind[(unfused <= limit) & (fused > limit)] = 0
    kind[(unfused > limit) & (fused <= limit)] = 1
    kind[(unfused == limit) & (kind < 0)] = 2
    kind[(unfused == above) & (kind < 0)] = 3
    return kind


# ---- normals -----------------------------------------------------------------------------------------------------------

NORMALS_TIE_CELLS = ((3, -2, 0), (-7, 5, 1), (0, 0, -5), (-3, -8, -1))
NORMALS_TIE_GROUPS = 12


def normals_rint_ties():
    """12 groups: a centre row in the middle of a cell of the r = 2^-4 grid and 3 to 6 rows at offsets (k + 0.5) / s from
    it, the k taken three at a time from TIE_KS.  Every d_k * s seen from the centre row is exactly k + 0.5, so its
    moments are the Python integers under `groups` (N, S [3], M [3][3]) iff q rounds ties to even.  The centres are at
    least six cells apart."""
    r, step = F(TIE_RADIUS), F(1.0 / TIE_S)
    points, groups, at = [], [], 0
    for g in range(NORMALS_TIE_GROUPS):
        cell = np.asarray(NORMALS_TIE_CELLS[g % 4], D) + np.asarray([8 * (g // 4), 0, 0], D)
        ctr = ((cell + 0.5) * TIE_RADIUS).astype(F)
        first, ks = len(points), []
        points.append(ctr)
        for _ in range(3 + g % 4):
            k = [TIE_KS[(at + a) % len(TIE_KS)] for a in range(3)]
            at += 3
            p = ctr + (np.asarray(k, F) + F(0.5)) * step
            assert p.dtype == F and all(frac(p[a]) == frac(ctr[a]) + Fraction(2 * k[a] + 1, 2 * TIE_S) for a in range(3))
            points.append(p), ks.append(k)
        q = [[half_even(k) for k in row] for row in ks]  # (the centre row itself adds q = 0)
        groups.append({"centre": first, "rows": list(range(first, len(points))), "ks": ks, "N": 1 + len(ks),
                       "S": [sum(row[a] for row in q) for a in range(3)],
                       "M": [[sum(row[a] * row[b] for row in q) for b in range(3)] for a in range(3)]})
    return {"name": "normals rintf ties", "points": np.asarray(points, F), "radius": TIE_RADIUS, "min_neighbors": 3,
            "viewpoint": EYE, "groups": groups}


def _base(k):
    """Corner k of a lattice of pitch 0.5 (eight cells of r = 2^-4) with both signs; corner 0 is CENTRE."""
    return np.asarray([0.25 - 0.5 * (k % 4), 0.5 - 0.5 * (k // 4 % 4), 1.0 - 0.5 * (k // 16)], D)


def _axis(m, negative=False):
    """The unit vector of axis m with the zero signs the kernel leaves: +0 as it stands, -0 once negated."""
    n = np.zeros(3, F)
    n[m] = 1
    return -n if negative else n


def _axis_views(points, m, eyes):
    """[{eye, normals [n, 3]}]: the normal is +-unit(m) and dot = w_m exactly, so a row is negated iff eye_m < p_m."""
    out = []
    for eye in eyes:
        eye = np.asarray(eye, F)
        out.append({"eye": eye, "normals": np.stack([_axis(m, bool(eye[m] < p[m])) for p in points])})
    return out


def _degenerate(name, points, views, counts=None, valid=None, curvature=None, claim=None, winner=None, m=3):
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    return {"name": name, "points": points, "radius": TIE_RADIUS, "min_neighbors": m, "views": views,
            "counts": np.full(n, n, np.uint32) if counts is None else np.asarray(counts, np.uint32),
            "valid": np.ones(n, bool) if valid is None else np.asarray(valid, bool), "curvature": curvature, "claim": claim,
            "winner": winner}


def _free_views(points):
    return [{"eye": np.asarray(e, F), "normals": None} for e in (EYE, (-3.0, 0.25, -2.0), points[0])]


def normals_degenerate():
    """Clouds at r = 2^-4 whose scatter matrix is degenerate, each at a corner of its own of a lattice of pitch 8 r, each
    with several viewpoints.  `counts` and `valid` hold by construction; `views[v]["normals"]` is the normal of every row
    by construction where the rule leaves no arithmetic (axis normals: the zeros carry the sign), else None; `curvature`
    is the f32 bit pattern of every valid row's curvature, or None; `claim` is what the scaled matrix B looks like and
    `winner` the index step 6 picks:

      isotropic   three equal diagonal entries, every a_pq == 0: every pair is skipped, V stays the identity, the tie
                  goes to index 0 and the normal is (1, 0, 0); curvature lam / ((lam + lam) + lam) = (float)(1/3)
      line        one diagonal entry, the rest of B zero: the two zero eigenvalues tie and the lower index wins
      plane       B is diagonal with one zero: that index wins
      line (1, 2, 0)  the pair (0, 1) is rotated once: theta = 3/4, t = 1/2, and a_00 - t a_01 is exactly 0; it ties with
                  a_22 == 0 and index 0 wins: the normal lies in the xy plane, across the line, from the restatement
      plane x = y     the pair (0, 1) is rotated once: theta = 0, t = 1, a_00 becomes exactly 0 and wins; the normal is
                  (x, -x, 0) with x from the restatement"""
    h = 2.0 ** -5
    cases, k = [], 0

    def base():
        nonlocal k
        k += 1
        return _base(k - 1)

    # isotropic: the octahedron with its centre, and the corners of a cube (opposite rows of the octahedron: d2 == r2)
    c = base()
    octa = np.asarray([c] + [c + s * h * np.eye(3)[a] for a in range(3) for s in (1, -1)], F)
    cases.append(_degenerate("octahedron", octa, _axis_views(octa, 0, [(0, 0, 0), (3.0, 0.5, 1.0), c]), curvature=THIRD,
                             claim="isotropic", winner=0))
    c = base()
    cube = np.asarray([c + 0.5 * h * np.asarray([sx, sy, sz]) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], F)
    cases.append(_degenerate("cube corners", cube, _axis_views(cube, 0, [(0, 0, 0), (-3.0, 0.5, 1.0), cube[7]]),
                             curvature=THIRD, claim="isotropic", winner=0))
    # identical points: N = 5 >= min_neighbors, mx == 0
    c = base()
    same = np.tile(c, (5, 1)).astype(F)
    zeros = np.zeros((5, 3), F)
    cases.append(_degenerate("five identical points", same, [{"eye": np.asarray(e, F), "normals": zeros} for e in (EYE, c)],
                             valid=np.zeros(5, bool), curvature=None, claim="zero"))
    # exactly m - 1, m and m + 1 neighbours at min_neighbors = m: tight groups of distinct points, eight cells apart
    for m in (3, 4, 9):
        rng = np.random.default_rng([31, m])
        pts, counts = [], []
        for size in (m - 1, m, m + 1):
            c = base()
            flat = rng.choice(16 ** 3, size=size, replace=False)
            off = np.stack([flat // 256, flat // 16 % 16, flat % 16], axis=1) * 2.0 ** -10
            pts.append(c + 2.0 ** -6 + off), counts.extend([size] * size)
        pts = np.concatenate(pts).astype(F)
        cases.append(_degenerate(f"groups of {m - 1}, {m}, {m + 1} at min_neighbors {m}", pts, _free_views(pts), counts=counts,
                                 valid=np.asarray(counts) >= m, m=m))
    # exact lines of five rows, pitch 2^-8
    step = 2.0 ** -8
    for axis, winner in ((0, 1), (1, 0), (2, 0)):  # B has one entry, at [axis][axis]; of the two zeros the lower index wins
        c = base()
        line = np.asarray([c + i * step * np.eye(3)[axis] for i in range(5)], F)
        eyes = [c + np.eye(3)[winner], c - np.eye(3)[winner], c + 2.0 * np.eye(3)[axis], line[2]]
        cases.append(_degenerate(f"line along axis {axis}", line, _axis_views(line, winner, eyes), curvature=0, claim="line",
                                 winner=winner))
    c = base()
    line = np.asarray([c + i * step * np.asarray([1.0, 2.0, 0.0]) for i in range(5)], F)
    cases.append(_degenerate("line along (1, 2, 0)", line, _free_views(line), curvature=0, claim="line (1, 2, 0)", winner=0))
    # exact planes of nine rows, pitch 2^-7
    step = 2.0 ** -7
    c = base()
    sheet = np.asarray([c + step * np.asarray([i, j, 0.0]) for i in (-1, 0, 1) for j in (-1, 0, 1)], F)
    eyes = [c + (0.3, -0.2, 1.5), c + (0.3, -0.2, -1.5), c + (2.0, 1.0, 0.0), sheet[0]]  # above, below, in the plane, a row's own
    cases.append(_degenerate("plane z = c", sheet, _axis_views(sheet, 2, eyes), curvature=0, claim="plane", winner=2))
    c = base()
    c[1] = c[0]  # on the plane x = y
    sheet = np.asarray([c + step * np.asarray([i, i, j]) for i in (-1, 0, 1) for j in (-1, 0, 1)], F)
    views = [{"eye": np.asarray(e, F), "normals": None, "dot": d}
             for e, d in ((c + (0.5, -0.5, 0.25), "positive"), (c + (-0.5, 0.5, 0.25), "negative"), (c + (1.5, 1.5, -2.0), "zero"),
                          (sheet[4], "zero"))]
    cases.append(_degenerate("plane x = y", sheet, views, curvature=0, claim="plane x = y", winner=0))
    return cases


ORIENT_KINDS = ("along", "against", "perpendicular", "+0", "-0", "nan", "nan in one")


def normals_orient_cases():
    """The two planes of normals_degenerate with an old normal per row, the kinds of ORIENT_KINDS in turn: along the
    plane's normal (dot > 0: kept), against it (dot < 0: negated), exactly perpendicular, (0, 0, 0), (-0, -0, -0) and NaN
    (dot is +0, -0 or NaN, none of them < 0: kept).  `unit` is the plane's normal up to sign; `sign[row]` is +1 where the
    result lies along `unit`, -1 where against it; `normals` the result by construction, where there is one."""
    nan = float("nan")
    step = 2.0 ** -7
    out = []
    for name, c, span, unit, perpendicular in (
            ("plane z = c", _base(20), ((1, 0, 0), (0, 1, 0)), (0.0, 0.0, 1.0), (1.0, -2.0, 0.0)),
            ("plane x = y", _base(21) * (1, 0, 1) + _base(21)[0] * np.asarray([0, 1, 0]), ((1, 1, 0), (0, 0, 1)), (1.0, -1.0, 0.0),
             (3.0, 3.0, -1.0))):
        pts = np.asarray([c + step * (i * np.asarray(span[0]) + j * np.asarray(span[1])) for i in (-1, 0, 1) for j in (-1, 0, 1)], F)
        old, kinds, sign = [], [], []
        for row in range(len(pts)):
            kind = ORIENT_KINDS[row % len(ORIENT_KINDS)]
            unit_old = np.asarray(unit) * (2.5 if row % 2 else 1.0)
            old.append({"along": unit_old, "against": -0.5 * np.asarray(unit), "perpendicular": np.asarray(perpendicular),
                        "+0": np.zeros(3), "-0": -np.zeros(3), "nan": np.full(3, nan), "nan in one": np.asarray([nan, 0.0, 0.0])}[kind])
            kinds.append(kind)
        out.append({"name": f"orient, {name}", "points": pts, "old_normals": np.asarray(old, F), "kinds": kinds,
                    "radius": TIE_RADIUS, "min_neighbors": 3, "unit": np.asarray(unit, D)})
    # the plane z = c: the raw normal is (0, 0, 1); a row is negated iff its kind is "against"
    out[0]["normals"] = np.stack([_axis(2, kind == "against") for kind in out[0]["kinds"]])
    out[1]["normals"] = None
    return out


# ---- knn and cluster ---------------------------------------------------------------------------------------------------

TIE_NS = (0, 1, 2, 3, 6, 7, 100, 101, 2046, 2047, 4, 5, 500, 501, 1000, 1001)


def _centre_q(ts, k):
    return sum(sorted(ts)[:k])


def _tie_cloud(name, centre, displacements, exact_rows):
    """displacements: [(D_x, D_y, D_z)] in units of 2^-20 whose length L is an odd integer: sqrtf(d2) * s = L / 2."""
    centre = np.asarray(centre, F)
    pts, halves = [centre], []
    for dv in displacements:
        L2 = sum(v * v for v in dv)
        L = int(round(L2 ** 0.5))
        assert L * L == L2 and L % 2 == 1 and L2 < 1 << 24
        p = centre + np.asarray(dv, F) * F(2.0 ** -20)
        assert all(frac(p[a]) == frac(centre[a]) + Fraction(dv[a], 1 << 20) for a in range(3))
        pts.append(p), halves.append(L)
    ts = [half_even((L - 1) // 2) for L in halves]
    return {"name": name, "points": np.asarray(pts, F), "radius": TIE_RADIUS, "halves": halves,
            "centre_q": {k: _centre_q(ts, k) for k in KNN_KS if k <= len(ts)}, "rows_q": None, "exact_rows": exact_rows}


def _axis_rows_q(positions, k):
    """Q of every row of a cloud on one axis at signed positions (units of 2^-20) by construction: the lattice distance
    of two rows is |P_i - P_j| / 2, an integer or a tie."""
    out = []
    for i, a in enumerate(positions):
        ts = []
        for j, b in enumerate(positions):
            if i != j:
                diff = abs(a - b)
                ts.append(diff // 2 if diff % 2 == 0 else half_even((diff - 1) // 2))
        out.append(sum(sorted(ts)[:k]) if len(ts) >= k else 0xFFFFFFFF)
    return out


def knn_rint_ties():
    """Clouds of a centre row and 32 others at r = 2^-4 whose distance from the centre is (n + 0.5) / s exactly.

    Three clouds on one axis each (x, y, z), 16 others in each direction at (2n + 1) * 2^-20, n in TIE_NS.  Seen from any
    row of such a cloud every lattice distance is an integer or a tie, and d2 = fl(d^2) has the exact root |d|, so
    `rows_q[k]` (every row's Q) and `stats[k]` are Python integers by construction.  One cloud with others in all six axis
    directions and at 3-4-5 displacements (3m, 4m, 0) * 2^-20 with m odd, signs and axes permuted: `centre_q[k]` is by
    construction (row 0), the other rows are the restatement's.  k runs over KNN_KS: with k = 32 every other of the centre
    counts, below that the k-th place falls between two ties.  The issue's own cloud is there too (ten others along +x)."""
    cases = []
    for axis, centre in ((0, CENTRE), (1, (-0.25, 0.5, -1.0)), (2, (0.25, -0.5, 1.0))):
        positions = [0] + [sgn * (2 * n + 1) for n in TIE_NS for sgn in (1, -1)]
        case = _tie_cloud(f"knn ties along axis {axis}", centre, [tuple(p if a == axis else 0 for a in range(3)) for p in positions[1:]],
                          exact_rows=True)
        case["rows_q"] = {k: _axis_rows_q(positions, k) for k in KNN_KS}
        cases.append(case)
    ten = (0, 1, 2, 3, 6, 7, 100, 101, 2046, 2047)
    case = _tie_cloud("knn ties, ten others along +x", CENTRE, [(2 * n + 1, 0, 0) for n in ten], exact_rows=True)
    case["rows_q"] = {k: _axis_rows_q([0] + [2 * n + 1 for n in ten], k) for k in (1, 8, 9, 10)}
    case["centre_q"][10] = _centre_q([half_even(n) for n in ten], 10)
    cases.append(case)
    mixed = []
    for i, n in enumerate((0, 1, 2, 3, 6, 7, 100, 101, 2046, 2047, 4, 5)):
        v = [0, 0, 0]
        v[i % 3] = (2 * n + 1) * (1 if i // 3 % 2 == 0 else -1)
        mixed.append(tuple(v))
    for i, m in enumerate((1, 3, 5, 7, 9, 11, 101, 103, 201, 203, 401, 403, 601, 603, 701, 703, 801, 803, 815, 817)):
        a, b = 3 * m * (1 if i % 2 else -1), 4 * m * (1 if i // 2 % 2 else -1)
        mixed.append(((a, b, 0), (0, a, b), (b, 0, a), (b, a, 0), (0, b, a))[i % 5])
    cases.append(_tie_cloud("knn ties in all directions and at 3-4-5", (-0.25, -0.5, 1.0), mixed, exact_rows=False))
    for case in cases:
        if case["rows_q"] is not None:
            case["stats"] = {}
            for k, q in case["rows_q"].items():
                assert q[0] == case["centre_q"][k]
                has = [v for v in q if v != 0xFFFFFFFF]
                case["stats"][k] = (len(has), sum(has), sum(v * v & 0xFFFFFFFF for v in has), sum(v * v >> 32 for v in has))
    return cases


EQUAL_U = 2.0 ** -10
EQUAL_T_NEAR, EQUAL_T_SHELL, EQUAL_T_EDGE = 3 * 512, 7 * 512, 32768


def knn_equal_kth():
    """One cloud at r = 2^-4: the centre row, a duplicate of it (t = 0), 4 others at (+-1, +-2, +-2) * 2^-10 (length 3 units:
    t = 1536), 40 others at the eight sign flips of (2, 3, 6) * 2^-10, five rows on each (length 7 units: one d2 bit
    pattern, t = 3584), and one at (r, 0, 0) (d2 == r2: t = 32768).  Sign flips keep the summation order and so the bits.
    For k = 8, 16 and 32 the k-th place of the centre row falls inside the 40: `centre_q[k]` by construction."""
    centre = np.asarray(CENTRE, F)
    pts = [centre, centre]
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        pts.append(centre + F(EQUAL_U) * np.asarray([sx, 2 * sy, -2 * sx], F))
    for _ in range(5):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    pts.append(centre + F(EQUAL_U) * np.asarray([2 * sx, 3 * sy, 6 * sz], F))
    pts.append(centre + np.asarray([TIE_RADIUS, 0, 0], F))
    ts = [0] + [EQUAL_T_NEAR] * 4 + [EQUAL_T_SHELL] * 40 + [EQUAL_T_EDGE]
    return {"name": "knn equal k-th", "points": np.asarray(pts, F), "radius": TIE_RADIUS, "centre_count": 47,
            "centre_q": {k: _centre_q(ts, k) for k in (1, 5, 6, 8, 16, 32)}}


WITNESS_TRIALS = 3000
WITNESS_PER_KIND = 10
WITNESS_STEPS = np.arange(-3, 4)
IN_PLACE_TRIALS = 8000
IN_PLACE_BASES = 48


def _draw_offsets(rng, r, trials):
    """[trials, 3] f64: (d_x, d_y) of magnitude 0.2 r to 0.6 r with random signs and d_z on the sphere of radius r, either
    sign.  |d_z| < 0.96 r: the two rows lie in cells at most one apart."""
    r64 = float(F(r))
    xy = rng.uniform(0.2, 0.6, size=(trials, 2)) * r64 * rng.choice([-1.0, 1.0], size=(trials, 2))
    xy = xy.astype(F).astype(D)
    r2 = float(F(r) * F(r))
    z = np.sqrt(r2 - xy[:, 0] ** 2 - xy[:, 1] ** 2) * rng.choice([-1.0, 1.0], size=trials)
    return np.c_[xy, z]


def _exact_kind(d, r2):
    """The kind of one pair from its f32 offset, in rationals."""
    unfused, fused, limit = sum3_unfused(d, d), sum3_fused(d, d), frac(r2)
    if unfused <= limit < fused:
        return 0
    if fused <= limit < unfused:
        return 1
    if unfused == limit:
        return 2
    if unfused == frac(np.nextafter(F(r2), F(np.inf))):
        return 3
    return -1


def _witness_rows(p_i, p_j):
    """[p_i, p_j, helper]: the helper is half an offset behind p_i, a clear neighbour of p_i and clearly none of p_j."""
    return np.stack([p_i, p_j, (p_i.astype(D) - 0.5 * (p_j.astype(D) - p_i.astype(D))).astype(F)])


def d2_witnesses(radius):
    """Pairs (p_i, p_j) at one radius whose d2 lies at the last bit of r2, of the four KINDS, at least 8 of each in each
    of two layouts:

      "origin"    a batch of three-row clouds, p_i the origin, so that p_j - p_i = p_j is exact
      "in place"  one cloud; the pairs sit at jittered corners of a lattice of pitch 5 r (at least 4 r apart) and p_j
                  was searched where it lies, stepping its z by ulps: d = p_j - p_i of the two stored values

    Each pair has a helper row behind p_i.  By construction p_i has 2 + inside neighbours, p_j 1 + inside, the helper 2; p_j
    has an other iff the pair is inside (k = 1), p_i has two iff it is (k = 2); with min_points = 1 the three rows are one
    cluster iff inside, else two.  `pairs`: [{kind, inside, d [3] f32}]; `found`: how many samples of each kind the search
    met, per layout."""
    r = F(radius)
    r2 = r * r
    rng = np.random.default_rng([20, int(round(radius * 10000))])
    out = {"name": f"d2 witnesses, r = {radius}", "radius": float(radius), "found": {}}
    # at the origin
    d = _draw_offsets(rng, radius, WITNESS_TRIALS).astype(F)
    z = _step_ulps(d[:, 2], WITNESS_STEPS)  # [trials, 7]
    cand = np.stack([np.broadcast_to(d[:, None, 0], z.shape), np.broadcast_to(d[:, None, 1], z.shape), z], axis=-1)
    kind = _kind(*_sum3_both(cand, cand), r2)
    out["found"]["origin"] = [int((kind == q).sum()) for q in range(4)]
    clouds, pairs = [], []
    for q in range(4):
        trial, step = np.nonzero(kind == q)
        taken = 0
        for t_, s_ in zip(trial, step):
            if taken == WITNESS_PER_KIND:
                break
            dv = cand[t_, s_]
            if _exact_kind(dv, r2) != q:
                continue  # (the f64 filter rounded twice)
            clouds.append(_witness_rows(np.zeros(3, F), dv)), pairs.append({"kind": q, "inside": q in (0, 2), "d": dv})
            taken += 1
        assert taken >= 8, (radius, "origin", KINDS[q], taken)
    out["origin"] = {"clouds": clouds, "pairs": pairs}
    # in place
    found, rows, pairs, picked = [0] * 4, [], [], [0] * 4
    for b in range(IN_PLACE_BASES):
        corner = np.asarray([b % 4 - 2, b // 4 % 4 - 2, b // 16 - 1], D) * 5.0 * float(r)
        p_i = (corner + rng.uniform(0.0, float(r), size=3)).astype(F)
        d = _draw_offsets(rng, radius, IN_PLACE_TRIALS)
        p_j = (p_i.astype(D)[None, :] + d).astype(F)
        z = _step_ulps(p_j[:, 2], WITNESS_STEPS)
        stored = np.stack([np.broadcast_to(p_j[:, None, 0], z.shape), np.broadcast_to(p_j[:, None, 1], z.shape), z], axis=-1)
        seen = stored - p_i[None, None, :]  # what the kernel sees: the difference of two stored f32, rounded
        assert seen.dtype == F
        kind = _kind(*_sum3_both(seen, seen), r2)
        for q in range(4):
            found[q] += int((kind == q).sum())
        for q in sorted(range(4), key=lambda q: picked[q]):  # the kind that has the fewest pairs so far, if this corner has it
            hit = None
            for t_, s_ in zip(*np.nonzero(kind == q)):
                if _exact_kind(seen[t_, s_], r2) == q:
                    hit = (t_, s_)
                    break
            if hit is not None:
                rows.append(_witness_rows(p_i, stored[hit])), pairs.append({"kind": q, "inside": q in (0, 2), "d": seen[hit]})
                picked[q] += 1
                break
    assert min(picked) >= 8, (radius, "in place", picked)
    out["found"]["in place"] = found
    out["in place"] = {"points": np.concatenate(rows), "pairs": pairs}
    return out


# ---- plane -------------------------------------------------------------------------------------------------------------

PLANE_TIE_T = 2.0 ** -6  # s = 64 / t = 4096
PLANE_TIE_S = 4096
PLANE_TIE_KZ = (0, 1, 2, 3, 6, 7, 62, 63, -1, -2, -3, -4, -7, -8, -63, -64)
PLANE_TIE_GROUPS = 8


def record_of(qs):
    """The 16-word record of step 5 from the q of the rows that take part, in Python ints."""
    kl = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    rec = [len(qs)] + [sum(q[a] for q in qs) for a in range(3)]
    rec += [sum((q[a] * q[b]) & 0x7FFFFFFF for q in qs) for a, b in kl]
    rec += [sum((q[a] * q[b]) >> 31 for q in qs) for a, b in kl]
    return rec


def plane_rint_ties():
    """8 clouds at t = 2^-6 (s = 4096) with one candidate, rows 0, 1, 2: p_a = CENTRE, p_b = p_a + (0.5, 0, 0),
    p_c = p_a + (0, 0.5, 0), so n = (0, 0, 1) exactly and d = e_z.  Six rows at e = ((k_x + 0.5), (k_y + 0.5), (k_z + 0.5)) / s,
    k_x and k_y from TIE_KS and |k_z + 0.5| < 64: inliers whose every e_k * s is a tie.  Two rows at e_z = +-2 t are no
    inliers.  `flags`, `record` (the 16 words of the first round) hold by construction iff q rounds ties to even."""
    a = np.asarray(CENTRE, F)
    step = F(1.0 / PLANE_TIE_S)
    cases, at = [], 0
    for g in range(PLANE_TIE_GROUPS):
        pts = [a, a + np.asarray([0.5, 0, 0], F), a + np.asarray([0, 0.5, 0], F)]
        qs, ks = [(0, 0, 0), (2048, 0, 0), (0, 2048, 0)], []
        for _ in range(6):
            k = [TIE_KS[at % len(TIE_KS)], TIE_KS[(at + 7) % len(TIE_KS)], PLANE_TIE_KZ[at % len(PLANE_TIE_KZ)]]
            at += 1
            p = a + (np.asarray(k, F) + F(0.5)) * step
            assert p.dtype == F and all(frac(p[c]) == frac(a[c]) + Fraction(2 * k[c] + 1, 2 * PLANE_TIE_S) for c in range(3))
            pts.append(p), ks.append(k), qs.append(tuple(half_even(v) for v in k))
        pts += [a + np.asarray([0.25, 0.125, 2 * PLANE_TIE_T], F), a + np.asarray([-0.125, 0.25, -2 * PLANE_TIE_T], F)]
        cases.append({"name": f"plane rintf ties {g}", "points": np.asarray(pts, F), "triples": np.asarray([[0, 1, 2]], np.uint32),
                      "t": PLANE_TIE_T, "ks": ks, "tie_rows": list(range(3, 9)), "flags": np.asarray([1] * 9 + [0] * 2, np.uint32),
                      "record": record_of(qs)})
    return cases


PLANE_WITNESS_T = 0.05
PLANE_WITNESS_TRIALS = 6000


def plane_threshold_witnesses():
    """One cloud at t = 0.05 with one candidate (rows 0, 1, 2, a tilted plane): 40 rows well inside the slab, 10 well
    outside it, and at least 8 rows each whose d = (n_x*e_x + n_y*e_y) + n_z*e_z satisfies fabsf(d) <= t only as the rule
    rounds it and only in the fused form fmaf(n_z, e_z, fmaf(n_x, e_x, n_y*e_y)): found by a seeded search that steps the
    z of a row near the slab's face by ulps.  `flags` (after refine = 0) holds by construction; `kinds[row]` is the index
    into KINDS or -1; `found` counts the search's samples."""
    import plane_restatement as PR

    t = F(PLANE_WITNESS_T)
    rng = np.random.default_rng(41)
    a = np.asarray([0.1, 0.2, 0.3], F)
    head = np.stack([a, a + np.asarray([0.5, 0.1, 0.05], F), a + np.asarray([-0.1, 0.45, 0.12], F)])
    normal, _, good = PR.candidates(head, [[0, 1, 2]])
    assert good[0]
    n = normal[0]
    n64 = n.astype(D)
    e1 = np.cross(n64, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n64, e1)

    def rows(count, offsets):
        uv = rng.uniform(-0.4, 0.4, size=(count, 2))
        return (a.astype(D) + uv[:, :1] * e1 + uv[:, 1:] * e2 + np.asarray(offsets)[:, None] * n64).astype(F)

    clear_in = rows(40, rng.uniform(-0.8, 0.8, size=40) * float(t))
    clear_out = rows(10, rng.uniform(1.5, 3.0, size=10) * float(t) * rng.choice([-1.0, 1.0], size=10))
    near = rows(PLANE_WITNESS_TRIALS, float(t) * rng.choice([-1.0, 1.0], size=PLANE_WITNESS_TRIALS))
    z = _step_ulps(near[:, 2], WITNESS_STEPS)
    stored = np.stack([np.broadcast_to(near[:, None, 0], z.shape), np.broadcast_to(near[:, None, 1], z.shape), z], axis=-1)
    e = stored - a[None, None, :]
    assert e.dtype == F
    unfused, fused = _sum3_both(np.broadcast_to(n, e.shape), e)
    kind = _kind(np.abs(unfused), np.abs(fused), t)
    found = [int((kind == q).sum()) for q in range(4)]
    picked, kinds = [], []
    for q in (0, 1):
        taken = 0
        for t_, s_ in zip(*np.nonzero(kind == q)):
            if taken == WITNESS_PER_KIND:
                break
            ev = e[t_, s_]
            exact = (abs(sum3_unfused(n, ev)) <= frac(t), abs(sum3_fused(n, ev)) <= frac(t))
            if exact != ((True, False), (False, True))[q]:
                continue
            picked.append(stored[t_, s_]), kinds.append(q)
            taken += 1
        assert taken >= 8, (KINDS[q], taken)
    points = np.concatenate([head, clear_in, clear_out, np.asarray(picked, F)])
    kinds = [-1] * (3 + 40 + 10) + kinds
    flags = np.asarray([1] * 43 + [0] * 10 + [1 if q == 0 else 0 for q in kinds[53:]], np.uint32)
    return {"name": "plane threshold witnesses", "points": points, "triples": np.asarray([[0, 1, 2]], np.uint32),
            "t": PLANE_WITNESS_T, "normal": n, "kinds": kinds, "flags": flags, "found": found}


CUT_KINDS = ("equal", "one ulp above", "one ulp below")  # L against (U*V) * 2^-20, in f64
CUT_PER_KIND = 5
CUT_T = 0.05


def cut_terms(p_a, p_b, p_c):
    """(L, (U*V) * 2^-20) of step 1 of the plane rule for one triple of f32 rows, in numpy f64, operation by operation."""
    a, b, c = (np.asarray(x, F).astype(D) for x in (p_a, p_b, p_c))
    u, v = b - a, c - a
    m = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    L = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    U = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    V = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return L, (U * V) * D(2.0 ** -20)


def plane_degenerate_cut():
    """Three-row clouds whose one candidate sits on the cut L > (U*V) * 2^-20 of step 1: L equal to the right-hand side
    (degenerate), the next f64 above it (good) and the next f64 below it (degenerate), CUT_PER_KIND of each.

    A random triple never comes within many thousands of f64 ulps of the cut, and a step of one f32 ulp in a coordinate of
    p_c moves L by 2^30 f64 ulps or not at all, so the search is a structured one.  With p_a the origin, u along one axis
    and v = (2^10 a, a + c, z) * 2^-33 in the other order of magnitude, L - (U*V) * 2^-20 is, exactly,
    |u|^2 2^-20 ((2^20 - 1) z^2 - delta) 2^-66 with delta = a^2 - (2^21 - 2) a c - (2^20 - 1) c^2, an integer that is small
    next to a^2 = 2^46 for a near (2^21 - 2) c.  A seeded choice of (a, c) with delta > 0, of the axes, the signs and a
    power-of-two scale, then a scan of z = sqrt((delta + j 2^14) / (2^20 - 1)) over quarter steps of j, rounded to f32,
    crosses the cut one f64 ulp at a time.  `good` is the rule's verdict."""
    rng = np.random.default_rng(61)
    K = (1 << 20) - 1
    cases, taken = [], [0] * 3
    while min(taken) < CUT_PER_KIND:
        c = int(rng.integers(4, 8))
        root = ((2 ** 21 - 2) * c + int(((2 ** 21 - 2) * c) ** 2 + 4 * K * c * c) ** 0.5) // 2
        a = int(root) + int(rng.integers(-3, 40))
        delta = a * a - (2 ** 21 - 2) * a * c - K * c * c
        if not (1 << 23 <= a and a + c < 1 << 24 and 0 < delta < 1 << 30):
            continue
        axes = rng.permutation(3)
        signs = rng.choice([-1.0, 1.0], size=3)
        scale = 2.0 ** int(rng.integers(-3, 3))
        want = int(np.argmin(taken))
        for j in np.arange(-6.0, 7.0, 0.25):
            z2 = (delta * 2.0 ** -66 + j * 2.0 ** -52) / K
            if z2 <= 0:
                continue
            v = np.asarray([a * 2.0 ** -23, (a + c) * 2.0 ** -33, z2 ** 0.5]) * signs * scale
            p_b, p_c = np.zeros(3, F), np.zeros(3, F)
            p_b[axes[0]] = scale
            p_c[axes] = v.astype(F)
            L, cut = cut_terms(np.zeros(3, F), p_b, p_c)
            kind = 0 if L == cut else 1 if L == np.nextafter(cut, np.inf) else 2 if L == np.nextafter(cut, -np.inf) else -1
            if kind == want:
                cases.append({"name": f"plane cut, {CUT_KINDS[kind]}, a = {a}, c = {c}", "points": np.stack([np.zeros(3, F), p_b, p_c]),
                              "triples": np.asarray([[0, 1, 2]], np.uint32), "t": CUT_T, "kind": kind, "good": kind == 1})
                taken[kind] += 1
                break
    return cases
