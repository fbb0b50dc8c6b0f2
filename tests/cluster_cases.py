"""Clouds that the cluster tests share (test_cluster_cpu.py, test_gpu_cluster.py)."""
import numpy as np

from outlier_cases import RADIUS, effectiveness_cloud

N_CLUMPS, CLUMP = 6, 5


def raw_bits(seed, n):
    """[n, 3] raw random bits (the recipe of test_gpu_cloud_normals.py): NaNs with payloads, infinities, -0.0, denormals and
    magnitudes far beyond the 21-bit cell range all occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def floaters_cloud():
    """(points [1560, 3] f32, is_outlier [1560] bool, is_clump [1560] bool): effectiveness_cloud() plus 6 clumps of 5 points,
    each clump within a ball of 0.02 and at least 3 RADIUS from everything else, shuffled.  Every clump row has four
    neighbours, so the radius filter keeps it."""
    base, outlier = effectiveness_cloud()
    rng = np.random.default_rng(4048)
    rows = [base.astype(np.float64)]
    n = 0
    while n < N_CLUMPS:
        c = rng.uniform([-1.5, -1.5, -1.0], [3.5, 1.5, 2.0])
        if np.linalg.norm(np.concatenate(rows) - c, axis=1).min() >= 3 * RADIUS + 0.05:
            step = rng.normal(size=(CLUMP, 3))
            step *= (0.018 * rng.uniform(0.2, 1.0, size=(CLUMP, 1))) / np.linalg.norm(step, axis=1, keepdims=True)
            rows.append(c + step)
            n += 1
    points = np.concatenate(rows).astype(np.float32)
    clump = np.r_[np.zeros(len(base), bool), np.ones(N_CLUMPS * CLUMP, bool)]
    outlier = np.r_[outlier, np.zeros(N_CLUMPS * CLUMP, bool)]
    perm = rng.permutation(len(points))
    return points[perm], outlier[perm], clump[perm]


def chain(n, order, r=0.05, stretch=None, spacing=0.9):
    """n points spaced `spacing` r along a line (off the axes), rows ascending, descending or shuffled along it.
    stretch = (k, factor): the link between points k and k + 1 is factor * r long instead."""
    steps = np.full(max(n - 1, 0), spacing * r, np.float64)
    if stretch is not None:
        steps[stretch[0]] = stretch[1] * r
    t = np.r_[0.0, np.cumsum(steps)][:n]
    d = np.float64([0.6, 0.48, 0.64])  # a unit vector
    points = (np.float64([0.31, -0.17, 0.23]) + t[:, None] * d).astype(np.float32)
    if order == "descending":
        points = points[::-1]
    elif order == "shuffled":
        points = points[np.random.default_rng(n).permutation(n)]
    else:
        assert order == "ascending"
    return np.ascontiguousarray(points)


def exact_chain(n, k):
    """n points on the x axis at multiples of 1/4 (exact in f32, r = 0.25, r2 = 0.0625 exact): neighbours are exactly r apart,
    except the link k -> k + 1, which is r + 2^-10."""
    x = np.arange(n, dtype=np.float64) * 0.25
    x[k + 1:] += 2.0**-10
    return np.stack([x, np.zeros(n), np.zeros(n)], axis=1).astype(np.float32)


def bridge(r=0.05):
    """(points, the bridge's row, min_points 10): two blobs of 40 points within balls of 0.2 r whose centres are 2.5 r
    apart, a tip point per blob 0.3 r from its centre towards the other blob, and one point midway between the centres: it
    is 0.95 r from either tip and at least 1.05 r from every blob point.  The blob and tip rows have 41 or more neighbours
    and are core at min_points = 10; the midway point has 3 (itself and the tips) and is not, so it is a border row and
    the two blobs, whose rows are at least 1.9 r apart, stay 2 clusters."""
    rng = np.random.default_rng(31)

    def blob(centre):
        step = rng.normal(size=(40, 3))
        step *= (0.2 * r * rng.uniform(0.0, 1.0, size=(40, 1)) ** (1 / 3)) / np.linalg.norm(step, axis=1, keepdims=True)
        return centre + step

    mid = np.float64([0.4, 0.4, 0.4])
    x = np.float64([1.0, 0.0, 0.0])
    parts = [blob(mid - 1.25 * r * x), (mid - 0.95 * r * x)[None], mid[None], (mid + 0.95 * r * x)[None], blob(mid + 1.25 * r * x)]
    return np.concatenate(parts).astype(np.float32), 41, 10


def border_ties():
    """(points, radius 1.0, min_points 5, expected labels) on multiples of 1/8, so every d2 is exact.
    Cluster A, rows 0-4: (0, 0, 0), (1, 0, 0), (.5, .5, 0), (.5, -.5, 0), (.5, 0, 0): each within 1 of the other four.
    Cluster B, rows 5-9: the same shape from (3.5, 0, 0) down to (2.5, 0, 0) (row 6).  Rows 1 and 6 are 1.5 apart: no link.
    Row 10 at (1.75, 0, 0): its core neighbours are row 1 and row 6, both at d2 = 0.5625 bit for bit: the lower row wins,
    cluster 0.
    Row 11 at (1.875, .25, 0): row 1 at d2 = 0.828125, row 6 at d2 = 0.453125: B is nearer though A's row is the lower
    one: cluster 1.
    Rows 10 and 11 have 4 neighbours each (themselves, each other, rows 1 and 6): below min_points = 5, so they are border
    rows and do not link A and B; every core row has at least 5."""
    a = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.0, 0.0]]
    b = [[3.5, 0.0, 0.0], [2.5, 0.0, 0.0], [3.0, 0.5, 0.0], [3.0, -0.5, 0.0], [3.0, 0.0, 0.0]]
    points = np.float32(a + b + [[1.75, 0.0, 0.0], [1.875, 0.25, 0.0]])
    return points, 1.0, 5, np.uint32([0] * 5 + [1] * 5 + [0, 1])


def pairs_far_apart(n, r=0.02):
    """(points [n, 3] f32, h): rows i and i + h, h = ceil(n / 2), sit within 0.3 r of each other at site i of a cubic lattice
    of pitch 4 r (the second a fixed 0.25 r off the first along x), so a site's rows are neighbours and no two sites' are."""
    h = (n + 1) // 2
    side = int(np.ceil(h ** (1.0 / 3.0)))
    while side**3 < h:
        side += 1
    s = np.arange(h, dtype=np.int64)
    site = np.stack([s % side, s // side % side, s // (side * side)], axis=1).astype(np.float64) * (4.0 * r) + 0.5 * r
    second = site[:n - h] + np.float64([0.25 * r, 0.0, 0.0])
    return np.concatenate([site, second]).astype(np.float32), h


def pairs_far_apart_expected(n, m):
    """(labels, sizes, roots) of pairs_far_apart(n) by construction."""
    h = (n + 1) // 2
    labels = np.full(n, 0xFFFFFFFF, np.uint32)
    if m >= 3:
        return labels, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    paired = n - h  # sites with two rows: the first `paired` sites
    if m == 1:
        labels[:h] = np.arange(h)
        labels[h:] = np.arange(paired)
        sizes = np.r_[np.full(paired, 2), np.full(h - paired, 1)].astype(np.uint32)
        return labels, sizes, np.arange(h, dtype=np.uint32)
    labels[:paired] = np.arange(paired)
    labels[h:] = np.arange(paired)
    return labels, np.full(paired, 2, np.uint32), np.arange(paired, dtype=np.uint32)


# ---- clouds for the union-find under contention (test_gpu_cluster_contention.py): r = 0.05, points `STEP` apart ----------

R_CONTENTION = 0.05
STEP = 0.9 * R_CONTENTION  # neighbours along a line; two steps are 1.8 r: no neighbours, even in f32 3 km from the origin
NOISE_SET = -1


def labels_of_sets(sets, core=None):
    """(labels [n] u32, sizes [C] u32, roots [C] u32) from the set number of every row (NOISE_SET: in no cluster) and the
    mask of its core rows (None: every member is core): the root of a set is its lowest core row, and the clusters are
    numbered by ascending root.  Nothing here looks at a point."""
    sets = np.asarray(sets, np.int64)
    n = len(sets)
    member = sets != NOISE_SET
    core = member if core is None else np.asarray(core, bool) & member
    count = int(sets.max()) + 1 if member.any() else 0
    root_of_set = np.full(count, n, np.int64)
    np.minimum.at(root_of_set, sets[core], np.flatnonzero(core))
    assert (root_of_set < n).all()  # every set has a core row
    order = np.argsort(root_of_set, kind="stable")
    number = np.empty(count, np.int64)
    number[order] = np.arange(count)
    labels = np.full(n, 0xFFFFFFFF, np.int64)
    labels[member] = number[sets[member]]
    sizes = np.bincount(labels[member], minlength=count)
    return labels.astype(np.uint32), sizes.astype(np.uint32), root_of_set[order].astype(np.uint32)


def chain_sets(n, order, cut=None):
    """The set of every row of chain(n, order, stretch=(cut, 1.001)): the rows at positions 0 .. cut along the chain are
    set 0, the rest set 1 (cut None: one set)."""
    position = np.arange(n)
    if order == "descending":
        position = position[::-1]
    elif order == "shuffled":
        position = np.random.default_rng(n).permutation(n)
    return np.zeros(n, np.int64) if cut is None else (position > cut).astype(np.int64)


def interleaved_lines(n, K, descending=False):
    """(points [n, 3] f32, line [n], ends [n] bool): row p lies on line p % K at position p // K (descending: counted from
    the line's far end), STEP apart along a direction off the axes; the lines stand 3 r apart on a square grid of
    ceil(sqrt(K)) a side.  ends: the first and the last point of every line.  Every line has at least 3 rows."""
    p = np.arange(n)
    line, at = p % K, p // K
    length = (n - line + K - 1) // K  # rows of the row's line
    assert length.min() >= 3
    if descending:
        at = length - 1 - at
    g = int(np.ceil(np.sqrt(K)))
    u, v, w = np.float64([0.6, 0.8, 0.0]), np.float64([-0.48, 0.36, 0.8]), np.float64([0.64, -0.48, 0.6])  # orthonormal
    pitch = 3.0 * R_CONTENTION
    points = (np.float64([-0.7, 0.4, 0.2]) + (line % g)[:, None] * pitch * u + (line // g)[:, None] * pitch * v
              + at[:, None] * STEP * w)
    return points.astype(np.float32), line, (at == 0) | (at == length - 1)


def lattice_sheet(side):
    """(points [side * side, 3] f32, kind [side * side]: neighbours in the sheet, 4 interior, 3 edge, 2 corner): a square
    lattice of pitch STEP in a plane off the axes, rows shuffled.  The diagonal is 1.27 r, so a row's neighbours are
    itself and the rows next to it along the two directions: counts 5, 4 and 3."""
    a, b = np.divmod(np.arange(side * side), side)
    u, v = np.float64([0.6, 0.8, 0.0]), np.float64([-0.48, 0.36, 0.8])
    points = np.float64([0.2, -0.3, 0.1]) + a[:, None] * STEP * u + b[:, None] * STEP * v
    kind = 4 - ((a == 0) | (a == side - 1)).astype(np.int64) - ((b == 0) | (b == side - 1)).astype(np.int64)
    perm = np.random.default_rng(side).permutation(side * side)
    return points[perm].astype(np.float32), kind[perm]


SHEET_SIDE = 260  # 67 600 rows: 67 tiles of 1024
COMB_TEETH, COMB_TOOTH = 66, 1024


def comb(cut=None, shuffled=False):
    """(points, sets): COMB_TEETH teeth of COMB_TOOTH rows, tooth t in rows [t L, (t + 1) L) along x from 0 at
    y = 2 t STEP, even teeth ascending away from the spine and odd teeth descending towards it; then the spine, 2 T - 1
    points at x = -STEP, y = s STEP, in the highest rows.  The spine point at even s is STEP from the first point of tooth
    s / 2; at odd s it is 1.27 r from the teeth and touches only the spine.  cut: the spine point 2 cut + 1 is left out,
    and the rows beyond it (teeth cut + 1 ..., spine points from 2 cut + 2) are set 1.  shuffled: under a seeded row
    permutation."""
    T, L = COMB_TEETH, COMB_TOOTH
    tooth, k = np.divmod(np.arange(T * L), L)
    along = np.where(tooth % 2 == 0, k, L - 1 - k)
    teeth = np.stack([along * STEP, 2 * tooth * STEP, np.zeros(T * L)], axis=1)
    s = np.arange(2 * T - 1)
    if cut is not None:
        s = s[s != 2 * cut + 1]
    spine = np.stack([np.full(len(s), -STEP), s * STEP, np.zeros(len(s))], axis=1)
    points = (np.float64([0.37, -0.21, 0.55]) + np.r_[teeth, spine]).astype(np.float32)
    sets = np.zeros(len(points), np.int64)
    if cut is not None:
        sets = np.r_[tooth > cut, s > 2 * cut + 1].astype(np.int64)
    if shuffled:
        perm = np.random.default_rng(COMB_TEETH).permutation(len(points))
        points, sets = points[perm], sets[perm]
    return np.ascontiguousarray(points), sets
