"""Clouds and candidates that the plane tests share (test_cloud_plane_cpu.py, test_gpu_cloud_plane.py)."""
import numpy as np

from cluster_cases import raw_bits  # noqa: F401  (the hostile rows of every cloud test)

F = np.float32
T_EXACT = 0.25


def exact_sheet():
    """(points, triples, t, expected flags): coordinates that are exact in f32, the planted triple (rows 0, 1, 2) spans the
    plane z = 0 with normal (0, 0, 1), so d = z exactly.  Rows at |z| == t are inliers, rows at t + 2^-10 are not."""
    rng = np.random.default_rng(11)
    xy = rng.integers(-256, 256, size=(700, 2)).astype(np.float64) / 64.0
    z = np.tile([0.0, T_EXACT, -T_EXACT, T_EXACT + 2.0 ** -10, -T_EXACT - 2.0 ** -10, 0.125, -0.125, 1.0, -3.5, 0.25 - 2.0 ** -10],
                70)
    points = np.c_[xy, z]
    points[0], points[1], points[2] = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    flags = (np.abs(points[:, 2]) <= T_EXACT).astype(np.uint32)
    return points.astype(F), np.uint32([[0, 1, 2]]), T_EXACT, flags


def parallel_sheets(first):
    """(points, triples): two sheets of 150 rows each at z = 0 and z = 4, on exact coordinates, one candidate on each;
    `first` (0 or 1) is the sheet whose candidate comes first.  Both count 150: the lower h wins."""
    rng = np.random.default_rng(12)
    xy = rng.integers(-256, 256, size=(300, 2)).astype(np.float64) / 64.0
    z = np.repeat([0.0, 4.0], 150)
    points = np.c_[xy, z]
    points[0:3, :2] = points[150:153, :2] = ((0, 0), (1, 0), (0, 1))
    cands = np.uint32([[0, 1, 2], [150, 151, 152]])
    return points.astype(F), cands[[first, 1 - first]]


def degenerate_cloud():
    """(points, triples, good): 40 rows on exact coordinates and candidates of every degenerate kind among good ones.
    Rows 0-2 span z = 0; 3, 4 are collinear with 0 and 1; 5 is a NaN row, 6 an infinite one; rows 7, 8 make a sine just
    below and just above 2^-10 with rows 0 and 1: u = (1, 0, 0), v = (X, 1, 0) has sine^2 = 1 / (X^2 + 1), and
    L = 1 against (U*V) * 2^-20 = (X^2 + 1) / 2^20 is degenerate at X = 1024 and good at X = 1023."""
    rng = np.random.default_rng(13)
    points = rng.integers(-64, 64, size=(40, 3)).astype(np.float64) / 64.0
    points[:, 2] = rng.integers(-8, 8, size=40) / 64.0
    points[0], points[1], points[2] = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    points[3], points[4] = (2, 0, 0), (-3, 0, 0)
    points[5], points[6] = (np.nan, 0.5, 0.5), (0.5, np.inf, 0.5)
    points[7], points[8] = (1024, 1, 0), (1023, 1, 0)
    triples = np.uint32([[0, 1, 2], [0, 0, 2], [0, 1, 3], [9, 10, 11], [0, 5, 2], [6, 1, 2], [0, 1, 7], [0, 1, 8], [3, 4, 0],
                         [1, 2, 2], [12, 13, 14], [4, 4, 4]])
    good = np.array([True, False, False, True, False, False, False, True, False, False, True, False])
    return points.astype(F), triples, good


def all_degenerate():
    points, triples, good = degenerate_cloud()
    return points, triples[~good]


def hostile_cloud():
    """1500 rows: a noisy sheet, a cube of clutter and 200 raw-bit rows (30 of them with a NaN or an infinity put in),
    shuffled."""
    rng = np.random.default_rng(14)
    sheet = np.c_[rng.uniform(-1, 1, size=(700, 2)), 0.3 + rng.normal(0, 0.004, 700)]
    cube = rng.uniform(-1, 1, size=(600, 3))
    points = np.r_[sheet, cube].astype(F)
    bad = raw_bits(15, 200)
    bad[np.arange(30), rng.integers(0, 3, size=30)] = rng.choice([np.nan, np.inf, -np.inf], size=30)  # 30 rows surely not finite
    points = np.r_[points, bad]
    return points[rng.permutation(len(points))]


def sheet_and_slab(n):
    """(points, triple, expected flags) for one candidate over n rows on exact coordinates: rows with i % 3 != 0 lie on the
    sheet z = 0, the others on a slab at z = 8; the triple (rows 1, 2, 1025) is on the sheet, t = 0.25."""
    i = np.arange(n, dtype=np.int64)
    points = np.empty((n, 3), F)
    points[:, 0] = (i % 1024) / 64.0
    points[:, 1] = (i // 1024) / 64.0
    points[:, 2] = np.where(i % 3 != 0, 0.0, 8.0)
    return points, np.uint32([[1, 2, 1025]]), (i % 3 != 0).astype(np.uint32)


def long_plane():
    """(points, triples, t): 3000 rows on a strip 40 m long at t = 0.001, the candidate's first row at the near end: the
    lattice of step 5 (t / 64) reaches 2^20 steps = 16.384 m, so more than half of the inliers are left out of the refit."""
    rng = np.random.default_rng(16)
    points = np.c_[rng.uniform(0, 40, 3000), rng.uniform(0, 1, 3000), rng.uniform(-0.0004, 0.0004, 3000)]
    points[0], points[1], points[2] = (0, 0, 0), (30, 0, 0), (0, 1, 0)
    return points.astype(F), np.uint32([[0, 1, 2]]), 0.001


SCENE_T = 0.01
SCENE_H = 256
SCENE_SEED = 0


def tabletop_scene():
    """(points, normals, colors, is_floor, is_box): about 20 000 rows.  A floor of 12 000 rows at z = 0 with |noise| <=
    t / 4; a box of 6 000 rows standing ON the floor (its lowest rows start 4 t above it) and a floating clump of 1 500
    rows, both at least 4 t from the floor; 500 planted rows far away.  Shuffled."""
    rng = np.random.default_rng(17)
    t = SCENE_T
    floor = np.c_[rng.uniform(-2, 2, size=(12000, 2)), rng.uniform(-t / 4, t / 4, 12000)]
    box = np.c_[rng.uniform(-0.5, 0.5, size=(6000, 2)), rng.uniform(4 * t, 0.6, 6000)]
    clump = np.c_[rng.uniform(1.2, 1.5, size=(1500, 2)), rng.uniform(1.0, 1.3, 1500)]
    far = rng.uniform(20, 60, size=(500, 3)) * rng.choice([-1.0, 1.0], size=(500, 3))
    points = np.r_[floor, box, clump, far].astype(F)
    kind = np.repeat([0, 1, 2, 3], [12000, 6000, 1500, 500])
    perm = rng.permutation(len(points))
    points, kind = points[perm], kind[perm]
    normals = rng.normal(size=points.shape).astype(F)
    colors = rng.integers(0, 256, size=points.shape).astype(np.uint8)
    return points, normals, colors, kind == 0, kind == 1
