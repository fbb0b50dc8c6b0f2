"""Outlier removal for resident clouds (a3d_point_clouds_select_device, a3d_point_clouds_knn_distance_device,
a3d_knn_distance_threshold) without a GPU: the C ABI (exported symbols, the header, the ctypes mirror, the Rust bindings,
every refusal that is decided on the host, with made-up device addresses: nothing is dereferenced), the threshold against
exact rational arithmetic, and the numpy restatement (outlier_restatement.py, the expected value of the GPU tests)
against an f64 brute force and against what the two filters are for."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import normals_restatement as NR
import outlier_restatement as R
from align3d_amd import DevicePointCloud, PointCloud, _abi
from outlier_cases import N_OUTLIERS, RADIUS, effectiveness_cloud, sentinel_edge_cloud
from test_cloud_normals_cpu import plane_and_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT, KNN, THRESHOLD = ("a3d_point_clouds_select_device", "a3d_point_clouds_knn_distance_device",
                          "a3d_knn_distance_threshold")
SENTINEL = 0x7777


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


# ---- the ABI, without a device -----------------------------------------------------------------------------------------


def test_symbols_are_exported_declared_mirrored_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    for name, arity in ((SELECT, 13), (KNN, 9), (THRESHOLD, 3)):
        assert hasattr(lib, name) and hasattr(diag, name)
        assert re.search(r"a3d_status\s+%s\s*\(" % name, header) and name in section
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == arity
    assert lib.a3d_abi_version() == 1
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys

    assert open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read() == gen_rust_sys.generate()
    for method in ("select", "select_many", "neighbor_distances", "neighbor_distances_many", "remove_radius_outliers",
                   "remove_radius_outliers_many", "remove_statistical_outliers", "remove_statistical_outliers_many",
                   "knn_distance_threshold"):
        assert callable(getattr(DevicePointCloud, method))


def test_the_rule_stands_verbatim_in_the_kernel_file_and_the_restatement():
    def rule(text, strip):
        lines = [ln.strip().lstrip(strip).strip() for ln in text.splitlines()]
        joined = " ".join(" ".join(lines).split())
        return joined[joined.index("1. Grid."):joined.index("statistics all zero.")]

    hip = open(os.path.join(ROOT, "align3d_amd", "csrc", "cloud_outliers.hip")).read()
    assert rule(hip, "/") == rule(R.__doc__, "")


def test_product_library_has_no_knob_for_the_feature():
    assert b"A3D_OUTLIERS" not in open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_OUTLIERS_K" in open(_abi.DIAG_LIB_PATH, "rb").read()


class _SelectArgs:
    """Two clouds of 4 rows at made-up, disjoint device addresses (cloud 0 with normals and colours), a made-up context
    and sentinel-filled result arrays: the checks under test fail before anything is dereferenced."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.ctx = C.c_void_p(0x900000)
        self.colors = (C.c_void_p * 2)(0x28000, None)
        self.values = (C.c_void_p * 2)(0x2C000, 0x2D000)
        self.lo, self.hi = (C.c_uint32 * 2)(1, 1), (C.c_uint32 * 2)(5, 5)
        self.out_points = (C.c_void_p * 2)(0x40000, 0x50000)
        self.out_normals = (C.c_void_p * 2)(0x60000, None)
        self.out_colors = (C.c_void_p * 2)(0x68000, None)
        self.out_index = (C.c_void_p * 2)(0x70000, 0x80000)
        self.capacities = (C.c_uint64 * 2)(4, 4)
        self.lens = (C.c_uint64 * 2)(SENTINEL, SENTINEL)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, colors=self.colors, n=2, values=self.values, lo=self.lo, hi=self.hi,
                 out_points=self.out_points, out_normals=self.out_normals, out_colors=self.out_colors,
                 out_index=self.out_index, capacities=self.capacities, lens=self.lens)
        a.update(override)
        return getattr(lib, SELECT)(a["ctx"], a["views"], a["colors"], a["n"], a["values"], a["lo"], a["hi"], a["out_points"],
                                    a["out_normals"], a["out_colors"], a["out_index"], a["capacities"], a["lens"])

    def untouched(self):
        return list(self.lens) == [SENTINEL] * 2


def test_select_empty_batch_is_ok_and_nulls_are_invalid(lib):
    assert getattr(lib, SELECT)(None, None, None, 0, None, None, None, None, None, None, None, None, None) == _abi.A3D_OK
    a = _SelectArgs()
    assert a.call(lib, n=0) == _abi.A3D_OK and a.untouched()
    for name in ("ctx", "views", "values", "lo", "hi", "out_points", "capacities", "lens"):
        a = _SelectArgs()
        assert a.call(lib, **{name: None}) == _abi.A3D_INVALID_PARAMETER, name
        assert a.untouched(), name
    for field in ("values", "out_points"):
        a = _SelectArgs()
        getattr(a, field)[1] = None
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched(), field
    a = _SelectArgs()
    a.views[0].points = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()


def test_select_clouds_of_2_to_the_32_points_or_within_a_tile_of_it_are_invalid(lib):
    for big in (1 << 32, (1 << 32) + 5, 1 << 40, (1 << 32) - 1, (1 << 32) - 1000):
        a = _SelectArgs()
        a.views[1].len = big
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, big
        assert a.untouched()


def test_select_output_for_a_field_the_cloud_lacks_is_missing_field(lib):
    a = _SelectArgs()
    a.out_normals[1] = 0xA0000  # cloud 1 has no normals
    assert a.call(lib) == _abi.A3D_MISSING_FIELD and a.untouched()
    a = _SelectArgs()
    a.out_colors[1] = 0xA0000  # cloud 1 has no colours
    assert a.call(lib) == _abi.A3D_MISSING_FIELD and a.untouched()
    a = _SelectArgs()
    assert a.call(lib, colors=None) == _abi.A3D_MISSING_FIELD and a.untouched()  # an output, but no colour table at all


def test_select_every_overlap_is_invalid(lib):
    """4 rows = 48 bytes of points or normals, 16 of values or index, 12 of colours."""
    cases = [
        ("out_points", 0, 0x10000), ("out_points", 0, 0x10000 + 36), ("out_points", 0, 0x30000),  # on points
        ("out_points", 1, 0x40000 + 24),  # two outputs on one buffer
        ("out_points", 0, 0x2C000 + 12),  # on the values' last word
        ("out_points", 1, 0x20000 + 47),  # on the last byte of cloud 0's normals
        ("out_normals", 0, 0x20000), ("out_normals", 0, 0x40000 + 44),
        ("out_colors", 0, 0x28000 + 11),  # on the input colours' last byte
        ("out_colors", 0, 0x10000 + 47), ("out_colors", 0, 0x70000 + 15),
        ("out_index", 0, 0x2D000), ("out_index", 1, 0x70000 + 12), ("out_index", 1, 0x68000 + 9),
    ]
    for field, i, address in cases:
        a = _SelectArgs()
        getattr(a, field)[i] = address
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
        assert a.untouched()


class _KnnArgs:
    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.ctx = C.c_void_p(0x900000)
        self.counts = (C.c_void_p * 2)(0x40000, None)
        self.qsum = (C.c_void_p * 2)(0x50000, 0x60000)
        self.stats = (C.c_uint64 * 8)(*[SENTINEL] * 8)
        self.dropped = (C.c_uint64 * 2)(SENTINEL, SENTINEL)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, n=2, radius=0.05, k=8, counts=self.counts, qsum=self.qsum,
                 stats=self.stats, dropped=self.dropped)
        a.update(override)
        return getattr(lib, KNN)(a["ctx"], a["views"], a["n"], a["radius"], a["k"], a["counts"], a["qsum"], a["stats"],
                                 a["dropped"])

    def untouched(self):
        return list(self.stats) == [SENTINEL] * 8 and list(self.dropped) == [SENTINEL] * 2


def test_knn_empty_batch_is_ok_and_nulls_are_invalid(lib):
    assert getattr(lib, KNN)(None, None, 0, 0.0, 99, None, None, None, None) == _abi.A3D_OK
    a = _KnnArgs()
    assert a.call(lib, n=0, radius=float("nan")) == _abi.A3D_OK and a.untouched()
    for name in ("ctx", "views", "qsum"):
        a = _KnnArgs()
        assert a.call(lib, **{name: None}) == _abi.A3D_INVALID_PARAMETER, name
        assert a.untouched(), name
    a = _KnnArgs()
    a.qsum[1] = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    a = _KnnArgs()
    a.views[1].points = None
    assert a.call(lib, k=0, qsum=None) == _abi.A3D_INVALID_PARAMETER and a.untouched()


@pytest.mark.parametrize("radius", [0.0, -0.0, -0.05, float("nan"), float("inf"), float("-inf"), 1e-30])
def test_knn_bad_radius_is_invalid(lib, radius):
    for k in (0, 8):
        a = _KnnArgs()
        assert a.call(lib, radius=radius, k=k) == _abi.A3D_INVALID_PARAMETER
        assert a.untouched()


def test_knn_k_above_32_and_huge_clouds_are_invalid(lib):
    for k in (33, 64, 0xFFFFFFFF):
        a = _KnnArgs()
        assert a.call(lib, k=k) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    for big in (1 << 32, 1 << 40, (1 << 32) - 1, (1 << 32) - 1000):
        a = _KnnArgs()
        a.views[0].len = big
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()


def test_knn_every_overlap_is_invalid(lib):
    cases = [("counts", 0, 0x10000 + 44), ("counts", 1, 0x10000), ("counts", 1, 0x40000 + 12), ("counts", 0, 0x60000),
             ("qsum", 0, 0x30000 + 47), ("qsum", 1, 0x50000 + 12), ("qsum", 1, 0x40000 - 12)]
    for field, i, address in cases:
        a = _KnnArgs()
        getattr(a, field)[i] = address
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
        assert a.untouched()


def test_python_wrappers_refuse_host_clouds_and_an_empty_list_is_empty():
    assert DevicePointCloud.select_many([], []) == [] and DevicePointCloud.select_many([], [], return_index=True) == ([], [])
    assert DevicePointCloud.neighbor_distances_many([], 0.05, 8) == ([], [], [])
    assert DevicePointCloud.remove_radius_outliers_many([], 0.05, 3) == []
    assert DevicePointCloud.remove_statistical_outliers_many([], 0.05, 8, 2.0, return_index=True) == ([], [])
    host = PointCloud([[1.0, 2.0, 3.0]])
    with pytest.raises(TypeError):
        DevicePointCloud.select_many([host], [[True]])
    with pytest.raises(TypeError):
        DevicePointCloud.neighbor_distances_many([host], 0.05, 8)
    with pytest.raises(_abi.InvalidParameter):
        DevicePointCloud.select_many([], [[True]])
    assert not hasattr(PointCloud, "remove_radius_outliers")


# ---- the threshold -----------------------------------------------------------------------------------------------------


def _threshold(lib, stats, std_ratio):
    out = C.c_uint32(SENTINEL)
    st = getattr(lib, THRESHOLD)((C.c_uint64 * 4)(*stats), std_ratio, C.byref(out))
    return st, out.value


def _exact(stats, std_ratio):
    """floor(mu + a * sigma) bracketed in exact rational arithmetic: the set of integers T such that the true value lies
    within 1e-6 of [T, T + 1) (the doubles of the rule are within 2^21 * 2^-50 of it)."""
    m, total, low, high = stats
    squares = low + (high << 32)
    mu = Fraction(total, m)
    var = Fraction(m * squares - total * total, m * (m - 1)) if m > 1 else Fraction(0)
    a = Fraction(std_ratio)
    # sqrt(var) between two rationals 1e-9 apart
    scale = 10**9
    root = math.isqrt(int(var * scale * scale))
    lo, hi = mu + a * Fraction(root, scale), mu + a * Fraction(root + 1, scale)
    eps = Fraction(1, 10**6)
    return {min(max(math.floor(v), 0), 0xFFFFFFFE) for v in (lo - eps, hi + eps)}


def test_threshold_against_exact_rational_arithmetic(lib):
    q = 32 * 32769
    cases = [
        ((0, 0, 0, 0), 2.0),                                     # m = 0
        (R.stats_of([777]), 3.0),                                # m = 1: no variance
        (R.stats_of([10, 20]), 1.0), (R.stats_of([10, 20]), 0.0),  # m = 2
        (R.stats_of([4321] * 50), 2.5),                          # all Q equal: num = 0
        ((1 << 20, (1 << 20) * q, ((1 << 20) * (q * q & 0xFFFFFFFF)), (1 << 20) * (q * q >> 32)), 2.0),  # 2^20 rows of the largest Q
        (R.stats_of(list(range(1000, 300000, 7))), 1.5),
        # half the rows at 0 and half at 2^20: num = m^2 2^40 / 4 far beyond 2^64
        ((1 << 24, (1 << 23) << 20, 0, (1 << 23) << 8), 2.0),
        ((1 << 24, (1 << 23) << 20, 0, (1 << 23) << 8), 1e9),    # T beyond 32 bits: the clamp
        ((1 << 24, (1 << 23) << 20, 0, (1 << 23) << 8), 8191.9999),
    ]
    for stats, ratio in cases:
        st, got = _threshold(lib, stats, ratio)
        assert st == _abi.A3D_OK, (stats, ratio)
        assert got == R.threshold(stats, ratio), (stats, ratio)
        if stats[0]:
            assert got in _exact(stats, ratio), (stats, ratio, got)
    assert _threshold(lib, (0, 0, 0, 0), 2.0)[1] == 0
    assert _threshold(lib, R.stats_of([777]), 3.0)[1] == 777
    assert _threshold(lib, R.stats_of([10, 20]), 1.0)[1] == 22  # 15 + sqrt(50)
    assert _threshold(lib, R.stats_of([4321] * 50), 2.5)[1] == 4321
    assert _threshold(lib, cases[5][0], 2.0)[1] == q
    big = (1 << 24) * ((1 << 23) << 40) - ((1 << 23) << 20) ** 2
    assert big > 1 << 64
    assert _threshold(lib, cases[8][0], 1e9)[1] == 0xFFFFFFFE
    assert DevicePointCloud.knn_distance_threshold((2, 30, 500), 1.0) == 22


def test_threshold_refusals(lib):
    ok = R.stats_of([10, 20])
    for ratio in (-1.0, float("nan"), float("inf")):
        st, got = _threshold(lib, ok, ratio)
        assert st == _abi.A3D_INVALID_PARAMETER and got == SENTINEL
    for bad in ((1 << 32, 0, 0, 0), (5, 1 << 53, 0, 0), (5, 0, 0, 1 << 42), (2, 30, 100, 0)):  # the last: num < 0
        st, got = _threshold(lib, bad, 1.0)
        assert st == _abi.A3D_INVALID_PARAMETER and got == SENTINEL, bad
    f = getattr(lib, THRESHOLD)
    out = C.c_uint32()
    assert f(None, 1.0, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert f((C.c_uint64 * 4)(*ok), 1.0, None) == _abi.A3D_INVALID_PARAMETER


# ---- the restatement ---------------------------------------------------------------------------------------------------


def test_restatement_against_f64_brute_force():
    """Per other, t = rint(fl(sqrt(fl(d2))) * fl(s)) against D * S in exact terms (D the distance of the two f32 points, S =
    32768 / r): the f32 chain makes at most 2 (the two differences, squared) + 1 (a product) + 2 (two sums) relative
    roundings of 2^-24 on d2, half of that after the root, then 1 for the root, 1 for s and 1 for the product: below
    6 * 2^-24 relative, times at most 32768 (1 + 2^-20): below 2^-7.  The rounding to the lattice adds 0.5.  The k smallest
    of two lists that differ by at most e elementwise have sums within k e.  A point the rule leaves out (d2 just above
    r2, or a cell two away) is at least r (1 - 2^-22) away, and every other within is at most r (1 + 2^-22) away, so the
    unbounded f64 search differs from the bounded one by less than 2^-6 per term.  Together: k (0.5 + 2^-5)."""
    p = plane_and_sphere()
    r = 0.08
    p64 = p.astype(np.float64)
    S = 32768.0 / float(np.float32(r))
    D = np.linalg.norm(p64[:, None, :] - p64[None, :, :], axis=2)
    np.fill_diagonal(D, np.inf)
    D.sort(axis=1)
    counts0, none, zeros = R.knn_distance(p, r, 0)
    assert none is None and zeros == (0, 0, 0, 0)
    assert np.array_equal(counts0, NR.moments(p, r)[1].astype(np.uint32))
    for k in (1, 8, 17, 32):
        counts, qsum, stats = R.knn_distance(p, r, k)
        assert np.array_equal(counts, counts0)
        has = qsum != R.NONE
        assert np.array_equal(has, counts.astype(np.int64) - 1 >= k) and 0 < has.sum()
        want = D[:, :k].sum(axis=1) * S
        err = np.abs(qsum[has].astype(np.float64) - want[has])
        print(f"k = {k}: {has.sum()} rows with a sum, largest |Q - f64| = {err.max():.3f} of the allowed {k * (0.5 + 2.0**-5):.3f}")
        assert err.max() <= k * (0.5 + 2.0**-5)
        assert stats == R.stats_of(qsum) and stats[0] == has.sum()
    assert has.sum() < len(p)  # at k = 32 some rows of the sphere lack others: both branches are met


def test_restatement_rows_slab_chunks_and_permutations_change_no_integer():
    p = np.r_[plane_and_sphere(3, 300, 200), np.float32([[np.nan, 0, 0], [np.inf, 1, 1], [1e30, 0, 0]])]
    whole = R.knn_distance(p, 0.08, 8)
    other = R.knn_distance(p, 0.08, 8, chunk=77, slab=False)
    assert np.array_equal(whole[0], other[0]) and np.array_equal(whole[1], other[1]) and whole[2] == other[2]
    assert (whole[0][-3:] == 0).all() and (whole[1][-3:] == R.NONE).all()  # dropped rows
    rows = np.sort(np.random.default_rng(1).choice(len(p), 100, replace=False))
    part = R.knn_distance(p, 0.08, 8, rows=rows)
    assert np.array_equal(part[0][rows], whole[0][rows]) and np.array_equal(part[1][rows], whole[1][rows])
    perm = np.random.default_rng(2).permutation(len(p))
    moved = R.knn_distance(p[perm], 0.08, 8)
    assert np.array_equal(moved[0], whole[0][perm]) and np.array_equal(moved[1], whole[1][perm]) and moved[2] == whole[2]


def test_restatement_duplicates_and_the_sentinel_edge():
    same = np.tile(np.float32([0.3, -0.2, 1.5]), (9, 1))
    counts, qsum, stats = R.knn_distance(same, 0.05, 8)
    assert (counts == 9).all() and (qsum == 0).all() and stats == (9, 0, 0, 0)  # a duplicate is an other at distance 0
    assert (R.knn_distance(same, 0.05, 9)[1] == R.NONE).all()
    for k in (1, 8, 9, 32):
        p = sentinel_edge_cloud(k)
        counts, qsum, stats = R.knn_distance(p, 0.05, k)
        assert np.array_equal(counts, np.repeat([k, k + 1, k + 2], [k, k + 1, k + 2]))
        assert (qsum[:k] == R.NONE).all() and (qsum[k:] != R.NONE).all() and stats[0] == 2 * k + 3


def test_select_restatement():
    v = np.uint32([0, 5, 6, 7, 0xFFFFFFFF, 5])
    assert R.select(v, 5, 6).tolist() == [1, 2, 5] and R.select(v, 7, 5).tolist() == []
    assert R.select(v, 0, 0xFFFFFFFF).tolist() == [0, 1, 2, 3, 4, 5] and R.select(v, 1, 0xFFFFFFFF).tolist() == [1, 2, 3, 4, 5]


def test_both_filters_remove_the_planted_outliers():
    """The radius filter at min_neighbors = 2 (one other row within RADIUS) removes exactly the 30 planted rows.  The
    statistical filter at k = 8, std_ratio = 2 removes all 30 (they have no others at all) and, of the 1 500 inliers, the
    sparse end of the distribution: measured here, on the restatement, 69 rows (4.6 %: the sphere is four times sparser
    than the plane, so the distribution of Q has two modes and its upper tail is heavier than a normal one's 2.3 %).  The
    cap is 5 %."""
    points, outlier = effectiveness_cloud()
    assert len(points) == 1500 + N_OUTLIERS and outlier.sum() == N_OUTLIERS
    kept = R.remove_radius_outliers(points, RADIUS, 2)
    assert np.array_equal(kept, np.flatnonzero(~outlier))
    kept, t = R.remove_statistical_outliers(points, RADIUS, 8, 2.0)
    gone = np.ones(len(points), bool)
    gone[kept] = False
    assert gone[outlier].all()
    lost = int(gone[~outlier].sum())
    print(f"statistical filter: threshold {t}, {lost} of 1500 inliers removed ({lost / 15:.2f} %)")
    assert lost <= 0.05 * 1500
