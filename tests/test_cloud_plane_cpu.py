"""Plane segmentation of resident clouds without a GPU: the two host-only entries (a3d_plane_hypotheses,
a3d_plane_from_moments) against the numpy restatement (plane_restatement.py) word for word and bit for bit, the refusals
that are decided on the host (with made-up device addresses: nothing is dereferenced), the header, the ctypes mirror and the
Rust bindings, and the restatement itself on clouds whose plane is known by construction."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import plane_restatement as R
from align3d_amd import DevicePointCloud, _abi
from plane_cases import (SCENE_H, SCENE_SEED, SCENE_T, degenerate_cloud, exact_sheet, long_plane, parallel_sheets,
                         tabletop_scene)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a3d_point_clouds_segment_plane_device", "a3d_plane_hypotheses", "a3d_plane_from_moments")
F = np.float32
Q = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------


def test_symbols_are_exported_declared_mirrored_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys

    text = open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    assert text == gen_rust_sys.generate()
    for name, arity in zip(NAMES, (13, 4, 6)):
        assert hasattr(lib, name) and hasattr(diag, name)
        assert re.search(r"a3d_status\s+%s\s*\(" % name, header) and name in section
        assert section.index("a3d_point_clouds_cluster_device(") < section.index(name + "(")  # after the cluster entry
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == arity
        assert "pub fn %s(" % name in text
    for method in ("segment_plane", "segment_plane_many", "split_plane", "split_plane_many", "remove_plane", "remove_plane_many",
                   "plane_hypotheses", "plane_from_moments"):
        assert callable(getattr(DevicePointCloud, method))


def test_the_rule_stands_verbatim_in_the_kernel_file_the_header_and_the_restatement():
    def rule(text, strip):
        lines = [ln.strip().lstrip(strip).strip() for ln in text.splitlines()]
        joined = " ".join(" ".join(lines).split())
        return joined[joined.index("1. Candidate plane of a triple."):joined.index("5 are repeated against it, then step 6.")]

    hip = open(os.path.join(ROOT, "align3d_amd", "csrc", "cloud_plane.hip")).read()
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    assert rule(hip, "/") == rule(R.__doc__, "") == rule(header, "*")
    assert "count[h] << 32 | (0xFFFFFFFF - h)" in rule(hip, "/") and "L > (U*V) * 2^-20" in rule(hip, "/")


def test_product_library_has_no_knob_for_the_feature():
    assert b"A3D_PLANE" not in open(_abi.LIB_PATH, "rb").read()
    diag = open(_abi.DIAG_LIB_PATH, "rb").read()
    assert b"A3D_PLANE_ROWS" in diag and b"A3D_PLANE_SPLIT" in diag and b"A3D_PLANE_COUNTERS" in diag


# ---- a3d_plane_hypotheses ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", (0, 1, 1 << 63, (1 << 64) - 1))
def test_hypotheses_equal_the_restatement_word_for_word(seed):
    for length in (1, 2, 3, 65, (1 << 32) - 1):
        for H in (0, 1, 4096):
            got = DevicePointCloud.plane_hypotheses(seed, length, H)
            want = R.hypotheses(seed, length, H)
            assert got.dtype == np.uint32 and got.shape == (H, 3) and np.array_equal(got, want)
            assert (got < length).all()
    # candidate h does not depend on H, and the indices spread over the cloud
    big = DevicePointCloud.plane_hypotheses(seed, 1000, 4096)
    assert np.array_equal(big[:7], DevicePointCloud.plane_hypotheses(seed, 1000, 7))
    assert len(np.unique(big)) > 950 and abs(float(big.mean()) - 499.5) < 15


def test_hypotheses_refusals(lib):
    out = (C.c_uint32 * 12)(*[0x7777] * 12)
    assert lib.a3d_plane_hypotheses(0, 0, 4, out) == _abi.A3D_INVALID_PARAMETER  # candidates of an empty cloud
    assert lib.a3d_plane_hypotheses(0, 1 << 32, 4, out) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_plane_hypotheses(0, 10, 4097, out) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_plane_hypotheses(0, 10, 4, None) == _abi.A3D_INVALID_PARAMETER
    assert list(out) == [0x7777] * 12
    assert lib.a3d_plane_hypotheses(0, 0, 0, None) == _abi.A3D_OK and lib.a3d_plane_hypotheses(5, 10, 0, out) == _abi.A3D_OK
    assert list(out) == [0x7777] * 12
    assert lib.a3d_plane_hypotheses(5, 10, 4, out) == _abi.A3D_OK and list(out) == R.hypotheses(5, 10, 4).reshape(-1).tolist()
    with pytest.raises(_abi.A3dError):
        DevicePointCloud.plane_hypotheses(0, 0, 3)
    with pytest.raises(_abi.A3dError):
        DevicePointCloud.plane_hypotheses(-1, 5, 3)


# ---- a3d_plane_from_moments -------------------------------------------------------------------------------------------------


def _record_of(q):
    """The record of step 5 for lattice rows q [n, 3], |q| <= 2^20 (products and sums fit int64 for n <= 2^20)."""
    q = np.asarray(q, np.int64).reshape(-1, 3)
    rec = [len(q)] + [int(q[:, k].sum()) for k in range(3)]
    prods = [q[:, k] * q[:, l] for k, l in R.KL]
    return rec + [int((P & 0x7FFFFFFF).sum()) for P in prods] + [int((P >> 31).sum()) for P in prods]


def _check(rec, point, t, fallback, valid=None):
    got, got_valid = DevicePointCloud.plane_from_moments(rec, point, t, fallback)
    want, want_valid, _ = R.plane_from_moments(rec, point, t, fallback)
    assert np.array_equal(_bits64(got), _bits64(want)), (got, want)
    assert got_valid == want_valid and (valid is None or got_valid == valid)
    return got


def test_from_moments_of_random_inlier_sets():
    rng = np.random.default_rng(21)
    for trial in range(40):
        n = int(rng.integers(10, 400))
        t = float(F(rng.uniform(0.001, 0.1)))
        normal = rng.normal(size=3)
        normal /= np.linalg.norm(normal)
        a = rng.uniform(-5, 5, size=3).astype(F)
        rows = rng.uniform(-1, 1, size=(n, 3))
        rows -= np.outer(rows @ normal, normal)  # on the plane through a, up to the rounding to f32
        points = (a + rows).astype(F)
        rec = R.moments(points, np.ones(n, bool), a, t)
        plane = _check(rec, a, t, (0, 0, 1), valid=True)
        assert abs(abs(float(plane[:3] @ normal)) - 1) < 1e-3 and plane[3] >= 0 and abs(np.linalg.norm(plane[:3]) - 1) < 1e-6


def test_from_moments_at_the_bounds_where_hi_and_lo_both_carry():
    corners = [(Q, Q, -Q), (-Q, Q, Q), (Q, -Q, Q)]
    rec = _record_of(corners)
    assert rec[4] == 0 and rec[10] == 3 << 9 and rec[11] == -(1 << 9)  # xx: Lo 0, Hi 3 * 2^9; xy: Hi negative
    _check(rec, (1.0, -2.0, 0.5), 0.01, (0, 0, 1), valid=True)
    rng = np.random.default_rng(22)
    many = rng.choice([-Q, Q, Q - 1, -Q + 1], size=(Q, 3))
    rec = _record_of(many)
    assert max(rec[4:10]) > 1 << 45 and max(abs(h) for h in rec[10:16]) > 1 << 27
    _check(rec, (100.0, 200.0, -300.0), 0.25, (1, 0, 0), valid=True)
    flat = np.c_[rng.choice([-Q, Q], size=(Q, 2)), np.zeros(Q, np.int64)]  # 2^20 rows at the bounds in the plane z = 0
    plane = _check(_record_of(flat), (0.0, 0.0, 2.0), 0.25, (1, 0, 0), valid=True)
    assert plane.tolist() == [0.0, 0.0, -1.0, 2.0]  # the origin is below the plane


def test_from_moments_falls_back_with_two_rows_and_with_all_rows_equal():
    a, fallback = F([0.5, -1.5, 2.0]), F([0.6, 0.0, 0.8])
    two = _record_of([(5, 0, 1), (-3, 2, 0)])
    plane = _check(two, a, 0.05, fallback, valid=False)
    assert np.array_equal(_bits64(np.abs(plane[:3])), _bits64(np.abs(fallback.astype(np.float64))))
    d = -((np.float64(fallback[0]) * a[0] + np.float64(fallback[1]) * a[1]) + np.float64(fallback[2]) * a[2])
    assert d < 0 and plane[3] == -d and plane[0] == -np.float64(fallback[0])  # c = a, and the sign rule still applies
    same = _record_of([(7, -2, 3)] * 50)
    _check(same, a, 0.05, fallback, valid=False)
    _check([0] * 16, a, 0.05, fallback, valid=False)


def test_from_moments_of_an_exact_lattice_plane_gives_the_axis_exactly():
    q = [(x, y, 0) for x in range(-6, 7) for y in range(-4, 5)]
    for z, want in ((3.0, [0.0, 0.0, -1.0, 3.0]), (-3.0, [0.0, 0.0, 1.0, 3.0])):
        plane = _check(_record_of(q), (0.25, -0.5, z), 0.5, (1, 0, 0), valid=True)
        assert plane.tolist() == want
    # the sign rule at d == 0: nothing is negated, whichever way the column points
    plane = _check(_record_of(q), (0.0, 0.0, 0.0), 0.5, (1, 0, 0), valid=True)
    assert abs(plane[2]) == 1.0 and plane[3] == 0.0 and plane[0] == plane[1] == 0.0
    tilted = [(x, y, x) for x in range(-6, 7) for y in range(-4, 5)]  # the plane z = x through a
    for a in ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0)):  # the origin on either side
        plane = _check(_record_of(tilted), a, 0.5, (1, 0, 0), valid=True)
        assert plane[3] > 0 and np.sign(plane[2]) == -np.sign(a[2])


def test_from_moments_refusals(lib):
    rec = (C.c_uint64 * 16)(*[m & R.MASK64 for m in _record_of([(1, 2, 3), (4, 5, 6), (7, 8, 10)])])
    a, f = (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(0, 0, 1)
    plane, valid = (C.c_double * 4)(7, 7, 7, 7), C.c_uint32(7)

    def call(m=rec, point=a, t=0.05, fallback=f, out=plane):
        return lib.a3d_plane_from_moments(m, point, t, fallback, out, C.byref(valid))

    for bad in (dict(m=None), dict(point=None), dict(fallback=None), dict(out=None), dict(t=0.0), dict(t=-1.0),
                dict(t=float("nan")), dict(t=float("inf")), dict(t=1e-40)):
        assert call(**bad) == _abi.A3D_INVALID_PARAMETER
    for word, value in ((0, 1 << 32), (1, 3 * Q + 1), (2, R.MASK64 - 3 * Q), (4, 3 * 0x7FFFFFFF + 1), (10, (3 << 9) + 1),
                        (12, R.MASK64 - (3 << 9))):
        spoilt = (C.c_uint64 * 16)(*rec)
        spoilt[word] = value
        assert call(m=spoilt) == _abi.A3D_INVALID_PARAMETER, word
    assert list(plane) == [7, 7, 7, 7] and valid.value == 7
    assert call() == _abi.A3D_OK and valid.value == 1
    assert lib.a3d_plane_from_moments(rec, a, 0.05, f, plane, None) == _abi.A3D_OK


# ---- the refusals of the device entry that are decided on the host -----------------------------------------------------------


class _Args:
    """Two clouds of 8 rows at made-up, disjoint device addresses, a made-up context and sentinel-filled host outputs: the
    checks under test fail before anything is dereferenced."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 8
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 8
        self.ctx = C.c_void_p(0x900000)
        self.triples = [np.uint32([[0, 1, 2], [3, 4, 7]]), np.uint32([[5, 6, 7]])]
        self.flags, self.counts = [0x40000, 0x50000], [0x60000, 0x70000]
        self.t, self.refine = 0.05, 0
        self.planes = (C.c_double * 8)(*[7.0] * 8)
        self.words = [(C.c_uint64 * 2)(7, 7) for _ in range(3)]

    def call(self, lib, **change):
        for k, v in change.items():
            setattr(self, k, v)
        tr = None if self.triples is None else (C.c_void_p * 2)(*[None if t is None else t.ctypes.data for t in self.triples])
        n_tr = (C.c_uint32 * 2)(*[0 if t is None else len(t) for t in (self.triples or [None, None])])
        if "n_triples" in change:
            n_tr = change["n_triples"]
        return lib.a3d_point_clouds_segment_plane_device(
            self.ctx, self.views, 2, self.t, self.refine, tr, n_tr,
            None if self.flags is None else (C.c_void_p * 2)(*self.flags),
            None if self.counts is None else (C.c_void_p * 2)(*self.counts), self.planes, *self.words)

    def untouched(self):
        return list(self.planes) == [7.0] * 8 and all(list(w) == [7, 7] for w in self.words)


def test_device_entry_refusals_decided_on_the_host(lib):
    cases = [dict(t=0.0), dict(t=-0.05), dict(t=float("nan")), dict(t=float("inf")), dict(refine=9),
             dict(triples=[np.zeros((4097, 3), np.uint32), np.uint32([[5, 6, 7]])]),
             dict(triples=[np.uint32([[0, 1, 8]]), np.uint32([[5, 6, 7]])]),  # an index == len
             dict(triples=[np.uint32([[0, 1, 2]]), np.uint32([[0xFFFFFFFF, 6, 7]])]),
             dict(triples=None), dict(flags=None), dict(flags=[0x40000, None]),
             dict(flags=[0x10000 + 92, 0x50000]),  # on the last word of cloud 0's points
             dict(flags=[0x20000, 0x50000]),  # on cloud 0's normals
             dict(flags=[0x40000, 0x40000 + 28]),  # two clouds' flags share a word
             dict(counts=[0x40000 + 28, 0x70000]),  # counts on the last word of the flags
             dict(counts=[0x60000, 0x60000 + 4])]  # cloud 0 has two candidates: its second count is cloud 1's first
    for change in cases:
        args = _Args()
        assert args.call(lib, **change) == _abi.A3D_INVALID_PARAMETER, change
        assert args.untouched(), change
    args = _Args()
    args.views[1].len = 1 << 32
    assert args.call(lib) == _abi.A3D_INVALID_PARAMETER and args.untouched()
    args = _Args()
    args.views[1].len = 0  # candidates of an empty cloud name rows past its end
    assert args.call(lib) == _abi.A3D_INVALID_PARAMETER and args.untouched()
    args = _Args()
    assert lib.a3d_point_clouds_segment_plane_device(None, args.views, 2, 0.05, 0, None, None, None, None, None, None, None,
                                                     None) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_point_clouds_segment_plane_device(None, None, 0, 0.0, 99, None, None, None, None, None, None, None,
                                                     None) == _abi.A3D_OK  # n == 0
    # two empty clouds without candidates: no plane, decided without a device
    args = _Args()
    args.views[0].len = args.views[1].len = 0
    assert args.call(lib, triples=[None, None]) == _abi.A3D_OK
    assert list(args.planes) == [0.0] * 8 and list(args.words[0]) == [0xFFFFFFFF] * 2
    assert list(args.words[1]) == [0, 0] and list(args.words[2]) == [0, 0]


# ---- the restatement on constructions ---------------------------------------------------------------------------------------


def test_restatement_on_exact_coordinates_ties_and_degenerate_candidates():
    points, triples, t, flags = exact_sheet()
    seg = R.segment(points, triples, t)
    assert seg.best == 0 and np.array_equal(seg.flags, flags) and seg.counts.tolist() == [int(flags.sum())]
    assert 0 < flags.sum() < len(flags) and seg.inliers == seg.refit_rows == int(flags.sum())
    for first in (0, 1):
        points, triples = parallel_sheets(first)
        seg = R.segment(points, triples, 0.25)
        assert seg.counts.tolist() == [150, 150] and seg.best == 0
        assert np.array_equal(np.flatnonzero(seg.flags) // 150, np.full(150, first))
    points, triples, good = degenerate_cloud()
    seg = R.segment(points, triples, 0.05)
    _, _, wanted = R.candidates(points, triples)
    assert np.array_equal(wanted, good) and (seg.counts[~good] == 0).all() and (seg.counts[good] >= 3).all()
    none = R.segment(points, triples[~good], 0.05)
    assert none.best == R.NONE and not none.flags.any() and not none.plane.any() and none.inliers == 0


def test_restatement_leaves_far_inliers_out_of_the_refit_and_refines():
    points, triples, t = long_plane()
    seg = R.segment(points, triples, t)
    assert seg.inliers == 3000 and 1000 < seg.refit_rows < 1400  # 16.384 of 40 metres
    assert abs(abs(seg.plane[2]) - 1) < 1e-6 and abs(seg.plane[3]) < 1e-3
    refined = R.segment(points, triples, t, refine=2)
    assert len(refined.moments) == 3 and refined.moments[0] == seg.moments[0]
    assert refined.moments[1][1:4] != seg.moments[0][1:4]  # taken against the centroid now


def test_restatement_finds_exactly_the_floor_of_the_scene_at_the_fixed_seed():
    points, _, _, floor, box = tabletop_scene()
    assert len(points) == 20000 and floor.sum() == 12000 and box.sum() == 6000
    triples = R.hypotheses(SCENE_SEED, len(points), SCENE_H)
    seg = R.segment(points, triples, SCENE_T)
    assert floor[triples[seg.best]].all()  # an all-floor triple wins
    assert np.array_equal(seg.flags.astype(bool), floor)  # and its inlier set is exactly the floor
    assert abs(abs(seg.plane[2]) - 1) < 1e-4 and abs(seg.plane[3]) < SCENE_T and seg.plane[3] >= 0
