"""Normals of resident clouds (a3d_point_clouds_estimate_normals_device) without a GPU: the numpy restatement of the rule
(normals_restatement.py, the expected value of the GPU tests) against numpy.linalg.eigh in f64 and against the rule's own
properties, and the C ABI: the exported symbol, the header, the ctypes mirror, and every refusal that is decided on the
host before any HIP call (with made-up device addresses: nothing is dereferenced)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normals_restatement as R
from align3d_amd import A3dError, DevicePointCloud, PointCloud, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "a3d_point_clouds_estimate_normals_device"
SENTINEL = 0x7777


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the _raw_bits recipe of test_gpu_voxel_downsample.py)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def plane_and_sphere(seed=7, n_plane=1000, n_sphere=500):
    """A noisy plane (sigma 2 mm over a 1 m square) plus a sphere of radius 0.4 m: about 1 500 points."""
    rng = np.random.default_rng(seed)
    plane = np.c_[rng.uniform(0, 1, (n_plane, 2)), 0.5 + rng.normal(0, 0.002, n_plane)]
    u = rng.normal(size=(n_sphere, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return np.r_[plane, u * 0.4 + [2.0, 0.0, 0.5]].astype(np.float32)


_cache = {}


def _estimated():
    if not _cache:
        p = plane_and_sphere()
        _cache["p"], _cache["out"] = p, R.estimate_normals(p, 0.08)
    return _cache["p"], _cache["out"]


# ---- the restatement ---------------------------------------------------------------------------------------------------


def test_restatement_against_eigh_in_f64():
    """For every valid row, (angle to eigh's eigenvector of A's smallest eigenvalue) x (l1 - l0) / l2 <= 16 * 2^-24: a
    first-order eigenvector perturbation bound with a few f32 roundings of the matrix."""
    p, (normals, curvature, counts, valid) = _estimated()
    assert valid.sum() > 1400 and np.median(counts[valid]) >= 8
    _, N, S, M = R.moments(p, 0.08)
    A, _ = R.scatter_matrix(N, S, M)
    w, V = np.linalg.eigh(A[valid])
    got = normals[valid].astype(np.float64)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4 * 2.0**-24
    angle = np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(V[:, :, 0], got), axis=1)))
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    print(f"largest angle {angle.max():.3g} rad, largest angle x relative gap {(angle * gap).max():.3g}")
    assert (angle * gap).max() <= 16 * 2.0**-24
    # curvature is the smallest eigenvalue's share of the trace
    assert np.abs(curvature[valid] - w[:, 0] / w.sum(axis=1)).max() <= 1e-5
    # the plane's rows (away from its border) see the plane, and look at the viewpoint: the origin is below z = 0.5
    inner = valid[:1000] & (np.abs(p[:1000, :2] - 0.5) < 0.4).all(axis=1)
    assert inner.sum() > 500 and (normals[:1000][inner][:, 2] < -0.97).all()
    # the sphere's rows point along the radius, away from the centre or towards it as the origin demands
    radial = (p[1000:] - np.float32([2.0, 0.0, 0.5])) / np.float32(0.4)
    ok = valid[1000:] & (counts[1000:] >= 7)  # (three or four neighbours on a sphere span any plane)
    assert ok.sum() > 20 and (np.abs((normals[1000:] * radial).sum(axis=1))[ok] > 0.9).all()
    assert ((normals[1000:] * -p[1000:]).sum(axis=1)[valid[1000:]] >= 0).all()


def test_the_slab_of_candidates_changes_no_integer():
    p = np.r_[plane_and_sphere(3, 300, 200), _raw_bits(5, 20)]
    a, b = R.moments(p, 0.08, chunk=64), R.moments(p, 0.08, chunk=500, slab=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_noise_free_plane_is_exact_and_the_sign_follows_the_viewpoint():
    """z = const: q_z = 0 for every neighbour, so only the (0,1) rotation acts and the normal is exactly (0, 0, +-1)."""
    rng = np.random.default_rng(11)
    p = np.c_[rng.uniform(-1, 1, (400, 2)), np.full(400, 0.75)].astype(np.float32)
    for viewpoint, z in (((0, 0, 5), 1.0), ((0, 0, -5), -1.0), (None, -1.0), ((3, 3, 0.75), 1.0)):
        # (the last viewpoint lies in the plane: dot == 0 keeps the sign the eigenvector came with, +1)
        normals, curvature, counts, valid = R.estimate_normals(p, 0.3, viewpoint=viewpoint)
        assert valid.all() and counts.min() >= 3
        assert (normals == np.float32([0, 0, z])).all(), viewpoint  # (by value: a negated 0 is -0)
        assert (curvature == 0).all()
    flipped, _, _, _ = R.estimate_normals(p, 0.3, old_normals=np.tile(np.float32([0.1, 0.2, -0.5]), (400, 1)))
    assert (flipped[:, 2] == -1).all()


def test_a_subset_of_rows_gets_the_bits_of_the_whole():
    p, whole = _estimated()
    rows = np.sort(np.random.default_rng(3).choice(len(p), size=200, replace=False))
    for slab in (True, False):
        part = R.estimate_normals(p, 0.08, rows=rows, slab=slab, chunk=64)
        assert np.array_equal(_bits(part[0][rows]), _bits(whole[0][rows])) and np.array_equal(part[2][rows], whole[2][rows])
        assert np.array_equal(_bits(part[1][rows]), _bits(whole[1][rows])) and np.array_equal(part[3][rows], whole[3][rows])


def test_permuting_the_rows_permutes_every_output_bit_for_bit():
    p, (normals, curvature, counts, valid) = _estimated()
    perm = np.random.default_rng(2).permutation(len(p))
    n2, c2, k2, v2 = R.estimate_normals(p[perm], 0.08)
    assert np.array_equal(_bits(n2), _bits(normals[perm])) and np.array_equal(_bits(c2), _bits(curvature[perm]))
    assert np.array_equal(k2, counts[perm]) and np.array_equal(v2, valid[perm])


def test_drop_and_validity_rules():
    # raw-bit rows are dropped (or, the few finite and near ones, alone): zeros, and they are nobody's neighbour
    p = plane_and_sphere(4, 300, 0)
    raw = _raw_bits(9, 40)
    kept_raw, _ = R.cells(raw, 0.08)
    assert (~kept_raw).sum() > 30
    mixed = np.r_[p[:150], raw, p[150:]]
    rows = np.r_[0:150, 190:340]
    alone = R.estimate_normals(p, 0.08)
    n, c, k, v = R.estimate_normals(mixed, 0.08)
    gone = np.r_[150:190][~kept_raw]
    assert (k[gone] == 0).all() and not v[gone].any() and (_bits(n[gone]) == 0).all() and (_bits(c[gone]) == 0).all()
    # the raw rows that are kept lie nowhere near the plane (z = 0.5), so the plane's rows come out as if alone
    assert (np.abs(raw[kept_raw][:, 2] - 0.5) > 0.2).all()
    assert np.array_equal(_bits(n[rows]), _bits(alone[0])) and np.array_equal(k[rows], alone[2])
    assert np.array_equal(_bits(c[rows]), _bits(alone[1])) and np.array_equal(v[rows], alone[3])
    # n identical points: mx == 0, invalid, count n
    same = np.tile(np.float32([0.3, -0.2, 1.5]), (7, 1))
    n, c, k, v = R.estimate_normals(same, 0.05)
    assert not v.any() and (k == 7).all() and (_bits(n) == 0).all() and (_bits(c) == 0).all()
    # fewer than min_neighbors
    tri = np.float32([[0, 0, 1], [0.01, 0, 1], [0, 0.01, 1]])
    assert R.estimate_normals(tri, 0.05)[3].all()
    n, c, k, v = R.estimate_normals(tri, 0.05, min_neighbors=4)
    assert not v.any() and (k == 3).all() and (_bits(n) == 0).all()
    n, c, k, v = R.estimate_normals(tri[:2], 0.05)
    assert not v.any() and (k == 2).all()
    # collinear points: valid, with some unit normal perpendicular to the line
    direction = np.float64([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    line = (np.float64([0.2, 0.1, 2.0]) + np.linspace(0, 0.1, 30)[:, None] * direction).astype(np.float32)
    n, c, k, v = R.estimate_normals(line, 0.03)
    assert v.all()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 1e-6
    # (the points are rounded to f32 and the offsets to the 2^-15 r lattice: the line is straight to about 1e-4 of r)
    assert np.abs(n.astype(np.float64) @ direction).max() <= 1e-3
    # the case that carries the issue's bound of 1e-6:
    exact = (np.float32([0.25, 0.5, 2.0]) + np.arange(30, dtype=np.float32)[:, None] * np.float32([0.0078125, 0.015625, 0])
             ).astype(np.float32)  # offsets that are exact in f32 and on the lattice: the moments see a perfect line
    n, c, k, v = R.estimate_normals(exact, 0.0625)
    d = np.float64([1.0, 2.0, 0.0]) / np.sqrt(5.0)
    assert v.all() and np.abs(n.astype(np.float64) @ d).max() <= 1e-6
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 1e-6


# ---- the ABI, without a device -----------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


class _Args:
    """Two clouds of 4 points at made-up, disjoint device addresses, a made-up context, and sentinel-filled result arrays:
    the checks under test fail before anything is dereferenced."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.ctx = C.c_void_p(0x900000)
        self.out_normals = (C.c_void_p * 2)(0x40000, 0x50000)
        self.out_curvature = (C.c_void_p * 2)(0x60000, None)
        self.out_counts = (C.c_void_p * 2)(0x70000, 0x80000)
        self.valid = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.dropped = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.radius, self.min_neighbors, self.orient = 0.05, 3, 0
        self.viewpoints = (C.c_float * 6)(0, 0, 0, 1, 2, 3)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, n=2, radius=self.radius, min_neighbors=self.min_neighbors,
                 viewpoints=self.viewpoints, orient=self.orient, out_normals=self.out_normals,
                 out_curvature=self.out_curvature, out_counts=self.out_counts, valid=self.valid, dropped=self.dropped)
        a.update(override)
        return getattr(lib, NAME)(a["ctx"], a["views"], a["n"], a["radius"], a["min_neighbors"], a["viewpoints"], a["orient"],
                                  a["out_normals"], a["out_curvature"], a["out_counts"], a["valid"], a["dropped"])

    def untouched(self):
        return list(self.valid) == [SENTINEL] * 2 and list(self.dropped) == [SENTINEL] * 2


def test_symbol_is_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    assert hasattr(lib, NAME)
    assert hasattr(_abi.load_library(_abi.DIAG_LIB_PATH), NAME)
    assert re.search(r"a3d_status\s+%s\s*\(" % NAME, header)
    assert NAME in _abi.SIGNATURES and len(_abi.SIGNATURES[NAME][1]) == 12
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    assert NAME in section
    assert lib.a3d_abi_version() == 1
    assert "#define A3D_ABI_VERSION 1" in header
    assert NAME in open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    for method in ("estimate_normals", "estimate_normals_many"):
        assert callable(getattr(DevicePointCloud, method))


def test_the_rule_stands_verbatim_in_the_kernel_file_and_the_restatement():
    def rule(text, strip):
        lines = [ln.strip().lstrip(strip).strip() for ln in text.splitlines()]
        joined = " ".join(" ".join(lines).split())
        return joined[joined.index("1. Grid."):joined.index("which camera saw each cell.")]

    hip = open(os.path.join(ROOT, "align3d_amd", "csrc", "cloud_normals.hip")).read()
    assert rule(hip, "/") == rule(R.__doc__, "")


def test_product_library_has_no_knob_for_the_feature():
    assert b"A3D_NORMALS" not in open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_NORMALS_ORDER" in open(_abi.DIAG_LIB_PATH, "rb").read()


def test_empty_batch_is_ok_and_touches_nothing(lib):
    f = getattr(lib, NAME)
    assert f(None, None, 0, 0.0, 0, None, 0, None, None, None, None, None) == _abi.A3D_OK
    a = _Args()
    assert a.call(lib, n=0) == _abi.A3D_OK
    assert a.call(lib, n=0, radius=float("nan"), min_neighbors=0) == _abi.A3D_OK
    assert a.untouched()


def test_null_arguments_are_invalid_without_a_device(lib):
    a = _Args()
    for name in ("ctx", "views", "out_normals", "valid"):
        assert a.call(lib, **{name: None}) == _abi.A3D_INVALID_PARAMETER, name
        assert a.untouched(), name


@pytest.mark.parametrize("radius", [0.0, -0.0, -0.05, float("nan"), float("inf"), float("-inf"), 1e-30])
def test_bad_radius_is_invalid_without_a_device(lib, radius):
    a = _Args()
    assert a.call(lib, radius=radius) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


@pytest.mark.parametrize("min_neighbors", [0, 1, 2])
def test_fewer_than_three_min_neighbors_is_invalid_without_a_device(lib, min_neighbors):
    a = _Args()
    assert a.call(lib, min_neighbors=min_neighbors) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_viewpoint_is_invalid_without_a_device(lib, bad):
    for k in range(6):
        a = _Args()
        a.viewpoints[k] = bad
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
        assert a.untouched()


def test_cloud_of_2_to_the_32_points_or_within_a_tile_of_it_is_invalid_without_a_device(lib):
    for big in (1 << 32, (1 << 32) + 5, 1 << 40, (1 << 32) - 1, (1 << 32) - 1000):
        a = _Args()
        a.views[1].len = big
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, big
        assert a.untouched()


def test_null_points_or_output_of_a_non_empty_cloud_are_invalid_without_a_device(lib):
    a = _Args()
    a.views[0].points = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    a = _Args()
    a.out_normals[1] = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


def test_orient_by_normals_on_a_cloud_without_normals_is_missing_field(lib):
    a = _Args()
    assert a.call(lib, orient=1) == _abi.A3D_MISSING_FIELD  # cloud 1 has no normals
    assert a.untouched()


def test_every_overlap_but_in_place_is_invalid_without_a_device(lib):
    """4 points = 48 bytes of normals, 16 of curvature or counts."""
    cases = [
        ("out_normals", 0, 0x10000),       # on the cloud's own points
        ("out_normals", 0, 0x10000 + 36),  # its start on the points' last row
        ("out_normals", 0, 0x30000),       # on the other cloud's points
        ("out_normals", 1, 0x40000),       # two outputs on one buffer
        ("out_normals", 1, 0x40000 + 24),
        ("out_curvature", 0, 0x10000 + 44),
        ("out_curvature", 0, 0x40000),     # curvature on the normals output
        ("out_curvature", 1, 0x60000 + 12),
        ("out_counts", 0, 0x30000),
        ("out_counts", 1, 0x70000 + 12),   # two count outputs, one word shared
        ("out_counts", 1, 0x50000 + 44),
    ]
    for orient in (0, 1):
        for field, i, address in cases:
            a = _Args()
            a.views[1].normals = 0xA0000
            getattr(a, field)[i] = address
            assert a.call(lib, orient=orient) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
            assert a.untouched()
    # the old normals are an input of orient_by_normals: only exactly in place may the output lie on them
    for address in (0x20000 + 12, 0x20000 - 12):
        a = _Args()
        a.views[1].normals = 0xA0000
        a.out_normals[0] = address
        assert a.call(lib, orient=1) == _abi.A3D_INVALID_PARAMETER, hex(address)
        assert a.untouched()
    a = _Args()
    a.views[1].normals = 0xA0000
    a.out_curvature[0] = 0x20000  # another output on the old normals
    assert a.call(lib, orient=1) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


def test_python_wrappers_refuse_host_clouds_and_an_empty_list_is_empty():
    assert DevicePointCloud.estimate_normals_many([], 0.05) == []
    assert DevicePointCloud.estimate_normals_many([], 0.05, curvature=True, counts=True) == ([], [], [])
    assert DevicePointCloud.estimate_normals_many([], 0.05, dropped=True) == ([], [])
    with pytest.raises(TypeError):
        DevicePointCloud.estimate_normals_many([PointCloud([[1.0, 2.0, 3.0]])], 0.05)
    with pytest.raises(_abi.InvalidParameter):
        DevicePointCloud.estimate_normals_many([], 0.05, orient="camera")
    assert not hasattr(PointCloud, "estimate_normals")
