"""Voxel-grid downsampling by cell mean (a3d_point_clouds_voxel_mean_device, DevicePointCloud.voxel_downsample(mode="mean"))
without a GPU: the exported symbol, the header, the ctypes mirror, every argument check that is decided on the host before
any HIP call (with made-up device addresses: nothing is dereferenced), the wrapper's `mode` and `return_counts` errors, and
the properties of the numpy restatement (voxel_mean_restatement.py) that the GPU tests take as the expected value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voxel_mean_restatement as M
import voxel_restatement as V
from align3d_amd import DevicePointCloud, InvalidParameter, PointCloud, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "a3d_point_clouds_voxel_mean_device"
LEN_SENTINEL = 0x7777
ORIGINS = (None, (0.013, -0.4, 7.5))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


class _Args:
    """Two clouds of 4 points at made-up, disjoint device addresses (cloud 0 with normals and colours, cloud 1 bare), a
    made-up context, and sentinel-filled result arrays: the checks under test fail before anything is dereferenced."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.ctx = C.c_void_p(0x900000)
        self.colors = (C.c_void_p * 2)(0xB0000, None)
        self.out_points = (C.c_void_p * 2)(0x40000, 0x50000)
        self.out_normals = (C.c_void_p * 2)(0x60000, None)
        self.out_colors = (C.c_void_p * 2)(0xC0000, None)
        self.out_index = (C.c_void_p * 2)(0x70000, 0x80000)
        self.out_counts = (C.c_void_p * 2)(0xD0000, 0xE0000)
        self.caps = (C.c_uint64 * 2)(4, 4)
        self.lens = (C.c_uint64 * 2)(LEN_SENTINEL, LEN_SENTINEL)
        self.dropped = (C.c_uint64 * 2)(LEN_SENTINEL, LEN_SENTINEL)
        self.voxel = 0.05
        self.origin = (C.c_float * 3)(0.0, 0.0, 0.0)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, colors=self.colors, n=2, voxel=self.voxel, origin=self.origin,
                 out_points=self.out_points, out_normals=self.out_normals, out_colors=self.out_colors,
                 out_index=self.out_index, out_counts=self.out_counts, caps=self.caps, lens=self.lens, dropped=self.dropped)
        a.update(override)
        return getattr(lib, NAME)(a["ctx"], a["views"], a["colors"], a["n"], a["voxel"], a["origin"], a["out_points"],
                                  a["out_normals"], a["out_colors"], a["out_index"], a["out_counts"], a["caps"], a["lens"],
                                  a["dropped"])

    def untouched(self):
        return list(self.lens) == [LEN_SENTINEL] * 2 and list(self.dropped) == [LEN_SENTINEL] * 2


# ---- the ABI, without a device -----------------------------------------------------------------------------------------


def test_symbol_is_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    assert hasattr(lib, NAME)
    assert hasattr(_abi.load_library(_abi.DIAG_LIB_PATH), NAME)
    assert re.search(r"a3d_status\s+%s\s*\(" % NAME, header)
    assert NAME in _abi.SIGNATURES and len(_abi.SIGNATURES[NAME][1]) == 14
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    assert NAME in section
    assert lib.a3d_abi_version() == 1
    assert "#define A3D_ABI_VERSION 1" in header
    assert NAME in open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()


def test_the_rule_stands_in_the_header_and_the_kernel_file():
    def text(path, comment):  # the file as one line of words, each line's comment mark taken off
        lines = [re.sub(comment, "", ln) for ln in open(os.path.join(ROOT, *path)).read().splitlines()]
        return " ".join(" ".join(lines).split())

    header = text(("include", "align3d_hip.h"), r"^\s*/?\*")
    hip = text(("align3d_amd", "csrc", "voxel_mean.hip"), r"^\s*//")
    for phrase in ("s = 32768.0f / v and u = v / 32768.0f", "q_k = (int) rintf(d_k * s), ties to even",
                   "m_k = (float)((double)S_k / (double)N) and out_k = ctr_k + m_k * u",
                   "r_k = (int) rintf(n_k * 1048576.0f)", "L = sqrt((T_x*T_x + T_y*T_y) + T_z*T_z) in f64",
                   "out_c = (2 C + N) / (2 N)", "A cell's representative is its lowest input index"):
        assert phrase in header, phrase
        assert phrase in hip, phrase


def test_product_library_has_no_knob_for_the_feature():
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_VOXEL" not in blob and b"A3D_DOWNSAMPLE" not in blob and b"A3D_MEAN" not in blob
    assert NAME.encode() in blob


def test_empty_batch_is_ok_and_touches_nothing(lib):
    f = getattr(lib, NAME)
    assert f(None, None, None, 0, 0.0, None, None, None, None, None, None, None, None, None) == _abi.A3D_OK
    a = _Args()
    assert a.call(lib, n=0) == _abi.A3D_OK
    assert a.call(lib, n=0, voxel=float("nan")) == _abi.A3D_OK
    assert a.untouched()


def test_null_arguments_are_invalid_without_a_device(lib):
    a = _Args()
    for name in ("ctx", "views", "out_points", "caps", "lens"):
        assert a.call(lib, **{name: None}) == _abi.A3D_INVALID_PARAMETER, name
        assert a.untouched(), name


@pytest.mark.parametrize("voxel", [0.0, -0.0, -0.05, float("nan"), float("inf"), float("-inf")])
def test_bad_voxel_size_is_invalid_without_a_device(lib, voxel):
    a = _Args()
    assert a.call(lib, voxel=voxel) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_origin_is_invalid_without_a_device(lib, bad):
    for axis in range(3):
        a = _Args()
        a.origin[axis] = bad
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
        assert a.untouched()


def test_cloud_of_2_to_the_32_points_or_within_a_tile_of_it_is_invalid_without_a_device(lib):
    for big in (1 << 32, (1 << 32) + 5, 1 << 40, (1 << 32) - 1, (1 << 32) - 1000):
        a = _Args()
        a.views[1].len = big
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, big
        assert a.untouched()


def test_null_points_of_a_non_empty_cloud_are_invalid_without_a_device(lib):
    a = _Args()
    a.views[0].points = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    a = _Args()
    a.out_points[1] = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()


def test_an_output_for_a_field_the_cloud_lacks_is_missing_field(lib):
    a = _Args()
    a.out_normals[1] = 0xA0000  # cloud 1 has no normals
    assert a.call(lib) == _abi.A3D_MISSING_FIELD
    assert a.untouched()
    a = _Args()
    a.out_colors[1] = 0xA0000  # cloud 1 has no colours
    assert a.call(lib) == _abi.A3D_MISSING_FIELD
    a = _Args()
    assert a.call(lib, colors=None) == _abi.A3D_MISSING_FIELD  # a colour output and no colour inputs at all
    assert a.untouched()


def test_every_overlap_is_invalid_without_a_device(lib):
    """There is no in-place form: an output may overlap no input and no other output (4 points = 48 bytes of points or
    normals, 16 of index or counts, 12 of colours)."""
    cases = [
        ("out_points", 0, 0x10000),       # exactly in place
        ("out_points", 0, 0x10000 + 12),  # shifted by a point
        ("out_points", 0, 0x10000 - 12),  # its end runs into the input
        ("out_points", 0, 0x30000),       # on the other cloud's points
        ("out_points", 1, 0x20000),       # on cloud 0's normals, which are read
        ("out_points", 1, 0xB0000 + 8),   # on cloud 0's colours, which are read
        ("out_points", 1, 0x40000 + 24),  # two outputs on one buffer
        ("out_normals", 0, 0x20000),
        ("out_normals", 0, 0x40000),      # normals on the points output
        ("out_index", 0, 0x10000 + 44),   # the index array's first word on the input's last
        ("out_index", 1, 0x70000 + 12),   # two index outputs, one word shared
        ("out_counts", 0, 0x10000 + 44),  # the counts' first word on the input's last
        ("out_counts", 1, 0xD0000 + 12),  # two count outputs, one word shared
        ("out_counts", 0, 0x70000),       # counts on the index output
        ("out_counts", 1, 0x50000 + 44),  # counts on the other cloud's points output
        ("out_counts", 0, 0xC0000 + 8),   # counts on the colour output's last row
        ("out_colors", 0, 0xB0000),       # colours in place
        ("out_colors", 0, 0xB0000 + 11),  # the output's first byte on the input's last
        ("out_colors", 0, 0xB0000 - 11),  # the output's last byte on the input's first
        ("out_colors", 0, 0x40000 + 47),  # one byte shared with the points output
        ("out_colors", 0, 0xD0000 + 15),  # one byte shared with the counts output
    ]
    for field, i, address in cases:
        a = _Args()
        getattr(a, field)[i] = address
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
        assert a.untouched()


def test_python_mode_and_return_counts_errors():
    assert DevicePointCloud.voxel_downsample_many([], 0.05, mode="mean") == []
    assert DevicePointCloud.voxel_downsample_many([], 0.05, mode="nearest") == []
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample_many([], 0.05, mode="median")
    with pytest.raises(InvalidParameter):
        DevicePointCloud._voxel_downsample([], 0.05, None, False, "nearest", True)
    with pytest.raises(TypeError):
        DevicePointCloud.voxel_downsample_many([PointCloud([[1.0, 2.0, 3.0]])], 0.05, mode="mean")
    # the instance method checks its arguments before it looks at the cloud
    stub = DevicePointCloud.__new__(DevicePointCloud)
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample(stub, 0.05, mode="centroid")
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample(stub, 0.05, return_counts=True)
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample(stub, 0.05, mode="nearest", return_counts=True)


# ---- the restatement ---------------------------------------------------------------------------------------------------


def _rows(p, n, c, k):
    """The output rows as one sorted [m, 10] uint32 array: a multiset that can be compared."""
    cols = [_bits(p)]
    if n is not None:
        cols.append(_bits(n))
    if c is not None:
        cols.append(c.astype(np.uint32))
    cols.append(k.astype(np.uint32)[:, None])
    r = np.concatenate(cols, axis=1)
    return r[np.lexsort(r.T[::-1])]


def _check_properties(points, normals, colors, voxel, origin, seed=1):
    out_p, out_n, out_c, index, counts, dropped = M.voxel_mean(points, normals, colors, voxel, origin)
    kept, key, _ = V.voxel_keys(points, voxel, origin)
    # len, dropped and the set of cells are the nearest-point downsample's
    near_index, near_dropped = V.voxel_downsample(points, voxel, origin)
    assert len(index) == len(near_index) and dropped == near_dropped == int((~kept).sum())
    assert np.array_equal(np.sort(key[index]), np.sort(key[near_index]))
    # representatives: the lowest index of each cell, strictly increasing; the counts add up
    assert (np.diff(index.astype(np.int64)) > 0).all() and index.dtype == np.uint32 and counts.dtype == np.uint32
    assert int(counts.astype(np.int64).sum()) == int(kept.sum())
    first_of = {}
    for i in np.flatnonzero(kept):
        first_of.setdefault(int(key[i]), int(i))
    assert sorted(first_of.values()) == index.tolist()
    # a cell of one row is that row, bit for bit
    single = counts == 1
    assert np.array_equal(_bits(out_p[single]), _bits(points[index[single]]))
    if normals is not None:
        assert np.array_equal(_bits(out_n[single]), _bits(normals[index[single]]))
    if colors is not None:
        assert np.array_equal(out_c[single], colors[index[single]])
    # within the bound of the exact mean
    exact = M.exact_mean(points, voxel, origin)
    bound = M.error_bound(points, voxel, origin)
    err = np.abs(out_p.astype(np.float64) - exact).max() if len(index) else 0.0
    print(f"v={voxel} origin={origin}: {len(index)} cells, largest |mean - exact| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    # permutation: the same multiset of rows
    perm = np.random.default_rng(seed).permutation(len(points))
    again = M.voxel_mean(points[perm], None if normals is None else normals[perm], None if colors is None else colors[perm],
                         voxel, origin)
    assert np.array_equal(_rows(out_p, out_n, out_c, counts), _rows(again[0], again[1], again[2], again[4]))
    assert np.array_equal(np.sort(key[perm][again[3]]), np.sort(key[index]))
    return out_p, out_n, out_c, index, counts


_fixture = {}


def _fixture_cloud():
    if not _fixture:
        from gpu_util import oracle_frame, to_range_image

        cloud = PointCloud.from_range_image(to_range_image(oracle_frame("sample1", 0)))
        assert cloud.len() > 100000
        rng = np.random.default_rng(5)
        _fixture["c"] = (np.ascontiguousarray(cloud.points, np.float32), np.ascontiguousarray(cloud.normals, np.float32),
                         rng.integers(0, 256, size=(cloud.len(), 3), dtype=np.uint8))
    return _fixture["c"]


@pytest.mark.parametrize("voxel,origin", [(0.02, None), (0.05, ORIGINS[1]), (0.005, None), (1e3, ORIGINS[1])])
def test_restatement_properties_on_a_fixture_cloud(voxel, origin):
    points, normals, colors = _fixture_cloud()
    out_p, out_n, out_c, index, counts = _check_properties(points, normals, colors, voxel, origin)
    if voxel == 1e3:
        assert len(index) <= 8 and counts.max() > len(points) // 8 and index[0] == 0  # a camera looks across the axes: a few cells
    else:
        assert (counts > 1).any() and len(index) < len(points)
    # mean normals of a surface are unit vectors (or zero where they cancel)
    norm = np.linalg.norm(out_n.astype(np.float64), axis=1)
    multi = counts > 1
    assert ((norm[multi] == 0) | (np.abs(norm[multi] - 1) <= 2.0**-22)).all() and (norm[multi] > 0).sum() > multi.sum() // 2


def test_all_singletons_come_back_bit_for_bit_in_input_order():
    rng = np.random.default_rng(8)
    points = rng.uniform(0.25, 3.25, size=(2047, 3)).astype(np.float32)
    normals = rng.normal(size=points.shape).astype(np.float32)
    colors = rng.integers(0, 256, size=points.shape, dtype=np.uint8)
    for origin in ORIGINS:
        out_p, out_n, out_c, index, counts, dropped = M.voxel_mean(points, normals, colors, 1e-5, origin)
        assert dropped == 0 and np.array_equal(index, np.arange(2047, dtype=np.uint32)) and (counts == 1).all()
        assert np.array_equal(_bits(out_p), _bits(points)) and np.array_equal(_bits(out_n), _bits(normals))
        assert np.array_equal(out_c, colors)


def test_drop_rule_and_hostile_normals():
    v = 0.5
    points = np.float32([[0.1, 0.1, 0.1], [np.nan, 0.0, 1.0], [0.2, 0.3, 0.4], [np.inf, 0.5, -1.0], [0.3, 0.2, 0.1],
                         [1e9, 0.0, 0.0], [0.4, 0.4, 0.4], [0.6, 0.1, 0.1], [0.15, 0.25, 0.35]])
    normals = np.float32([[0, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, 1, 0], [0, np.inf, 0], [1, 0, 0], [3.0, 0, 0], [0, 1, 0],
                          [0, 0, -2.0]])
    colors = np.arange(27, dtype=np.uint8).reshape(9, 3)
    out_p, out_n, out_c, index, counts, dropped = M.voxel_mean(points, normals, colors, v)
    assert dropped == 3 and index.tolist() == [0, 7] and counts.tolist() == [5, 1]
    # of the five rows of cell 0 only rows 0 and 8 have a normal that counts (NaN, inf and 3.0 do not; |-2| <= 2 does):
    # T = 2^20 * (0, 0, 1 - 2), so the mean normal is (0, 0, -1) exactly
    assert np.array_equal(out_n[0], np.float32([0, 0, -1])) and not np.signbit(out_n[0][:2]).any()
    assert np.array_equal(_bits(out_n[1]), _bits(normals[7])) and np.array_equal(out_c[1], colors[7])
    assert np.array_equal(_bits(out_p[1]), _bits(points[7]))
    rows = [0, 2, 4, 6, 8]
    assert np.abs(out_p[0].astype(np.float64) - points[rows].astype(np.float64).mean(axis=0)).max() <= M.error_bound(points[rows], v)
    # colours: (2 C + N) / (2 N)
    C_sum = colors[rows].astype(np.int64).sum(axis=0)
    assert out_c[0].tolist() == ((2 * C_sum + 5) // 10).tolist()
    # only hostile normals in a cell of two: zero
    p2 = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]])
    _, n2, _, _, k2, _ = M.voxel_mean(p2, np.float32([[np.nan, 0, 0], [0, 2.5, 0]]), None, v)
    assert k2.tolist() == [2] and (_bits(n2) == 0).all()


def test_cancelling_normals_give_zero():
    p = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [0.35, 0.3, 0.3]])
    n = np.float32([[0.6, 0, 0.8], [-0.6, 0, -0.8], [0.25, -0.5, 0.125], [-0.25, 0.5, -0.125]])
    _, out_n, _, _, counts, _ = M.voxel_mean(p, n, None, 0.5)
    assert counts.tolist() == [4] and (_bits(out_n) == 0).all()  # +0.0, not -0.0


def test_colour_rounding_at_exact_halves():
    p = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]])
    c = np.uint8([[0, 254, 10], [1, 255, 13]])  # means 0.5, 254.5, 11.5: half up
    _, _, out_c, _, _, _ = M.voxel_mean(p, None, c, 0.5)
    assert out_c.tolist() == [[1, 255, 12]]
    p4 = np.float32([[0.1, 0.1, 0.1]] * 4)
    c4 = np.uint8([[0, 0, 255], [0, 1, 255], [1, 1, 255], [1, 0, 255]])  # 0.5 -> 1; 0.5 -> 1; 255 stays
    assert M.voxel_mean(p4, None, c4, 0.5)[2].tolist() == [[1, 1, 255]]
    c3 = np.uint8([[0, 0, 0], [0, 0, 1], [1, 0, 1]])  # thirds never tie: 1/3 -> 0, 0, 2/3 -> 1
    assert M.voxel_mean(p4[:3], None, c3, 0.5)[2].tolist() == [[0, 0, 1]]


def test_exact_lattice_offsets_give_the_exact_mean():
    v = np.float32(0.25)  # a power of two: centres and offsets are exact, so the mean of lattice offsets is exact
    cells = np.float32([[3, -2, 0], [-7, 5, 1]])
    centre = (cells + np.float32(0.5)) * v
    off = (np.int32([[100, -200, 300], [-100, 200, -300], [16, 32, 64], [0, 0, 4]]) / np.float32(32768.0) * v).astype(np.float32)
    points = np.concatenate([centre[0] + off, centre[1] + off[:2]]).astype(np.float32)
    out_p, _, _, index, counts, _ = M.voxel_mean(points, None, None, float(v))
    assert counts.tolist() == [4, 2] and index.tolist() == [0, 4]
    assert np.array_equal(out_p[1], centre[1])  # the two offsets cancel
    assert np.array_equal(out_p[0], (centre[0].astype(np.float64) + off.astype(np.float64).mean(axis=0)).astype(np.float32))


def test_accumulator_edge_passes_2_to_the_32():
    """270 213 points at ctr +- 0.4999 v of one cell: |S_k| = 270213 * 16381 > 2^32, and the mean is that corner."""
    v = np.float32(0.25)
    centre = (np.float32([2, -3, 4]) + np.float32(0.5)) * v
    for sign in (1.0, -1.0):
        p = np.tile(centre + np.float32(sign * 0.4999) * v, (270213, 1)).astype(np.float32)
        out_p, _, _, index, counts, dropped = M.voxel_mean(p, None, None, float(v))
        q = np.rint((p[0] - centre) * (np.float32(32768.0) / v))
        assert (np.abs(q) == 16381).all() and 270213 * 16381 > 2**32
        assert counts.tolist() == [270213] and index.tolist() == [0] and dropped == 0
        assert np.abs(out_p[0].astype(np.float64) - p[0]).max() <= M.error_bound(p, float(v))
