"""The C ABI of the voxel-grid downsample of resident clouds (a3d_point_clouds_voxel_downsample_device) without a GPU:
the exported symbol, the header, the ctypes mirror, every argument check that is decided on the host before any HIP
call (with made-up device addresses: nothing is dereferenced), and the properties of the numpy restatement
(voxel_restatement.py) that the GPU tests take as the expected value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voxel_restatement as V
from align3d_amd import DevicePointCloud, PointCloud, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "a3d_point_clouds_voxel_downsample_device"
LEN_SENTINEL = 0x7777


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
        self.out_points = (C.c_void_p * 2)(0x40000, 0x50000)
        self.out_normals = (C.c_void_p * 2)(0x60000, None)
        self.out_index = (C.c_void_p * 2)(0x70000, 0x80000)
        self.caps = (C.c_uint64 * 2)(4, 4)
        self.lens = (C.c_uint64 * 2)(LEN_SENTINEL, LEN_SENTINEL)
        self.dropped = (C.c_uint64 * 2)(LEN_SENTINEL, LEN_SENTINEL)
        self.voxel = 0.05
        self.origin = (C.c_float * 3)(0.0, 0.0, 0.0)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, n=2, voxel=self.voxel, origin=self.origin, out_points=self.out_points,
                 out_normals=self.out_normals, out_index=self.out_index, caps=self.caps, lens=self.lens,
                 dropped=self.dropped)
        a.update(override)
        return getattr(lib, NAME)(a["ctx"], a["views"], a["n"], a["voxel"], a["origin"], a["out_points"], a["out_normals"],
                                  a["out_index"], a["caps"], a["lens"], a["dropped"])

    def untouched(self):
        return (list(self.lens) == [LEN_SENTINEL] * 2 and list(self.dropped) == [LEN_SENTINEL] * 2
                and list(self.out_points) == [0x40000, 0x50000] and list(self.out_index) == [0x70000, 0x80000])


def test_symbol_is_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    assert hasattr(lib, NAME)
    assert hasattr(_abi.load_library(_abi.DIAG_LIB_PATH), NAME)
    assert re.search(r"a3d_status\s+%s\s*\(" % NAME, header)
    assert NAME in _abi.SIGNATURES and len(_abi.SIGNATURES[NAME][1]) == 11
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    assert NAME in section
    assert lib.a3d_abi_version() == 1
    assert "#define A3D_ABI_VERSION 1" in header
    for method in ("voxel_downsample", "voxel_downsample_many"):
        assert callable(getattr(DevicePointCloud, method))


def test_product_library_has_no_knob_for_the_feature():
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_VOXEL" not in blob and b"A3D_DOWNSAMPLE" not in blob


def test_empty_batch_is_ok_and_touches_nothing(lib):
    f = getattr(lib, NAME)
    assert f(None, None, 0, 0.0, None, None, None, None, None, None, None) == _abi.A3D_OK
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


def test_cloud_of_2_to_the_32_points_is_invalid_without_a_device(lib):
    for big in (1 << 32, (1 << 32) + 5, 1 << 40):
        a = _Args()
        a.views[1].len = big
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
        assert a.untouched()


def test_null_points_of_a_non_empty_cloud_are_invalid_without_a_device(lib):
    a = _Args()
    a.views[0].points = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    a = _Args()
    a.out_points[1] = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER
    assert list(a.lens) == [LEN_SENTINEL] * 2 and list(a.dropped) == [LEN_SENTINEL] * 2


def test_normals_output_for_a_cloud_without_normals_is_missing_field(lib):
    a = _Args()
    a.out_normals[1] = 0xA0000
    assert a.call(lib) == _abi.A3D_MISSING_FIELD
    assert list(a.lens) == [LEN_SENTINEL] * 2 and list(a.dropped) == [LEN_SENTINEL] * 2


def test_every_overlap_is_invalid_without_a_device(lib):
    """There is no in-place form: an output may overlap no input and no other output (4 points = 48 bytes, 16 of index)."""
    cases = [
        ("out_points", 0, 0x10000),       # exactly in place
        ("out_points", 0, 0x10000 + 12),  # shifted by a point
        ("out_points", 0, 0x10000 - 12),  # its end runs into the input
        ("out_points", 0, 0x30000),       # on the other cloud's points
        ("out_points", 1, 0x20000),       # on cloud 0's normals, which are read
        ("out_points", 1, 0x40000),       # two outputs on one buffer
        ("out_points", 1, 0x40000 + 24),
        ("out_normals", 0, 0x20000),
        ("out_normals", 0, 0x40000),      # normals on the points output
        ("out_index", 0, 0x10000 + 44),   # the index array's first word on the input's last
        ("out_index", 1, 0x70000 + 12),   # two index outputs, one word shared
        ("out_index", 1, 0x50000),
    ]
    for field, i, address in cases:
        a = _Args()
        getattr(a, field)[i] = address
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
        assert list(a.lens) == [LEN_SENTINEL] * 2 and list(a.dropped) == [LEN_SENTINEL] * 2


def test_python_wrappers_refuse_host_clouds_and_an_empty_list_is_empty():
    assert DevicePointCloud.voxel_downsample_many([], 0.05) == []
    with pytest.raises(TypeError):
        DevicePointCloud.voxel_downsample_many([PointCloud([[1.0, 2.0, 3.0]])], 0.05)


def _fixture_cloud():
    from gpu_util import oracle_frame, to_range_image

    cloud = PointCloud.from_range_image(to_range_image(oracle_frame("sample1", 0)))
    assert cloud.len() > 100000
    return cloud


@pytest.mark.parametrize("voxel,origin", [(0.02, None), (0.05, (0.013, -0.4, 7.5)), (0.005, None)])
def test_restatement_properties_on_a_fixture_cloud(voxel, origin):
    cloud = _fixture_cloud()
    points, normals = cloud.points, cloud.normals
    kept, key, _ = V.voxel_keys(points, voxel, origin)
    out_p, out_n, index, dropped = V.voxel_downsample_cloud(points, normals, voxel, origin)
    assert dropped == int((~kept).sum()) == 0  # a depth camera's points are finite and near
    # one output per occupied key, and it lies in that key's cell
    assert len(index) == len(np.unique(key[kept])) < len(points)
    assert np.array_equal(np.sort(key[index]), np.unique(key[kept]))
    # a subsequence of the input, rows bit for bit
    assert (np.diff(index.astype(np.int64)) > 0).all()
    assert np.array_equal(out_p.view(np.uint32), points[index].view(np.uint32))
    assert np.array_equal(out_n.view(np.uint32), normals[index].view(np.uint32))
    # the winner is nearest to the centre, the lowest index among equals
    _, _, dist = V.voxel_keys(points, voxel, origin)
    best = {}
    for i in np.flatnonzero(kept)[:20000]:
        k = int(key[i])
        if k not in best or dist[i] < dist[best[k]]:
            best[k] = i
    first = {int(key[i]): int(i) for i in index}
    # (keys whose every point lies in the first 20000: the others may have a later winner)
    counts = dict(zip(*np.unique(key[kept], return_counts=True)))
    seen = dict(zip(*np.unique(key[np.flatnonzero(kept)[:20000]], return_counts=True)))
    checked = 0
    for k, i in best.items():
        if counts[k] == seen[k]:
            assert first[k] == i
            checked += 1
    assert checked > 100
    # a second application with the same grid is the identity
    again_p, again_n, again_index, again_dropped = V.voxel_downsample_cloud(out_p, out_n, voxel, origin)
    assert again_dropped == 0 and np.array_equal(again_index, np.arange(len(out_p), dtype=np.uint32))
    assert np.array_equal(again_p.view(np.uint32), out_p.view(np.uint32))


def test_restatement_drop_rule_and_ties():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pts = np.asarray([
        [0.25, 0.25, 0.25],   # 0: cell (0,0,0) of v = 1, off centre
        [0.75, 0.75, 0.75],   # 1: the same cell, mirrored about the centre: equal dist, the lower index wins
        [nan, 0.0, 0.0],      # 2: dropped
        [0.0, inf, 0.0],      # 3: dropped
        [0.0, 0.0, -inf],     # 4: dropped
        [1048576.0, 0.0, 0.0],   # 5: cell 2^20: dropped
        [1048575.5, 0.0, 0.0],   # 6: cell 2^20 - 1: kept
        [-1048576.0, 0.0, 0.0],  # 7: cell -2^20: kept
        [-1048576.5, 0.0, 0.0],  # 8: cell -2^20 - 1: dropped
        [0.5, 0.5, 0.5],      # 9: the centre of cell (0,0,0): wins over 0 and 1
        [-0.0, -0.0, -0.0],   # 10: cell (0,0,0) again (floor(-0.0) = -0.0 = 0)
        [1.0, 0.0, 0.0],      # 11: on a cell face: belongs to the upper cell (1,0,0)
        [-1e-30, 0.0, 0.0],   # 12: just below a face: cell (-1,0,0)
    ], np.float32)
    index, dropped = V.voxel_downsample(pts, 1.0)
    assert dropped == 5
    assert index.tolist() == [6, 7, 9, 11, 12]
    index, _ = V.voxel_downsample(pts[:2], 1.0)
    assert index.tolist() == [0]
    index, _ = V.voxel_downsample(pts[[1, 0]], 1.0)
    assert index.tolist() == [0]
