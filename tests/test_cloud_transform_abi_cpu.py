"""The C ABI of Transform * PointCloud on resident clouds (a3d_point_clouds_transform_device / _merge_device,
src/pointcloud.rs:40-52) without a GPU: exported symbols, the header, the ctypes mirror, and the argument checks that are
decided on the host before any HIP call."""
import ctypes as C
import os
import re

import pytest

from align3d_amd import PointCloud, Transform, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a3d_point_clouds_transform_device", "a3d_point_clouds_merge_device")
SENTINEL = 0x5A5A5A50


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _args():
    """One cloud of 4 points at made-up device addresses, a made-up context and sentinel-filled output tables: the checks
    under test fail before anything is dereferenced."""
    views = (_abi.PointCloudViewC * 1)()
    views[0].points, views[0].normals, views[0].len = 0x10000, 0x20000, 4
    fake_ctx = C.c_void_p(0x30000)
    outs = (C.c_void_p * 1)(SENTINEL)
    return views, fake_ctx, outs


def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert re.search(r"a3d_status\s+%s\s*\(" % name, header), name
        assert name in _abi.SIGNATURES, name
        assert hasattr(_abi.load_library(_abi.DIAG_LIB_PATH), name), name
    assert len(_abi.SIGNATURES["a3d_point_clouds_transform_device"][1]) == 6
    assert len(_abi.SIGNATURES["a3d_point_clouds_merge_device"][1]) == 8
    assert lib.a3d_abi_version() == 1
    assert "#define A3D_ABI_VERSION 1" in header


def test_product_library_has_no_knob_for_the_kernel_variants():
    assert b"A3D_CLOUD_TRANSFORM" not in open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_CLOUD_TRANSFORM_PPT" in open(_abi.DIAG_LIB_PATH, "rb").read()


def test_transform_null_arguments_are_invalid_without_a_device(lib):
    f = lib.a3d_point_clouds_transform_device
    views, fake_ctx, outs = _args()
    pose = (_abi.PoseC * 1)()
    assert f(None, views, pose, 1, outs, None) == _abi.A3D_INVALID_PARAMETER      # ctx
    assert f(fake_ctx, None, pose, 1, outs, None) == _abi.A3D_INVALID_PARAMETER   # d_clouds
    assert f(fake_ctx, views, pose, 1, None, None) == _abi.A3D_INVALID_PARAMETER  # the output table
    assert f(None, None, None, 1, None, None) == _abi.A3D_INVALID_PARAMETER
    assert outs[0] == SENTINEL


def test_merge_null_arguments_are_invalid_without_a_device(lib):
    f = lib.a3d_point_clouds_merge_device
    views, fake_ctx, _ = _args()
    out, n = C.c_void_p(0x40000), C.c_uint64(7)
    assert f(None, views, None, 1, out, None, 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER      # ctx
    assert f(fake_ctx, None, None, 1, out, None, 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER   # d_clouds
    assert f(fake_ctx, views, None, 1, None, None, 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER  # the output array
    assert n.value == 7  # untouched
    assert f(fake_ctx, views, None, 1, out, None, 4, None) == _abi.A3D_INVALID_PARAMETER         # out_len


def test_empty_batch_is_ok(lib):
    assert lib.a3d_point_clouds_transform_device(None, None, None, 0, None, None) == _abi.A3D_OK
    views, fake_ctx, outs = _args()
    assert lib.a3d_point_clouds_transform_device(fake_ctx, views, None, 0, outs, outs) == _abi.A3D_OK
    assert outs[0] == SENTINEL
    assert lib.a3d_point_clouds_merge_device(None, None, None, 0, None, None, 0, None) == _abi.A3D_OK
    n = C.c_uint64(7)
    assert lib.a3d_point_clouds_merge_device(fake_ctx, views, None, 0, None, None, 0, C.byref(n)) == _abi.A3D_OK
    assert n.value == 0  # the merge of no clouds has no points


def test_transform_times_transform_is_unchanged():
    assert isinstance(Transform() * Transform(), Transform)
    a, b = Transform((1, 2, 3), (0, 1, 0, 0)), Transform((0.5, 0, -1), (0, 0, 0, 1))
    c = a * b
    assert isinstance(c, Transform)
    assert c.t.tolist() == [0.5, 2.0, 4.0] and c.q.tolist() == [0.0, 1.0, 0.0, 0.0]


def test_host_cloud_on_the_right_stays_an_error():
    with pytest.raises(TypeError):
        Transform() * PointCloud([[1.0, 2.0, 3.0]])
