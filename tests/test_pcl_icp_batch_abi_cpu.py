"""CPU checks of the batched point-cloud ICP entry points (a3d_pcl_icp_batch_*, include/align3d_hip.h): exported, mirrored
in SIGNATURES with the header's arity, malformed arguments are statuses that leave the outputs alone, an empty batch
needs no device, and IcpBatch takes resident clouds only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from align3d_amd import IcpBatch, IcpParams, PointCloud, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "a3d_pcl_icp_batch_new_device": 5,
    "a3d_pcl_icp_batch_align_device": 4,
    "a3d_pcl_icp_batch_results": 3,
    "a3d_pcl_icp_batch_last_device_ms": 2,
    "a3d_pcl_icp_batch_free": 1,
}


def test_symbols_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for path in (None, _abi.DIAG_LIB_PATH):
        lib = _abi.load_library(path)
        for name in NAMES:
            assert hasattr(lib, name), name
    for name, arity in NAMES.items():
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == arity, name
        m = re.search(r"a3d_status\s+%s\s*\(([^;]*?)\)\s*;" % name, body)
        assert m, f"{name} not declared in the header"
        assert len(m.group(1).split(",")) == arity, name


def test_null_arguments_leave_outputs_untouched():
    lib = _abi.load_library()
    prm = IcpParams.default().to_c()
    views = (_abi.PointCloudViewC * 1)()
    fake_ctx = C.create_string_buffer(64)  # never dereferenced: every call below fails its argument check first
    ctx = C.cast(fake_ctx, C.c_void_p)
    out = C.c_void_p(0x1234)
    assert lib.a3d_pcl_icp_batch_new_device(None, C.byref(prm), 1, views, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_pcl_icp_batch_new_device(ctx, None, 1, views, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_pcl_icp_batch_new_device(ctx, C.byref(prm), 1, None, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_pcl_icp_batch_new_device(ctx, C.byref(prm), 1, views, None) == _abi.A3D_INVALID_PARAMETER
    assert out.value == 0x1234
    assert b"null argument" in lib.a3d_last_error()
    # a target without points is refused before anything touches the device, and the message names the pair
    assert lib.a3d_pcl_icp_batch_new_device(ctx, C.byref(prm), 1, views, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert out.value == 0x1234 and b"pair 0" in lib.a3d_last_error()
    poses = (_abi.PoseC * 1)()
    poses[0].t[0] = 7.0
    status = np.full(1, 99, np.int32)
    sp = status.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.a3d_pcl_icp_batch_align_device(None, views, poses, sp) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_pcl_icp_batch_results(None, poses, sp) == _abi.A3D_INVALID_PARAMETER
    ms = C.c_float(-1.0)
    assert lib.a3d_pcl_icp_batch_last_device_ms(None, C.byref(ms)) == _abi.A3D_INVALID_PARAMETER
    assert poses[0].t[0] == 7.0 and status[0] == 99 and ms.value == -1.0
    assert lib.a3d_pcl_icp_batch_free(None) == _abi.A3D_OK


def test_empty_batch_is_ok_and_its_align_is_a_no_op():
    lib = _abi.load_library()
    prm = IcpParams.default().to_c()
    fake_ctx = C.create_string_buffer(64)  # an empty batch never touches its context
    h = C.c_void_p()
    assert lib.a3d_pcl_icp_batch_new_device(C.cast(fake_ctx, C.c_void_p), C.byref(prm), 0, None, C.byref(h)) == _abi.A3D_OK
    assert h.value
    poses = (_abi.PoseC * 1)()
    poses[0].t[0] = 7.0
    status = np.full(1, 99, np.int32)
    sp = status.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.a3d_pcl_icp_batch_align_device(h, None, poses, sp) == _abi.A3D_OK
    assert lib.a3d_pcl_icp_batch_align_device(h, None, None, None) == _abi.A3D_OK
    assert lib.a3d_pcl_icp_batch_results(h, poses, sp) == _abi.A3D_OK
    ms = C.c_float(-1.0)
    assert lib.a3d_pcl_icp_batch_last_device_ms(h, C.byref(ms)) == _abi.A3D_OK and ms.value == 0.0
    assert poses[0].t[0] == 7.0 and status[0] == 99
    assert lib.a3d_pcl_icp_batch_results(h, None, None) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_pcl_icp_batch_free(h) == _abi.A3D_OK


def test_icp_batch_refuses_host_clouds():
    cloud = PointCloud(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError):
        IcpBatch(None, IcpParams.default(), [cloud])  # refused before the context is looked at
