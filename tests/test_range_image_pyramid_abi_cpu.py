"""The C ABI of the device pyramid of resident range images (a3d_range_image_set_colors, a3d_range_image_compute_intensity,
a3d_range_image_pyramids; src/range_image/structure.rs:266-351) without a GPU: exported symbols, header and ctypes
declarations, and the argument checks that run before any HIP call."""
import ctypes as C
import os

import pytest

from align3d_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"a3d_range_image_set_colors": 2, "a3d_range_image_compute_intensity": 2, "a3d_range_image_pyramids": 6}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert f"a3d_status {name}(" in header, name
        assert name in _abi.SIGNATURES, name
        assert len(_abi.SIGNATURES[name][1]) == arity, name
    assert lib.a3d_abi_version() == 1


def test_null_arguments_are_invalid_without_a_device(lib):
    rgb = (C.c_uint8 * 3)()
    assert lib.a3d_range_image_set_colors(None, rgb) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_set_colors(None, None) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_compute_intensity(None, 1) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_compute_intensity((C.c_void_p * 2)(None, None), 2) == _abi.A3D_INVALID_PARAMETER
    out = (C.c_void_p * 4)(11, 12, 13, 14)
    assert lib.a3d_range_image_pyramids(None, 1, 3, 1.0, 1, out) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_pyramids((C.c_void_p * 1)(None), 1, 3, 1.0, 1, None) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_pyramids((C.c_void_p * 1)(None), 1, 3, 1.0, 1, out) == _abi.A3D_INVALID_PARAMETER
    # the scalar checks come before any image is looked at
    fake = (C.c_void_p * 1)(16)  # never dereferenced
    for levels, sigma in ((0, 1.0), (17, 1.0), (3, 3.5), (3, float("nan")), (3, float("inf"))):
        assert lib.a3d_range_image_pyramids(fake, 1, levels, sigma, 1, out) == _abi.A3D_INVALID_PARAMETER, (levels, sigma)
    assert list(out) == [11, 12, 13, 14]  # no handle written


def test_empty_batch_is_ok_and_touches_nothing(lib):
    assert lib.a3d_range_image_compute_intensity(None, 0) == _abi.A3D_OK
    assert lib.a3d_range_image_pyramids(None, 0, 3, 1.0, 1, None) == _abi.A3D_OK
    out = (C.c_void_p * 2)(21, 22)
    assert lib.a3d_range_image_pyramids((C.c_void_p * 1)(None), 0, 3, 1.0, 1, out) == _abi.A3D_OK
    assert list(out) == [21, 22]
