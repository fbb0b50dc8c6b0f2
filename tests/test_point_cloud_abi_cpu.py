"""The C ABI of the device range image -> point cloud conversion (a3d_range_image_to_point_cloud[s],
src/range_image/structure.rs:375-406) without a GPU: exported symbols, ctypes signatures and the argument checks that
run before any HIP call."""
import ctypes as C

import pytest

from align3d_amd import _abi

NAMES = ("a3d_range_image_to_point_cloud", "a3d_range_image_to_point_clouds", "a3d_range_image_has_normals")


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_symbols_are_exported_and_declared(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["a3d_range_image_to_point_cloud"][1]) == 5
    assert len(_abi.SIGNATURES["a3d_range_image_to_point_clouds"][1]) == 6
    assert len(_abi.SIGNATURES["a3d_range_image_has_normals"][1]) == 2
    assert lib.a3d_abi_version() == 1


def test_null_arguments_are_invalid_without_a_device(lib):
    n = C.c_uint64(7)
    fake = C.c_void_p(16)  # never dereferenced: the image check fails first
    assert lib.a3d_range_image_to_point_cloud(None, fake, None, 10, C.byref(n)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_range_image_to_point_cloud(None, None, None, 10, None) == _abi.A3D_INVALID_PARAMETER
    assert n.value == 7  # nothing written
    caps = (C.c_uint64 * 1)(10)
    lens = (C.c_uint64 * 1)(7)
    imgs = (C.c_void_p * 1)(None)
    outs = (C.c_void_p * 1)(16)
    st = lib.a3d_range_image_to_point_clouds(None, 1, outs, None, caps, lens)
    assert st == _abi.A3D_INVALID_PARAMETER
    st = lib.a3d_range_image_to_point_clouds(imgs, 1, outs, None, caps, lens)  # a NULL image inside the batch
    assert st == _abi.A3D_INVALID_PARAMETER
    assert lens[0] == 7
    out = C.c_int32(5)
    assert lib.a3d_range_image_has_normals(None, C.byref(out)) == _abi.A3D_INVALID_PARAMETER
    assert out.value == 5


def test_empty_batch_is_ok_and_touches_nothing(lib):
    assert lib.a3d_range_image_to_point_clouds(None, 0, None, None, None, None) == _abi.A3D_OK
    lens = (C.c_uint64 * 1)(7)
    assert lib.a3d_range_image_to_point_clouds((C.c_void_p * 1)(None), 0, (C.c_void_p * 1)(None), None,
                                               (C.c_uint64 * 1)(0), lens) == _abi.A3D_OK
    assert lens[0] == 7
