"""a3d_voxel_map_retain without a GPU, as test_voxel_map_abi_cpu.py: the exported symbol, its header text and ctypes
mirror, every refusal that is decided on the host (a map allocates nothing before its first point, so a made-up context
does: nothing is dereferenced), the success on a map that holds no table yet, and the Python wrapper's argument checks."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from align3d_amd import DeviceVoxelMap, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7777
FAKE_CTX = 0x900000
EMPTY_STATS = dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


@pytest.fixture()
def handle(lib):
    h = C.c_void_p()
    assert lib.a3d_voxel_map_new(C.c_void_p(FAKE_CTX), 0.05, None, 1, 0, C.byref(h)) == _abi.A3D_OK
    yield h
    lib.a3d_voxel_map_free(h)


def _stats(lib, h):
    s = _abi.VoxelMapStatsC()
    assert lib.a3d_voxel_map_get_stats(h, C.byref(s)) == _abi.A3D_OK
    return s.as_dict()


def _f3(*v):
    return (C.c_float * 3)(*v)


class _Call:
    """Three marks, sentinel-filled results."""

    def __init__(self):
        self.marks = (C.c_uint64 * 3)(0, 5, 1 << 63)
        self.out = (C.c_uint64 * 3)(SENTINEL, SENTINEL, SENTINEL)
        self.removed = C.c_uint64(SENTINEL)

    def call(self, lib, h, lo=None, hi=None, min_seq=0, marks="own", n=3, out="own"):
        return lib.a3d_voxel_map_retain(h, lo, hi, min_seq, self.marks if marks == "own" else marks, n,
                                        self.out if out == "own" else out, C.byref(self.removed))

    def untouched(self):
        return list(self.out) == [SENTINEL] * 3 and self.removed.value == SENTINEL


def test_symbol_is_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    name = "a3d_voxel_map_retain"
    assert hasattr(lib, name) and hasattr(diag, name)
    decl = re.search(r"a3d_status\s+a3d_voxel_map_retain\s*\((.*?)\);", section, re.S)
    assert decl
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["a3d_voxel_map* map", "const float box_min[3]", "const float box_max[3]", "uint64_t min_seq",
                      "const uint64_t* marks", "uint64_t n_marks", "uint64_t* out_marks", "uint64_t* out_removed"]
    restype, argtypes = _abi.SIGNATURES[name]
    assert restype is _abi.SIGNATURES["a3d_voxel_map_clear"][0]
    assert argtypes == [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64, U64P, C.c_uint64, U64P, U64P]
    # the header states the rule, the contract, the slots rule, the marks and what a failure leaves
    text = " ".join(section.split())
    for needle in ("seq >= min_seq", "box_min[k] <= p[k] <= box_max[k]", "inserted as ONE cloud without a pose",
                   "cells = total = k and dropped_total = 0", "growths is unchanged",
                   "smallest power of two >= max(2 k, 2 * reserve_cells, 64)", "the next point offered gets seq k",
                   "the effect of a3d_voxel_map_clear", "survivors whose OLD seq is < marks[i]",
                   "a mark >= the old total gives k", "On ANY failure", "the map is unchanged",
                   "total / 8 bytes of bitmap and total / 16 of prefixes"):
        assert needle in text, needle
    assert lib.a3d_abi_version() == 1 and "#define A3D_ABI_VERSION 1" in header
    for method in ("retain", "compact"):
        assert callable(getattr(DeviceVoxelMap, method))


def test_refusals_are_decided_on_the_host_and_change_nothing(lib, handle):
    lo, hi = _f3(-1, -1, -1), _f3(1, 1, 1)
    a = _Call()
    assert lib.a3d_voxel_map_retain(None, lo, hi, 0, a.marks, 3, a.out, C.byref(a.removed)) == _abi.A3D_INVALID_PARAMETER
    assert a.untouched()
    # one box pointer NULL alone
    assert a.call(lib, handle, lo=lo) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert a.call(lib, handle, hi=hi) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    # a NaN bound, on either corner and any axis
    for axis in range(3):
        for which in (0, 1):
            corners = [_f3(-1, -1, -1), _f3(1, 1, 1)]
            corners[which][axis] = float("nan")
            assert a.call(lib, handle, lo=corners[0], hi=corners[1]) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    # marks or out_marks NULL with n_marks > 0
    assert a.call(lib, handle, marks=None) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert a.call(lib, handle, out=None) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert a.call(lib, handle, marks=None, out=None, n=1) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert _stats(lib, handle) == EMPTY_STATS


def test_a_map_without_a_table_retains_nothing_and_translates_every_mark_to_zero(lib, handle):
    for lo, hi in ((None, None), (_f3(-1, -1, -1), _f3(1, 1, 1)), (_f3(float("-inf"), 0, 0), _f3(float("inf"), 1, 1)),
                   (_f3(1, 1, 1), _f3(-1, -1, -1))):
        for min_seq in (0, 1, (1 << 64) - 1):
            a = _Call()
            assert a.call(lib, handle, lo=lo, hi=hi, min_seq=min_seq) == _abi.A3D_OK
            assert list(a.out) == [0, 0, 0] and a.removed.value == 0
            assert _stats(lib, handle) == EMPTY_STATS
    # no marks, no removed count
    assert lib.a3d_voxel_map_retain(handle, None, None, 0, None, 0, None, None) == _abi.A3D_OK
    assert _stats(lib, handle) == EMPTY_STATS


def test_python_wrapper_checks_its_arguments(lib):
    ctx = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX))
    m = DeviceVoxelMap(ctx, 0.05, normals=False)
    assert m.retain() == 0 and m.compact() == 0
    assert m.retain(box=((-1, -1, -1), (1, 1, 1)), min_seq=7) == 0
    removed, new = m.retain(marks=np.asarray([0, 3, 1 << 63], np.uint64))
    assert removed == 0 and new.dtype == np.uint64 and new.tolist() == [0, 0, 0]
    removed, new = m.retain(marks=[])
    assert removed == 0 and new.dtype == np.uint64 and new.shape == (0,)
    removed, new = m.retain(marks=[1, 2])
    assert removed == 0 and new.tolist() == [0, 0]
    for box in ((0, 0, 0), ((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1, 1)), ((0, 0, 0),), 3.0):
        with pytest.raises(_abi.InvalidParameter):
            m.retain(box=box)
    for marks in (np.zeros((2, 2), np.uint64), np.asarray([0.5, 2.0]), np.asarray([-1, 4]), 5):
        with pytest.raises(_abi.InvalidParameter):
            m.retain(marks=marks)
    for min_seq in (-1, 1 << 64):
        with pytest.raises(_abi.InvalidParameter):
            m.retain(min_seq=min_seq)
    with pytest.raises(_abi.A3dError) as e:  # the library's refusal, through the wrapper
        m.retain(box=((0, float("nan"), 0), (1, 1, 1)))
    assert e.value.status == _abi.A3D_INVALID_PARAMETER
    assert m.stats() == EMPTY_STATS
    m.free()
