"""The C ABI of colours on resident clouds and in the voxel map without a GPU: the exported symbols, the header, the
ctypes mirror, and every refusal of the new entries that is decided on the host before any HIP call (made-up device
addresses and a made-up context: nothing is dereferenced), which must leave the result arrays untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from align3d_amd import DevicePointCloud, DeviceVoxelMap, PointCloud, _abi
from align3d_amd.range_image import DeviceRangeImage
from colors_util import row_colors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_NAMES = {"a3d_range_image_has_colors": 2, "a3d_range_image_to_point_clouds_rgb": 7}
CLOUD_NAMES = {"a3d_point_clouds_merge_rgb_device": 10, "a3d_point_clouds_voxel_downsample_rgb_device": 13,
               "a3d_voxel_map_new_rgb": 7, "a3d_voxel_map_insert_rgb": 7, "a3d_voxel_map_extract_rgb": 7}
SENTINEL = 0x7777
FAKE_CTX = C.c_void_p(0x900000)
INVALID, MISSING, OK = _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD, _abi.A3D_OK


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_symbols_are_exported_declared_in_their_sections_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    images = header[header.index("---- range images resident on the device"):header.index("---- ImageIcp")]
    clouds = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    for names, section in ((IMAGE_NAMES, images), (CLOUD_NAMES, clouds)):
        for name, arity in names.items():
            assert hasattr(lib, name) and hasattr(diag, name), name
            assert re.search(r"a3d_status\s+%s\s*\(" % name, section), name
            assert len(re.findall(r"\b%s\s*\(" % name, header)) == 1, name
            assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == arity, name
    assert lib.a3d_abi_version() == 1 and "#define A3D_ABI_VERSION 1" in header
    assert C.sizeof(_abi.PointCloudViewC) == 24  # colours travel beside the views, not in them
    text = " ".join(clouds.split())
    assert "16 + 12 (+ 12 with normals) (+ 4 with colours) bytes per slot" in text
    assert "Colours and multi-GPU maps are NOT built" not in text
    for cls, methods in ((DevicePointCloud, ("has_colors", "download_colors", "_colors_array")),
                         (DeviceRangeImage, ("has_colors",))):
        for method in methods:
            assert callable(getattr(cls, method)), method


def test_product_library_gains_no_environment_knob():
    blob = open(_abi.LIB_PATH, "rb").read()
    for needle in (b"A3D_COLOR", b"A3D_COLOUR", b"A3D_RGB", b"A3D_VOXEL", b"A3D_CLOUD", b"A3D_POINT"):
        assert needle not in blob, needle


def test_host_point_cloud_carries_colours_through_the_mask():
    from align3d_amd import CameraIntrinsics, RangeImage

    rng = np.random.default_rng(1)
    h, w = 5, 7
    pts = rng.normal(size=(h, w, 3)).astype(np.float32)
    mask = rng.choice(np.asarray([0, 1, 2, 255], np.uint8), size=(h, w))
    rgb = row_colors(3, h * w).reshape(h, w, 3)
    cam = CameraIntrinsics(500.0, 500.0, w / 2, h / 2, w, h)
    cloud = PointCloud.from_range_image(RangeImage(pts, mask, cam, colors=rgb))
    assert cloud.colors.dtype == np.uint8 and np.array_equal(cloud.colors, rgb.reshape(-1, 3)[mask.reshape(-1) != 0])
    assert PointCloud.from_range_image(RangeImage(pts, mask, cam)).colors is None
    assert PointCloud(pts.reshape(-1, 3)).colors is None
    with pytest.raises(_abi.InvalidParameter):
        PointCloud(pts.reshape(-1, 3), colors=rgb.reshape(-1, 3)[:-1])


def test_image_entries_refuse_null_arguments_without_a_device(lib):
    out = C.c_int32(SENTINEL)
    assert lib.a3d_range_image_has_colors(None, C.byref(out)) == INVALID and out.value == SENTINEL
    assert lib.a3d_range_image_has_colors(C.c_void_p(0x1000), None) == INVALID
    f = lib.a3d_range_image_to_point_clouds_rgb
    assert f(None, 0, None, None, None, None, None) == OK
    images = (C.c_void_p * 1)(None)
    points, colors = (C.c_void_p * 1)(0x10000), (C.c_void_p * 1)(0x20000)
    caps, lens = (C.c_uint64 * 1)(4), (C.c_uint64 * 1)(SENTINEL)
    for args in ((None, 1, points, None, colors, caps, lens), (images, 1, None, None, colors, caps, lens),
                 (images, 1, points, None, colors, None, lens), (images, 1, points, None, colors, caps, None),
                 (images, 1, points, None, colors, caps, lens)):  # the last: a NULL image in the table
        assert f(*args) == INVALID
        assert lens[0] == SENTINEL


class _Merge:
    """Two clouds of 4 points with colours at made-up, disjoint device addresses."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, 0x40000, 4
        self.colors = (C.c_void_p * 2)(0x50000, 0x60000)
        self.out_len = C.c_uint64(SENTINEL)
        self.a = dict(ctx=FAKE_CTX, views=self.views, colors=self.colors, poses=None, n=2, out_points=0x70000,
                      out_normals=0x80000, out_colors=0x90000, capacity=8, out_len=C.byref(self.out_len))

    def call(self, lib, **override):
        a = dict(self.a)
        a.update(override)
        return lib.a3d_point_clouds_merge_rgb_device(a["ctx"], a["views"], a["colors"], a["poses"], a["n"], a["out_points"],
                                                     a["out_normals"], a["out_colors"], a["capacity"], a["out_len"])

    def untouched(self):
        return self.out_len.value == SENTINEL


def test_merge_rgb_refusals_without_a_device(lib):
    a = _Merge()
    for name in ("ctx", "views", "out_points", "out_len"):
        assert a.call(lib, **{name: None}) == INVALID and a.untouched(), name
    # a colour output needs colours on every non-empty cloud: a NULL array, a NULL entry
    assert a.call(lib, colors=None) == MISSING and a.untouched()
    a.colors[1] = None
    assert a.call(lib) == MISSING and a.untouched()
    a = _Merge()
    # the colour output (24 bytes) may overlap no input and no other output
    for address in (0x50000, 0x50000 + 11, 0x50000 - 23, 0x60000 + 6, 0x10000 + 47, 0x40000, 0x70000, 0x70000 + 95,
                    0x80000 - 23):
        assert a.call(lib, out_colors=address) == INVALID and a.untouched(), hex(address)
    # ... and the other outputs may not lie on a colour input (12 bytes each)
    assert a.call(lib, out_points=0x50000 + 11) == INVALID and a.untouched()
    assert a.call(lib, out_normals=0x60000 - 95) == INVALID and a.untouched()
    # n == 0: A3D_OK, length 0, nothing else looked at
    n = C.c_uint64(SENTINEL)
    assert lib.a3d_point_clouds_merge_rgb_device(None, None, None, None, 0, None, None, None, 0, C.byref(n)) == OK
    assert n.value == 0
    # capacity one short: refused on the host, the total reported
    assert a.call(lib, capacity=7) == INVALID and a.out_len.value == 8


class _Downsample:
    """Two clouds of 4 points, the second without normals and without colours, at made-up addresses."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.colors = (C.c_void_p * 2)(0x90000, None)
        self.out_points = (C.c_void_p * 2)(0x40000, 0x50000)
        self.out_normals = (C.c_void_p * 2)(0x60000, None)
        self.out_colors = (C.c_void_p * 2)(0xA0000, None)
        self.out_index = (C.c_void_p * 2)(0x70000, 0x80000)
        self.caps = (C.c_uint64 * 2)(4, 4)
        self.lens = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.dropped = (C.c_uint64 * 2)(SENTINEL, SENTINEL)

    def call(self, lib, **override):
        a = dict(ctx=FAKE_CTX, views=self.views, colors=self.colors, n=2, voxel=0.05, origin=None,
                 out_points=self.out_points, out_normals=self.out_normals, out_colors=self.out_colors,
                 out_index=self.out_index, caps=self.caps, lens=self.lens, dropped=self.dropped)
        a.update(override)
        return lib.a3d_point_clouds_voxel_downsample_rgb_device(
            a["ctx"], a["views"], a["colors"], a["n"], a["voxel"], a["origin"], a["out_points"], a["out_normals"],
            a["out_colors"], a["out_index"], a["caps"], a["lens"], a["dropped"])

    def untouched(self):
        return list(self.lens) == [SENTINEL] * 2 and list(self.dropped) == [SENTINEL] * 2


def test_downsample_rgb_refusals_without_a_device(lib):
    a = _Downsample()
    for name in ("ctx", "views", "out_points", "caps", "lens"):
        assert a.call(lib, **{name: None}) == INVALID and a.untouched(), name
    assert a.call(lib, n=0) == OK and a.untouched()
    f = lib.a3d_point_clouds_voxel_downsample_rgb_device
    assert f(None, None, None, 0, 0.0, None, None, None, None, None, None, None, None) == OK
    # a colour output for a cloud without colours: a NULL entry, a NULL array
    a.out_colors[1] = 0xB0000
    assert a.call(lib) == MISSING and a.untouched()
    assert a.call(lib, colors=None) == MISSING and a.untouched()
    # overlaps (4 rows: 12 bytes of colours, 48 of points, 16 of indices)
    cases = [
        ("out_colors", 0, 0x90000),       # exactly on its input
        ("out_colors", 0, 0x90000 + 11),  # the output's first byte on the input's last
        ("out_colors", 0, 0x90000 - 11),
        ("out_colors", 0, 0x10000 + 47),  # on the last byte of the points that are read
        ("out_colors", 0, 0x40000 + 47),  # on the last byte of a points output
        ("out_colors", 0, 0x50000),       # on the other cloud's points output
        ("out_colors", 0, 0x70000 - 11),  # its last byte on the first of an index output
        ("out_points", 1, 0x90000 - 47),  # a points output that ends on the colour input's first byte
        ("out_index", 1, 0xA0000 + 8),    # an index output on the colour output's last word
    ]
    for field, i, address in cases:
        a = _Downsample()
        getattr(a, field)[i] = address
        assert a.call(lib) == INVALID and a.untouched(), (field, i, hex(address))
    # two colour outputs that share a byte
    a = _Downsample()
    a.views[1].normals, a.colors[1] = 0x38000, 0x98000
    a.out_colors[1] = 0xA0000 + 11
    assert a.call(lib) == INVALID and a.untouched()


def _new_map(lib, colors, normals=1):
    h = C.c_void_p()
    assert lib.a3d_voxel_map_new_rgb(FAKE_CTX, 0.05, None, normals, colors, 0, C.byref(h)) == OK and h.value
    return h


def _stats(lib, h):
    s = _abi.VoxelMapStatsC()
    assert lib.a3d_voxel_map_get_stats(h, C.byref(s)) == OK
    return s.as_dict()


def test_voxel_map_rgb_refusals_without_a_device(lib):
    h = C.c_void_p()
    assert lib.a3d_voxel_map_new_rgb(None, 0.05, None, 1, 1, 0, C.byref(h)) == INVALID and not h.value
    assert lib.a3d_voxel_map_new_rgb(FAKE_CTX, 0.05, None, 1, 1, 0, None) == INVALID
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.a3d_voxel_map_new_rgb(FAKE_CTX, voxel, None, 1, 1, 0, C.byref(h)) == INVALID and not h.value
    assert lib.a3d_voxel_map_new_rgb(FAKE_CTX, 0.05, None, 1, 1, 1 << 32, C.byref(h)) == INVALID and not h.value
    empty = dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)
    views = (_abi.PointCloudViewC * 2)()
    views[0].points, views[0].normals, views[0].len = 0x10000, 0x20000, 4
    views[1].points, views[1].normals, views[1].len = 0x30000, 0x40000, 4
    coloured, plain = _new_map(lib, 1), _new_map(lib, 0)
    dropped, cells = (C.c_uint64 * 2)(SENTINEL, SENTINEL), C.c_uint64(SENTINEL)

    def quiet():
        return list(dropped) == [SENTINEL] * 2 and cells.value == SENTINEL and _stats(lib, coloured) == empty

    # a non-empty cloud without colours offered to a map with colours: a NULL array, a NULL entry, the old entry
    assert lib.a3d_voxel_map_insert_rgb(coloured, views, None, None, 2, dropped, C.byref(cells)) == MISSING and quiet()
    assert lib.a3d_voxel_map_insert_rgb(coloured, views, (C.c_void_p * 2)(0x50000, None), None, 2, dropped,
                                        C.byref(cells)) == MISSING and quiet()
    assert lib.a3d_voxel_map_insert(coloured, views, None, 2, dropped, C.byref(cells)) == MISSING and quiet()
    assert lib.a3d_voxel_map_insert_rgb(None, views, None, None, 2, dropped, C.byref(cells)) == INVALID and quiet()
    assert lib.a3d_voxel_map_insert_rgb(coloured, None, None, None, 2, dropped, C.byref(cells)) == INVALID and quiet()
    assert lib.a3d_voxel_map_insert_rgb(coloured, views, None, None, 0, dropped, C.byref(cells)) == OK and quiet()
    # empty clouds offer nothing and need no colours: A3D_OK without a device, the cell count reported
    views[0].len = views[1].len = 0
    assert lib.a3d_voxel_map_insert_rgb(coloured, views, None, None, 2, dropped, C.byref(cells)) == OK
    assert list(dropped) == [0, 0] and cells.value == 0 and _stats(lib, coloured) == empty
    # extract: colours asked of a map without them; NULL arguments; overlapping outputs (4 rows: 12 bytes of colours)
    n = C.c_uint64(SENTINEL)
    f = lib.a3d_voxel_map_extract_rgb
    assert f(plain, 0x50000, None, 0x60000, None, 4, C.byref(n)) == MISSING and n.value == SENTINEL
    assert f(plain, 0x50000, 0x70000, None, None, 4, C.byref(n)) == OK and n.value == 0  # (a map made with normals)
    n = C.c_uint64(SENTINEL)
    assert f(None, 0x50000, None, 0x60000, None, 4, C.byref(n)) == INVALID
    assert f(coloured, None, None, 0x60000, None, 4, C.byref(n)) == INVALID
    assert f(coloured, 0x50000, None, 0x60000, None, 4, None) == INVALID
    for points, normals, colors, index in ((0x50000, None, 0x50000 + 47, None), (0x50000, None, 0x50000 - 11, None),
                                           (0x50000, 0x60000, 0x60000 + 47, None), (0x50000, None, 0x70000, 0x70000 + 11),
                                           (0x50000, None, 0x70000 + 15, 0x70000)):
        assert f(coloured, points, normals, colors, index, 4, C.byref(n)) == INVALID, (points, normals, colors, index)
    assert n.value == SENTINEL
    # ... by the first 3 * capacity bytes, no further: byte 12 of the colour buffer is free
    assert f(coloured, 0x50000, None, 0x50000 - 12, None, 4, C.byref(n)) == OK and n.value == 0
    for h in (coloured, plain):
        lib.a3d_voxel_map_free(h)


def test_python_wrappers_without_a_device():
    assert DevicePointCloud.from_range_images([], colors=True) == []
    assert DevicePointCloud.d_colors is None
    sig = DeviceVoxelMap.__init__.__code__.co_varnames
    assert "colors" in sig
