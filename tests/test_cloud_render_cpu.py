"""Rendering resident clouds and the voxel map into range images (a3d_point_cloud_render_device / a3d_voxel_map_render,
PinholeCamera::project_to_image, src/camera.rs:177-202) without a GPU: the numpy restatement against the reference's
known answers and its rounding rule, the exported symbols, the header, the ctypes mirror, and the argument checks that
are decided on the host before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_restatement as R
from align3d_amd import CameraIntrinsics, DevicePointCloud, DeviceVoxelMap, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a3d_point_cloud_render_device", "a3d_voxel_map_render")
SENTINEL = 0x5A5A5A50
F = np.float32
INVALID = _abi.A3D_INVALID_PARAMETER


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


# ---- the restatement ------------------------------------------------------------------------------------------------

def _one(point, fx=50.0, fy=50.0, cx=0.0, cy=0.0, w=100, h=100, radius=0.0):
    return R.render(np.asarray([point], F), None, None, None, fx, fy, cx, cy, w, h, radius)


def test_restatement_reproduces_the_reference_known_answers():
    """camera.rs:209-243 (test_project / test_project_to_image): fx = fy = 50, cx = cy = 0, 100 x 100, Transform::eye()."""
    eye = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    for pose in (None, eye):
        for point, (col, row) in (((1.0, 1.0, 1.0), (50, 50)), ((1.0, 1.5, 1.0), (50, 75))):
            p = R.camera_points(np.asarray([point], F), pose)
            u, v = R.project(p, 50.0, 50.0, 0.0, 0.0)
            assert (float(u[0]), float(v[0])) == (float(col), float(row))
            out = R.render(np.asarray([point], F), None, None, pose, 50.0, 50.0, 0.0, 0.0, 100, 100, 0.0)
            assert out["mask"].sum() == 1 and out["mask"][row, col] == 1 and out["index"][row, col] == 0
            assert out["points"][row, col].tolist() == list(point)


def test_round_is_half_away_from_zero():
    below_half = np.nextafter(F(0.5), F(0))
    assert float(below_half) == float(F(0.49999997))
    x = np.asarray([0.5, -0.5, 1.5, 2.5, -2.5, below_half, -below_half, 639.5, 0.0, -0.0, 8388607.5, 16777216.0, 3e9], F)
    want = np.asarray([1, -1, 2, 3, -3, 0, 0, 640, 0, 0, 8388608, 16777216, 3e9], F)
    assert R.round_half_away(x).tolist() == want.tolist()
    assert np.isnan(R.round_half_away(np.asarray([np.nan], F))[0])
    assert R.round_half_away(np.asarray([np.inf, -np.inf], F)).tolist() == [np.inf, -np.inf]
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.uniform(-700, 700, 100000), rng.integers(-1400, 1400, 100000) / 2.0]).astype(F)
    ref = np.asarray([np.sign(t) * np.floor(abs(t) + 0.5) for t in v.astype(np.float64)], np.float64)  # exact in f64
    assert np.array_equal(R.round_half_away(v).astype(np.float64), ref)
    assert not np.array_equal(np.round(v), R.round_half_away(v))  # half-to-even differs


def _column_of(u, w=640):
    """The column a row with projection u lands in (None: dropped): z = 1, fx = 1, cx = 0, so u = x exactly."""
    out = R.render(np.asarray([[u, 0.0, 1.0]], F), None, None, None, 1.0, 1.0, 0.0, 0.0, w, 1, 0.0)
    cols = np.nonzero(out["mask"][0])[0]
    return None if len(cols) == 0 else int(cols[0])


def test_borders_follow_the_rounded_coordinate():
    below_half = float(np.nextafter(F(0.5), F(0)))
    assert _column_of(-0.5) is None                 # round(-0.5) = -1
    assert _column_of(-below_half) == 0             # round = -0.0, and -0.0 >= 0
    assert _column_of(below_half) == 0              # (u + 0.5) as i32 would say 1: u + 0.5 rounds to 1.0 in f32
    assert float(F(below_half) + F(0.5)) == 1.0
    assert _column_of(639.5) is None                # w - 0.5 rounds to w
    assert _column_of(float(np.nextafter(F(639.5), F(0)))) == 639
    for bad in (np.nan, np.inf, -np.inf):
        assert _column_of(bad) is None


def test_rows_behind_the_camera_and_non_finite_depths_are_dropped():
    for z in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        assert _one((0.0, 0.0, z))["mask"].sum() == 0
    empty = _one((0.0, 0.0, -1.0))
    assert (empty["index"] == R.NO_ROW).all() and not empty["points"].any()


def test_nearest_row_wins_and_ties_go_to_the_lowest_index():
    pts = np.asarray([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [0, 0, 3.0]], F)
    out = R.render(pts, None, None, None, 10.0, 10.0, 2.0, 2.0, 5, 5, 0.0)
    assert out["index"][2, 2] == 1 and out["mask"].sum() == 1


def test_footprint_is_capped_clipped_and_dropped_with_its_centre():
    # radius * fx / z = 2.5 -> half-width 2; centre (0, 0): clipped to 3 x 3
    out = R.render(np.asarray([[0, 0, 1.0]], F), None, None, None, 10.0, 10.0, 0.0, 0.0, 9, 9, 0.25)
    assert out["mask"].sum() == 9 and out["mask"][:3, :3].all()
    # the cap: radius * fx / z = 100 -> 8, a 17 x 17 block in a 40 x 40 image
    out = R.render(np.asarray([[0, 0, 1.0]], F), None, None, None, 10.0, 10.0, 20.0, 20.0, 40, 40, 10.0)
    assert out["mask"].sum() == 17 * 17 and out["mask"][12:29, 12:29].all()
    # a centre one pixel outside: the whole row is dropped although its footprint would reach in
    out = R.render(np.asarray([[-0.1, 0, 1.0]], F), None, None, None, 10.0, 10.0, 0.0, 0.0, 9, 9, 0.25)
    assert out["mask"].sum() == 0


# ---- the ABI --------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert hasattr(diag, name), name
        assert re.search(r"a3d_status\s+%s\s*\(" % name, header), name
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["a3d_point_cloud_render_device"][1]) == 13
    assert len(_abi.SIGNATURES["a3d_voxel_map_render"][1]) == 11
    assert header.count("camera.rs:177-202") >= 2
    assert "#define A3D_RENDER_MAX_HALF_WIDTH 8" in header
    assert lib.a3d_abi_version() == 1
    assert "#define A3D_ABI_VERSION 1" in header
    assert callable(DevicePointCloud.render) and callable(DeviceVoxelMap.render)


def test_product_library_has_no_knob_for_the_splat_variants():
    assert b"A3D_CLOUD_RENDER" not in open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_CLOUD_RENDER_SPLAT" in open(_abi.DIAG_LIB_PATH, "rb").read()


def _cloud_call(lib, ctx=0x30000, view=True, out=True, fx=500.0, fy=500.0, cx=320.0, cy=240.0, w=640, h=480, radius=0.0):
    """The cloud entry on made-up addresses: every check under test fails before anything is dereferenced."""
    v = _abi.PointCloudViewC()
    v.points, v.normals, v.len = 0x10000, 0x20000, 4
    handle = C.c_void_p(SENTINEL)
    st = lib.a3d_point_cloud_render_device(C.c_void_p(ctx) if ctx else None, C.byref(v) if view else None, None, None, fx, fy,
                                           cx, cy, w, h, radius, None, C.byref(handle) if out else None)
    return st, handle.value


def _map_call(lib, m=0x30000, out=True, fx=500.0, fy=500.0, cx=320.0, cy=240.0, w=640, h=480, radius=0.0):
    handle = C.c_void_p(SENTINEL)
    st = lib.a3d_voxel_map_render(C.c_void_p(m) if m else None, None, fx, fy, cx, cy, w, h, radius, None,
                                  C.byref(handle) if out else None)
    return st, handle.value


BAD_CAMERAS = [
    dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 15), dict(w=1 << 31, h=1), dict(w=1 << 40, h=1 << 40),
    dict(radius=float("nan")), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=-1e-30),
    dict(fx=0.0), dict(fx=-500.0), dict(fy=0.0), dict(fy=-1.0), dict(fx=1e-60), dict(fx=float("nan")), dict(fy=float("inf")),
    dict(fx=1e300), dict(cx=float("nan")), dict(cy=float("-inf")),
]


def test_null_arguments_are_invalid_without_a_device(lib):
    assert _cloud_call(lib, ctx=0) == (INVALID, SENTINEL)
    assert _cloud_call(lib, view=False) == (INVALID, SENTINEL)
    assert _cloud_call(lib, out=False)[0] == INVALID
    assert _map_call(lib, m=0) == (INVALID, SENTINEL)
    assert _map_call(lib, out=False)[0] == INVALID


@pytest.mark.parametrize("bad", BAD_CAMERAS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_cameras_are_invalid_without_a_device(lib, bad):
    assert _cloud_call(lib, **bad) == (INVALID, SENTINEL)
    assert _map_call(lib, **bad) == (INVALID, SENTINEL)


def test_too_many_rows_and_null_points_are_invalid_without_a_device(lib):
    v = _abi.PointCloudViewC()
    handle = C.c_void_p(SENTINEL)
    args = (None, None, 500.0, 500.0, 320.0, 240.0, 640, 480, 0.0, None, C.byref(handle))
    v.points, v.normals, v.len = 0x10000, None, 0xFFFFFFFF
    assert lib.a3d_point_cloud_render_device(C.c_void_p(0x30000), C.byref(v), *args) == INVALID
    v.points, v.len = None, 4
    assert lib.a3d_point_cloud_render_device(C.c_void_p(0x30000), C.byref(v), *args) == INVALID
    # an index plane laid over the points it is made from
    v.points, v.len = 0x10000, 4
    over = args[:9] + (C.c_void_p(0x10008),) + args[10:]
    assert lib.a3d_point_cloud_render_device(C.c_void_p(0x30000), C.byref(v), *over) == INVALID
    assert handle.value == SENTINEL


def test_python_wrappers_refuse_wrong_types_before_any_call():
    cloud = DevicePointCloud.__new__(DevicePointCloud)
    cloud.ctx, cloud.n, cloud.d_points, cloud.d_normals, cloud.d_colors = None, 0, None, None, None
    with pytest.raises(TypeError):
        cloud.render((500.0, 500.0, 320.0, 240.0, 640, 480))
    with pytest.raises(TypeError):
        cloud.render(CameraIntrinsics(500.0, 500.0, 320.0, 240.0, 640, 480), camera_to_world=np.eye(4))
    m = DeviceVoxelMap.__new__(DeviceVoxelMap)
    m.ctx, m.handle = None, None
    with pytest.raises(TypeError):
        m.render(None)
    with pytest.raises(TypeError):
        m.render(CameraIntrinsics(500.0, 500.0, 320.0, 240.0, 640, 480), camera_to_world=(0, 0, 0))
