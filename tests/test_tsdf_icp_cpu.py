"""Aligning against the TSDF volume (a3d_tsdf_volume_sample_device, a3d_tsdf_volume_icp_*) without a GPU, as
test_voxel_map_icp_cpu.py: the exported symbols, their header text and ctypes mirror, every refusal that is decided on the
host (a made-up volume and made-up device addresses do: nothing is dereferenced), the Python wrappers' argument checks,
and the restatement itself (tsdf_icp_restatement.py) against an ANALYTIC field: a room corner and a sphere, whose
distance and direction are known in closed form."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import oracle_lib as O
import tsdf_icp_restatement as R
from align3d_amd import DevicePointCloud, DeviceTsdfVolume, IcpParams, PointCloud, Transform, _abi
from gpu_util import small_pose, transform_diff
from voxel_map_icp_restatement import transform_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_VOLUME = 0x30000
FAKE_CTX = 0x900000
SENTINEL = 0x77
F = np.float32
NAMES = {
    "a3d_tsdf_volume_sample_device": ["a3d_tsdf_volume* volume", "const float* d_queries", "uint64_t m",
                                      "const a3d_pose* pose_host", "float* d_out_distance", "float* d_out_normals"],
    "a3d_tsdf_volume_icp_align_device": ["a3d_tsdf_volume* volume", "const a3d_icp_params* params",
                                         "const a3d_point_cloud_view* d_source", "const a3d_pose* initial_host",
                                         "a3d_pose* out_pose"],
    "a3d_tsdf_volume_icp_accumulate_device": ["a3d_tsdf_volume* volume", "const a3d_icp_params* params",
                                              "const a3d_point_cloud_view* d_source", "const a3d_pose* pose",
                                              "a3d_gn_state* out_state"],
    "a3d_tsdf_volume_icp_last_device_ms": ["a3d_tsdf_volume* volume", "float* out_ms"],
}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _filled(ctype):
    v = ctype()
    C.memset(C.byref(v), SENTINEL, C.sizeof(v))
    return v


def _untouched(v):
    return bytes(v) == bytes([SENTINEL]) * C.sizeof(v)


def _view(points=0x10000, normals=0x20000, n=8):
    v = _abi.PointCloudViewC()
    v.points, v.normals, v.len = points, normals, n
    return v


def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    section = header[header.index("---- Aligning against the volume"):header.index("---- R3dTree")]
    for name, want in NAMES.items():
        assert hasattr(lib, name) and hasattr(diag, name), name
        decl = re.search(r"a3d_status\s+" + name + r"\s*\((.*?)\);", section, re.S)
        assert decl, name
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == want, name
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is _abi.SIGNATURES["a3d_tsdf_volume_clear"][0] and len(argtypes) == len(want), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    P = C.c_void_p
    assert _abi.SIGNATURES["a3d_tsdf_volume_sample_device"][1] == [P, P, C.c_uint64, C.POINTER(_abi.PoseC), P, P]
    assert _abi.SIGNATURES["a3d_tsdf_volume_icp_align_device"][1] == [
        P, C.POINTER(_abi.IcpParamsC), C.POINTER(_abi.PointCloudViewC), C.POINTER(_abi.PoseC), C.POINTER(_abi.PoseC)]
    assert _abi.SIGNATURES["a3d_tsdf_volume_icp_accumulate_device"][1] == [
        P, C.POINTER(_abi.IcpParamsC), C.POINTER(_abi.PointCloudViewC), C.POINTER(_abi.PoseC), C.POINTER(_abi.GnStateC)]
    assert _abi.SIGNATURES["a3d_tsdf_volume_icp_last_device_ms"][1] == [P, C.POINTER(C.c_float)]
    # the header states the rule, what it is not, and what stays out of scope
    text = " ".join(section.replace("*", " ").split())
    for needle in ("g = (q - origin) / v per component", "D = tri(g), step 3 of the raycast rule unchanged",
                   "NO CORRESPONDENCE unless |D| < 1", "tri(g + ex) - tri(g - ex)", "summed left to right",
                   "in the WORLD frame (nothing is rotated back)", "n points out of the surface", "d = D tau",
                   "d2 = d d", "0x7FC00000", "NOT Icp over a3d_tsdf_volume_extract_surface's point cloud",
                   "a robust kernel, colour terms, several sources per call, a coarse-to-fine schedule and an analytic one-cell gradient",
                   "the volume is never written", "maps the source AS GIVEN into the volume's world frame",
                   "max_iterations (0 returns the initial pose bit for bit)", "never the volume's size",
                   "allocated on first use, freed with it"):
        assert needle in text, needle
    makefile = open(os.path.join(ROOT, "align3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btsdf_icp\.hip\b", makefile, re.M)
    assert lib.a3d_abi_version() == 1
    for method in ("sample", "align", "accumulate", "last_device_ms"):
        assert callable(getattr(DeviceTsdfVolume, method))


def test_sample_refusals_are_decided_on_the_host_and_touch_nothing(lib):
    m = 16
    queries = (C.c_float * (3 * m))()
    dist = (C.c_float * m)(*[7.0] * m)
    nrm = (C.c_float * (3 * m))(*[7.0] * (3 * m))
    fn = lib.a3d_tsdf_volume_sample_device
    vol = C.c_void_p(FAKE_VOLUME)
    q, s, d = C.addressof(queries), C.addressof(dist), C.addressof(nrm)

    def untouched():
        return list(dist) == [7.0] * m and list(nrm) == [7.0] * (3 * m)

    assert fn(None, q, m, None, s, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    for args in ((None, m, None, s, d), (q, m, None, None, d), (q, m, None, s, None)):
        assert fn(vol, *args) == _abi.A3D_INVALID_PARAMETER and untouched()
    for big in (1 << 31, 1 << 40):
        assert fn(vol, q, big, None, s, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    # outputs that overlap each other, or the queries (by one byte at either end)
    assert fn(vol, q, m, None, s, s) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(vol, q, m, None, s, s + 4 * m - 1) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(vol, q, m, None, d + 12 * m - 1, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(vol, q, m, None, q + 12 * m - 1, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(vol, q, m, None, s, q - 12 * m + 1) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert b"overlap" in lib.a3d_last_error()
    # m == 0 is fine and touches nothing, whatever the pointers
    assert fn(vol, None, 0, None, None, None) == _abi.A3D_OK
    assert fn(vol, q, 0, None, s, s) == _abi.A3D_OK and untouched()
    assert fn(None, q, 0, None, s, d) == _abi.A3D_INVALID_PARAMETER


@pytest.mark.parametrize("entry", ["align", "accumulate"])
def test_icp_refusals_are_decided_on_the_host_and_touch_nothing(lib, entry):
    prm = IcpParams(max_iterations=3).to_c()
    pose = Transform.eye().to_c()
    fn = lib.a3d_tsdf_volume_icp_align_device if entry == "align" else lib.a3d_tsdf_volume_icp_accumulate_device
    out = _filled(_abi.PoseC if entry == "align" else _abi.GnStateC)
    vol = C.c_void_p(FAKE_VOLUME)

    def call(volume=vol, params=C.byref(prm), view=_view(), out_=C.byref(out)):
        return fn(volume, params, C.byref(view) if view is not None else None, C.byref(pose), out_)

    assert call(volume=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(params=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(view=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(out_=None) == _abi.A3D_INVALID_PARAMETER
    assert call(view=_view(points=None)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    for n in (0, 1 << 31, 1 << 40):
        assert call(view=_view(n=n)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
        assert call(view=_view(n=n, normals=None)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)  # before the normals
    assert call(view=_view(normals=None)) == _abi.A3D_MISSING_FIELD and _untouched(out)
    assert b"source" in lib.a3d_last_error()
    ms = C.c_float(7.0)
    assert lib.a3d_tsdf_volume_icp_last_device_ms(None, C.byref(ms)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_tsdf_volume_icp_last_device_ms(vol, None) == _abi.A3D_INVALID_PARAMETER and ms.value == 7.0


def _fake_cloud(ctx, n=8, normals=True):
    c = DevicePointCloud.__new__(DevicePointCloud)
    c.ctx, c.n = ctx, n
    c.d_points, c.d_normals = C.c_void_p(0x10000), (C.c_void_p(0x20000) if normals else None)
    return c


def test_python_wrappers_check_their_arguments(lib):
    ctx = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX))
    other = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX + 0x1000))
    vol = DeviceTsdfVolume.__new__(DeviceTsdfVolume)  # (a volume needs a device: the wrapper around a made-up handle)
    vol.ctx, vol.handle = ctx, C.c_void_p(FAKE_VOLUME)
    prm = IcpParams(max_iterations=2)
    try:
        dist, nrm = vol.sample(np.empty((0, 3), F))
        assert dist.dtype == nrm.dtype == F and dist.shape == (0,) and nrm.shape == (0, 3)
        dist, nrm = vol.sample(_fake_cloud(ctx, n=0))
        assert dist.shape == (0,) and nrm.shape == (0, 3)
        for bad in (np.zeros(3, F), np.zeros((4, 2), F), np.zeros((2, 3, 3), F)):
            with pytest.raises(_abi.InvalidParameter):
                vol.sample(bad)
        host = PointCloud(np.zeros((4, 3), F), np.zeros((4, 3), F))
        for call in (lambda c: vol.align(c, prm), lambda c: vol.accumulate(c, prm), lambda c: vol.sample(c)):
            with pytest.raises(_abi.InvalidParameter):
                call(_fake_cloud(other))
        for call in (lambda c: vol.align(c, prm), lambda c: vol.accumulate(c, prm, Transform.eye())):
            with pytest.raises(TypeError, match="there is no host fallback"):
                call(host)
            with pytest.raises(_abi.A3dError) as e:  # the library's refusal, through the wrapper
                call(_fake_cloud(ctx, normals=False))
            assert e.value.status == _abi.A3D_MISSING_FIELD
            with pytest.raises(_abi.A3dError) as e:
                call(_fake_cloud(ctx, n=0))
            assert e.value.status == _abi.A3D_INVALID_PARAMETER
    finally:
        vol.handle = C.c_void_p()  # nothing to free


# ---- the restatement against an analytic field -----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def field():
    return R.FieldRestatement(R.corner_volume())


def test_restatement_gives_the_analytic_distance_and_normal_on_the_walls(field):
    """Within 0.08 of one wall, at least 0.3 from the other two and 0.4 from the sphere, every voxel of the 4 x 4 x 4
    neighbourhood (it reaches 0.1 from the query along each axis, 0.18 from the wall, and stays 0.2 from the other walls
    and 0.22 from the sphere) holds the distance to that one wall, inside the truncation 0.2 and observed: D is LINEAR there, trilinear interpolation reproduces a linear function, and the central difference its slope.  What is
    left is rounding: D = sd / tau <= 0.75 is stored and interpolated in f32 (a handful of operations, each within half
    an ulp of a value below 1, 6e-8), so d = D tau is within 1e-6 m of the analytic distance with room to spare; the
    gradient's own axis is a difference of two such values 0.5 apart and the other two axes are differences of
    values that differ by rounding only, so n is within 1e-5 of the wall's normal per component."""
    rng = np.random.default_rng(3)
    for axis, at in enumerate(R.PLANES):
        q = rng.uniform(at + 0.3, 1.35, size=(400, 3))
        q[:, axis] = at + rng.uniform(-0.08, 0.08, size=400)
        others = np.delete(q - np.asarray(R.PLANES), axis, axis=1).min(axis=1)
        sphere = np.linalg.norm(q - np.asarray(R.CENTRE), axis=1) - R.RADIUS
        q = q[(others >= 0.3) & (sphere >= 0.4)].astype(F)
        assert len(q) > 100, (axis, len(q))
        d, n, value, direction = field.sample(q)
        assert value.all() and direction.all()
        want = q.astype(np.float64)[:, axis] - at
        assert np.allclose(R.signed_distance(q), want, atol=0, rtol=0)  # (the wall is the nearest surface)
        assert np.abs(d - want).max() < 1e-6, (axis, np.abs(d - want).max())
        e = np.zeros(3)
        e[axis] = 1.0
        assert np.abs(n - e).max() < 1e-5, (axis, np.abs(n - e).max())


def test_restatement_gives_no_value_and_no_direction_where_the_rule_says_so(field):
    q = np.asarray([[0.7, 0.7, 0.4],          # in the room, near the floor: a value and a direction
                    [5.0, 0.7, 0.7],          # outside the volume
                    [np.nan, 0.7, 0.7], [0.7, np.inf, 0.7],
                    [0.02, 0.7, 0.7],         # deep behind the wall x = 0.3 (sd < -tau): never observed
                    [1.4, 0.6, 0.7]           # free space, beyond the truncation of every surface: |D| = 1
                    ], F)
    d, n, value, direction = field.sample(q)
    assert value.tolist() == [True, False, False, False, False, True]
    assert direction.tolist() == [True, False, False, False, False, False]
    assert d.view(np.uint32)[1:5].tolist() == [R.NAN_BITS] * 4 and not n[1:].view(np.uint32).any()
    assert abs(d[0] - 0.05) < 1e-6 and d[5] == field.volume.tau
    # a pose applied first is the same as moving the queries
    pose = O.exp_se3([0.02, -0.03, 0.01, 0.01, 0.02, -0.015])
    pts, _ = R.corner_surfaces(4, 300)
    a, b = field.sample(pts, pose), field.sample(O.transform_points(pose, pts))
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
               for x, y in zip(a, b))


def test_restatement_recovers_the_offset_of_the_source(field):
    """5 000 points on the walls and the sphere, seen from a frame about 0.01 rad / 0.01 m away: five iterations recover
    that offset within 2e-3 rad / 2e-3 m (the bound of test_gpu_voxel_map_icp.py for the same claim), and fewer than 1 %
    of the points find no correspondence, at the start and at the end."""
    offset = small_pose(7, rot=0.01, trans=0.01).to_c()
    inverse = _abi.PoseC()
    O.load().orc_inverse(C.byref(offset), C.byref(inverse))
    world_p, world_n = R.corner_surfaces(5, 5000)
    src_p, src_n = O.transform_points(inverse, world_p), transform_normals(inverse, world_n)
    status, pose = field.align(src_p, src_n, IcpParams(max_iterations=5).to_c())
    ang, tr = transform_diff(Transform.from_c(pose), offset)
    print(f"restated align: d_angle {ang:.3g} rad, d_trans {tr:.3g} m")
    assert status == _abi.A3D_OK and ang < 2e-3 and tr < 2e-3, (status, ang, tr)
    for T in (Transform.eye().to_c(), pose):
        lost = (~field.sample(src_p, T)[3]).sum()
        assert lost < 0.01 * len(src_p), lost
    state = field.accumulate(src_p, src_n, pose, IcpParams(max_iterations=5).to_c())
    assert state["count"] > 4500
