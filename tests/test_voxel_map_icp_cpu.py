"""Aligning against the voxel map (a3d_voxel_map_nearest_device, a3d_voxel_map_icp_*) without a GPU, as
test_voxel_map_retain_abi_cpu.py: the exported symbols, their header text and ctypes mirror, every refusal that is
decided on the host (a made-up context and made-up device addresses do: nothing is dereferenced), what a map without a
table answers on the host, the Python wrappers' argument checks, and the restatement of the association itself
(voxel_map_icp_restatement.py) against a brute-force nearest over all rows."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import voxel_map_icp_restatement as R
from align3d_amd import DevicePointCloud, DeviceVoxelMap, IcpParams, PointCloud, Transform, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_CTX = 0x900000
SENTINEL = 0x77
EMPTY_STATS = dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)
NAMES = {
    "a3d_voxel_map_nearest_device": ["a3d_voxel_map* map", "const float* d_queries", "uint64_t m", "const a3d_pose* pose_host",
                                     "uint32_t* d_out_seq", "float* d_out_dist2"],
    "a3d_voxel_map_icp_align_device": ["a3d_voxel_map* map", "const a3d_icp_params* params",
                                       "const a3d_point_cloud_view* d_source", "const a3d_pose* initial_host",
                                       "a3d_pose* out_pose"],
    "a3d_voxel_map_icp_accumulate_device": ["a3d_voxel_map* map", "const a3d_icp_params* params",
                                            "const a3d_point_cloud_view* d_source", "const a3d_pose* pose",
                                            "a3d_gn_state* out_state"],
    "a3d_voxel_map_icp_last_device_ms": ["a3d_voxel_map* map", "float* out_ms"],
}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _new(lib, normals=1):
    h = C.c_void_p()
    assert lib.a3d_voxel_map_new(C.c_void_p(FAKE_CTX), 0.05, None, normals, 0, C.byref(h)) == _abi.A3D_OK
    return h


@pytest.fixture()
def handle(lib):
    h = _new(lib)
    yield h
    lib.a3d_voxel_map_free(h)


@pytest.fixture()
def bare(lib):
    h = _new(lib, normals=0)
    yield h
    lib.a3d_voxel_map_free(h)


def _stats(lib, h):
    s = _abi.VoxelMapStatsC()
    assert lib.a3d_voxel_map_get_stats(h, C.byref(s)) == _abi.A3D_OK
    return s.as_dict()


def _filled(ctype):
    """A sentinel-filled instance of a ctypes struct."""
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
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    for name, want in NAMES.items():
        assert hasattr(lib, name) and hasattr(diag, name), name
        decl = re.search(r"a3d_status\s+" + name + r"\s*\((.*?)\);", section, re.S)
        assert decl, name
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == want, name
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is _abi.SIGNATURES["a3d_voxel_map_clear"][0] and len(argtypes) == len(want), name
    P = C.c_void_p
    assert _abi.SIGNATURES["a3d_voxel_map_nearest_device"][1] == [P, P, C.c_uint64, C.POINTER(_abi.PoseC), P, P]
    assert _abi.SIGNATURES["a3d_voxel_map_icp_align_device"][1] == [
        P, C.POINTER(_abi.IcpParamsC), C.POINTER(_abi.PointCloudViewC), C.POINTER(_abi.PoseC), C.POINTER(_abi.PoseC)]
    assert _abi.SIGNATURES["a3d_voxel_map_icp_accumulate_device"][1] == [
        P, C.POINTER(_abi.IcpParamsC), C.POINTER(_abi.PointCloudViewC), C.POINTER(_abi.PoseC), C.POINTER(_abi.GnStateC)]
    assert _abi.SIGNATURES["a3d_voxel_map_icp_last_device_ms"][1] == [P, C.POINTER(C.c_float)]
    # the header states the rule, what it is in plain words, and what it is not
    text = " ".join(section.replace("*", " ").split())
    for needle in ("c_k = floorf((q_k - o_k) / v)", "c + d, d in {-1, 0, 1}^3", "decided per axis, before the key is packed",
                   "a borrow or carry never reaches another axis's field", "bits(d2) << 32 | seq",
                   "does not depend on slot order, table size, growth history or timing", "seq 0xFFFFFFFF and d2 +inf",
                   "the exact nearest stored row wherever that row lies within about one cell of q",
                   "distances <= 0.75 v when |q - o| / v < 2^12", "NOT the reference's R3dTree::nearest",
                   "maps the source AS GIVEN into the map's frame", "max_iterations (0 returns the initial pose bit for bit)",
                   "never the table's slot count", "allocated on first use, freed with it"):
        assert needle in text, needle
    assert lib.a3d_abi_version() == 1
    for method in ("nearest", "align", "accumulate", "last_device_ms"):
        assert callable(getattr(DeviceVoxelMap, method))


def test_nearest_refusals_are_decided_on_the_host_and_touch_nothing(lib, handle):
    m = 16
    queries = (C.c_float * (3 * m))()
    seq = (C.c_uint32 * m)(*[0x77777777] * m)
    d2 = (C.c_float * m)(*[7.0] * m)
    fn = lib.a3d_voxel_map_nearest_device
    q, s, d = C.addressof(queries), C.addressof(seq), C.addressof(d2)

    def untouched():
        return list(seq) == [0x77777777] * m and list(d2) == [7.0] * m

    assert fn(None, q, m, None, s, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    for args in ((None, m, None, s, d), (q, m, None, None, d), (q, m, None, s, None)):
        assert fn(handle, *args) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(handle, q, 1 << 31, None, s, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    # outputs that overlap each other, or the queries (by one byte at either end)
    assert fn(handle, q, m, None, s, s) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(handle, q, m, None, s, s + 4 * m - 1) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(handle, q, m, None, q + 12 * m - 1, d) == _abi.A3D_INVALID_PARAMETER and untouched()
    assert fn(handle, q, m, None, s, q - 4 * m + 1) == _abi.A3D_INVALID_PARAMETER and untouched()
    # m == 0 is fine and touches nothing, whatever the pointers
    assert fn(handle, None, 0, None, None, None) == _abi.A3D_OK
    assert fn(handle, q, 0, None, s, s) == _abi.A3D_OK and untouched()
    assert fn(None, q, 0, None, s, d) == _abi.A3D_INVALID_PARAMETER
    assert _stats(lib, handle) == EMPTY_STATS


@pytest.mark.parametrize("entry", ["align", "accumulate"])
def test_icp_refusals_are_decided_on_the_host_and_touch_nothing(lib, handle, bare, entry):
    prm = IcpParams(max_iterations=3).to_c()
    pose = Transform.eye().to_c()
    fn = lib.a3d_voxel_map_icp_align_device if entry == "align" else lib.a3d_voxel_map_icp_accumulate_device
    out = _filled(_abi.PoseC if entry == "align" else _abi.GnStateC)

    def call(map_=handle, params=C.byref(prm), view=_view(), out_=C.byref(out)):
        return fn(map_, params, C.byref(view) if view is not None else None, C.byref(pose), out_)

    assert call(map_=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(params=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(view=None) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    assert call(out_=None) == _abi.A3D_INVALID_PARAMETER
    assert call(view=_view(points=None)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
    for n in (0, 1 << 31, 1 << 40):
        assert call(view=_view(n=n)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)
        assert call(map_=bare, view=_view(n=n)) == _abi.A3D_INVALID_PARAMETER and _untouched(out)  # before the normals
    assert call(map_=bare) == _abi.A3D_MISSING_FIELD and _untouched(out)
    assert call(map_=bare, view=_view(normals=None)) == _abi.A3D_MISSING_FIELD and _untouched(out)
    assert call(view=_view(normals=None)) == _abi.A3D_MISSING_FIELD and _untouched(out)
    assert b"source" in lib.a3d_last_error()
    assert _stats(lib, handle) == EMPTY_STATS and _stats(lib, bare) == EMPTY_STATS


def test_a_map_without_a_table_answers_on_the_host(lib, handle):
    """Nothing was inserted: no point can find a row.  max_iterations == 0 returns the initial pose; any iteration fails
    to solve with the pose where it started; an accumulation is empty."""
    start = _abi.PoseC()
    start.t[:] = [0.25, -1.5, 3.0]
    start.q[:] = [0.0, 0.6, 0.0, 0.8]
    view = _view()
    for initial, want in ((C.byref(start), start), (None, Transform.eye().to_c())):
        for iterations, status in ((0, _abi.A3D_OK), (4, _abi.A3D_SOLVE_FAILED)):
            prm = IcpParams(max_iterations=iterations).to_c()
            out = _filled(_abi.PoseC)
            assert lib.a3d_voxel_map_icp_align_device(handle, C.byref(prm), C.byref(view), initial, C.byref(out)) == status
            assert bytes(out) == bytes(want)
    prm = IcpParams(max_iterations=4).to_c()
    g = _filled(_abi.GnStateC)
    assert lib.a3d_voxel_map_icp_accumulate_device(handle, C.byref(prm), C.byref(view), None, C.byref(g)) == _abi.A3D_OK
    state = g.as_dict()
    assert state["count"] == 0 and not state["H"].any() and not state["g"].any() and state["ssq"] == 0
    ms = C.c_float(7.0)
    assert lib.a3d_voxel_map_icp_last_device_ms(handle, C.byref(ms)) == _abi.A3D_OK and ms.value == 0.0
    assert lib.a3d_voxel_map_icp_last_device_ms(None, C.byref(ms)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_icp_last_device_ms(handle, None) == _abi.A3D_INVALID_PARAMETER
    assert _stats(lib, handle) == EMPTY_STATS


def _fake_cloud(ctx, n=8, normals=True):
    c = DevicePointCloud.__new__(DevicePointCloud)
    c.ctx, c.n = ctx, n
    c.d_points, c.d_normals = C.c_void_p(0x10000), (C.c_void_p(0x20000) if normals else None)
    return c


def test_python_wrappers_check_their_arguments(lib):
    ctx = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX))
    other = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX + 0x1000))
    m = DeviceVoxelMap(ctx, 0.05)
    prm = IcpParams(max_iterations=2)
    seq, d2 = m.nearest(np.empty((0, 3), np.float32))
    assert seq.dtype == np.uint32 and d2.dtype == np.float32 and seq.shape == d2.shape == (0,)
    seq, d2 = m.nearest(_fake_cloud(ctx, n=0))
    assert seq.shape == d2.shape == (0,)
    for bad in (np.zeros(3, np.float32), np.zeros((4, 2), np.float32), np.zeros((2, 3, 3), np.float32)):
        with pytest.raises(_abi.InvalidParameter):
            m.nearest(bad)
    host = PointCloud(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32))
    for call in (lambda c: m.align(c, prm), lambda c: m.accumulate(c, prm, Transform.eye()), lambda c: m.nearest(c)):
        with pytest.raises(_abi.InvalidParameter):
            call(_fake_cloud(other))
    for call in (lambda c: m.align(c, prm), lambda c: m.accumulate(c, prm, Transform.eye())):
        with pytest.raises(TypeError):
            call(host)
        with pytest.raises(_abi.A3dError) as e:  # the library's refusal, through the wrapper
            call(_fake_cloud(ctx, normals=False))
        assert e.value.status == _abi.A3D_MISSING_FIELD
        with pytest.raises(_abi.A3dError) as e:
            call(_fake_cloud(ctx, n=0))
        assert e.value.status == _abi.A3D_INVALID_PARAMETER
    # a map without a table: the library answers on the host
    start = Transform.from_c(_pose((0.5, 0.25, -1.0), (0.0, 0.0, 0.6, 0.8)))
    got = m.align(_fake_cloud(ctx), IcpParams(max_iterations=0), initial=start)
    assert bytes(got.to_c()) == bytes(start.to_c())
    with pytest.raises(_abi.A3dError) as e:
        m.align(_fake_cloud(ctx), prm)
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    assert m.accumulate(_fake_cloud(ctx), prm, start)["count"] == 0 and m.last_device_ms() == 0.0
    assert m.stats() == EMPTY_STATS
    m.free()


def _pose(t, q):
    p = _abi.PoseC()
    p.t[:], p.q[:] = t, q
    return p


VOXEL = 0.05
ORIGIN = (0.013, -0.4, 0.021)


@pytest.fixture(scope="module")
def scene():
    points, normals = R.surfaces(1, 3000)
    return R.MapRestatement(points, normals, VOXEL, ORIGIN)


def test_restatement_is_the_exact_nearest_row_within_three_quarters_of_a_cell(scene):
    """Coordinates within a few metres and v = 0.05: |q - o| / v < 2^12, so every row within 0.75 v of a query lies in
    the query's 27 cells and the association is the brute-force nearest over ALL rows, index and d2 bit for bit.  No
    such query is left out."""
    q, normal = R.surfaces(2, 2000)
    off = np.random.default_rng(3).uniform(-0.06, 0.06, size=(len(q), 1)).astype(np.float32)
    q = q + normal * off  # from on the surfaces to beyond the reach of the search
    assert np.abs((q - scene.origin) / scene.voxel).max() < 2 ** 12
    seq, d2, row = scene.nearest(q)
    bf_seq, bf_d2, bf_row = R.brute_force(scene.rows, scene.seq, q)
    near = np.sqrt(bf_d2.astype(np.float64)) <= 0.75 * VOXEL
    assert near.sum() > 500 and (~near).sum() > 500, (near.sum(), len(q))  # (both sides of the reach are exercised)
    assert np.array_equal(seq[near], bf_seq[near]) and np.array_equal(row[near], bf_row[near])
    assert np.array_equal(d2[near].view(np.uint32), bf_d2[near].view(np.uint32))
    # beyond: a row that is found is a stored row at the stated distance, never nearer than the true nearest
    found = row >= 0
    assert np.array_equal(seq[~found], np.full((~found).sum(), R.NONE_SEQ, np.uint32)) and np.isposinf(d2[~found]).all()
    assert np.array_equal(scene.seq[row[found]], seq[found]) and (d2[found] >= bf_d2[found]).all()
    assert np.array_equal(R.dist2(q[found], scene.rows[row[found]]).view(np.uint32), d2[found].view(np.uint32))


def test_restatement_drops_what_the_map_drops_and_honours_a_pose(scene):
    q = np.asarray([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e9, 0, 0], [0, -1e9, 0], [0.5, 0.5, 0.0]], np.float32)
    seq, d2, row = scene.nearest(q)
    assert seq[:5].tolist() == [R.NONE_SEQ] * 5 and np.isposinf(d2[:5]).all() and (row[:5] == -1).all() and row[5] >= 0
    import oracle_lib as O

    pose = O.exp_se3([0.3, -0.2, 0.1, 0.02, -0.03, 0.01])
    pts, _ = R.surfaces(4, 200)
    a, b = scene.nearest(pts, pose), scene.nearest(O.transform_points(pose, pts))
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def test_restatement_skips_a_neighbour_per_axis_before_the_key_is_packed():
    for axis, end, query, trap, fair in R.borrow_cases():
        q = np.asarray([query], np.float32)
        assert np.array_equal(q, np.asarray([query], np.float64)), "the case is exact in f32"
        if trap is not None:
            m = R.MapRestatement(np.asarray([trap], np.float32), np.asarray([[0, 0, 1]], np.float32), 1.0)
            seq, d2, row = m.nearest(q)
            assert seq[0] == R.NONE_SEQ and np.isposinf(d2[0]) and row[0] == -1, (axis, end)
        rows = [fair] if trap is None else [trap, fair]
        m = R.MapRestatement(np.asarray(rows, np.float32), np.asarray([[0, 0, 1]] * len(rows), np.float32), 1.0)
        seq, d2, row = m.nearest(q)
        assert seq[0] == len(rows) - 1 and d2[0] == 1.0, (axis, end)
    # the case of the issue: a query in cell z = -2^20 and a row in the cell the borrowed key would name, (0, -1, 2^20 - 1)
    case = [c for c in R.borrow_cases() if c[0] == 2 and c[1] == 0][0]
    assert case[2] == [0.5, 0.5, -R.LIM + 0.5] and case[3] == [0.5, -0.5, R.LIM - 0.5]
