"""Normals of resident clouds from their own neighbourhoods (a3d_point_clouds_estimate_normals_device,
DevicePointCloud.estimate_normals / estimate_normals_many) on the GPU.

Every comparison is on uint32 views, bit for bit, and the expected value is always the numpy restatement of the rule
(normals_restatement.py), never the code under test.  The raw call writes into buffers that are filled with a canary word
from end to end, with CANARY_WORDS more of it on both sides.  The one tolerance (the pose of an alignment between two
clouds with estimated normals, against the oracle's ICP on the same host arrays) is the 1e-4 / 1e-4 of
test_gpu_pcl_icp.py.

The restatement is brute force over pairs, so the sizes are what it can afford in a few seconds: the size grid runs every
radius up to 2049 points, and so does the cloud of 20 000 at 0.02, 0.1 and 1e-5, where its candidate slabs are thin.  At
1e3 (one cell of 20 000 records: 4e8 pairs) the restatement is computed for 512 seeded rows against all 20 000 candidates
and those rows are compared bit for bit; every row's count and the valid total are checked as well."""
import ctypes as C
import os

import numpy as np
import pytest

import normals_restatement as R
import oracle_lib as O
from align3d_amd import (A3dError, DevicePointCloud, DeviceVoxelMap, Icp, IcpParams, PointCloud, RangeImageBuilder,
                         SlamTbDataset, Transform, _abi)
from align3d_amd._abi import PoseC
from gpu_util import transform_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 2, 63, 64, 65, 2047, 2049)
RADII = (0.02, 0.1, 1e3, 1e-5)
CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)
BATCH_LENGTHS = (1, 0, 63, 64, 65, 300, 513, 1025, 0, 2, 130, 7)  # 1025: a cloud of two tiles


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the recipe of test_gpu_voxel_downsample.py): NaNs with payloads, infinities, -0.0, denormals
    and magnitudes far beyond the 21-bit cell range all occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _cube(seed, n, lo=0.25, side=0.5):
    return np.random.default_rng(seed).uniform(lo, lo + side, size=(n, 3)).astype(np.float32)


def _device_cloud(ctx, points, normals=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals))


class _Guarded:
    """A device buffer of `count` elements of `width` words, canary-filled from end to end, CANARY_WORDS more on both
    sides."""

    def __init__(self, ctx, count, width):
        self.ctx, self.count, self.width = ctx, count, width
        self.words = 2 * CANARY_WORDS + width * count
        self.base = ctx.to_device(np.full(self.words, CANARY, np.uint32))
        self.ptr = C.c_void_p(self.base.value + 4 * CANARY_WORDS)

    def read(self):
        """(the body as [count, width] uint32, True iff both guards are intact)."""
        w = self.ctx.to_host(self.base, np.empty(self.words, np.uint32))
        body = w[CANARY_WORDS:self.words - CANARY_WORDS].reshape(self.count, self.width)
        return body, bool((w[:CANARY_WORDS] == CANARY).all() and (w[self.words - CANARY_WORDS:] == CANARY).all())

    def free(self):
        self.ctx.free(self.base)


def _call(ctx, clouds, radius, viewpoints=None, min_neighbors=3, orient=0, curvature=True, counts=True):
    """The raw call on resident clouds into guarded buffers.  Returns (status, valid, dropped, per cloud {normals [len, 3],
    curvature [len], counts [len]: uint32 bodies or None}); asserts the guards."""
    n = len(clouds)
    g_normals = [_Guarded(ctx, c.len(), 3) for c in clouds]
    g_curv = [_Guarded(ctx, c.len(), 1) if curvature else None for c in clouds]
    g_counts = [_Guarded(ctx, c.len(), 1) if counts else None for c in clouds]
    valid, dropped = (C.c_uint64 * n)(*[12345] * n), (C.c_uint64 * n)(*[12345] * n)
    eyes = None
    if viewpoints is not None:
        eyes = (C.c_float * (3 * n))(*np.asarray(viewpoints, np.float32).reshape(-1).tolist())
    views = (_abi.PointCloudViewC * n)(*[c.view() for c in clouds])
    st = ctx.lib.a3d_point_clouds_estimate_normals_device(
        ctx.handle, views, n, radius, min_neighbors, eyes, orient, (C.c_void_p * n)(*[g.ptr for g in g_normals]),
        (C.c_void_p * n)(*[g.ptr for g in g_curv]) if curvature else None,
        (C.c_void_p * n)(*[g.ptr for g in g_counts]) if counts else None, valid, dropped)
    outs = []
    for gn, gc, gk in zip(g_normals, g_curv, g_counts):
        out = {}
        for name, g in (("normals", gn), ("curvature", gc), ("counts", gk)):
            out[name] = None
            if g is not None:
                body, intact = g.read()
                assert intact, f"the call wrote outside its {name} buffer"
                out[name] = body if name == "normals" else body[:, 0]
                g.free()
        outs.append(out)
    return st, list(valid), list(dropped), outs


def _assert_matches(out, got_valid, got_dropped, expected, points, radius):
    """One cloud's buffers against the restatement's (normals, curvature, counts, valid): every row is written."""
    normals, curvature, counts, valid = expected
    kept, _ = R.cells(points, radius)
    assert (got_valid, got_dropped) == (int(valid.sum()), int((~kept).sum()))
    assert np.array_equal(out["normals"], _bits(normals).reshape(-1, 3))
    if out["curvature"] is not None:
        assert np.array_equal(out["curvature"], _bits(curvature))
    if out["counts"] is not None:
        assert np.array_equal(out["counts"], counts)


def test_size_and_radius_grid(ctx):
    for k, n in enumerate(SIZES):
        points = _cube(100 + k, n)
        cloud = _device_cloud(ctx, points)
        for radius in RADII:
            eye = (0.1, -0.3, 2.0)
            expected = R.estimate_normals(points, radius, viewpoint=eye)
            if radius == 1e3 and n:
                assert (expected[2] == n).all() and expected[3].all() == (n >= 3)
            if radius == 1e-5 and n:
                assert (expected[2] == 1).all() and not expected[3].any()  # every point alone
            if radius == 0.1 and n == 2049:
                assert expected[3].all() and 5 < expected[2].min() < expected[2].max() < 200
            for extras in (True, False):
                st, valid, dropped, outs = _call(ctx, [cloud], radius, [eye], curvature=extras, counts=extras)
                assert st == _abi.A3D_OK, (n, radius)
                _assert_matches(outs[0], valid[0], dropped[0], expected, points, radius)
        cloud.free()


def _cube_and_sheet():
    """20 000 points: 12 000 uniform in a 3 m cube and 8 000 on a noisy strip of 2.5 m x 0.1 m (32 000 per square metre)."""
    rng = np.random.default_rng(77)
    cube = rng.uniform(0.25, 3.25, size=(12000, 3))
    sheet = np.c_[rng.uniform(0.3, 2.8, 8000), rng.uniform(1.0, 1.1, 8000), 1.5 + rng.normal(0, 0.001, 8000)]
    return np.r_[cube, sheet].astype(np.float32)[rng.permutation(20000)]


def test_cube_and_sheet_of_twenty_thousand(ctx):
    points = _cube_and_sheet()
    cloud = _device_cloud(ctx, points)
    for radius in (0.02, 0.1, 1e-5):
        expected = R.estimate_normals(points, radius, viewpoint=(1.5, 1.0, 4.0))
        if radius == 0.1:
            assert expected[2].min() == 1 and expected[2].max() > 300  # counts from 1 to hundreds
            on_sheet = expected[2] > 300
            assert on_sheet.sum() > 5000 and (expected[0][on_sheet][:, 2] > 0.99).all()  # the sheet looks up at the viewpoint
        st, valid, dropped, outs = _call(ctx, [cloud], radius, [(1.5, 1.0, 4.0)])
        assert st == _abi.A3D_OK
        _assert_matches(outs[0], valid[0], dropped[0], expected, points, radius)
    # everything in one cell: 20 tiles, every thread walks one run of 20 000 records, 20 000 atomics on one slot
    rows = np.sort(np.random.default_rng(78).choice(20000, size=512, replace=False))
    normals, curvature, counts, ok = R.estimate_normals(points, 1e3, viewpoint=(1.5, 1.0, 4.0), rows=rows, slab=False)
    assert (counts[rows] == 20000).all() and ok[rows].all()
    st, valid, dropped, outs = _call(ctx, [cloud], 1e3, [(1.5, 1.0, 4.0)])
    assert st == _abi.A3D_OK and valid[0] == 20000 and dropped[0] == 0
    assert (outs[0]["counts"] == 20000).all()  # N = n for every row
    assert np.array_equal(outs[0]["normals"][rows], _bits(normals[rows]).reshape(-1, 3))
    assert np.array_equal(outs[0]["curvature"][rows], _bits(curvature[rows]))
    got = outs[0]["normals"].view(np.float32)
    assert (np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) < 1e-6).all()  # the other rows hold unit normals too
    cloud.free()


def test_negative_cells_lattice_points_duplicates_and_hostile_rows(ctx):
    rng = np.random.default_rng(5)
    r = np.float32(0.0625)
    lattice = (rng.integers(-3, 3, size=(600, 3)).astype(np.float32) * r).astype(np.float32)  # exactly on k * r, many twice
    negative = _cube(6, 700, lo=-1.0, side=0.3)
    duplicated = np.repeat(_cube(7, 100, lo=-0.2, side=0.3), 3, axis=0)
    raw = _raw_bits(8, 300)
    points = np.r_[lattice, negative, duplicated, raw][rng.permutation(1900)]
    kept, cell = R.cells(points, r)
    assert 100 < (~kept).sum() < 300 and (cell[kept] < 0).any()
    expected = R.estimate_normals(points, r, viewpoint=(0.5, 0.5, 0.5))
    assert expected[3].sum() > 1000 and (expected[2][~kept] == 0).all() and (_bits(expected[0][~kept]) == 0).all()
    cloud = _device_cloud(ctx, points)
    st, valid, dropped, outs = _call(ctx, [cloud], float(r), [(0.5, 0.5, 0.5)])
    assert st == _abi.A3D_OK and dropped[0] == (~kept).sum()
    _assert_matches(outs[0], valid[0], dropped[0], expected, points, r)
    # min_neighbors decides validity and nothing else
    expected = R.estimate_normals(points, r, min_neighbors=9, viewpoint=(0.5, 0.5, 0.5))
    st, valid, dropped, outs = _call(ctx, [cloud], float(r), [(0.5, 0.5, 0.5)], min_neighbors=9)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], valid[0], dropped[0], expected, points, r)
    cloud.free()
    # only hostile rows: everything dropped or alone
    cloud = _device_cloud(ctx, raw)
    expected = R.estimate_normals(raw, 0.05)
    st, valid, dropped, outs = _call(ctx, [cloud], 0.05)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], valid[0], dropped[0], expected, raw, 0.05)
    cloud.free()


_batch = {}


def _batch_recipe():
    """129 clouds of unequal sizes (empty ones among them; every sixteenth carries raw-bit rows), a viewpoint each, and
    the restatement of each cloud alone; cloud i is the same in every batch size.  Built once."""
    if not _batch:
        clouds, eyes, expected = [], [], []
        for i in range(129):
            rng = np.random.default_rng([4242, i])
            n = BATCH_LENGTHS[i % len(BATCH_LENGTHS)]
            side = 0.05 * max(1.0, n / 4.0) ** (1.0 / 3.0)
            points = (rng.uniform(-2.0, 2.0, size=3) + rng.uniform(0.0, side, size=(n, 3))).astype(np.float32)
            if i % 16 == 5 and n > 10:
                points[::7] = _raw_bits(i, len(points[::7]))
            eye = rng.uniform(-3.0, 3.0, size=3).astype(np.float32)
            clouds.append(points), eyes.append(eye)
            expected.append(R.estimate_normals(points, 0.05, viewpoint=eye))
        _batch.update(clouds=clouds, eyes=eyes, expected=expected)
    return _batch


@pytest.mark.parametrize("n_clouds", [65, 129])
def test_batches_of_unequal_clouds_with_a_viewpoint_each(ctx, n_clouds):
    b = _batch_recipe()
    clouds = [_device_cloud(ctx, p) for p in b["clouds"][:n_clouds]]
    st, valid, dropped, outs = _call(ctx, clouds, 0.05, b["eyes"][:n_clouds])
    assert st == _abi.A3D_OK
    assert sum(valid) > 1000 and sum(dropped) > 50 and sum(1 for c in clouds if c.len() == 0) >= 10
    for i in range(n_clouds):
        _assert_matches(outs[i], valid[i], dropped[i], b["expected"][i], b["clouds"][i], 0.05)
    for c in clouds:
        c.free()


def test_the_same_cloud_twice_in_a_batch_gets_the_bits_it_gets_alone(ctx):
    points, other = _cube(31, 1500, side=0.4), _cube(32, 900, side=0.4)  # the clouds overlap in space
    a, b, c = _device_cloud(ctx, points), _device_cloud(ctx, other), _device_cloud(ctx, points)
    eye = (0.0, 0.0, 0.0)
    st, valid1, dropped1, alone = _call(ctx, [a], 0.05, [eye])
    assert st == _abi.A3D_OK and valid1[0] > 1000
    st, valid, dropped, outs = _call(ctx, [a, b, c, a], 0.05, [eye, eye, eye, eye])
    assert st == _abi.A3D_OK and valid[0] == valid[2] == valid[3] == valid1[0]
    for k in (0, 2, 3):  # no neighbour leaks across jobs
        for name in ("normals", "curvature", "counts"):
            assert np.array_equal(outs[k][name], alone[0][name]), (k, name)
    _assert_matches(alone[0], valid1[0], dropped1[0], R.estimate_normals(points, 0.05, viewpoint=eye), points, 0.05)
    for x in (a, b, c):
        x.free()


def test_two_runs_give_the_same_bits_and_a_row_permutation_permutes_them(ctx):
    points = np.r_[_cube(41, 5000, side=0.6), _raw_bits(42, 50)]
    perm = np.random.default_rng(43).permutation(len(points))
    cloud, shuffled = _device_cloud(ctx, points), _device_cloud(ctx, points[perm])
    st, valid, dropped, first = _call(ctx, [cloud], 0.05)
    st2, valid2, dropped2, second = _call(ctx, [cloud], 0.05)
    st3, valid3, dropped3, moved = _call(ctx, [shuffled], 0.05)
    assert st == st2 == st3 == _abi.A3D_OK and valid == valid2 == valid3 and dropped == dropped2 == dropped3
    assert valid[0] > 4000
    for name in ("normals", "curvature", "counts"):
        assert np.array_equal(first[0][name], second[0][name]), name
        assert np.array_equal(moved[0][name], first[0][name][perm]), name  # (what a float accumulation would fail)
    _assert_matches(first[0], valid[0], dropped[0], R.estimate_normals(points, 0.05), points, 0.05)
    cloud.free(), shuffled.free()


@pytest.mark.parametrize("knob,value", [("A3D_NORMALS_ORDER", "input"), ("A3D_NORMALS_AHEAD", "1"), ("A3D_NORMALS_LDS", "1")])
def test_the_forms_the_diagnostics_build_keeps_give_the_same_bits(ctx, diag_ctx, monkeypatch, knob, value):
    # 3030 rows (the last wave of the last tile is partly dead) and a second cloud of 65 in the same call; at radius 0.05
    # runs of a few records, at 1e3 one run of more than 64 records per cloud (the LDS form stages it in several trips)
    points = np.r_[_cube(51, 3000, side=0.5), _raw_bits(52, 30)]
    small = _cube(53, 65, side=0.2)
    clouds, diag_clouds = [_device_cloud(ctx, p) for p in (points, small)], [_device_cloud(diag_ctx, p) for p in (points, small)]
    for radius in (0.05, 1e3):
        monkeypatch.delenv(knob, raising=False)
        st, valid, dropped, outs = _call(ctx, clouds, radius)
        monkeypatch.setenv(knob, value)
        st2, valid2, dropped2, diag = _call(diag_ctx, diag_clouds, radius)
        assert st == st2 == _abi.A3D_OK and valid == valid2 and dropped == dropped2 and valid[0] > 2000
        for k in range(2):
            for name in ("normals", "curvature", "counts"):
                assert np.array_equal(outs[k][name], diag[k][name]), (radius, k, name)
    for c in clouds + diag_clouds:
        c.free()


_frames = {}


def _sample1_frames(ctx):
    """Frames 0 and 1 of sample1 as resident clouds with their image normals; built once per session."""
    if not _frames:
        ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
        frames = [ds.get(i) for i in range(2)]
        cam, _, _, depth_scale = frames[0]
        built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(
            cam, [(f[1], f[2]) for f in frames], depth_scale)
        images = [pyramid[0] for pyramid in built]
        _frames["clouds"] = DevicePointCloud.from_range_images(images)
        for im in images:
            im.free()
    return _frames["clouds"]


def test_orient_by_normals_in_place_on_negated_image_normals(ctx):
    thin = _sample1_frames(ctx)[0].voxel_downsample(0.03)
    points, image_normals = thin.download()
    assert 5000 < len(points) < 20000
    old = (-image_normals).astype(np.float32)
    cloud = _device_cloud(ctx, points, old)
    expected = R.estimate_normals(points, 0.09, old_normals=old)
    views = (_abi.PointCloudViewC * 1)(cloud.view())
    valid, dropped = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    st = ctx.lib.a3d_point_clouds_estimate_normals_device(ctx.handle, views, 1, 0.09, 3, None, 1,
                                                          (C.c_void_p * 1)(cloud.d_normals), None, None, valid, dropped)
    assert st == _abi.A3D_OK and valid[0] == expected[3].sum() > 0.9 * len(points) and dropped[0] == 0
    got_points, got = cloud.download()
    assert np.array_equal(_bits(got_points), _bits(points))
    assert np.array_equal(_bits(got), _bits(expected[0]))
    ok = expected[3]
    assert ((got[ok] * old[ok]).sum(axis=1) >= 0).all()
    thin.free(), cloud.free()


def test_clouds_with_estimated_normals_align_like_the_oracle_and_enter_the_map(ctx):
    thinned = DevicePointCloud.voxel_downsample_many(_sample1_frames(ctx), 0.02)
    image_normals = [t.download()[1] for t in thinned]
    for t in thinned:  # drop the image normals: the clouds come as a lidar scan would
        ctx.free(t.d_normals)
        t.d_normals = None
    valid = DevicePointCloud.estimate_normals_many(thinned, 0.06, viewpoints=[None, Transform.eye()])
    target, source = thinned
    assert target.d_normals is not None and valid[0] > 0.95 * target.len() and valid[1] > 0.95 * source.len()
    tgt_p, tgt_n = target.download()
    src_p, src_n = source.download()
    ok = np.linalg.norm(tgt_n, axis=1) > 0.5
    cos = (tgt_n[ok] * image_normals[0][ok]).sum(axis=1)
    print(f"median angle between estimated and image normals: {np.degrees(np.arccos(np.clip(np.median(cos), -1, 1))):.2f} deg")
    # (no gate on the angle: a pixel-grid normal of an unfiltered depth image is noisy at the scale of a pixel, the
    # estimate averages over 6 cm.)  The same side of the surface as the camera saw:
    assert np.mean(cos > 0) > 0.6
    prm = IcpParams.default()
    icp = Icp.new(ctx, prm, target)
    T_gpu = icp.align(source)
    tree = O.KdTree(tgt_p)
    out = PoseC()
    tv, sv = O.pcl_view(tgt_p, tgt_n), O.pcl_view(src_p, src_n)
    p = prm.to_c()
    assert O.load().orc_pcl_icp_align(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(out), None) == 0
    ang, tr = transform_diff(T_gpu, out)
    print(f"[frame 1 against frame 0, estimated normals, {target.len()} / {source.len()} points] d_angle={ang:.3e} d_trans={tr:.3e}")
    assert ang <= 1e-4 and tr <= 1e-4
    assert np.linalg.norm(T_gpu.t) < 0.1  # a frame's worth of motion
    vmap = DeviceVoxelMap(ctx, 0.02, normals=True)
    assert vmap.insert(target) == 0 and vmap.cells() == target.len()
    icp.free(), vmap.free()
    for t in thinned:
        t.free()


def test_python_wrappers_allocate_overwrite_and_free(ctx):
    points = _cube(61, 800, side=0.3)
    expected = R.estimate_normals(points, 0.05, viewpoint=(1.0, 2.0, 3.0))
    cloud = _device_cloud(ctx, points)
    assert cloud.d_normals is None
    valid, curvature, counts = cloud.estimate_normals(0.05, viewpoint=(1.0, 2.0, 3.0), curvature=True, counts=True)
    assert cloud.d_normals is not None and valid == expected[3].sum()
    assert np.array_equal(_bits(cloud.download()[1]), _bits(expected[0]))
    assert np.array_equal(_bits(curvature), _bits(expected[1])) and np.array_equal(counts, expected[2])
    # overwrite: the same buffer, new contents; a Transform gives its translation as the viewpoint
    before = cloud.d_normals.value if hasattr(cloud.d_normals, "value") else cloud.d_normals
    pose = Transform(t=(-1.0, 0.5, -2.0), q=(0.0, 0.6, 0.0, 0.8))
    assert cloud.estimate_normals(0.05, viewpoint=pose, min_neighbors=5) == R.estimate_normals(points, 0.05, 5)[3].sum()
    after = cloud.d_normals.value if hasattr(cloud.d_normals, "value") else cloud.d_normals
    assert before == after
    want = R.estimate_normals(points, 0.05, 5, viewpoint=(-1.0, 0.5, -2.0))
    assert np.array_equal(_bits(cloud.download()[1]), _bits(want[0]))
    # orient="normals" keeps each valid row on the side it was
    assert cloud.estimate_normals(0.05, orient="normals") == expected[3].sum()
    again = R.estimate_normals(points, 0.05, old_normals=want[0])
    assert np.array_equal(_bits(cloud.download()[1]), _bits(again[0]))
    bare = _device_cloud(ctx, points)
    with pytest.raises(A3dError):
        bare.estimate_normals(0.05, orient="normals")
    assert bare.d_normals is None
    with pytest.raises(A3dError):
        bare.estimate_normals(-1.0)
    assert bare.d_normals is None  # a failed call leaves the cloud without normals
    empty = _device_cloud(ctx, np.empty((0, 3), np.float32))
    assert DevicePointCloud.estimate_normals_many([bare, empty], 0.05, counts=True)[0] == [expected_origin_valid(points), 0]
    hostile = _device_cloud(ctx, np.r_[points[:100], _raw_bits(62, 20)])
    n_valid, n_dropped = hostile.estimate_normals(0.05, dropped=True)
    assert n_dropped == (~R.cells(np.r_[points[:100], _raw_bits(62, 20)], 0.05)[0]).sum() > 10
    hostile.free()
    for x in (cloud, bare, empty):
        x.free()
        assert x.d_points is None and x.d_normals is None


def expected_origin_valid(points):
    return int(R.estimate_normals(points, 0.05)[3].sum())
