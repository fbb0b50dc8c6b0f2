"""Voxel-grid downsampling of resident clouds (a3d_point_clouds_voxel_downsample_device, DevicePointCloud.voxel_downsample
/ voxel_downsample_many) on the GPU.

Every comparison is on uint32 views, bit for bit, and the expected value is always the numpy restatement of the
definition (voxel_restatement.py), never the code under test.  The raw call writes into buffers that are filled with a
canary word from end to end, with CANARY_WORDS more of it on both sides: whatever the call did not have to write must
still hold it.  The one tolerance (the pose of an alignment against a downsampled map, against the oracle's ICP on the
same host arrays) is the 1e-4 / 1e-4 of test_gpu_pcl_icp.py."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import voxel_restatement as V
from align3d_amd import (A3dError, Context, DevicePointCloud, Icp, IcpBatch, IcpParams, InvalidParameter, PointCloud,
                         RangeImageBuilder, SlamTbDataset, Transform, TrajectoryBuilder, _abi)
from align3d_amd._abi import PoseC
from gpu_util import transform_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 63, 64, 65, 2047, 2049, 270213)
VOXELS = (0.005, 0.02, 0.1, 1e3, 1e-5)  # 1e3: everything in one voxel; 1e-5: every point of a small cloud alone
ORIGINS = (None, (0.013, -0.4, 7.5))
CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)
MAP_FRAMES = 8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uniform(seed, n, with_normals=True):
    """([n, 3] seeded points in the 3 m cube [0.25, 3.25)^3, [n, 3] unit-free 'normals' or None).  The cube lies inside
    one cell of a 1e3 grid under both ORIGINS (under the second one at negative cell coordinates)."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(0.25, 3.25, size=(n, 3)).astype(np.float32)
    normals = rng.normal(size=(n, 3)).astype(np.float32) if with_normals else None
    return points, normals


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the recipe of test_gpu_cloud_transform.py): NaNs with payloads, infinities, -0.0, denormals
    and magnitudes far beyond the 21-bit cell range all occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


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


def _call(ctx, clouds, voxel, origin, want_normals=True, want_index=True, capacities=None):
    """The raw call on resident clouds into guarded buffers.  Returns (status, lens, dropped, per cloud {points, normals,
    index: [capacity, width] uint32 bodies or None}); asserts the guards."""
    n = len(clouds)
    caps = [c.len() for c in clouds] if capacities is None else list(capacities)
    g_points = [_Guarded(ctx, k, 3) for k in caps]
    g_normals = [_Guarded(ctx, k, 3) if want_normals and c.d_normals is not None else None for c, k in zip(clouds, caps)]
    g_index = [_Guarded(ctx, k, 1) if want_index else None for k in caps]
    lens, dropped = (C.c_uint64 * n)(*[12345] * n), (C.c_uint64 * n)(*[12345] * n)
    o = None if origin is None else (C.c_float * 3)(*origin)
    views = (_abi.PointCloudViewC * n)(*[c.view() for c in clouds])
    st = ctx.lib.a3d_point_clouds_voxel_downsample_device(
        ctx.handle, views, n, voxel, o, (C.c_void_p * n)(*[g.ptr for g in g_points]),
        (C.c_void_p * n)(*[g.ptr if g else None for g in g_normals]) if want_normals else None,
        (C.c_void_p * n)(*[g.ptr for g in g_index]) if want_index else None, (C.c_uint64 * n)(*caps), lens, dropped)
    outs = []
    for gp, gn, gi in zip(g_points, g_normals, g_index):
        out = {}
        for name, g in (("points", gp), ("normals", gn), ("index", gi)):
            out[name] = None
            if g is not None:
                out[name], intact = g.read()
                assert intact, f"the call wrote outside its {name} buffer"
                g.free()
        outs.append(out)
    return st, list(lens), list(dropped), outs


def _assert_matches(out, got_len, got_dropped, points, normals, voxel, origin, expected=None):
    """One cloud's buffers against the restatement; everything behind the kept rows still holds the canary."""
    exp_p, exp_n, exp_i, exp_dropped = expected or V.voxel_downsample_cloud(points, normals, voxel, origin)
    m = len(exp_i)
    assert (got_len, got_dropped) == (m, exp_dropped)
    assert np.array_equal(out["points"][:m], _bits(exp_p).reshape(-1, 3))
    assert (out["points"][m:] == CANARY).all()
    if out["normals"] is not None:
        assert np.array_equal(out["normals"][:m], _bits(exp_n).reshape(-1, 3))
        assert (out["normals"][m:] == CANARY).all()
    if out["index"] is not None:
        assert np.array_equal(out["index"][:m, 0], exp_i)
        assert (out["index"][m:] == CANARY).all()


_world = {}


def _sample1_world(ctx):
    """MAP_FRAMES frames of sample1 as resident clouds, their odometry poses (IcpBatch over the consecutive pairs, as
    examples/pcl_map.py) and the merged map; built once per session."""
    if not _world:
        ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
        frames = [ds.get(i) for i in range(MAP_FRAMES)]
        cam, _, _, depth_scale = frames[0]
        built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(
            cam, [(f[1], f[2]) for f in frames], depth_scale)
        images = [pyramid[0] for pyramid in built]
        clouds = DevicePointCloud.from_range_images(images)
        for im in images:
            im.free()
        batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
        poses, status = batch.align(clouds[1:])
        batch.free()
        traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
        camera_to_world = [traj.current_camera_to_world()]
        for k, (now_to_previous, st) in enumerate(zip(poses, status)):
            if st == 0:
                traj.accumulate(now_to_previous, float(k + 1))
            camera_to_world.append(traj.current_camera_to_world())
        merged = DevicePointCloud.merge(clouds, camera_to_world)
        assert merged.len() == sum(c.len() for c in clouds) > MAP_FRAMES * 200000 and merged.d_normals is not None
        _world.update(clouds=clouds, poses=camera_to_world, merged=merged, host=merged.download())
    return _world


def test_size_and_parameter_grid(ctx):
    for k, n in enumerate(SIZES):
        points, normals = _uniform(100 + k, n)
        with_n, without_n = _device_cloud(ctx, points, normals), _device_cloud(ctx, points, None)
        for voxel in VOXELS:
            for origin in ORIGINS:
                expected = V.voxel_downsample_cloud(points, normals, voxel, origin)
                if voxel == 1e3 and n:
                    assert len(expected[2]) == 1
                if voxel == 1e-5 and n == 2047:
                    assert len(expected[2]) == n  # every point alone
                if voxel == 0.1 and n == 270213:
                    assert 20000 < len(expected[2]) <= 31 ** 3  # a 3 m cube touches 30 or 31 cells per axis: ~10 points each
                for cloud, nrm in ((with_n, normals), (without_n, None)):
                    for want_index in (True, False):
                        st, lens, dropped, outs = _call(ctx, [cloud], voxel, origin, want_index=want_index)
                        assert st == _abi.A3D_OK, (n, voxel, origin)
                        assert (outs[0]["normals"] is None) == (nrm is None) and (outs[0]["index"] is None) == (not want_index)
                        _assert_matches(outs[0], lens[0], dropped[0], points, nrm, voxel, origin, expected)
        with_n.free(), without_n.free()


def test_cloud_of_more_chunks_than_tiles(ctx):
    # the smallest cloud whose tiles hold two chunks: 4096 * 1024 + 1 points are 4097 chunks of 1024, above the 4096 tiles a
    # cloud may have, so 2049 tiles of 2 chunks, the last of them with one point
    points, _ = _uniform(150, 4096 * 1024 + 1, with_normals=False)
    cloud = _device_cloud(ctx, points, None)
    st, lens, dropped, outs = _call(ctx, [cloud], 0.02, None)
    assert st == _abi.A3D_OK and outs[0]["normals"] is None and outs[0]["index"] is not None
    _assert_matches(outs[0], lens[0], dropped[0], points, None, 0.02, None)
    cloud.free()


def test_merged_map_of_fixture_frames(ctx):
    w = _sample1_world(ctx)
    points, normals = w["host"]
    for voxel in VOXELS:
        for origin in ORIGINS:
            expected = V.voxel_downsample_cloud(points, normals, voxel, origin)
            if voxel == 0.02:
                assert len(expected[2]) < len(points) // 4  # eight frames of one scene: mostly duplicates
            st, lens, dropped, outs = _call(ctx, [w["merged"]], voxel, origin)
            assert st == _abi.A3D_OK
            _assert_matches(outs[0], lens[0], dropped[0], points, normals, voxel, origin, expected)
    # without normals and without the index, once
    st, lens, dropped, outs = _call(ctx, [w["merged"]], 0.02, None, want_normals=False, want_index=False)
    assert st == _abi.A3D_OK and outs[0]["normals"] is None and outs[0]["index"] is None
    _assert_matches(outs[0], lens[0], dropped[0], points, None, 0.02, None)


def test_hostile_bit_patterns_exercise_the_drop_rule(ctx):
    for k, n in enumerate((65, 2049, 100003)):
        points, normals = _raw_bits(4000 + k, n), _raw_bits(5000 + k, n)
        assert np.isnan(points).any() and np.isinf(points).any()
        cloud = _device_cloud(ctx, points, normals)
        for voxel, origin in ((0.02, None), (1e3, (0.5, -2.0, 1e-3)), (1e25, None), (3e37, (-1e30, 1e30, 0.0)), (1e-40, None)):
            expected = V.voxel_downsample_cloud(points, normals, voxel, origin)
            if n == 100003:  # points are dropped and points are kept; under the huge cells some distances are +inf
                kept, _, dist = V.voxel_keys(points, voxel, origin)
                assert expected[3] > 0 and len(expected[2]) > 0 and (voxel < 1e20 or np.isinf(dist[kept]).any())
            st, lens, dropped, outs = _call(ctx, [cloud], voxel, origin)
            assert st == _abi.A3D_OK
            _assert_matches(outs[0], lens[0], dropped[0], points, normals, voxel, origin, expected)
        cloud.free()


def test_exact_duplicates_keep_the_lowest_index(ctx):
    rng = np.random.default_rng(61)
    base, _ = _uniform(60, 5000, with_normals=False)
    pick = rng.integers(0, len(base), size=40000)
    points = base[pick]
    normals = rng.normal(size=points.shape).astype(np.float32)  # the copies differ in their normals only
    exp_p, exp_n, exp_i, _ = expected = V.voxel_downsample_cloud(points, normals, 0.05)
    # on the host: every kept row is the FIRST copy of its point
    first_copy = {}
    for i, b in enumerate(pick):
        first_copy.setdefault(int(b), i)
    assert all(first_copy[int(pick[i])] == int(i) for i in exp_i) and len(exp_i) < len(base)
    cloud = _device_cloud(ctx, points, normals)
    st, lens, dropped, outs = _call(ctx, [cloud], 0.05, None)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], lens[0], dropped[0], points, normals, 0.05, None, expected)
    cloud.free()


def test_equal_distances_faces_negative_coordinates_and_minus_zero(ctx):
    v = np.float32(0.25)  # a power of two: cell centres and the offsets below are exact in f32
    rng = np.random.default_rng(62)
    cells = rng.integers(-40, 40, size=(3000, 3)).astype(np.float32)
    centre = (cells + np.float32(0.5)) * v
    delta = (rng.integers(1, 120, size=(3000, 3)) / 1024.0).astype(np.float32)  # < v / 2
    mirrored = np.empty((6000, 3), np.float32)
    mirrored[0::2], mirrored[1::2] = centre + delta, centre - delta
    mirrored = mirrored[rng.permutation(6000)]
    _, key, dist = V.voxel_keys(mirrored, v)
    order = np.lexsort((dist, key))
    same = key[order][1:] == key[order][:-1]
    assert (dist[order][1:][same] == dist[order][:-1][same]).sum() >= 2500  # pairs of one cell at one distance
    faces = (rng.integers(-40, 40, size=(3000, 3)).astype(np.float32) * v)  # on cell faces, edges and corners
    faces[::7] *= np.float32(-0.0)  # rows of -0.0 / +0.0
    assert np.signbit(faces).any() and (faces == 0).any()
    points = np.concatenate([mirrored, faces, -mirrored[:100], np.zeros((3, 3), np.float32), -np.zeros((3, 3), np.float32)])
    cloud = _device_cloud(ctx, points, None)
    for origin in (None, (0.125, -0.25, 0.0625)):
        st, lens, dropped, outs = _call(ctx, [cloud], float(v), origin)
        assert st == _abi.A3D_OK
        _assert_matches(outs[0], lens[0], dropped[0], points, None, float(v), origin)
    cloud.free()


def test_order_independence(ctx):
    points, normals = _uniform(70, 50000)
    voxel = 0.1
    kept, key, dist = V.voxel_keys(points, voxel)
    assert kept.all()
    order = np.lexsort((dist, key))
    same = key[order][1:] == key[order][:-1]
    # on the host, before the GPU is touched: the minimal distance of every voxel is unique (a voxel's entries are sorted
    # by distance, so two equal neighbours anywhere in it would include a tie at its head)
    assert same.sum() > 20000 and not (dist[order][1:][same] == dist[order][:-1][same]).any()
    perm = np.random.default_rng(71).permutation(len(points))
    a, b = _device_cloud(ctx, points, normals), _device_cloud(ctx, points[perm], normals[perm])
    ra, ia = a.voxel_downsample(voxel, return_index=True)
    rb, ib = b.voxel_downsample(voxel, return_index=True)
    assert ra.len() == rb.len() == len(V.voxel_downsample(points, voxel)[0])
    assert np.array_equal(np.sort(perm[ib]), ia)  # the same input rows are kept

    def rows(dc):
        p, nrm = dc.download()
        r = np.concatenate([_bits(p), _bits(nrm)], axis=1)
        return r[np.lexsort(r.T[::-1])]

    assert np.array_equal(rows(ra), rows(rb))
    for x in (a, b, ra, rb):
        x.free()


def test_idempotence(ctx):
    for (points, normals), voxel, origin in ((_uniform(80, 270213), 0.02, (0.013, -0.4, 7.5)), (_uniform(81, 2049), 0.1, None)):
        cloud = _device_cloud(ctx, points, normals)
        once, index = cloud.voxel_downsample(voxel, origin, return_index=True)
        exp_p, exp_n, exp_i, _ = V.voxel_downsample_cloud(points, normals, voxel, origin)
        assert np.array_equal(index, exp_i) and index.dtype == np.uint32
        twice, index2 = once.voxel_downsample(voxel, origin, return_index=True)
        assert np.array_equal(index2, np.arange(once.len(), dtype=np.uint32))
        for dc in (once, twice):
            p, nrm = dc.download()
            assert dc.len() == len(exp_i) and np.array_equal(_bits(p), _bits(exp_p)) and np.array_equal(_bits(nrm), _bits(exp_n))
        for x in (cloud, once, twice):
            x.free()


def test_batch_equals_single_calls_and_runs_are_identical(ctx):
    sizes = (270213, 0, 2049, 65, 100001, 1, 0, 4096)
    hosts = [_uniform(900 + i, n, with_normals=i != 2) for i, n in enumerate(sizes)]
    assert hosts[2][1] is None
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    voxel, origin = 0.05, (0.5, 0.25, -0.125)
    runs = [_call(ctx, clouds, voxel, origin) for _ in range(2)]
    for st, lens, dropped, outs in runs:
        assert st == _abi.A3D_OK
        for out, got_len, got_dropped, (p, nrm) in zip(outs, lens, dropped, hosts):
            _assert_matches(out, got_len, got_dropped, p, nrm, voxel, origin)
    for a, b in zip(runs[0][3], runs[1][3]):
        for name in ("points", "normals", "index"):
            assert (a[name] is None and b[name] is None) or np.array_equal(a[name], b[name])
    # each cloud passed alone gives what it gave in the batch
    for i, cloud in enumerate(clouds):
        st, lens, dropped, outs = _call(ctx, [cloud], voxel, origin)
        assert st == _abi.A3D_OK and lens[0] == runs[0][1][i] and dropped[0] == runs[0][2][i]
        for name in ("points", "normals", "index"):
            assert (outs[0][name] is None and runs[0][3][i][name] is None) or np.array_equal(outs[0][name], runs[0][3][i][name])
    # the Python batch form: one call, a list, normals iff the input has them
    many = DevicePointCloud.voxel_downsample_many(clouds, voxel, origin)
    assert len(many) == len(clouds)
    for dc, (p, nrm) in zip(many, hosts):
        exp_p, exp_n, exp_i, _ = V.voxel_downsample_cloud(p, nrm, voxel, origin)
        got_p, got_n = dc.download()
        assert dc.len() == len(exp_i) and np.array_equal(_bits(got_p), _bits(exp_p))
        assert (got_n is None) == (nrm is None) == (dc.d_normals is None)
        if nrm is not None:
            assert np.array_equal(_bits(got_n), _bits(exp_n))
    # host clouds and mixed contexts are refused as _resident_batch refuses them
    with pytest.raises(TypeError):
        DevicePointCloud.voxel_downsample_many([clouds[0], PointCloud(hosts[3][0])], voxel)
    other = Context(0)
    foreign = _device_cloud(other, *hosts[3])
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample_many([clouds[0], foreign], voxel)
    foreign.free()
    other.close()
    with pytest.raises(A3dError) as e:
        clouds[0].voxel_downsample(-1.0)
    assert e.value.status == _abi.A3D_INVALID_PARAMETER
    for x in (*clouds, *many):
        x.free()


def test_capacity_one_short_writes_nothing_and_reports_every_count(ctx):
    sizes = (70001, 2049, 0, 30000)
    hosts = [_uniform(950 + i, n) for i, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    voxel = 0.1
    counts = [len(V.voxel_downsample(p, voxel)[0]) for p, _ in hosts]
    assert counts[1] > 1 and counts[2] == 0
    for short in (0, 1, 3):
        caps = list(counts)
        caps[short] -= 1
        st, lens, dropped, outs = _call(ctx, clouds, voxel, None, capacities=caps)
        assert st == _abi.A3D_INVALID_PARAMETER
        assert lens == counts and dropped == [0] * len(sizes)
        for out in outs:
            for name in ("points", "normals", "index"):
                assert (out[name] == CANARY).all(), name
    # exactly enough is enough
    st, lens, dropped, outs = _call(ctx, clouds, voxel, None, capacities=counts)
    assert st == _abi.A3D_OK and lens == counts
    for out, got_len, got_dropped, (p, nrm) in zip(outs, lens, dropped, hosts):
        _assert_matches(out, got_len, got_dropped, p, nrm, voxel, None)
    for x in clouds:
        x.free()


def test_downsampled_map_is_an_icp_target_and_agrees_with_the_oracle(ctx):
    w = _sample1_world(ctx)
    voxel = 0.02
    thin, index = w["merged"].voxel_downsample(voxel, return_index=True)
    map_p, map_n = thin.download()
    exp_p, exp_n, exp_i, exp_dropped = V.voxel_downsample_cloud(*w["host"], voxel)
    assert np.array_equal(index, exp_i) and np.array_equal(_bits(map_p), _bits(exp_p)) and np.array_equal(_bits(map_n), _bits(exp_n))
    assert np.isfinite(map_p).all()
    # frame to map: a fixture frame under its odometry pose against the thinned map
    k = MAP_FRAMES // 2
    source = w["poses"][k] * w["clouds"][k]
    src_p, src_n = source.download()
    prm = IcpParams(max_iterations=5)
    icp = Icp.new(ctx, prm, thin)  # the kd-tree builds over the downsampled cloud
    T_gpu = icp.align(source)      # raises unless the status is A3D_OK
    tree = O.KdTree(map_p)
    out = PoseC()
    tv, sv = O.pcl_view(map_p, map_n), O.pcl_view(src_p, src_n)
    p = prm.to_c()
    assert O.load().orc_pcl_icp_align(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(out), None) == 0
    ang, tr = transform_diff(T_gpu, out)
    print(f"[frame {k} against the map of {thin.len()} points (v = {voxel})] d_angle={ang:.3e} d_trans={tr:.3e}")
    assert ang <= 1e-4 and tr <= 1e-4
    batch = IcpBatch(ctx, prm, [thin])
    _, status = batch.align([source])
    assert status[0] == 0
    icp.free(), batch.free()
    for x in (thin, source):
        x.free()
