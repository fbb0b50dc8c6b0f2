"""&Transform * &PointCloud (src/pointcloud.rs:40-52 over Transform::transform_vectors / transform_normals,
src/transform.rs:164-187) on resident clouds: DevicePointCloud.transformed / transform_ / transform_many / merge and
Transform * DevicePointCloud (a3d_point_clouds_transform_device / a3d_point_clouds_merge_device).

Every comparison is on uint32 views, bit for bit, and the expected value is always the oracle's orc_transform_points /
orc_transform_normals under the same pose (the same f32 expression, neither side contracted) — never the code under test.
No tolerance is involved except where the reference's own test states one (1e-5, transform.rs:364-388)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (A3dError, DevicePointCloud, Icp, IcpBatch, IcpParams, InvalidParameter, PointCloud,
                         RangeImageBuilder, SlamTbDataset, Transform, TrajectoryBuilder, _abi)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 270213, 500000)
CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle(pose_c, points, normals):
    """(orc_transform_points, orc_transform_normals or None) of host arrays under a PoseC."""
    out_p = O.transform_points(pose_c, points)
    if normals is None:
        return out_p, None
    normals = np.ascontiguousarray(normals, np.float32)
    out_n = np.empty_like(normals)
    O.load().orc_transform_normals(C.byref(pose_c), _abi.ptr(normals), normals.size // 3, _abi.ptr(out_n))
    return out_p, out_n


def _finite(seed, n):
    """[n, 3] seeded finite f32: magnitudes 1e-30 .. 1e30 of both signs, +-0.0 and a few subnormals."""
    rng = np.random.default_rng(seed)
    a = (rng.choice([-1.0, 1.0], size=(n, 3)) * 10.0 ** rng.uniform(-30, 30, size=(n, 3))).astype(np.float32)
    flat = a.reshape(-1)
    specials = np.asarray([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.17549421e-38], np.float32)
    idx = rng.choice(flat.size, size=min(flat.size, 2 * specials.size), replace=False)
    flat[idx] = specials[np.arange(idx.size) % specials.size]
    assert np.isfinite(a).all()
    return a


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the _synthetic recipe of test_gpu_point_cloud_from_image.py): NaNs with payloads,
    infinities, -0.0 and denormals all occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _unit_quaternion(rng):
    q = rng.normal(size=4).astype(np.float32)
    return q / np.float32(np.sqrt(np.float32(np.sum(q * q))))


def _y_pi_pose():
    """The pose of the reference's test_mul_op (transform.rs:332-335): a rotation of pi about y, translation (0, 0, 3)."""
    p = O.exp_se3([0, 0, 0, 0, np.float32(np.pi), 0])
    p.t[:] = [0.0, 0.0, 3.0]
    return Transform.from_c(p)


def _poses(seed, n_random=2):
    rng = np.random.default_rng(seed)
    out = [Transform.eye(), _y_pi_pose()]
    out += [Transform(rng.uniform(-3, 3, size=3), _unit_quaternion(rng)) for _ in range(n_random)]
    out.append(Transform((1.0, -2.0, 0.5), (0.3, -1.2, 2.0, 0.7)))  # deliberately not a unit quaternion: used as given
    return out


def _device_cloud(ctx, points, normals=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals))


def _assert_cloud_bits(dc, points, normals):
    got_p, got_n = dc.download()
    assert dc.len() == len(points)
    assert np.array_equal(_bits(got_p), _bits(points))
    if normals is None:
        assert got_n is None and dc.d_normals is None
    else:
        assert got_n is not None and np.array_equal(_bits(got_n), _bits(normals))


def _sample1_clouds(ctx, n_frames):
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(n_frames)]
    cam, _, _, depth_scale = frames[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(
        cam, [(f[1], f[2]) for f in frames], depth_scale)
    images = [pyramid[0] for pyramid in built]
    clouds = DevicePointCloud.from_range_images(images)
    for im in images:
        im.free()
    return clouds


@pytest.mark.parametrize("with_normals", [True, False])
def test_bit_identity_with_the_oracle(ctx, with_normals):
    for k, n in enumerate(SIZES):
        points = _finite(1000 + k, n)
        normals = _finite(2000 + k, n) if with_normals else None
        dc = _device_cloud(ctx, points, normals)
        for T in _poses(3000 + k):
            exp_p, exp_n = _oracle(T.to_c(), points, normals)
            out = T * dc  # Transform.__mul__ -> DevicePointCloud.transformed
            assert isinstance(out, DevicePointCloud) and out is not dc
            _assert_cloud_bits(out, exp_p, exp_n)
            out.free()
        _assert_cloud_bits(dc, points, normals)  # the input is untouched
        dc.free()


def test_reference_known_answers(ctx):
    # transform.rs:364-388: exp([1,2,3,.4,.5,.3]) applied to (5.5, 6.4, 7.8), within the reference's 1e-5
    T = Transform.from_c(O.exp_se3([1.0, 2.0, 3.0, 0.4, 0.5, 0.3]))
    dc = _device_cloud(ctx, np.asarray([[5.5, 6.4, 7.8], [1.0, 2.0, 3.0]], np.float32))
    out = T * dc
    got = out.download()[0]
    assert np.linalg.norm(got[0].astype(np.float64) - [8.9848175, 6.9635687, 9.880962]) < 1e-5
    assert np.linalg.norm(got[1].astype(np.float64) - [3.5280778, 2.8378963, 5.8994026]) < 1e-5
    out.free()
    # transform.rs:321-346 (test_mul_op): the identity returns the points; pi about y then (0, 0, 3) takes (1, 2, 3) to
    # (-1, 2, 0) (cos(f32(pi) / 2) = -4.4e-8 instead of 0 moves the result by ~3e-7: inside the same 1e-5)
    ident = Transform.eye() * dc
    assert np.array_equal(_bits(ident.download()[0]), _bits(dc.download()[0]))
    out = _y_pi_pose() * dc
    assert np.linalg.norm(out.download()[0][1].astype(np.float64) - [-1.0, 2.0, 0.0]) < 1e-5
    for x in (ident, out, dc):
        x.free()


def test_non_finite_inputs(ctx):
    for k, n in enumerate((65, 2049, 100003)):
        points, normals = _raw_bits(4000 + k, n), _raw_bits(5000 + k, n)
        assert np.isnan(points).any() and np.isinf(points).any()
        dc = _device_cloud(ctx, points, normals)
        for T in _poses(6000 + k, n_random=1):
            exp = _oracle(T.to_c(), points, normals)
            out = dc.transformed(T)
            for got, want in zip(out.download(), exp):
                # NaN exactly where the oracle has NaN (payload and sign of a computed NaN differ between x86 and the GPU
                # by design and are not compared), the same bits everywhere else
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan)
                assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
            out.free()
        # without poses every bit survives, NaN payloads included: the raw call and merge(transforms=None)
        out = DevicePointCloud._allocate(ctx, n, True)
        v = dc.view()
        st = ctx.lib.a3d_point_clouds_transform_device(ctx.handle, C.byref(v), None, 1, (C.c_void_p * 1)(out.d_points),
                                                       (C.c_void_p * 1)(out.d_normals))
        assert st == _abi.A3D_OK
        _assert_cloud_bits(out, points, normals)
        copy = DevicePointCloud.merge([dc])
        _assert_cloud_bits(copy, points, normals)
        for x in (out, copy, dc):
            x.free()


def _guarded(ctx, n_points):
    """A device buffer of n_points points with CANARY_WORDS canary words before and after: (base, pointer to the points)."""
    words = np.full(2 * CANARY_WORDS + 3 * n_points, CANARY, np.uint32)
    base = ctx.to_device(words)
    return base, C.c_void_p(base.value + 4 * CANARY_WORDS)


def _read_guarded(ctx, base, n_points):
    words = ctx.to_host(base, np.empty(2 * CANARY_WORDS + 3 * n_points, np.uint32))
    body = words[CANARY_WORDS:CANARY_WORDS + 3 * n_points].view(np.float32).reshape(-1, 3)
    return words[:CANARY_WORDS], body, words[CANARY_WORDS + 3 * n_points:]


def test_batch_equals_single_calls_and_writes_nothing_else(ctx):
    sizes = (1, 64, 0, 2049, 77, 270213, 4096, 65, 100001)
    rng = np.random.default_rng(77)
    hosts = [(_finite(7000 + i, n), _finite(7100 + i, n) if i % 3 else None) for i, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    poses = [Transform(rng.uniform(-2, 2, size=3), _unit_quaternion(rng)) for _ in sizes]
    assert len({tuple(T.q.tolist() + T.t.tolist()) for T in poses}) == len(sizes)
    # the Python batch form: one ABI call; each result is the single-cloud result and the oracle's
    batch = DevicePointCloud.transform_many(clouds, poses)
    assert len(batch) == len(clouds)
    for dc, (p, nrm), T, got in zip(clouds, hosts, poses, batch):
        exp_p, exp_n = _oracle(T.to_c(), p, nrm)
        _assert_cloud_bits(got, exp_p, exp_n)
        single = dc.transformed(T)
        _assert_cloud_bits(single, exp_p, exp_n)
        single.free()
    # the raw call into buffers with canary words on both sides of every output
    n = len(clouds)
    g_points = [_guarded(ctx, s) for s in sizes]
    g_normals = [_guarded(ctx, s) if nrm is not None else None for s, (_, nrm) in zip(sizes, hosts)]
    views = (_abi.PointCloudViewC * n)(*[c.view() for c in clouds])
    st = ctx.lib.a3d_point_clouds_transform_device(
        ctx.handle, views, (_abi.PoseC * n)(*[T.to_c() for T in poses]), n,
        (C.c_void_p * n)(*[g[1] for g in g_points]), (C.c_void_p * n)(*[g[1] if g else None for g in g_normals]))
    assert st == _abi.A3D_OK
    for s, (p, nrm), T, gp, gn in zip(sizes, hosts, poses, g_points, g_normals):
        exp_p, exp_n = _oracle(T.to_c(), p, nrm)
        for g, want in ((gp, exp_p), (gn, exp_n)):
            if g is None:
                continue
            before, body, after = _read_guarded(ctx, g[0], s)
            assert (before == CANARY).all() and (after == CANARY).all()
            assert np.array_equal(_bits(body), _bits(want))
            ctx.free(g[0])
    # an output normals entry for a cloud without normals: A3D_MISSING_FIELD
    i = next(k for k, (_, nrm) in enumerate(hosts) if nrm is None and sizes[k] > 0)
    v = clouds[i].view()
    st = ctx.lib.a3d_point_clouds_transform_device(ctx.handle, C.byref(v), None, 1, (C.c_void_p * 1)(batch[i].d_points),
                                                   (C.c_void_p * 1)(batch[i].d_points))
    assert st == _abi.A3D_MISSING_FIELD
    for x in (*clouds, *batch):
        x.free()


def test_in_place_and_overlap_rules(ctx):
    n = 70001
    points, normals = _finite(8000, n), _finite(8001, n)
    T = _poses(8002)[2]
    exp_p, exp_n = _oracle(T.to_c(), points, normals)
    a, b = _device_cloud(ctx, points, normals), _device_cloud(ctx, points, normals)
    out = a.transformed(T)
    assert b.transform_(T) is b
    _assert_cloud_bits(out, exp_p, exp_n)
    _assert_cloud_bits(b, exp_p, exp_n)
    # an output that partially overlaps its input (input + one point): refused, nothing written
    room = np.concatenate([points, np.zeros((1, 3), np.float32)])
    d_room = ctx.to_device(room)
    view = _abi.PointCloudViewC()
    view.points, view.normals, view.len = d_room, None, n
    pose = T.to_c()

    def call(views, count, outs_points, outs_normals=None):
        return ctx.lib.a3d_point_clouds_transform_device(ctx.handle, views, (_abi.PoseC * count)(*[pose] * count), count,
                                                         outs_points, outs_normals)

    st = call(C.byref(view), 1, (C.c_void_p * 1)(d_room.value + 12))
    assert st == _abi.A3D_INVALID_PARAMETER
    assert np.array_equal(_bits(ctx.to_host(d_room, np.empty_like(room))), _bits(room))
    # output 0 on input 1, two outputs on one buffer, points written over the normals that are being read
    two = (_abi.PointCloudViewC * 2)(a.view(), out.view())
    assert call(two, 2, (C.c_void_p * 2)(out.d_points, b.d_points)) == _abi.A3D_INVALID_PARAMETER
    assert call(two, 2, (C.c_void_p * 2)(b.d_points, b.d_points)) == _abi.A3D_INVALID_PARAMETER
    va = a.view()
    st = call(C.byref(va), 1, (C.c_void_p * 1)(a.d_normals), (C.c_void_p * 1)(b.d_normals))
    assert st == _abi.A3D_INVALID_PARAMETER
    _assert_cloud_bits(a, points, normals)
    _assert_cloud_bits(out, exp_p, exp_n)
    _assert_cloud_bits(b, exp_p, exp_n)
    # exactly in place through the raw call is allowed, points on points and normals on normals
    assert call(C.byref(va), 1, (C.c_void_p * 1)(a.d_points), (C.c_void_p * 1)(a.d_normals)) == _abi.A3D_OK
    _assert_cloud_bits(a, exp_p, exp_n)
    ctx.free(d_room)
    for x in (a, b, out):
        x.free()


def test_merge(ctx):
    sizes = (2049, 0, 64, 100001, 1)
    rng = np.random.default_rng(91)
    hosts = [(_finite(9000 + i, n), _finite(9100 + i, n)) for i, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    poses = [Transform(rng.uniform(-2, 2, size=3), _unit_quaternion(rng)) for _ in sizes]
    total = sum(sizes)
    expected = [_oracle(T.to_c(), p, nrm) for (p, nrm), T in zip(hosts, poses)]
    merged = DevicePointCloud.merge(clouds, poses)
    assert merged.len() == total
    _assert_cloud_bits(merged, np.concatenate([e[0] for e in expected]), np.concatenate([e[1] for e in expected]))
    # transforms=None: the concatenation of the downloads, bit for bit
    plain = DevicePointCloud.merge(clouds)
    downloads = [c.download() for c in clouds]
    _assert_cloud_bits(plain, np.concatenate([d[0] for d in downloads]), np.concatenate([d[1] for d in downloads]))
    # capacity = total - 1: refused, *out_len = total, the output as it was
    sentinel = np.full((total, 3), np.float32(-7.25))
    d_out = ctx.to_device(sentinel)
    n = len(clouds)
    views = (_abi.PointCloudViewC * n)(*[c.view() for c in clouds])
    pose_arr = (_abi.PoseC * n)(*[T.to_c() for T in poses])
    n_out = C.c_uint64(0)
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, views, pose_arr, n, d_out, None, total - 1, C.byref(n_out))
    assert st == _abi.A3D_INVALID_PARAMETER and n_out.value == total
    assert np.array_equal(ctx.to_host(d_out, np.empty_like(sentinel)), sentinel)
    # exactly enough is enough
    n_out = C.c_uint64(0)
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, views, pose_arr, n, d_out, None, total, C.byref(n_out))
    assert st == _abi.A3D_OK and n_out.value == total
    assert np.array_equal(_bits(ctx.to_host(d_out, np.empty_like(sentinel))), _bits(np.concatenate([e[0] for e in expected])))
    # the output may overlap no input
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, views, pose_arr, n, clouds[0].d_points, None, total, C.byref(n_out))
    assert st == _abi.A3D_INVALID_PARAMETER
    _assert_cloud_bits(clouds[0], *hosts[0])
    ctx.free(d_out)
    # mixed normals: A3D_MISSING_FIELD from the call, InvalidParameter from merge(); normals=False gives the points only
    bare = _device_cloud(ctx, hosts[2][0], None)
    mixed = [clouds[0], bare, clouds[3]]
    mviews = (_abi.PointCloudViewC * 3)(*[c.view() for c in mixed])
    mtotal = sum(c.len() for c in mixed)
    d_p, d_n = ctx.malloc(mtotal * 12), ctx.malloc(mtotal * 12)
    n_out = C.c_uint64(5)
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, mviews, None, 3, d_p, d_n, mtotal, C.byref(n_out))
    assert st == _abi.A3D_MISSING_FIELD
    ctx.free(d_p), ctx.free(d_n)
    with pytest.raises(InvalidParameter):
        DevicePointCloud.merge(mixed)
    with pytest.raises(A3dError) as e:
        DevicePointCloud.merge(mixed, normals=True)
    assert e.value.status == _abi.A3D_MISSING_FIELD
    points_only = DevicePointCloud.merge(mixed, [poses[0], poses[2], poses[3]], normals=False)
    _assert_cloud_bits(points_only, np.concatenate([expected[0][0], expected[2][0], expected[3][0]]), None)
    for x in (merged, plain, bare, points_only, *clouds):
        x.free()


def test_merged_cloud_is_an_icp_target(ctx):
    clouds = _sample1_clouds(ctx, 3)
    poses = [Transform.eye(), Transform((0.01, 0.0, -0.02), (0.0, 0.0, 0.0, 1.0)),
             Transform.from_c(O.exp_se3([0.02, -0.01, 0.0, 0.0, 0.01, 0.0]))]
    world = DevicePointCloud.transform_many(clouds, poses)
    merged = DevicePointCloud.merge(clouds, poses)
    assert merged.len() == sum(c.len() for c in clouds) and merged.d_normals is not None
    prm = IcpParams(max_iterations=3)
    icp = Icp(ctx, prm, merged)
    T = icp.align(world[1])  # raises unless the status is A3D_OK
    assert np.isfinite(T.t).all() and np.isfinite(T.q).all()
    batch = IcpBatch(ctx, prm, [merged])
    _, status = batch.align([world[1]])
    assert status[0] == 0
    icp.free(), batch.free()
    for x in (merged, *world, *clouds):
        x.free()


def test_frames_to_map_on_the_device(ctx):
    """The chain the feature exists for: build_many -> from_range_images -> IcpBatch.align -> TrajectoryBuilder ->
    merge(clouds, camera_to_world), against the oracle applied to each downloaded cloud under the same pose."""
    clouds = _sample1_clouds(ctx, 6)
    batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
    poses, status = batch.align(clouds[1:])
    traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
    camera_to_world = [traj.current_camera_to_world()]
    for k, (now_to_previous, st) in enumerate(zip(poses, status)):
        if st == 0:  # (a pair that failed keeps the previous pose, as examples/pcl_map.py does)
            traj.accumulate(now_to_previous, float(k + 1))
        camera_to_world.append(traj.current_camera_to_world())
    assert len(camera_to_world) == len(clouds) == 6
    merged = DevicePointCloud.merge(clouds, camera_to_world)
    expected = [_oracle(T.to_c(), *c.download()) for c, T in zip(clouds, camera_to_world)]
    assert merged.len() == sum(c.len() for c in clouds) > 6 * 100000
    _assert_cloud_bits(merged, np.concatenate([e[0] for e in expected]), np.concatenate([e[1] for e in expected]))
    batch.free()
    for x in (merged, *clouds):
        x.free()


def test_seeding_kdtree_icp_with_a_prior(ctx):
    clouds = _sample1_clouds(ctx, 2)
    prm = IcpParams.default()
    batch = IcpBatch(ctx, prm, [clouds[0]])
    (T,), status = batch.align([clouds[1]])
    assert status[0] == 0
    seeded = T * clouds[1]
    _assert_cloud_bits(seeded, *_oracle(T.to_c(), *clouds[1].download()))
    icp = Icp(ctx, prm, clouds[0])
    correction = icp.align(seeded)  # raises unless the status is A3D_OK
    # the size of the residual correction is reported, not asserted (nothing derives it)
    print(f"seeded Icp: residual correction angle {correction.angle():.3e} rad, "
          f"translation {float(np.linalg.norm(correction.t)):.3e}")
    icp.free(), batch.free()
    for x in (seeded, *clouds):
        x.free()
