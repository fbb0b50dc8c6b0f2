"""Aligning against the TSDF volume on the GPU: DeviceTsdfVolume.sample / accumulate / align
(a3d_tsdf_volume_sample_device, a3d_tsdf_volume_icp_*).

Every expected value comes from tsdf_icp_restatement.py: the field query in numpy f32 on tsdf_restatement.Volume.tri, one
iteration from the oracle's bricks, the loop of pcl_icp.rs.  `sample` is compared bit for bit (uint32 views); an
accumulation by count and by gn_rel_err < 1e-6 against sums taken in f64 (the bound of test_gpu_voxel_map_icp.py for the
same engine); a pose within 1e-4 rad and 1e-4 m of the restatement's end-to-end run (the project's parity bound).  The
scene is the analytic one of test_tsdf_icp_cpu.py: a room corner and a sphere in a 32^3 volume at v = 0.05, set through
upload; the sources are prefixes of 5 000 points on those surfaces, moved by a small pose.  The edge cases live in 16^3
volumes whose voxel coordinates are exact in f32."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tsdf_icp_restatement as R
import tsdf_restatement as TS
from align3d_amd import (A3dError, CameraIntrinsics, DevicePointCloud, DeviceTsdfVolume, IcpParams, PointCloud, RangeImage,
                         Transform, _abi)
from gpu_util import gn_rel_err, small_pose, transform_diff
from voxel_map_icp_restatement import transform_normals

pytestmark = pytest.mark.gpu

F = np.float32
SOURCE_LENS = (1, 63, 64, 65, 257, 1025, 5000)


def _inverse(pose):
    out = _abi.PoseC()
    O.load().orc_inverse(C.byref(pose), C.byref(out))
    return out


def _moved(pose, points, normals):
    return O.transform_points(pose, points), transform_normals(pose, normals)


def _dev(ctx, points, normals=None):
    return DevicePointCloud(ctx, PointCloud(points, normals))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_sample(got, want, what=""):
    dist, nrm = got
    assert dist.dtype == nrm.dtype == F and nrm.shape == (len(dist), 3)
    bad = np.flatnonzero(_bits(dist) != _bits(want[0]))
    assert len(bad) == 0, (what, bad[:5], dist[bad[:5]], want[0][bad[:5]])
    bad = np.flatnonzero((_bits(nrm) != _bits(want[1])).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], nrm[bad[:5]], want[1][bad[:5]])


def _volume_of(ctx, restated):
    """The restated volume on the device, set through upload."""
    vol = DeviceTsdfVolume(ctx, (restated.nx, restated.ny, restated.nz), float(restated.v), restated.origin,
                           truncation=float(restated.tau))
    vol.upload(restated.D, restated.W)
    return vol


class _Scene:
    def __init__(self):
        self.field = R.FieldRestatement(R.corner_volume())
        # the source: points of the scene's surfaces, seen from a frame a small pose away
        self.offset = small_pose(7, rot=0.01, trans=0.01).to_c()
        self.src_p, self.src_n = _moved(_inverse(self.offset), *R.corner_surfaces(5, SOURCE_LENS[-1]))


@pytest.fixture(scope="module")
def scene():
    return _Scene()


@pytest.fixture(scope="module")
def volume(ctx, scene):
    vol = _volume_of(ctx, scene.field.volume)
    yield vol
    vol.free()


@pytest.fixture(scope="module")
def source(ctx, scene):
    """The resident sources: a prefix of the 5 000 points per length."""
    clouds = {m: _dev(ctx, scene.src_p[:m], scene.src_n[:m]) for m in SOURCE_LENS}
    yield clouds
    for c in clouds.values():
        c.free()


# ---- sample ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", SOURCE_LENS)
def test_sample_is_the_restatement_bit_for_bit(scene, volume, source, m):
    want = scene.field.sample(scene.src_p[:m])
    assert want[3].sum() >= min(m, 1) and (m < 1000 or want[3].sum() > 0.99 * m)
    _assert_sample(volume.sample(source[m]), want, "resident queries")
    _assert_sample(volume.sample(scene.src_p[:m]), want, "host queries")
    pose = O.exp_se3([0.02, -0.03, 0.01, 0.01, 0.02, -0.015])
    _assert_sample(volume.sample(source[m], Transform.from_c(pose)), scene.field.sample(scene.src_p[:m], pose), "under a pose")


def _edge_volume():
    """16^3 at v = 0.25 with a binary origin, tau = 0.75: q = origin + g v is exact in f32 for the g used here, and so is
    g back from q.  The base field is a plane through the volume, |D| <= 0.675; then the constructed spots."""
    vol = TS.Volume((16, 16, 16), 0.25, (0.5, -0.25, 0.125), 0.75, 64, False)
    k, j, i = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    vol.D[...] = (0.04 * (i - 7.5) + 0.02 * (j - 7.5) - 0.03 * (k - 7.5)).astype(F)
    vol.W[...] = 1
    vol.W[5, 5, 5] = 0                    # a hole
    vol.D[10, 10, 10] = -0.0              # -0 at a voxel whose upper neighbours are negative: D = -0 comes out
    for dk, dj, di in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)][1:]:
        vol.D[10 + dk, 10 + dj, 10 + di] = -0.25
    vol.D[2, 12, 12], vol.D[2, 12, 8] = 1.0, -1.0  # exactly at the truncation
    vol.D[1:7, 9:15, 1:6] = 0.5           # k 1..6, j 9..14, i 1..5: a locally constant field
    vol.D[12, 3, 12] = np.inf             # an uploaded +inf
    return vol


EDGE_QUERIES = {  # name: (g, value, direction)
    "plain": ((7.25, 6.5, 8.75), True, True),
    "hole at the centre": ((4.5, 4.5, 4.5), False, False),
    "hole in one gradient sample": ((3.5, 4.5, 4.5), True, False),
    "floor(g) = 0 on x": ((0.5, 4.5, 9.5), True, False),
    "floor(g) = 0 on z": ((7.5, 4.5, 0.25), True, False),
    "floor(g) + 1 = n - 1 on x": ((14.5, 7.5, 9.5), True, False),
    "floor(g) + 1 = n - 1 on y": ((7.5, 14.75, 9.5), True, False),
    "the last voxel itself": ((15.0, 7.5, 9.5), False, False),
    "outside": ((20.0, 7.5, 7.5), False, False),
    "below": ((7.5, -0.5, 7.5), False, False),
    "NaN": ((np.nan, 7.5, 7.5), False, False),
    "infinite": ((7.5, np.inf, 7.5), False, False),
    "minus infinite": ((7.5, 7.5, -np.inf), False, False),
    "D = 1": ((12.0, 12.0, 2.0), True, False),
    "D = -1": ((8.0, 12.0, 2.0), True, False),
    "D = -0": ((10.0, 10.0, 10.0), True, None),
    "constant field": ((3.5, 11.5, 3.5), True, False),
    "+inf at the centre": ((11.5, 2.5, 11.5), True, False),
    "+inf in one gradient sample": ((10.5, 2.5, 11.5), True, False),
}


def test_sample_at_constructed_edges(ctx):
    restated = _edge_volume()
    field = R.FieldRestatement(restated)
    g = np.asarray([case[0] for case in EDGE_QUERIES.values()], F)
    with np.errstate(invalid="ignore"):
        q = (restated.origin + g * restated.v).astype(F)
    d, n, value, direction = field.sample(q)
    for row, (name, (_, want_value, want_direction)) in enumerate(EDGE_QUERIES.items()):  # the cases are what they claim
        assert value[row] == want_value, name
        assert want_direction is None or direction[row] == want_direction, name
    names = list(EDGE_QUERIES)
    at = names.index
    assert d[at("D = 1")] == F(0.75) and d[at("D = -1")] == F(-0.75) and d[at("constant field")] == F(0.375)
    assert _bits(d)[at("D = -0")] == 0x80000000 and np.isposinf(d[at("+inf at the centre")])
    assert (_bits(d)[~value] == R.NAN_BITS).all() and not _bits(n)[~direction].any()
    vol = _volume_of(ctx, restated)
    _assert_sample(vol.sample(q), (d, n), "edges")
    # the same queries reached through a pose (a translation by a binary amount: still exact)
    shift = O.pose(t=(0.5, -0.25, 1.0))
    with np.errstate(invalid="ignore"):
        _assert_sample(vol.sample((q - F([0.5, -0.25, 1.0])).astype(F), Transform.from_c(shift)), (d, n), "edges, under a pose")
    vol.free()


# ---- accumulate -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", SOURCE_LENS)
def test_accumulate_is_the_restatements_iteration(scene, volume, source, m):
    prm = IcpParams(max_iterations=5)
    for name, T in (("eye", Transform.eye()), ("small pose", small_pose(2))):
        ref = scene.field.accumulate(scene.src_p[:m], scene.src_n[:m], T.to_c(), prm.to_c())
        gpu = volume.accumulate(source[m], prm, T)
        eh, eg, es = gn_rel_err(gpu, ref)
        print(f"accumulate m={m} {name}: count {gpu['count']} / {ref['count']}, rel err H {eh:.3g} g {eg:.3g} ssq {es:.3g}")
        assert gpu["count"] == ref["count"] and (m < 5000 or ref["count"] > 1000), (name, gpu["count"], ref["count"])
        assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (name, eh, eg, es)
    assert volume.accumulate(source[m], prm)["count"] == scene.field.accumulate(
        scene.src_p[:m], scene.src_n[:m], Transform.eye().to_c(), prm.to_c())["count"]  # pose=None is the identity


# ---- align ----------------------------------------------------------------------------------------------------------------


def _assert_pose(got, want, what):
    ang, tr = transform_diff(got, want)
    print(f"align {what}: d_angle {ang:.3g} rad, d_trans {tr:.3g} m")
    assert ang <= 1e-4 and tr <= 1e-4, (what, ang, tr)


@pytest.mark.parametrize("m", SOURCE_LENS)
@pytest.mark.parametrize("run", ["default x5", "weight 0.7 x3"])
def test_align_is_the_restatements_end_to_end_run(scene, volume, source, m, run):
    prm = IcpParams(max_iterations=5) if run == "default x5" else IcpParams(max_iterations=3, weight=0.7)
    status, want = scene.field.align(scene.src_p[:m], scene.src_n[:m], prm.to_c())
    try:
        got, got_status = volume.align(source[m], prm), _abi.A3D_OK
    except A3dError as e:
        got, got_status = None, e.status
    # (m = 1: one point gives a singular system, so the solve fails, here as there)
    assert got_status == status == (_abi.A3D_SOLVE_FAILED if m == 1 else _abi.A3D_OK), (m, got_status, status)
    if got is None:
        return
    _assert_pose(got, want, f"m={m} {run}")
    assert volume.last_device_ms() > 0.0
    if m == 5000:  # the alignment finds the pose the source was moved by
        ang, tr = transform_diff(got, scene.offset)
        print(f"align m={m} {run}: {ang:.3g} rad, {tr:.3g} m from the offset")
        assert ang < 2e-3 and tr < 2e-3, (ang, tr)


def test_align_starts_from_the_initial_pose(ctx, scene, volume, source):
    big = O.exp_se3([3.0, -2.0, 2.5, 0.3, -0.2, 0.25])
    initial = Transform.from_c(big)
    # no iteration: the initial pose comes back bit for bit (None: eye)
    for m in (1, 5000):
        assert bytes(volume.align(source[m], IcpParams(max_iterations=0), initial=initial).to_c()) == bytes(big)
        assert bytes(volume.align(source[m], IcpParams(max_iterations=0)).to_c()) == bytes(Transform.eye().to_c())
    # a source seen from a frame `big` away: aligned from `big`, it comes back as the restatement's run from `big` does
    far_p, far_n = _moved(_inverse(big), scene.src_p[:1025], scene.src_n[:1025])
    prm = IcpParams(max_iterations=5)
    status, want = scene.field.align(far_p, far_n, prm.to_c(), initial=big)
    assert status == _abi.A3D_OK
    cloud = _dev(ctx, far_p, far_n)
    got = volume.align(cloud, prm, initial=initial)
    _assert_pose(got, want, "from an initial pose")
    ang, tr = transform_diff(got, O.compose(scene.offset, big))
    assert ang < 2e-3 and tr < 2e-3, (ang, tr)
    assert not scene.field.sample(far_p)[2].any()  # from eye nothing lies inside the volume: no point has a value
    with pytest.raises(A3dError) as e:
        volume.align(cloud, prm)
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    cloud.free()


# ---- the gates at their edges ---------------------------------------------------------------------------------------------


def _plane_volume():
    """16^3 at v = 2^-4, origin 0, tau = 2^-2: D = clip((z - 0.5) / tau, -1, 1) = clip((k - 8) / 4, -1, 1), exact in f32.
    At x = y = 0.5 (g = 8: t = 0 on both axes) and z = 0.5 + e, 0 <= e < 2^-4: D = 4 e, d = e, G = (0, 0, 0.5), n = (0, 0, 1),
    every value exact."""
    vol = TS.Volume((16, 16, 16), 2.0 ** -4, (0.0, 0.0, 0.0), 0.25, 64, False)
    k = np.arange(16, dtype=np.float64)
    vol.D[...] = np.clip((k - 8.0) / 4.0, -1.0, 1.0).astype(F)[:, None, None]
    vol.W[...] = 1
    return vol


def test_gates_at_the_edge(ctx):
    """A point whose d2 equals max_distance^2 is kept (the reference rejects d2 > max_distance^2 only), one ulp beyond
    is not; and source normals whose dot product with n = (0, 0, 1) steps through the floats around the strict angle cut
    are kept or rejected as the reference's acos test does."""
    restated = _plane_volume()
    field = R.FieldRestatement(restated)
    vol = _volume_of(ctx, restated)
    up = np.asarray([[0.0, 0.0, 1.0]], F)
    reach = F(2.0 ** -5)
    prm = IcpParams(max_iterations=1, max_distance=float(reach))
    at = np.asarray([[0.5, 0.5, 0.5 + 2.0 ** -5]], F)
    beyond = at.copy()
    beyond[0, 2] = np.nextafter(at[0, 2], F(1.0))
    for q, count in ((at, 1), (beyond, 0)):
        d, n, value, direction = field.sample(q)
        assert direction[0] and n[0].tolist() == [0.0, 0.0, 1.0], "the field answers: the gate decides"
        d2 = F(d[0] * d[0])
        assert (d2 == reach * reach) == (q is at) and (d2 > reach * reach) == (q is not at)
        _assert_sample(vol.sample(q), (d, n))
        src = _dev(ctx, q, up)
        got = vol.accumulate(src, prm, Transform.eye())
        want = field.accumulate(q, up, Transform.eye().to_c(), prm.to_c())
        assert got["count"] == want["count"] == count, (q, got["count"], want["count"])
        if count:
            assert got["ssq"] == want["ssq"] == reach * reach
        src.free()
    # the strict angle gate: sn = (s, 0, c) with c the floats around the cut, so that sn . n == c exactly at the identity
    thr = F(IcpParams.default().max_normal_angle)
    cut = C.c_float()
    assert _abi.load_library(_abi.DIAG_LIB_PATH).a3d_acos_gate_threshold(thr, 1, C.byref(cut)) == 0
    c = np.asarray([cut.value], F).view(np.int32)[0] + np.arange(-20, 21, dtype=np.int32)
    c = c.view(F)
    assert (c > 0).all() and (c < 1).all()
    s = np.sqrt(1.0 - c.astype(np.float64) ** 2).astype(F)
    normals = np.stack([s, np.zeros_like(s), c], axis=1)
    col = np.arange(len(c))
    points = np.stack([0.25 + col * 2.0 ** -7, np.full(len(c), 0.5), np.full(len(c), 0.5 + 2.0 ** -6)], axis=1).astype(F)
    prm = IcpParams(max_iterations=1, max_normal_angle=float(thr))
    want = field.accumulate(points, normals, Transform.eye().to_c(), prm.to_c())
    rejects = O.acos_gate_rejects(c, prm.to_c().max_normal_angle, strict=True)
    assert 0 < rejects.sum() < len(c) and want["count"] == (~rejects).sum(), "both sides of the cut are exercised"
    src = _dev(ctx, points, normals)
    got = vol.accumulate(src, prm, Transform.eye())
    assert got["count"] == want["count"], (got["count"], want["count"])
    eh, eg, es = gn_rel_err(got, want)
    assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (eh, eg, es)
    src.free(), vol.free()


# ---- the volume is only read ----------------------------------------------------------------------------------------------


def _snapshot(vol):
    D, W, _ = vol.download()
    return D.tobytes(), W.tobytes()


def test_the_volume_is_unchanged(ctx, scene, volume, source):
    before = _snapshot(volume)
    prm = IcpParams(max_iterations=3)
    first = volume.align(source[1025], prm)
    volume.sample(source[1025]), volume.accumulate(source[1025], prm, Transform.eye())
    assert _snapshot(volume) == before
    assert bytes(volume.align(source[1025], prm).to_c()) == bytes(first.to_c())  # the same pose bits on a second run
    with pytest.raises(A3dError) as e:  # every point is gated out
        volume.align(source[1025], IcpParams(max_iterations=5, max_distance=1e-9))
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    bare = _dev(ctx, scene.src_p[:65])
    for call in (lambda: volume.align(bare, prm), lambda: volume.accumulate(bare, prm, Transform.eye())):
        with pytest.raises(A3dError) as e:  # a source without normals
            call()
        assert e.value.status == _abi.A3D_MISSING_FIELD
    bare.free()
    assert _snapshot(volume) == before
    # the other volume calls may follow: a fresh volume of the same contents, and this one after a clear and an upload
    # of the saved records, align to the same pose bits
    twin = _volume_of(ctx, scene.field.volume)
    assert bytes(twin.align(source[1025], prm).to_c()) == bytes(first.to_c())
    twin.free()
    volume.clear()
    assert not any(_snapshot(volume)[0])
    with pytest.raises(A3dError) as e:  # nothing observed: no point has a value
        volume.align(source[1025], prm)
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    volume.upload(scene.field.volume.D, scene.field.volume.W)
    assert _snapshot(volume) == before
    assert bytes(volume.align(source[1025], prm).to_c()) == bytes(first.to_c())
    # and after an integrate (a flat wall at z = 1 seen through a 16 x 12 camera: it changes the volume) undone by an upload
    points = np.zeros((12, 16, 3), F)
    points[..., 2] = 1.0
    image = RangeImage(points, np.ones((12, 16), np.uint8), CameraIntrinsics(20.0, 20.0, 8.0, 6.0, 16, 12)).device(ctx)
    volume.integrate(image, Transform.eye())
    assert _snapshot(volume) != before
    volume.upload(scene.field.volume.D, scene.field.volume.W)
    assert _snapshot(volume) == before
    assert bytes(volume.align(source[1025], prm).to_c()) == bytes(first.to_c())
    image.free()
