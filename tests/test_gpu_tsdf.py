"""The dense TSDF volume on the GPU (a3d_tsdf_volume_integrate / a3d_tsdf_volume_raycast, DeviceTsdfVolume).

Every comparison is on bits.  The expected volume (D, W, colours) and the expected model image (points, mask, normals,
colours) are the numpy restatement's (tsdf_restatement.py, written from the rules in align3d_hip.h and the reference's
camera.rs and transform.rs).  The restatement also says why each ray ended, so every case checks that its inputs do what
they are meant to: hits, misses, rays that start behind a surface, rays that leave one through its back face."""
import ctypes as C

import numpy as np
import pytest

import tsdf_restatement as T
from align3d_amd import (A3dError, CameraIntrinsics, Context, DeviceTsdfVolume, MsIcpParams, MultiscaleAlign, RangeImage,
                         RangeImageBuilder, Transform, _abi)
from align3d_amd.range_image import DeviceRangeImage
from data_util import SlamTbSample

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, MISSING = _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD
BELOW_HALF = float(np.nextafter(F(0.5), F(0)))  # 0.49999997

# (dims, voxel size, origin): 16 x 12 x 10, and 67 x 5 x 3 because nx is not a multiple of 64
VOLUMES = {"16x12x10": ((16, 12, 10), 0.1, (-0.8, -0.6, -0.5)), "67x5x3": ((67, 5, 3), 0.03, (-1.0, -0.07, -0.04))}
CAMERAS = {"24x20": CameraIntrinsics(21.3, 20.7, 11.5, 9.75, 24, 20), "65x3": CameraIntrinsics(40.0, 41.0, 32.0, 1.0, 65, 3)}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _unit_pose(seed):
    """As test_gpu_cloud_render._unit_pose: a seeded rotation, normalised in f32, and a translation within half a metre."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(F)
    q = (q / np.sqrt(np.sum(q.astype(np.float64) ** 2))).astype(F)
    return Transform(rng.uniform(-0.5, 0.5, 3).astype(F), q)


def _pose_tuple(transform):
    return transform.t, transform.q


def _frame(seed, cam, depth=(0.15, 1.2)):
    """A seeded range image in the camera's own frame: a smooth surface with a step in it, mask holes, and kept pixels
    whose z is NaN, +-inf, 0 or negative."""
    rng = np.random.default_rng(seed)
    w, h = cam.width, cam.height
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lo, hi = depth
    z = lo + (hi - lo) * (0.5 + 0.5 * np.sin(cols * rng.uniform(0.1, 0.5) + rng.uniform(0, 6)) * np.cos(rows * rng.uniform(0.1, 0.7)))
    z = np.where(cols > w * rng.uniform(0.3, 0.7), z, z * 0.6 + 0.05).astype(F)
    mask = (rng.random((h, w)) < 0.85).astype(np.uint8)
    bad = rng.permutation(w * h)[:6]
    z.reshape(-1)[bad[:min(6, len(bad))]] = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], F)[:len(bad)]
    mask.reshape(-1)[bad] = 1
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        pts = np.stack([(cols - cam.cx) * z64 / cam.fx, (rows - cam.cy) * z64 / cam.fy, z64], -1).astype(F)
    return RangeImage(pts, mask, cam, colors=rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


def _upload(ctx, host, colors=True):
    dev = DeviceRangeImage(ctx, host)
    if colors:
        dev.set_colors(host.colors)
    return dev


def _intr(cam):
    return cam.fx, cam.fy, cam.cx, cam.cy


def _restate(vol, host, c2w):
    return vol.integrate(host.points, host.mask, host.colors, _intr(host.intrinsics), _pose_tuple(c2w.inverse()))


def _assert_volume(dev, want, label):
    D, W, rgb = dev.download()
    assert np.array_equal(_bits(W), _bits(want.W)), label
    assert np.array_equal(_bits(D), _bits(want.D)), label
    assert (rgb is None) == (want.C is None), label
    if rgb is not None:
        assert np.array_equal(rgb, want.C), label


def _new_pair(ctx, dims, v, origin, tau, max_weight, colors):
    dev = DeviceTsdfVolume(ctx, dims, v, origin, truncation=tau, max_weight=max_weight, colors=colors)
    return dev, T.Volume(dims, v, origin, dev.truncation, max_weight, colors)


# ---- 1. integrate against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
@pytest.mark.parametrize("cam_name", sorted(CAMERAS))
@pytest.mark.parametrize("vol_name", sorted(VOLUMES))
def test_integrate_parity(ctx, vol_name, cam_name, colors):
    """n = 1, 2 and 5 frames in turn with max_weight = 3, then 70 frames in one call (two chunks) and one by one."""
    dims, v, origin = VOLUMES[vol_name]
    cam = CAMERAS[cam_name]
    seeds = [1000 * len(vol_name) + 100 * cam.width + f for f in range(70)]
    hosts = [_frame(s, cam) for s in seeds]
    poses = [_unit_pose(s + 7) for s in seeds]
    images = [_upload(ctx, host, colors) for host in hosts]
    back = images[0].download(normals=False, intensity=False, colors=colors)  # (an upload keeps every bit, NaN included)
    assert np.array_equal(_bits(back.points), _bits(hosts[0].points)) and np.array_equal(back.mask, hosts[0].mask)
    dev, want = _new_pair(ctx, dims, v, origin, None, 3, colors)
    assert dev.truncation == float(F(4) * F(v)) and dev.info()["dims"] == dims and dev.info()["colors"] == colors
    _assert_volume(dev, want, "new")
    first = 0
    for n in (1, 2, 5):
        dev.integrate_many(images[first:first + n], poses[first:first + n])
        for f in range(first, first + n):
            _restate(want, hosts[f], poses[f])
        first += n
        _assert_volume(dev, want, (vol_name, cam_name, colors, n))
    dev.clear()
    _assert_volume(dev, T.Volume(dims, v, origin, dev.truncation, 3, colors), "cleared")
    # 70 frames cross the 64-frame chunk; the same frames one call each give the same bits
    dev.integrate_many(images, poses)
    want = T.Volume(dims, v, origin, dev.truncation, 3, colors)
    touched = sum(_restate(want, host, pose) for host, pose in zip(hosts, poses))
    _assert_volume(dev, want, (vol_name, cam_name, colors, 70))
    single, _ = _new_pair(ctx, dims, v, origin, None, 3, colors)
    for image, pose in zip(images, poses):
        single.integrate(image, pose)
    _assert_volume(single, want, (vol_name, cam_name, colors, "one by one"))
    # the inputs do what they are meant to: the cap is reached, voxels stay unobserved, both signs and the saturated
    # distance occur
    assert touched > 0 and want.W.max() == 3.0 and (want.W == 0).any()
    seen = want.W > 0
    assert (want.D[seen] == 1.0).any() and (want.D[seen] < 0).any()
    for image in images:
        image.free()
    dev.free(), single.free()


def test_voxels_exactly_on_the_truncation_and_the_image_borders(ctx):
    """No rotation, fx = fy = 2, cx = cy = 0, v = 1 / 4: a voxel at (x, y, 1) projects to (2 x, 2 y) exactly.  Column 0 of
    the volume lands on u = -0.5 (skipped) or -0.49999997 (kept), column 8 on u = 3.5 = w - 0.5 (skipped); with every depth 1
    and tau = 1 / 2 the layer at z = 1.5 has sdf == -tau (kept) and the layer at z = 1.75 is skipped."""
    cam = CameraIntrinsics(2.0, 2.0, 0.0, 0.0, 4, 2)
    pts = np.zeros((2, 4, 3), F)
    pts[..., 2] = 1.0
    host = RangeImage(pts, np.ones((2, 4), np.uint8), cam, colors=np.full((2, 4, 3), 200, np.uint8))
    image = _upload(ctx, host)
    for ox, first_column_kept in ((-0.25, False), (-BELOW_HALF / 2, True)):
        dev, want = _new_pair(ctx, (9, 4, 6), 0.25, (ox, -0.25, 0.5), 0.5, 64, True)
        dev.integrate(image, Transform.eye())
        _restate(want, host, Transform.eye())
        _assert_volume(dev, want, ox)
        # layers k: z = 0.5 + k / 4; rows j: y = -0.25 + j / 4, so j = 1 is v = 0
        assert (want.W[2, 1, 0] == 1.0) == first_column_kept and want.W[2, 1, 1] == 1.0
        assert want.W[2, 0, 1] == 0 and want.W[2, 1, 8] == 0 and want.W[2, 1, 7] == 1.0  # v = -0.5; u = 3.5; u = 3
        assert want.W[4, 1, 1] == 1.0 and want.D[4, 1, 1] == -1.0 and want.W[5].sum() == 0
        dev.free()
    image.free()


# ---- 2. raycast against the restatement ------------------------------------------------------------------------------

SCENE = ((16, 12, 10), 0.1, (-0.8, -0.6, 0.5), 0.3)  # dims, v, origin, tau: x in [-0.8, 0.7], y in [-0.6, 0.5], z in [0.5, 1.4]
FUSED_FROM = (Transform.eye(), Transform((0.1, -0.05, 0.0), (0.0, 0.08715574, 0.0, 0.9961947)),
              Transform((-0.12, 0.04, 0.02), (0.0610485, 0.0, 0.0, 0.99813479)))


def _scene(ctx, colors):
    """A bumpy wall about a metre in front of three nearby cameras, with holes."""
    dims, v, origin, tau = SCENE
    dev, want = _new_pair(ctx, dims, v, origin, tau, 64, colors)
    cam = CAMERAS["24x20"]
    hosts = [_frame(50 + f, cam, depth=(0.9, 1.15)) for f in range(len(FUSED_FROM))]
    images = [_upload(ctx, host, colors) for host in hosts]
    dev.integrate_many(images, FUSED_FROM)
    for host, pose in zip(hosts, FUSED_FROM):
        _restate(want, host, pose)
    for image in images:
        image.free()
    return dev, want


# (name, camera_to_world, z_near, z_far, step)
RAYS = (
    ("front", Transform.eye(), 0.3, 1.6, 0.15),
    ("front fine", FUSED_FROM[1], 0.25, 1.7, 0.05),
    ("oblique", Transform((0.3, 0.1, 0.1), (0.0, -0.17364818, 0.0, 0.98480775)), 0.2, 1.8, 0.1),
    ("random", _unit_pose(11), 0.1, 2.0, 0.1),
    ("looking away", Transform((0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)), 0.3, 1.6, 0.15),
    ("behind the surface", Transform((0.0, 0.0, 1.1), (0.0, 0.0, 0.0, 1.0)), 0.01, 1.0, 0.07),
    ("behind, looking back", Transform((0.0, 0.0, 1.3), (0.0, 1.0, 0.0, 0.0)), 0.02, 1.0, 0.05),
    ("z_far before the surface", Transform.eye(), 0.3, 0.7, 0.1),
    ("one sample", Transform.eye(), 0.9, 0.95, 0.1),
)


def _raycast(dev, cam, pose, z_near, z_far, step):
    image = dev.raycast(cam, pose, z_near, z_far, step)
    try:
        assert image.shape == (cam.height, cam.width) and image.has_normals() and image.has_colors() == dev.colors
        host = image.download(normals=True, intensity=False, colors=dev.colors)
        k = host.intrinsics
        assert (k.fx, k.fy, k.cx, k.cy) == (cam.fx, cam.fy, cam.cx, cam.cy)
        with pytest.raises(A3dError):
            image.download(intensity=True)  # (no intensities until somebody asks)
        return {"points": host.points, "mask": host.mask, "normals": host.normals, "colors": host.colors}
    finally:
        image.free()


def _assert_image(got, want, label):
    assert np.array_equal(got["mask"], want["mask"]), label
    assert np.array_equal(_bits(got["points"]), _bits(want["points"])), label
    assert np.array_equal(_bits(got["normals"]), _bits(want["normals"])), label
    assert (got["colors"] is None) == (want["colors"] is None), label
    if want["colors"] is not None:
        assert np.array_equal(got["colors"], want["colors"]), label
    empty = got["mask"] == 0
    assert not _bits(got["points"])[empty].any() and not _bits(got["normals"])[empty].any(), label  # +0, no sign bit
    assert set(np.unique(got["mask"]).tolist()) <= {0, 1}, label


@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
def test_raycast_parity(ctx, colors):
    dev, want = _scene(ctx, colors)
    _assert_volume(dev, want, "scene")
    seen = {"hits": 0, "bare": 0, "left": 0, "behind": 0, "ran out": 0}
    for cam_name, cam in sorted(CAMERAS.items()):
        for name, pose, z_near, z_far, step in RAYS:
            label = (name, cam_name, colors)
            exp = want.raycast(_intr(cam), cam.width, cam.height, _pose_tuple(pose), z_near, z_far, step)
            got = _raycast(dev, cam, pose, z_near, z_far, step)
            _assert_image(got, exp, label)
            hit = exp["mask"] == 1
            bare = hit & ~_bits(exp["normals"]).any(axis=-1)
            seen["hits"] += int(hit.sum())
            seen["bare"] += int(bare.sum())
            seen["left"] += int((exp["reason"] == T.LEFT_FROM_BEHIND).sum())
            seen["behind"] += int(exp["started_behind"].sum())
            seen["ran out"] += int((exp["reason"] == T.RAN_OUT).sum())
            if name in ("looking away", "z_far before the surface", "one sample", "behind the surface"):
                assert not hit.any(), label
            if name == "one sample":
                assert exp["samples"] == 1
            if name == "behind the surface":
                assert exp["started_behind"].any() and not (exp["reason"] == T.LEFT_FROM_BEHIND).any(), label
            if name == "behind, looking back":
                assert (exp["reason"] == T.LEFT_FROM_BEHIND).any(), label
            if name == "front fine" and cam_name == "24x20":
                assert hit.sum() > 100 and (hit & ~bare).sum() > 50 and bare.any(), label  # zero normals beside holes
                if colors:
                    assert exp["colors"][hit].any(), label
    assert all(count > 0 for count in seen.values()), seen
    _assert_volume(dev, want, "a raycast does not change the volume")
    dev.free()


def test_same_bits_on_a_second_run_and_from_the_diagnostics_library(ctx, diag_ctx):
    cam = CAMERAS["24x20"]
    name, pose, z_near, z_far, step = RAYS[1]
    results = []
    for context in (ctx, ctx, diag_ctx):
        dev, want = _scene(context, True)
        results.append((dev.download(), _raycast(dev, cam, pose, z_near, z_far, step), _raycast(dev, cam, pose, z_near, z_far, step)))
        dev.free()
    exp = want.raycast(_intr(cam), cam.width, cam.height, _pose_tuple(pose), z_near, z_far, step)
    for (D, W, rgb), image, again in results:
        assert np.array_equal(_bits(D), _bits(want.D)) and np.array_equal(_bits(W), _bits(want.W)) and np.array_equal(rgb, want.C)
        _assert_image(image, exp, name)
        _assert_image(again, exp, name)


def test_same_bits_whatever_scratch_arenas_and_spare_blocks_hold():
    """The frame table lives in scratch region 3, the model image in a pooled arena, the volume in a block the context
    may hand back from a freed one: each filled with 0x00, 0xFF and 0x5A before the same calls."""
    own = Context(0)
    cam = CAMERAS["24x20"]
    name, pose, z_near, z_far, step = RAYS[1]
    dev, want = _scene(own, True)
    exp = want.raycast(_intr(cam), cam.width, cam.height, _pose_tuple(pose), z_near, z_far, step)
    _assert_image(_raycast(dev, cam, pose, z_near, z_far, step), exp, "before")
    dev.free()  # (its block is now a spare one, the image's arena is back in the pool)
    for byte in (0x00, 0xFF, 0x5A):
        filled = own.selftest_fill_scratch(byte)
        assert filled[3] > 0 and filled[6] > 0 and filled[7] > 0, filled
        dev, _ = _scene(own, True)
        _assert_volume(dev, want, byte)
        _assert_image(_raycast(dev, cam, pose, z_near, z_far, step), exp, byte)
        dev.free()
    own.close()


# ---- 3. real frames --------------------------------------------------------------------------------------------------

def test_three_real_frames_fused_raycast_and_aligned(ctx):
    """Level 2 (160 x 120) of three sample1 frames into 64^3: the restatement matches, and the raycast model image goes
    through pyramid(2) and MultiscaleAlign like any resident image."""
    s = SlamTbSample("sample1")
    ids = s.ids[:3]
    cam0 = CameraIntrinsics(*s.intrinsics(ids[0]), 640, 480)
    built = RangeImageBuilder(ctx).pyramid_levels(3).build_many(cam0, [s.load(i) for i in ids], s.depth_scale(ids[0]))
    levels = [pyramid[2] for pyramid in built]
    hosts = [lv.download(normals=False, intensity=False, colors=True) for lv in levels]
    assert hosts[0].mask.shape == (120, 160)
    world = Transform.from_matrix4(s.rt_cam(ids[0])).inverse()
    poses = [world * Transform.from_matrix4(s.rt_cam(i)) for i in ids]  # frame 0 is the world
    dims, v, origin = (64, 64, 64), 0.04, (-1.28, -1.28, 0.2)
    dev, want = _new_pair(ctx, dims, v, origin, None, 64, True)
    dev.integrate_many(levels, poses)
    touched = sum(_restate(want, host, pose) for host, pose in zip(hosts, poses))
    assert touched > 20000
    _assert_volume(dev, want, "sample1")
    k = hosts[0].intrinsics
    cam = CameraIntrinsics(k.fx, k.fy, k.cx, k.cy, 160, 120)
    step = float(F(0.5) * F(dev.truncation))
    exp = want.raycast(_intr(cam), 160, 120, _pose_tuple(poses[0]), 0.3, 3.0, step)
    model = dev.raycast(cam, poses[0], 0.3, 3.0)  # (step: half the truncation)
    got = model.download(normals=True, intensity=False, colors=True)
    _assert_image({"points": got.points, "mask": got.mask, "normals": got.normals, "colors": got.colors}, exp, "sample1")
    assert exp["mask"].sum() > 5000 and _bits(exp["normals"]).any(axis=-1).sum() > 4000
    # a first-class image: two levels, then the target of a multiscale alignment of the next frame
    target = model.pyramid(2)
    source = levels[1].pyramid(2)
    assert target[0] is model and target[1].shape == (60, 80)
    params = MsIcpParams(MsIcpParams.default().pyramid[:2]).customize(lambda i, p: setattr(p, "max_iterations", 3))
    aligner = MultiscaleAlign.new(ctx, params, target)
    pose = aligner.align(source)
    assert np.isfinite(pose.t).all() and np.isfinite(pose.q).all() and abs(float(np.linalg.norm(pose.q)) - 1.0) < 1e-3
    aligner.free()
    for lv in (target[1], source[1], model):
        lv.free()
    for pyramid in built:
        for lv in pyramid:
            lv.free()
    dev.free()


# ---- 4. errors on the device -----------------------------------------------------------------------------------------

def test_errors_on_the_device(ctx):
    own = Context(0)
    cam = CAMERAS["24x20"]
    host = _frame(3, cam)
    mine, foreign = _upload(own, host, colors=False), _upload(ctx, host, colors=True)
    coloured, want = _new_pair(own, (16, 12, 10), 0.1, (-0.8, -0.6, -0.5), None, 3, True)
    plain = DeviceTsdfVolume(own, (16, 12, 10), 0.1, (-0.8, -0.6, -0.5))
    good = _upload(own, host, colors=True)
    coloured.integrate(good, _unit_pose(1))
    _restate(want, host, _unit_pose(1))
    _assert_volume(coloured, want, "before")
    lib, poses = own.lib, (_abi.PoseC * 2)(Transform.eye().to_c(), Transform.eye().to_c())

    def integrate(volume, *images):
        handles = (C.c_void_p * len(images))(*[im.handle for im in images])
        return lib.a3d_tsdf_volume_integrate(volume.handle, handles, poses, len(images))

    assert integrate(coloured, good, foreign) == INVALID   # an image of another context (the good one is not fused either)
    assert integrate(coloured, good, mine) == MISSING      # an image without colours
    assert integrate(coloured, good, good) == _abi.A3D_OK
    _restate(want, host, Transform.eye()), _restate(want, host, Transform.eye())
    _assert_volume(coloured, want, "after the refused calls")  # unchanged by them
    with pytest.raises(A3dError):
        coloured.integrate(mine, Transform.eye())
    with pytest.raises(A3dError):
        coloured.integrate(foreign, Transform.eye())
    with pytest.raises(TypeError):
        coloured.integrate(host, Transform.eye())          # a host image: there is no hidden upload
    with pytest.raises(TypeError):
        coloured.raycast(cam, np.eye(4, dtype=F), 0.3, 2.0)
    with pytest.raises(A3dError):
        coloured.raycast(cam, Transform.eye(), 0.3, 0.2)
    with pytest.raises(A3dError):
        coloured.raycast(cam, Transform.eye(), 0.3, 2.0, step=1e-6)
    with pytest.raises(A3dError):
        DeviceTsdfVolume(own, (16, 12, 1), 0.1, (0.0, 0.0, 0.0))
    _assert_volume(coloured, want, "after the refused raycasts")
    # a volume without colours takes either image and ignores the colours; its download has none
    plain.integrate_many([mine, good], [Transform.eye(), _unit_pose(2)])
    D, W, rgb = plain.download()
    assert rgb is None and W.max() >= 1.0
    records = np.empty((10, 12, 16, 2), F)
    assert lib.a3d_tsdf_volume_download(plain.handle, _abi.ptr(records), _abi.ptr(np.empty((10, 12, 16), np.uint32))) == MISSING
    image = plain.raycast(cam, Transform.eye(), 0.3, 2.0)
    assert image.ctx is own and not image.has_colors()
    image.free()
    for thing in (mine, good, coloured, plain):
        thing.free()
    foreign.free()
    own.close()
