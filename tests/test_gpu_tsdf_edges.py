"""TSDF integrate and raycast on the GPU at the rules' edges (tsdf_edge_cases.py): uploaded fields on exact values, the
smallest and the longest volumes, weights at 2^24 and at the cap, a frame table of unlike frames, images made on the
device, the sample count at its limit.

Every comparison is on bits, through test_gpu_tsdf's _assert_volume and _assert_image, against the numpy restatement
(tsdf_restatement.py, written from the rules in align3d_hip.h).  tests/test_tsdf_edge_cases_cpu.py proves that each case is
what it claims to be and that its expectation changes under the slip it targets."""
import numpy as np
import pytest

import test_gpu_tsdf as G
import test_gpu_tsdf_surface as GS
import tsdf_edge_cases as E
import tsdf_restatement as T
from align3d_amd import A3dError, CameraIntrinsics, DevicePointCloud, DeviceTsdfVolume, RangeImage, Transform

pytestmark = pytest.mark.gpu

LIBRARIES = ("product", "diagnostics")


def _context(request, library):
    return request.getfixturevalue("ctx" if library == "product" else "diag_ctx")


def _host(frame):
    cam = CameraIntrinsics(*frame["intrinsics"], frame["width"], frame["height"])
    return RangeImage(frame["points"], frame["mask"], cam, colors=frame["colors"])


def _pair(ctx, case, colors, max_weight=64, tau=None):
    """The device volume and the restatement's, both holding the case's field when it has one."""
    tau = case.get("tau") if tau is None else tau
    dev = DeviceTsdfVolume(ctx, case["dims"], case["v"], case["origin"], truncation=tau, max_weight=max_weight, colors=colors)
    want = T.Volume(case["dims"], case["v"], case["origin"], dev.truncation, max_weight, colors)
    if "D" in case:
        dev.upload(case["D"], case["W"], case["C"] if colors else None)
        want.D, want.W = case["D"].copy(), case["W"].copy()
        if colors:
            want.C = case["C"].copy()
        G._assert_volume(dev, want, "uploaded")
    return dev, want


def _restate(want, frame, pose):
    return want.integrate(frame["points"], frame["mask"], frame["colors"], frame["intrinsics"],
                          G._pose_tuple(Transform(*pose).inverse()))


def _cast_both(dev, want, cam, pose, z_near, z_far, step, label):
    exp = want.raycast(cam[:4], cam[4], cam[5], pose, z_near, z_far, step)
    got = G._raycast(dev, CameraIntrinsics(*cam), Transform(*pose), z_near, z_far, step)
    G._assert_image(got, exp, label)
    return exp


# ---- A. layered fields -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
@pytest.mark.parametrize("library", LIBRARIES)
def test_layered_fields(request, library, colors):
    ctx = _context(request, library)
    hits = 0
    for case in E.layered_cases():
        dev, want = _pair(ctx, case, colors)
        cam = case["intrinsics"] + (case["width"], case["height"])
        exp = _cast_both(dev, want, cam, E.EYE, case["z_near"], case["z_far"], case["step"], (case["name"], library, colors))
        hits += int(exp["mask"].sum())
        G._assert_volume(dev, want, "a raycast does not change the volume")
        dev.free()
    assert hits > 50


def test_layered_fields_in_one_pixel_a_long_row_and_a_column(ctx):
    for name in ("exact zero", "plain tie", "hole"):
        case = next(c for c in E.layered_cases() if c["name"] == name)
        dev, want = _pair(ctx, case, True)
        for shape, cam in E.SHAPE_CAMERAS.items():
            exp = _cast_both(dev, want, cam, E.EYE, case["z_near"], case["z_far"], case["step"], (name, shape))
            assert exp["mask"].shape == (cam[5], cam[4]) and (name == "hole" or exp["mask"].any())
        dev.free()


# ---- B. the smallest volume and the longest ones -----------------------------------------------------------------------------

@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
def test_the_one_cell_volume(ctx, colors):
    case = E.one_cell_case()
    dev, want = _pair(ctx, case, colors)
    cam = case["intrinsics"] + (case["width"], case["height"])
    for name, z_near, z_far, step in case["rays"]:
        exp = _cast_both(dev, want, cam, E.EYE, z_near, z_far, step, name)
        assert exp["mask"].any() == (name == "through the cell") and not G._bits(exp["normals"]).any()
    GS._assert_surface(dev, 1, "one cell")
    dev.free()


@pytest.mark.parametrize("axis", (0, 1, 2), ids=("1024x2x2", "2x1024x2", "2x2x1024"))
def test_the_longest_volumes(ctx, axis):
    case = E.stick_case(axis)
    dev, want = _pair(ctx, case, True)
    for name, cam, pose, z_near, z_far, step in case["rays"]:
        exp = _cast_both(dev, want, cam, pose, z_near, z_far, step, (case["name"], name))
        assert exp["mask"].any(), name
    mesh = GS._assert_surface(dev, 1, case["name"])
    assert len(mesh["faces"]) > 100 and mesh["voxel"].max() > 3000
    GS._assert_surface(dev, 2, (case["name"], "min_weight 2"))
    dev.clear()
    want = T.Volume(case["dims"], case["v"], case["origin"], dev.truncation, 64, True)
    images = [G._upload(ctx, _host(frame)) for frame in case["frames"]]
    dev.integrate_many(images, [Transform(*pose) for pose in case["poses"]])
    touched = [_restate(want, frame, pose) for frame, pose in zip(case["frames"], case["poses"])]
    assert min(touched) > 150
    G._assert_volume(dev, want, (case["name"], "fused"))
    for image in images:
        image.free()
    dev.free()


def test_volume_sizes_and_weight_caps_at_their_limits(ctx):
    for axis in range(3):
        for bad in (1, 1025):
            dims = [2, 2, 2]
            dims[axis] = bad
            with pytest.raises(A3dError):
                DeviceTsdfVolume(ctx, dims, 0.1, (0.0, 0.0, 0.0))
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(A3dError):
            DeviceTsdfVolume(ctx, (2, 2, 2), 0.1, (0.0, 0.0, 0.0), max_weight=bad)
    dev = DeviceTsdfVolume(ctx, (2, 2, 2), 0.1, (0.0, 0.0, 0.0), max_weight=1 << 24)
    assert dev.info()["max_weight"] == 1 << 24
    dev.free()


# ---- C. integrate on uploaded fields -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
@pytest.mark.parametrize("cap", (E.TOP, E.SMALL_CAP), ids=("2^24", "5"))
@pytest.mark.parametrize("library", LIBRARIES)
def test_weights_up_to_2_24_and_around_the_cap(request, library, cap, colors):
    ctx = _context(request, library)
    case = E.weight_case()
    dev, want = _pair(ctx, case, colors, max_weight=cap)
    images = [G._upload(ctx, _host(frame), colors) for frame in case["frames"]]
    for f, (image, frame, pose) in enumerate(zip(images, case["frames"], case["poses"])):
        dev.integrate(image, Transform(*pose))
        assert _restate(want, frame, pose) == want.D.size
        G._assert_volume(dev, want, (library, cap, colors, f))
    assert want.W.max() == cap and np.isinf(want.D).any() and not np.isnan(want.D).any()
    for image in images:
        image.free()
    dev.free()


# ---- D. the frame table --------------------------------------------------------------------------------------------------------

def _table_pair(ctx, colors, max_weight=64):
    dims, v, origin = E.TABLE_VOLUME
    return G._new_pair(ctx, dims, v, origin, None, max_weight, colors)


@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
def test_one_call_of_frames_of_four_sizes(ctx, colors):
    frames, poses = E.mixed_frames()
    images = [G._upload(ctx, _host(frame), colors) for frame in frames]
    transforms = [Transform(*pose) for pose in poses]
    dev, want = _table_pair(ctx, colors)
    dev.integrate_many(images, transforms)
    assert all(_restate(want, frame, pose) > 0 for frame, pose in zip(frames, poses))
    G._assert_volume(dev, want, "one call")
    single, _ = _table_pair(ctx, colors)
    for image, transform in zip(images, transforms):
        single.integrate(image, transform)
    G._assert_volume(single, want, "one call each")
    for thing in images + [dev, single]:
        thing.free()


def test_calls_of_64_65_128_and_129_frames(ctx):
    pool = E.chunk_pool()
    images = [G._upload(ctx, _host(frame)) for frame in pool]
    dev, _ = _table_pair(ctx, True, max_weight=3)  # (the cap is reached, as in test_integrate_parity)
    for n in E.CHUNK_SIZES:
        picks, poses = E.chunk_call(n)
        transforms = [Transform(*pose) for pose in poses]
        dev.clear()
        dev.integrate_many([images[p] for p in picks], transforms)
        want = T.Volume(*E.TABLE_VOLUME, dev.truncation, 3, True)
        for p, pose in zip(picks, poses):
            _restate(want, pool[p], pose)
        G._assert_volume(dev, want, n)
        assert want.W.max() == 3 and (want.W == 0).any()
    # the 129 frames again, cut by the caller into calls of 1, 63 and 65
    dev.clear()
    for first, last in ((0, 1), (1, 64), (64, 129)):
        dev.integrate_many([images[p] for p in picks[first:last]], transforms[first:last])
    G._assert_volume(dev, want, "1 + 63 + 65")
    plain, want = _table_pair(ctx, False)  # (and without colours, across one cut)
    picks, poses = E.chunk_call(65)
    plain.integrate_many([images[p] for p in picks], [Transform(*pose) for pose in poses])
    for p, pose in zip(picks, poses):
        _restate(want, pool[p], pose)
    G._assert_volume(plain, want, "65, plain")
    for thing in images + [dev, plain]:
        thing.free()


# ---- E. images made on the device ------------------------------------------------------------------------------------------------

def _fuse_back(ctx, image, label):
    """Fuses a resident image that no upload made into the second volume from both poses; the expectation is the
    restatement fed the image as downloaded.  Some voxel reads the image's last pixel, others its last row and column."""
    host = image.download(normals=False, intensity=False, colors=True)
    h, w = host.mask.shape
    frame = {"points": host.points, "mask": host.mask, "colors": host.colors, "intrinsics": E.MODEL_CAMERA[:4]}
    dims, v, origin, tau = E.SECOND_VOLUME
    dev, want = G._new_pair(ctx, dims, v, origin, tau, 64, True)
    for pose in E.SECOND_POSES:
        dev.integrate(image, Transform(*pose))
        assert _restate(want, frame, pose) > 100
        _, row, col = want.last_pixels
        assert ((row == h - 1) & (col == w - 1)).any() and ((row == h - 1) & (col < w - 1)).any() and (col == w - 1).any(), label
        G._assert_volume(dev, want, label)
    dev.free()
    return host


def test_a_raycast_image_and_a_rendered_image_fused_back(ctx):
    scene, want_scene = G._scene(ctx, True)
    cam = CameraIntrinsics(*E.MODEL_CAMERA)
    pose, z_near, z_far, step = E.MODEL_RAY
    model = scene.raycast(cam, Transform(*pose), z_near, z_far, step)
    host = _fuse_back(ctx, model, "raycast")
    exp = want_scene.raycast(E.MODEL_CAMERA[:4], cam.width, cam.height, pose, z_near, z_far, step)
    assert np.array_equal(host.mask, exp["mask"]) and np.array_equal(G._bits(host.points), G._bits(exp["points"]))
    assert host.mask[-1, -1] == 1
    cloud = DevicePointCloud.from_range_image(model, colors=True)
    rendered = cloud.render(cam, None, E.RENDER_RADIUS)
    assert rendered.has_colors()
    again = _fuse_back(ctx, rendered, "rendered")
    assert again.mask[-1, -1] == 1 and again.mask.sum() >= host.mask.sum()
    for thing in (rendered, cloud, model, scene):
        thing.free()


# ---- F. the K rule ---------------------------------------------------------------------------------------------------------

def test_4096_samples_are_taken_and_4097_refused(ctx):
    case = dict(E.LAYERED)
    case["D"], case["W"], case["C"] = E.layered_field(E.K_PROFILE)
    dev, want = _pair(ctx, case, True)
    for name, z_near, z_far, step, K in E.k_cases():
        if K is None:
            with pytest.raises(A3dError):
                dev.raycast(CameraIntrinsics(*E.K_CAMERA), Transform.eye(), z_near, z_far, step)
            G._assert_volume(dev, want, name)
            continue
        exp = _cast_both(dev, want, E.K_CAMERA, E.EYE, z_near, z_far, step, name)
        assert exp["samples"] == K == E.samples(z_near, z_far, step), name
        if K in (7, 8, 4096):  # the crossing lies behind sample 3072 of 4096, and between samples 6 and 7 of the short rays
            assert exp["mask"].all() == (K != 7) and exp["mask"].any() == (K != 7), name
    dev.free()
