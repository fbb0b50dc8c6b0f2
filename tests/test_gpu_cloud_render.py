"""Rendering resident clouds and the voxel map into range images on the GPU (a3d_point_cloud_render_device,
a3d_voxel_map_render; PinholeCamera::project_to_image, src/camera.rs:177-202).

Every comparison is on bits.  The expected image is the numpy restatement's (render_restatement.py, written from
camera.rs and transform.rs): points, mask, normals, colours and the index plane.  A colour and a normal follow their
row, so the expected ones are colors_in[index] and transform_normal(normals_in[index])."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import render_restatement as R
from align3d_amd import (A3dError, CameraIntrinsics, Context, DevicePointCloud, DeviceVoxelMap, MsIcpParams, MultiscaleAlign,
                         PointCloud, RangeImageBuilder, Transform, _abi)
from data_util import SlamTbSample
from gpu_util import oracle_pyramid, transform_diff

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = _abi.A3D_INVALID_PARAMETER
SENTINEL = 0x5A5A5A50
BELOW_HALF = float(np.nextafter(F(0.5), F(0)))  # 0.49999997
Z_SHARED = np.asarray([0.5, 0.75, 1.0, 1.25, 1.9375], F)  # depths many rows have in common: equal z bits


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _unit_pose(seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(F)
    q = (q / np.sqrt(np.sum(q.astype(np.float64) ** 2))).astype(F)
    return Transform(rng.uniform(-0.5, 0.5, 3).astype(F), q)


def _cloud_rows(seed, n, cam, exact_borders):
    """[n, 3] f32 rows in the CAMERA's frame: projections all over the image and a two-pixel rim around it, depths that
    many rows share, duplicated rows (same pixel AND same z bits), depths of 0, -0, < 0, NaN, +-inf, footprints at the
    four corners, centres just outside the image, and (exact_borders: fx = fy a power of two, cx = cy = 0, z = 1, so that
    u = x * fx exactly) projections exactly on -0.5, w - 0.5 and 0.49999997."""
    rng = np.random.default_rng(seed)
    w, h = cam.width, cam.height
    u = rng.uniform(-2.0, w + 2.0, n)
    v = rng.uniform(-2.0, h + 2.0, n)
    z = np.where(rng.random(n) < 0.6, rng.choice(Z_SHARED, n), rng.uniform(0.5, 2.0, n).astype(F)).astype(F)
    fixed = []
    for cu, cv in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):                    # footprints clipped at the corners
        fixed.append((cu, cv, 1.0))
    for cu, cv in ((-0.6, h / 2), (w - 0.4, h / 2), (w / 2, -0.7), (w / 2, h - 0.45)):  # centres just outside
        fixed.append((cu, cv, 0.5))
    if exact_borders:
        for e in (-0.5, -BELOW_HALF, BELOW_HALF, w - 0.5, float(np.nextafter(F(w - 0.5), F(0)))):
            fixed.append((e, min(h - 1, 0.25), 1.0))
        for e in (-0.5, -BELOW_HALF, BELOW_HALF, h - 0.5, float(np.nextafter(F(h - 0.5), F(0)))):
            fixed.append((min(w - 1, 0.25), e, 1.0))
    k = min(len(fixed), n)
    if k:
        sel = rng.permutation(len(fixed))[:k]  # (a cloud shorter than the list takes a seeded part of it)
        at = rng.permutation(n)[:k]
        for i, j in zip(at, sel):
            u[i], v[i], z[i] = fixed[j]
    z64 = z.astype(np.float64)
    pts = np.stack([(u - cam.cx) * z64 / cam.fx, (v - cam.cy) * z64 / cam.fy, z64], -1).astype(F)
    if n >= 16:  # duplicates: the lowest index must win; and depths no camera sees
        dup = rng.permutation(n)[:n // 4]
        pts[dup] = pts[rng.permutation(n)[:n // 4]]
        bad = rng.permutation(n)[:6]
        pts[bad, 2] = np.asarray([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], F)
    return pts


def _device_cloud(ctx, points, normals, colors):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


def _download(image, index):
    host = image.download(normals=image.has_normals(), intensity=False, colors=image.has_colors())
    return {"points": host.points, "mask": host.mask, "normals": host.normals, "colors": host.colors, "index": index,
            "k": (host.intrinsics.fx, host.intrinsics.fy, host.intrinsics.cx, host.intrinsics.cy)}


def _render(source, cam, camera_to_world, radius):
    image, index = source.render(cam, camera_to_world, radius, return_index=True)
    try:
        assert image.shape == (cam.height, cam.width) and index.shape == image.shape and index.dtype == np.uint32
        return _download(image, index)
    finally:
        image.free()


def _assert_same(got, want, label):
    assert np.array_equal(got["mask"], want["mask"]), label
    assert np.array_equal(got["index"], want["index"]), label
    assert np.array_equal(_bits(got["points"]), _bits(want["points"])), label
    for name in ("normals", "colors"):
        assert (got[name] is None) == (want[name] is None), (label, name)
    if want["normals"] is not None:
        assert np.array_equal(_bits(got["normals"]), _bits(want["normals"])), label
    if want["colors"] is not None:
        assert np.array_equal(got["colors"], want["colors"]), label


def _assert_empty_pixels_are_zero(got, label):
    empty = got["mask"] == 0
    assert (got["index"][empty] == R.NO_ROW).all() and (got["index"][~empty] != R.NO_ROW).all(), label
    assert not _bits(got["points"])[empty].any(), label  # +0: no sign bit either
    if got["normals"] is not None:
        assert not _bits(got["normals"])[empty].any(), label
    if got["colors"] is not None:
        assert not got["colors"][empty].any(), label
    assert set(np.unique(got["mask"]).tolist()) <= {0, 1}, label


# ---- 1. restatement parity ------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 63), (3, 65), (64, 48), (160, 120)]  # (width, height)
LENS = (0, 1, 255, 256, 257, 5003)
FIELDS = ((True, True, False), (False, False, True), (False, True, False), (True, False, True), (True, True, True),
          (False, False, False))  # (normals, colours, pose)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_parity(ctx, shape):
    w, h = shape
    cams = (CameraIntrinsics(64.0, 64.0, 0.0, 0.0, w, h),                                     # exact borders
            CameraIntrinsics(525.0 * w / 640.0 + 0.37, 523.5 * w / 640.0, w / 2 - 0.5, h / 2 + 0.25, w, h))
    case = 0
    winners = ties = 0
    for ci, cam in enumerate(cams):
        radii = (0.0, 1.9 / cam.fx, 40.0 / cam.fx)  # half-widths 0; 0-3 over z in [0.5, 2); the cap of 8
        for n in LENS:
            pts_cam = _cloud_rows(100 * w + 10 * h + n + ci, n, cam, exact_borders=ci == 0)
            rng = np.random.default_rng(n + 7)
            normals_in = rng.normal(size=(n, 3)).astype(F)
            colors_in = rng.integers(0, 256, (n, 3), dtype=np.uint8)
            for radius in radii:
                # (every combination meets every radius and both cameras; radius 0 without a pose at 256 and 5003 rows)
                with_normals, with_colors, with_pose = FIELDS[(case + case // 3) % len(FIELDS)]
                case += 1
                c2w = _unit_pose(case) if with_pose else None
                # the cloud lives in the world: camera_to_world applied to the camera-frame rows (any f32 values do)
                pts = R.camera_points(pts_cam, (c2w.t, c2w.q)) if with_pose else pts_cam
                w2c = None
                if with_pose:
                    inv = c2w.inverse()
                    w2c = (inv.t, inv.q)
                nrm, col = (normals_in if with_normals else None), (colors_in if with_colors else None)
                cloud = _device_cloud(ctx, pts, nrm, col)
                label = (shape, ci, n, radius, with_normals, with_colors, with_pose)
                try:
                    got = _render(cloud, cam, c2w, radius)
                finally:
                    cloud.free()
                want = R.render(pts, nrm, col, w2c, cam.fx, cam.fy, cam.cx, cam.cy, w, h, radius)
                _assert_same(got, want, label)
                _assert_empty_pixels_are_zero(got, label)
                assert got["k"] == (cam.fx, cam.fy, cam.cx, cam.cy), label
                winners += int(want["mask"].sum())
                if n >= 256 and not with_pose and radius == 0.0:
                    # the inputs do what they are meant to: rows that share a pixel with equal z bits exist
                    keep, ui, vi, _, _ = R.footprints(pts, cam.fx, cam.fy, cam.cx, cam.cy, w, h, 0.0)
                    key = (vi * w + ui) << 32 | _bits(pts[keep, 2]).astype(np.int64)
                    ties += len(key) - len(np.unique(key))
    assert winners > 0 and ties > 0


def test_exact_borders_on_the_device(ctx):
    """z = 1, fx = fy = 1, cx = cy = 0: u = x exactly.  -0.5 and w - 0.5 are dropped, -0.49999997 and 0.49999997 land in
    column 0 ((u + 0.5) as i32 would put the latter in column 1)."""
    w, h = 640, 2
    us = np.asarray([-0.5, -BELOW_HALF, BELOW_HALF, w - 0.5, np.nextafter(F(w - 0.5), F(0)), 0.5, 1.5, 2.5], F)
    for axis in (0, 1):
        pts = np.zeros((len(us), 3), F)
        pts[:, axis], pts[:, 2] = us, 1.0
        pts[:, 1 - axis] = np.arange(len(us)) % 2  # (spread over two lines of the other axis)
        cam = CameraIntrinsics(1.0, 1.0, 0.0, 0.0, *((w, h) if axis == 0 else (h, w)))
        cloud = _device_cloud(ctx, pts, None, None)
        got = _render(cloud, cam, None, 0.0)
        cloud.free()
        landed = {int(k): (int(r), int(c)) for (r, c), k in np.ndenumerate(got["index"]) if k != R.NO_ROW}
        want = {1: 0, 2: 0, 4: w - 1, 5: 1, 6: 2, 7: 3}  # row -> coordinate along `axis`; rows 0 and 3 are dropped
        # (rows 1 and 2 both land on coordinate 0, on different lines of the other axis)
        assert {k: rc[1 - axis] for k, rc in landed.items()} == want, (axis, landed)
        _assert_same(got, R.render(pts, None, None, None, 1.0, 1.0, 0.0, 0.0, cam.width, cam.height, 0.0), axis)


# ---- 2. determinism --------------------------------------------------------------------------------------------------

def test_same_bits_every_time_and_from_both_splat_forms(ctx, diag_ctx, monkeypatch):
    cam = CameraIntrinsics(70.0, 69.0, 31.5, 24.25, 64, 48)
    pts = _cloud_rows(5, 5003, cam, exact_borders=False)
    rng = np.random.default_rng(5)
    nrm, col = rng.normal(size=(len(pts), 3)).astype(F), rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    for radius in (0.0, 1.9 / cam.fx, 40.0 / cam.fx):
        want = R.render(pts, nrm, col, None, cam.fx, cam.fy, cam.cx, cam.cy, 64, 48, radius)
        cloud = _device_cloud(ctx, pts, nrm, col)
        _assert_same(_render(cloud, cam, None, radius), want, ("product", radius))
        _assert_same(_render(cloud, cam, None, radius), want, ("product again", radius))
        cloud.free()
        cloud = _device_cloud(diag_ctx, pts, nrm, col)
        for form in ("0", "1"):  # the atomic alone; the load that skips it (diagnostics build: A3D_CLOUD_RENDER_SPLAT)
            monkeypatch.setenv("A3D_CLOUD_RENDER_SPLAT", form)
            _assert_same(_render(cloud, cam, None, radius), want, ("diag", form, radius))
        monkeypatch.delenv("A3D_CLOUD_RENDER_SPLAT")
        cloud.free()


# ---- 3. round trip on real data -------------------------------------------------------------------------------------

def _frame0(ctx, levels=1, frame=0):
    s = SlamTbSample("sample1")
    cam = CameraIntrinsics(*s.intrinsics(frame), 640, 480)
    return cam, RangeImageBuilder(ctx).pyramid_levels(levels).build(cam, *s.load(frame), s.depth_scale(frame))


def test_round_trip_of_a_real_frame(ctx):
    """image -> cloud -> image under the frame's own camera: every kept pixel wins itself."""
    cam, (src,) = _frame0(ctx)
    host = src.download(intensity=False)
    cloud = DevicePointCloud.from_range_image(src, colors=True)
    got = _render(cloud, cam, None, 0.0)
    keep = host.mask != 0
    assert keep.sum() > 100000 and cloud.len() == int(keep.sum())
    assert np.array_equal(got["mask"], keep.astype(np.uint8))
    assert np.array_equal(_bits(got["points"])[keep], _bits(host.points)[keep])
    assert np.array_equal(_bits(got["normals"])[keep], _bits(host.normals)[keep])
    assert np.array_equal(got["colors"][keep], host.colors[keep])
    want_index = np.where(keep, np.cumsum(keep.reshape(-1)).reshape(keep.shape) - 1, R.NO_ROW).astype(np.uint32)
    assert np.array_equal(got["index"], want_index)
    _assert_empty_pixels_are_zero(got, "round trip")
    cloud.free()
    src.free()


# ---- 4. the map form ------------------------------------------------------------------------------------------------

def _filled_map(ctx):
    m = DeviceVoxelMap(ctx, 0.05, normals=True, colors=True)
    for g in range(3):
        rng = np.random.default_rng(40 + g)
        pts = rng.uniform([-1.0, -0.8, 0.6], [1.0, 0.8, 2.4], (1500, 3)).astype(F)
        cloud = _device_cloud(ctx, pts, rng.normal(size=(1500, 3)).astype(F), rng.integers(0, 256, (1500, 3), dtype=np.uint8))
        m.insert(cloud, _unit_pose(90 + g) if g else None)
        cloud.free()
    return m


def _assert_map_equals_extract(m, label):
    cams = (CameraIntrinsics(60.0, 61.0, 31.5, 23.5, 64, 48), CameraIntrinsics(140.0, 140.0, 80.0, 60.0, 160, 120))
    poses = (None, Transform((0.05, -0.02, -0.4), (0.0, 0.0, 0.0, 1.0)), _unit_pose(3))
    stats = m.stats()
    for cam in cams:
        for c2w in poses:
            for radius in (0.0, 0.025, 1.0):
                got = _render(m, cam, c2w, radius)
                cloud = m.extract()
                want = _render(cloud, cam, c2w, radius)
                assert cloud.len() == stats["cells"]
                cloud.free()
                _assert_same(got, want, (label, cam.width, radius))
                _assert_empty_pixels_are_zero(got, label)
                assert (got["normals"] is not None) and (got["colors"] is not None)
    assert m.stats() == stats  # (a render does not change the map)
    return got


def test_map_render_equals_extract_then_render(ctx):
    m = _filled_map(ctx)
    assert m.cells() > 2000
    last = _assert_map_equals_extract(m, "filled")
    assert last["mask"].sum() > 0
    removed = m.retain(box=((-0.5, -0.5, 0.0), (0.6, 0.7, 2.0)))
    assert removed > 0 and m.cells() > 100
    _assert_map_equals_extract(m, "retained")
    m.clear()
    empty = _assert_map_equals_extract(m, "cleared")
    assert empty["mask"].sum() == 0
    m.free()
    fresh = DeviceVoxelMap(ctx, 0.05, normals=False, colors=False)  # nothing ever inserted, no fields
    image, index = fresh.render(CameraIntrinsics(60.0, 60.0, 2.0, 1.0, 5, 3), None, 0.5, return_index=True)
    assert not image.has_normals() and not image.has_colors() and (index == R.NO_ROW).all()
    assert not image.download(normals=False, intensity=False, colors=False).mask.any()
    image.free()
    fresh.free()


# ---- 5. a rendered image is a first-class image ---------------------------------------------------------------------

def _pose_bits(T):
    p = T.to_c()
    return np.asarray(list(p.t) + list(p.q), F).view(np.uint32)


def test_rendered_image_through_pyramid_and_multiscale_align(ctx):
    """Render -> pyramid(3) -> MultiscaleAlign target.  The pose equals, bit for bit, the pose through a download and
    RangeImage.pyramid (upload and render agree in every field), and the C++ oracle's on the downloaded level 0 within
    the project's 1e-4 rad / 1e-4 m (test_end_to_end_multiscale_align)."""
    prm = MsIcpParams.default().customize(lambda i, p: setattr(p, "max_iterations", 3))
    cam, (lv0,) = _frame0(ctx)
    cloud = DevicePointCloud.from_range_image(lv0, colors=True)
    lv0.free()
    rendered = cloud.render(cam, None, 0.0)
    cloud.free()
    host = rendered.download(intensity=False)
    with pytest.raises(A3dError):
        rendered.download(intensity=True)  # (no intensities and no map until somebody asks)
    _, src = _frame0(ctx, levels=3, frame=1)
    tgt = rendered.pyramid(3)
    assert tgt[0] is rendered
    T = MultiscaleAlign.new(ctx, prm, tgt).align(src)
    tgt_up = host.pyramid(ctx, 3)
    T_up = MultiscaleAlign.new(ctx, prm, tgt_up).align(src)
    assert np.array_equal(_pose_bits(T), _pose_bits(T_up))
    for a, b in zip(tgt, tgt_up):
        x, y = a.download(), b.download()
        assert np.array_equal(x.intensities, y.intensities) and np.array_equal(_bits(x.intensity_map), _bits(y.intensity_map))
        assert np.array_equal(_bits(x.points), _bits(y.points)) and np.array_equal(x.mask, y.mask)
    # the oracle on the downloaded level 0
    lib, ptr = O.load(), _abi.ptr
    luma = np.empty((480, 640), np.uint8)
    lib.orc_rgb_to_luma_u8(ptr(np.ascontiguousarray(host.colors)), 640 * 480, ptr(luma))
    k = host.intrinsics
    pyr = [O.Frame(host.points, host.mask, k.fx, k.fy, k.cx, k.cy, host.normals, luma.reshape(-1), O.intensity_map(luma),
                   colors=np.ascontiguousarray(host.colors))]
    for _ in range(2):
        pyr.append(O.pyr_down(pyr[-1]))
    st, T_ref = O.multiscale_align(prm.to_c_array(), 3, pyr, oracle_pyramid("sample1", 1, use_bilateral=False), threads=4)
    ang, tr = transform_diff(T, T_ref)
    print(f"rendered target against the oracle: {ang:.3e} rad, {tr:.3e} m")
    assert st == 0 and ang <= 1e-4 and tr <= 1e-4, (ang, tr)
    for lv in (*tgt, *tgt_up, *src):
        lv.free()


# ---- 6. errors on the device ----------------------------------------------------------------------------------------

def _free_device_memory():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_errors_on_the_device(ctx):
    own = Context(0)
    m = _filled_map(own)
    cloud = m.extract()
    cam = CameraIntrinsics(60.0, 61.0, 31.5, 23.5, 64, 48)
    image = m.render(cam, None, 0.025)  # the scratch and the arena pool of this context exist from here on
    image.free()
    stats = m.stats()
    view = cloud.view()
    lib = own.lib

    def call(which, fx=60.0, fy=61.0, w=30000, h=30000, radius=0.0, out=True):
        handle = C.c_void_p(SENTINEL)
        ref = C.byref(handle) if out else None
        if which == "cloud":
            st = lib.a3d_point_cloud_render_device(own.handle, C.byref(view), cloud.d_colors, None, fx, fy, 31.5, 23.5, w, h,
                                                   radius, None, ref)
        else:
            st = lib.a3d_voxel_map_render(m.handle, None, fx, fy, 31.5, 23.5, w, h, radius, None, ref)
        assert handle.value == SENTINEL
        return st

    before = _free_device_memory()
    for _ in range(50):  # (each would take a 7 GB z-buffer if anything were allocated before the refusal)
        for which in ("cloud", "map"):
            assert call(which, radius=float("nan")) == INVALID
            assert call(which, radius=-0.5) == INVALID
            assert call(which, fx=0.0) == INVALID
            assert call(which, fy=-3.0) == INVALID
            assert call(which, w=0) == INVALID
            assert call(which, w=1 << 16, h=1 << 15) == INVALID
            assert call(which, w=64, h=48, out=False) == INVALID
    # nothing was allocated and kept: a leak of one z-buffer per call would be hundreds of GB (other users of the device
    # may move the figure by a little)
    assert before - _free_device_memory() < (256 << 20)
    assert m.stats() == stats
    # the wrappers: wrong types raise, there is no host fallback; the index plane is [h][w]
    with pytest.raises(TypeError):
        cloud.render((60.0, 61.0, 31.5, 23.5, 64, 48))
    with pytest.raises(TypeError):
        m.render(cam, camera_to_world=np.eye(4, dtype=F))
    with pytest.raises(A3dError):
        cloud.render(cam, None, radius=-1.0)
    with pytest.raises(A3dError):
        m.render(CameraIntrinsics(60.0, 61.0, 31.5, 23.5, 0, 48))
    image, index = m.render(CameraIntrinsics(60.0, 61.0, 31.5, 23.5, 33, 7), None, 0.0, return_index=True)
    assert index.shape == (7, 33) == image.shape
    image.free()
    # a cloud and a map only ever render on their own context: the image is that context's
    image = cloud.render(cam)
    assert image.ctx is own
    image.free()
    assert m.stats() == stats
    cloud.free()
    m.free()
    own.close()
