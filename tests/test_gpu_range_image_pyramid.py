"""RangeImage::pyramid and compute_intensity / compute_intensity_map (src/range_image/structure.rs:266-351) on resident
images from any source (a3d_range_image_pyramids, a3d_range_image_compute_intensity, a3d_range_image_set_colors): bit for
bit the device builder's own pyramids, and bit for bit the oracle on images that do not come from depth."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (A3dError, BilateralFilter, CameraIntrinsics, Context, MsIcpParams, MultiscaleAlign, RangeImage,
                         RangeImageBuilder, _abi, compute_intensity_batch, pyramids)
from align3d_amd.range_image import DeviceRangeImage
from data_util import SlamTbSample
from gpu_util import oracle_pyramid, transform_diff

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _k(intr):
    return (intr.fx, intr.fy, intr.cx, intr.cy)


def _assert_same(a, b):
    """Two host RangeImages, array for array and bit for bit."""
    assert np.array_equal(a.mask, b.mask)
    assert np.array_equal(_bits(a.points), _bits(b.points))
    for name in ("normals", "intensity_map"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(_bits(x), _bits(y)), name
    for name in ("colors", "intensities"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(x, y), name
    assert _k(a.intrinsics) == _k(b.intrinsics)


def _free(*levels):
    for lv in levels:
        lv.free()


# ---- 1. the builder's own pyramid ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(480, 640), (90, 150), (134, 262), (34, 66)])
@pytest.mark.parametrize("bilateral", [False, True])
def test_builder_equivalence(ctx, shape, bilateral):
    h, w = shape
    s = SlamTbSample("sample1")
    depth, rgb = s.load(0)
    depth, rgb = np.ascontiguousarray(depth[:h, :w]), np.ascontiguousarray(rgb[:h, :w])
    cam = CameraIntrinsics(*s.intrinsics(0), w, h)
    for sigma in (0.6, 1.0, 2.0, 3.0):
        b = RangeImageBuilder(ctx).blur_sigma(sigma)
        if bilateral:
            b = b.with_bilateral_filter(BilateralFilter.default())
        ref = b.pyramid_levels(3).build(cam, depth, rgb, s.depth_scale(0))
        lv0 = b.pyramid_levels(1).build(cam, depth, rgb, s.depth_scale(0))[0]
        got = lv0.pyramid(3, sigma)
        assert got[0] is lv0 and len(got) == 3
        for g, r in zip(got, ref):
            _assert_same(g.download(), r.download())
        _free(*got, *ref)


# ---- 2. oracle parity on images that do not come from depth -------------------------------------------------------

SPECIAL = np.asarray([0.0, -0.0, 1e-42, -1e-39, 3e38, -3.4e38, 1e30, np.nan, np.inf, -np.inf], np.float32)


def _random_image(seed, h, w, normals=True, colors=True):
    rng = np.random.default_rng(seed)

    def vectors():
        v = (rng.standard_normal((h, w, 3)) * 10).astype(np.float32)
        flat = v.reshape(-1)
        idx = rng.choice(flat.size, size=max(1, flat.size // 12), replace=False)
        flat[idx] = rng.choice(SPECIAL, size=idx.size)
        return v

    pts = vectors()
    mask = rng.choice(np.asarray([0, 1, 1, 1, 2, 255], np.uint8), size=(h, w))
    return RangeImage(pts, mask, CameraIntrinsics(525.0, 523.5, w / 2 - 0.5, h / 2 + 0.25, w, h),
                      normals=vectors() if normals else None,
                      colors=rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if colors else None)


def _oracle_pyramid(host, levels, sigma, with_intensity):
    """RangeImage::pyramid through the oracle, without assuming normals or colours (oracle_lib.pyr_down does)."""
    lib, ptr = O.load(), _abi.ptr
    k = host.intrinsics
    pyr = [dict(points=host.points, mask=host.mask, normals=host.normals, colors=host.colors, k=(k.fx, k.fy, k.cx, k.cy))]
    for _ in range(levels - 1):
        p = pyr[-1]
        sh, sw = p["mask"].shape
        dh, dw = sh // 2, sw // 2
        pts, mask = np.empty((dh, dw, 3), np.float32), np.empty((dh, dw), np.uint8)
        lib.orc_resize_range_points(ptr(p["points"]), ptr(p["mask"]), sw, sh, dw, dh, ptr(pts), ptr(mask))
        nrm = col = None
        if p["normals"] is not None:
            nrm = np.empty((dh, dw, 3), np.float32)
            lib.orc_resize_range_normals(ptr(p["normals"]), ptr(p["mask"]), sw, sh, dw, dh, ptr(nrm))
        if p["colors"] is not None:
            col = np.empty((dh, dw, 3), np.uint8)
            lib.orc_rgb_pyr_down(ptr(p["colors"]), sw, sh, sigma, ptr(col))
        pyr.append(dict(points=pts, mask=mask, normals=nrm, colors=col, k=tuple(x * 0.5 for x in p["k"])))
    for p in pyr:
        p["intensities"] = p["imap"] = None
        if with_intensity:
            h, w = p["mask"].shape
            luma = np.empty((h, w), np.uint8)
            lib.orc_rgb_to_luma_u8(ptr(np.ascontiguousarray(p["colors"])), w * h, ptr(luma))
            p["intensities"], p["imap"] = luma.reshape(-1), O.intensity_map(luma)
    return pyr


def _assert_oracle_level(dev, ref):
    got = dev.download(normals=ref["normals"] is not None, intensity=ref["intensities"] is not None,
                       colors=ref["colors"] is not None)
    _assert_same(got, RangeImage(ref["points"], ref["mask"], CameraIntrinsics(*ref["k"], 0, 0), normals=ref["normals"],
                                 colors=ref["colors"], intensities=ref["intensities"], intensity_map=ref["imap"]))


def _upload(ctx, host):
    dev = DeviceRangeImage(ctx, host)
    if host.colors is not None:
        dev.set_colors(host.colors)
    return dev


@pytest.mark.parametrize("shape", [(48, 64), (37, 101), (90, 150), (34, 20)])
def test_oracle_parity_and_level0_untouched(ctx, shape):
    h, w = shape
    seed = 0
    for levels in range(1, 6):
        if (h >> (levels - 1)) < 2 or (w >> (levels - 1)) < 2:
            continue
        for normals, colors in ((True, True), (False, True), (True, False), (False, False)):
            seed += 1
            sigma = (0.0, 1.0, 2.5, 0.6)[seed % 4]
            host = _random_image(seed, h, w, normals, colors)
            dev = _upload(ctx, host)
            before = dev.download(normals=normals, intensity=False, colors=colors)
            got = dev.pyramid(levels, sigma, with_intensity=colors)
            ref = _oracle_pyramid(host, levels, sigma, with_intensity=colors)
            assert len(got) == levels and got[0] is dev
            for g, r in zip(got, ref):
                _assert_oracle_level(g, r)
            # level 0: points, mask, normals and colours bit-unchanged; intensities only with with_intensity
            after = dev.download(normals=normals, intensity=False, colors=colors)
            _assert_same(before, after)
            if not colors:
                with pytest.raises(A3dError):
                    dev.download(normals=False, intensity=True, colors=False)
            _free(*got)


# ---- 3. a batch gives the bits of one call per image --------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 37, 64, 65])
def test_batch_equals_singles(ctx, n):
    hosts = [_random_image(1000 + i, 40, 52, normals=i % 3 != 0) for i in range(n)]
    batch = pyramids([_upload(ctx, h) for h in hosts], 4, 1.0)
    for host, got in zip(hosts, batch):
        single = _upload(ctx, host).pyramid(4, 1.0)
        for g, s in zip(got, single):
            _assert_same(g.download(normals=host.normals is not None), s.download(normals=host.normals is not None))
        _free(*single, *got)


# ---- 4. compute_intensity on its own ------------------------------------------------------------------------------

def test_compute_intensity_matches_oracle(ctx):
    # one batch of mixed widths (a cell per thread), one of widths that are multiples of four (four cells per thread)
    for shapes in ([(48, 64), (37, 101), (1, 1), (5, 3), (2, 7)], [(8, 12), (16, 640), (3, 4)]):
        hosts = [_random_image(2000 + i, h, w, normals=False) for i, (h, w) in enumerate(shapes)]
        devs = [_upload(ctx, h) for h in hosts]
        compute_intensity_batch(devs)
        devs[0].compute_intensity()  # again, in place over the first result
        for host, dev in zip(hosts, devs):
            ref = _oracle_pyramid(host, 1, 1.0, with_intensity=True)[0]
            got = dev.download(normals=False)
            assert np.array_equal(got.intensities, ref["intensities"])
            assert np.array_equal(_bits(got.intensity_map), _bits(ref["imap"]))
            dev.free()
    # an uploaded image that came with intensities and a map: recomputed in place from the colours
    fr = oracle_pyramid("sample1", 0, levels=1, use_bilateral=False)[0]
    host = RangeImage(fr.points, fr.mask, CameraIntrinsics(fr.fx, fr.fy, fr.cx, fr.cy, fr.w, fr.h), normals=fr.normals,
                      colors=fr.colors, intensities=np.zeros_like(fr.intensities),
                      intensity_map=np.zeros_like(fr.intensity_map))
    dev = _upload(ctx, host).compute_intensity()
    got = dev.download()
    assert np.array_equal(got.intensities, fr.intensities)
    assert np.array_equal(_bits(got.intensity_map), _bits(fr.intensity_map))
    dev.free()


# ---- 6. end to end: host level-0 images -> device pyramid -> MultiscaleAlign --------------------------------------

def _pose_bits(T):
    p = T.to_c()
    return np.asarray(list(p.t) + list(p.q), np.float32).view(np.uint32)


def test_end_to_end_multiscale_align(ctx):
    s = SlamTbSample("sample1")
    prm = MsIcpParams.default().customize(lambda i, p: setattr(p, "max_iterations", 3))
    builder = RangeImageBuilder(ctx).with_bilateral_filter(BilateralFilter.default())

    def build(i, levels):
        return builder.pyramid_levels(levels).build(CameraIntrinsics(*s.intrinsics(i), 640, 480), *s.load(i), s.depth_scale(i))

    hosts = []
    for i in (0, 1):
        lv0 = build(i, 1)[0]
        hosts.append(lv0.download())
        lv0.free()
    tgt, src = (h.pyramid(ctx, 3) for h in hosts)
    T = MultiscaleAlign.new(ctx, prm, tgt).align(src)
    full = [build(i, 3) for i in (0, 1)]
    T_builder = MultiscaleAlign.new(ctx, prm, full[0]).align(full[1])
    assert np.array_equal(_pose_bits(T), _pose_bits(T_builder))
    st, T_ref = O.multiscale_align(prm.to_c_array(), 3, oracle_pyramid("sample1", 0), oracle_pyramid("sample1", 1), threads=4)
    ang, tr = transform_diff(T, T_ref)
    assert st == 0 and ang <= 1e-4 and tr <= 1e-4, (ang, tr)
    _free(*tgt, *src, *full[0], *full[1])


# ---- 7. errors: the stated status, no handle, level 0 untouched ---------------------------------------------------

def test_errors(ctx):
    lib = ctx.lib
    host = _random_image(3000, 32, 48)
    dev = _upload(ctx, host)
    before = dev.download(intensity=False)

    def call(images, levels, sigma, with_intensity):
        arr = (C.c_void_p * len(images))(*[None if im is None else im.handle.value for im in images])
        out = (C.c_void_p * 64)()
        st = lib.a3d_range_image_pyramids(arr, len(images), levels, sigma, with_intensity, out)
        assert all(o is None for o in out)
        return st

    INVALID, MISSING = _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD
    assert call([dev], 3, 3.5, 1) == INVALID
    assert call([dev], 2, float("nan"), 1) == INVALID
    assert call([dev], 0, 1.0, 1) == INVALID
    assert call([dev], 17, 1.0, 1) == INVALID
    assert call([dev], 6, 1.0, 1) == INVALID  # 32 >> 5 = 1: the coarsest side would be below 2
    other = _upload(ctx, _random_image(3001, 36, 48))
    assert call([dev, other], 3, 1.0, 1) == INVALID  # mixed sizes
    assert call([dev, None], 3, 1.0, 1) == INVALID   # a null handle
    ctx2 = Context(0)
    foreign = _upload(ctx2, host)
    assert call([dev, foreign], 3, 1.0, 1) == INVALID  # mixed contexts
    foreign.free()
    ctx2.close()
    plain = DeviceRangeImage(ctx, _random_image(3002, 32, 48, colors=False))
    assert call([plain], 3, 1.0, 1) == MISSING  # with_intensity without colours
    assert call([dev, plain], 3, 1.0, 1) == MISSING
    # set_colors on an image that has colours: a builder image, or one that was given them already
    s = SlamTbSample("sample1")
    built = RangeImageBuilder(ctx).pyramid_levels(1).build(CameraIntrinsics(*s.intrinsics(0), 640, 480), *s.load(0),
                                                           s.depth_scale(0))[0]
    rgb = np.zeros((480, 640, 3), np.uint8)
    assert lib.a3d_range_image_set_colors(built.handle, _abi.ptr(rgb)) == INVALID
    assert lib.a3d_range_image_set_colors(dev.handle, _abi.ptr(host.colors)) == INVALID
    assert lib.a3d_range_image_compute_intensity((C.c_void_p * 1)(plain.handle.value), 1) == MISSING
    # level 0 untouched by every failed call, and still without intensities
    _assert_same(before, dev.download(intensity=False))
    with pytest.raises(A3dError):
        dev.download(intensity=True)
    assert np.array_equal(built.download().colors, s.load(0)[1])
    _free(dev, other, plain, built)
