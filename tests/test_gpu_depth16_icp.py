"""Level 0 of device-built pyramids carries the filtered u16 depth plane its points were back-projected from, and the
alignment kernel rebuilds both level-0 points from it instead of reading them (DEPTH16, image_icp.hip).  The poses must
not move by a single bit: against the diagnostics build with the points read (A3D_ICP_DEPTH16=0), against the same
pyramids downloaded and uploaded again (never flagged), as a batch, a lone pair and under pinned tiling, with and without
the bilateral filter, at sizes that are not multiples of 32 or 4 and at more than one depth scale.  The plane's premise is
checked pixel by pixel against a host back-projection in f32."""
import ctypes as C
import os

import numpy as np
import pytest

from align3d_amd import (BilateralFilter, CameraIntrinsics, IcpParams, MsIcpParams, MultiscaleAlign, MultiscaleAlignBatch,
                         RangeImageBuilder, SlamTbDataset, _abi)
from data_util import GOLDEN

pytestmark = pytest.mark.gpu


def _frames(w, h, holes):
    """Four sample1 frames cropped (or edge-padded) to w x h, optionally with large invalid regions."""
    ds = SlamTbDataset.load(os.path.join(GOLDEN, "rgbd", "sample1"))
    cam, _, _, scale = ds.get(0)
    out = []
    for i in (0, 1, 4, 5):
        _, depth, rgb, _ = ds.get(i)
        ph, pw = max(0, h - depth.shape[0]), max(0, w - depth.shape[1])
        depth = np.pad(depth, ((0, ph), (0, pw)), mode="edge")[:h, :w].copy()
        rgb = np.pad(rgb, ((0, ph), (0, pw), (0, 0)), mode="edge")[:h, :w].copy()
        if holes:
            r0 = (i * 37) % max(1, h // 2)
            depth[r0:r0 + h // 5, w // 6:w // 2] = 0
        out.append((np.ascontiguousarray(depth), np.ascontiguousarray(rgb)))
    k = w / 640.0
    return CameraIntrinsics(cam.fx * k, cam.fy * k, cam.cx * k, cam.cy * k, w, h), out, scale


def _build(c, cam, frames, scale, filt):
    b = RangeImageBuilder(c)
    if filt:
        b = b.with_bilateral_filter(BilateralFilter.default())
    return b.build_many(cam, frames, scale)


def _host_copy(pyr):
    host = [lv.download(colors=False) for lv in pyr]
    for lv in host:
        lv._device = None
    return host


PAIRS = [(0, 1), (2, 3), (1, 2)]


def _batch(c, prm, tp, sp):
    """The poses as float32 matrices with each pair's status appended (a failed solve is an outcome to match too)."""
    b = MultiscaleAlignBatch(c, prm, tp, sp)
    poses, status = b.align()
    b.free()
    m = np.stack([p.matrix() for p in poses]).astype(np.float32).reshape(len(poses), -1)
    return np.concatenate([m, status.view(np.float32)[:, None]], 1)


def _lone(c, prm, t, s):
    a = MultiscaleAlign.new(c, prm, t)
    m = a.align(s).matrix()
    a.free()
    return np.asarray(m, np.float32)[None]


def _same(a, b):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.abs(a - b).max()


CASES = [  # (w, h, holes, bilateral filter, depth scale: None = the dataset's)
    (640, 480, True, True, None),
    (640, 480, True, False, 0.001),
    (150, 90, False, True, None),
    (641, 479, True, False, None),
    (641, 479, False, True, 0.0012),
]


@pytest.mark.parametrize("w,h,holes,filt,scale", CASES)
def test_depth16_changes_no_bit(ctx, diag_ctx, monkeypatch, w, h, holes, filt, scale):
    cam, frames, ds_scale = _frames(w, h, holes)
    scale = ds_scale if scale is None else scale
    pyr = _build(ctx, cam, frames, scale, filt)
    dpyr = _build(diag_ctx, cam, frames, scale, filt)
    host = [_host_copy(p) for p in pyr]
    ms3x15 = MsIcpParams.repeat(3, IcpParams())
    for prm in (MsIcpParams.default(), ms3x15):
        tp, sp = [pyr[a] for a, _ in PAIRS], [pyr[b] for _, b in PAIRS]
        fast = _batch(ctx, prm, tp, sp)
        assert not fast[:, -1].view(np.int32).any()
        # the diagnostics build's own pyramids: points rebuilt, then points read
        dtp, dsp = [dpyr[a] for a, _ in PAIRS], [dpyr[b] for _, b in PAIRS]
        _same(fast, _batch(diag_ctx, prm, dtp, dsp))
        monkeypatch.setenv("A3D_ICP_DEPTH16", "0")
        _same(fast, _batch(diag_ctx, prm, dtp, dsp))
        monkeypatch.delenv("A3D_ICP_DEPTH16")
        # the same pyramids uploaded from host arrays (never flagged: the points are read)
        htp, hsp = [host[a] for a, _ in PAIRS], [host[b] for _, b in PAIRS]
        _same(fast, _batch(ctx, prm, htp, hsp))
        # a mixed batch (one pair uploaded) falls back to reading the points everywhere: the same bits
        _same(fast, _batch(ctx, prm, [htp[0]] + tp[1:], [hsp[0]] + sp[1:]))
        # a lone pair (a3d_multiscale_align)
        _same(_lone(ctx, prm, pyr[0], pyr[1]), _lone(ctx, prm, host[0], [lv.device(ctx) for lv in host[1]]))
        # pinned tiling
        ctx.set_tiling(24)
        try:
            _same(_batch(ctx, prm, tp, sp), _batch(ctx, prm, htp, hsp))
        finally:
            ctx.set_tiling(0)


def _download_depth16(c, lv):
    h, w = lv.shape
    out = np.empty((h, w), np.uint16)
    bp = (C.c_float * 5)()
    flag = C.c_int32()
    st = c.lib.a3d_range_image_download_depth16(lv.handle, _abi.ptr(out), bp, C.byref(flag))
    return st, out, np.array(bp[:], np.float32), flag.value


@pytest.mark.parametrize("w,h,holes,filt,scale", CASES)
def test_depth_plane_back_projects_to_the_points(diag_ctx, w, h, holes, filt, scale):
    """Pixel by pixel: the stored level-0 point is the f32 back-projection of the stored depth (the operations of
    backproject_px in their order; numpy's f32 division is IEEE), and mask == (depth != 0)."""
    cam, frames, ds_scale = _frames(w, h, holes)
    scale = ds_scale if scale is None else scale
    for pyr in _build(diag_ctx, cam, frames, scale, filt):
        st, d, bp, flag = _download_depth16(diag_ctx, pyr[0])
        assert st == _abi.A3D_OK and flag == 1
        fx, fy, cx, cy, sc = (np.float32(v) for v in bp)
        assert (fx, fy, cx, cy, sc) == (np.float32(cam.fx), np.float32(cam.fy), np.float32(cam.cx), np.float32(cam.cy),
                                        np.float32(scale))
        got = pyr[0].download(normals=False, intensity=False, colors=False)
        rows, cols = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        z = d.astype(np.float32) * sc
        x = ((cols - cx) * z) / fx
        y = ((rows - cy) * z) / fy
        ref = np.stack([x, y, z], -1).astype(np.float32)
        ref[d == 0] = 0.0
        assert np.array_equal(got.points.view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(got.mask != 0, d != 0)
        assert (d != 0).any()
        # only level 0 carries a plane
        for lv in pyr[1:]:
            assert _download_depth16(diag_ctx, lv)[0] == _abi.A3D_MISSING_FIELD
    # an uploaded image never does
    up = _host_copy(_build(diag_ctx, cam, frames[:1], scale, filt)[0])[0].device(diag_ctx)
    assert _download_depth16(diag_ctx, up)[0] == _abi.A3D_MISSING_FIELD
