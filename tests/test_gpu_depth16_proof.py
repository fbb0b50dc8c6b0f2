"""Level 0 of the image ICP rebuilds its points in straight-line code (backproject_px_proven) only for images whose size and
back-projection constants pass the host proof (backproject_proven, devmath.hpp); a batch with any image that fails it
reads the points.  Either way the poses are the diagnostics build's with the points read (A3D_ICP_DEPTH16=0), bit for
bit: principal points on a pixel (zero numerators), negative focal lengths, several depth scales, batches, lone pairs and
mixed batches where one pair's images fail the proof."""
import ctypes as C
import os

import numpy as np
import pytest

from align3d_amd import CameraIntrinsics, IcpParams, MsIcpParams, MultiscaleAlign, MultiscaleAlignBatch, RangeImageBuilder, SlamTbDataset, _abi
from data_util import GOLDEN

pytestmark = pytest.mark.gpu


def _frames(w, h):
    ds = SlamTbDataset.load(os.path.join(GOLDEN, "rgbd", "sample1"))
    cam, _, _, scale = ds.get(0)
    out = []
    for i in (0, 1, 4, 5):
        _, depth, rgb, _ = ds.get(i)
        ph, pw = max(0, h - depth.shape[0]), max(0, w - depth.shape[1])
        depth = np.pad(depth, ((0, ph), (0, pw)), mode="edge")[:h, :w].copy()
        rgb = np.pad(rgb, ((0, ph), (0, pw), (0, 0)), mode="edge")[:h, :w].copy()
        out.append((np.ascontiguousarray(depth), np.ascontiguousarray(rgb)))
    return cam, out, scale


def _proven(c, lv):
    h, w = lv.shape
    plane = np.empty((h, w), np.uint16)
    bp = (C.c_float * 5)()
    flag, ok = C.c_int32(), C.c_int32()
    assert c.lib.a3d_range_image_download_depth16(lv.handle, _abi.ptr(plane), bp, C.byref(flag)) == _abi.A3D_OK
    assert flag.value == 1
    assert c.lib.a3d_backproject_proven(w, h, bp, C.byref(ok)) == _abi.A3D_OK
    return ok.value


def _batch(c, prm, tp, sp):
    b = MultiscaleAlignBatch(c, prm, tp, sp)
    poses, status = b.align()
    b.free()
    m = np.stack([p.matrix() for p in poses]).astype(np.float32).reshape(len(poses), -1)
    return np.concatenate([m, status.view(np.float32)[:, None]], 1)


def _lone(c, prm, t, s):
    """The pose, or the status of a failed solve (an outcome to match too)."""
    a = MultiscaleAlign.new(c, prm, t)
    try:
        return np.asarray(a.align(s).matrix(), np.float32)[None]
    except _abi.A3dError as e:
        return np.array([[e.status]], np.int32).view(np.float32)
    finally:
        a.free()


def _same(a, b):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.abs(a - b).max()


PAIRS = [(0, 1), (2, 3)]

CASES = [  # (w, h, fx sign, cx, cy: None = the dataset's, depth scale: None = the dataset's, proof expected)
    (640, 480, 1, 320.0, 240.0, None, 1),     # a column and a row on the principal point: +0 numerators
    (641, 479, 1, 320.0, 239.0, 0.0002, 1),
    (640, 480, -1, 319.5, 239.5, 0.001, 1),   # a negative focal length without a zero numerator
    (150, 90, 1, None, None, 0.0012, 1),
    (640, 480, -1, 320.0, 240.0, None, 0),    # negative fx with a column at cx: the points are read
    (160, 120, 1, None, None, 200.0, 0),      # |(col - cx) z| reaches 1e9
]


@pytest.mark.parametrize("w,h,sx,cx,cy,scale,expect", CASES)
def test_depth16_proof_changes_no_bit(ctx, diag_ctx, monkeypatch, w, h, sx, cx, cy, scale, expect):
    cam0, frames, ds_scale = _frames(w, h)
    k = w / 640.0
    cam = CameraIntrinsics(sx * cam0.fx * k, cam0.fy * k, cam0.cx * k if cx is None else cx,
                           cam0.cy * k if cy is None else cy, w, h)
    scale = ds_scale if scale is None else scale
    pyr = RangeImageBuilder(ctx).build_many(cam, frames, scale)
    dpyr = RangeImageBuilder(diag_ctx).build_many(cam, frames, scale)
    assert all(_proven(diag_ctx, p[0]) == expect for p in dpyr)
    # a batch of images that pass the proof (the bench's own size and camera) to mix with
    okcam, okframes, okscale = _frames(640, 480)
    okpyr = RangeImageBuilder(ctx).build_many(okcam, okframes, okscale)
    dokpyr = RangeImageBuilder(diag_ctx).build_many(okcam, okframes, okscale)
    assert all(_proven(diag_ctx, p[0]) == 1 for p in dokpyr)
    for prm in (MsIcpParams.default(), MsIcpParams.repeat(3, IcpParams())):
        tp, sp = [pyr[a] for a, _ in PAIRS], [pyr[b] for _, b in PAIRS]
        dtp, dsp = [dpyr[a] for a, _ in PAIRS], [dpyr[b] for _, b in PAIRS]
        mtp, msp = tp + [okpyr[0]], sp + [okpyr[1]]
        dmtp, dmsp = dtp + [dokpyr[0]], dsp + [dokpyr[1]]
        fast, mixed, lone = _batch(ctx, prm, tp, sp), _batch(ctx, prm, mtp, msp), _lone(ctx, prm, pyr[0], pyr[1])
        _same(fast, _batch(diag_ctx, prm, dtp, dsp))
        _same(mixed, _batch(diag_ctx, prm, dmtp, dmsp))
        monkeypatch.setenv("A3D_ICP_DEPTH16", "0")
        _same(fast, _batch(diag_ctx, prm, dtp, dsp))
        _same(mixed, _batch(diag_ctx, prm, dmtp, dmsp))
        _same(lone, _lone(diag_ctx, prm, dpyr[0], dpyr[1]))
        monkeypatch.delenv("A3D_ICP_DEPTH16")
