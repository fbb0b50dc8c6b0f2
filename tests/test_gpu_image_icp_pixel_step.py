"""Level 0 of image ICP on device-built pyramids rebuilds both points of a pixel from the depth planes.  Its pixel loop
carries the source pixel's row and column across the thread's stride of 256 pixels instead of dividing every index by the
width (src_advance, image_icp.hip), divides by the focal lengths in three operations where the host sweep allows it
(div_short, devmath.hpp), and converts the gathered depth straight from the register's low half.  None of it may move a
bit: the product build against the diagnostics build with A3D_ICP_DEPTH16=0, which reads the points the frame builder
stored and uses none of that arithmetic — counts, all 58 sums and final poses bit for bit — and also against the
diagnostics build in its default form and with A3D_ICP_SHORT_DIV=0 (the five-operation instantiation); the product
against the oracle with the project's tolerances (counts exact, sums within 1e-6 of its f64 sums, poses within 1e-4).

Shapes, chosen for the carry: 24 x 16 (width below the stride: ten rows per step, lanes out of range), 256 x 6
(remainder 0), 257 x 5 (a wrap with remainder 1), 300 x 7 (a wrap on some steps only), 640 x 4 under pinned tilings 1
(ten steps per thread) and 3 (tiles that begin mid-row, a partial last tile), and the 64 x 48 pyramids of
test_gpu_image_icp_step_order through a batch (all three levels).  Every frame has depth holes on both sides.  The
cameras of 24 x 16, 256 x 6 and 300 x 7 have their principal point on an integer column of the image, so under the
identity pose the points of that column lie exactly on an optical axis plane and the projection's numerator is an exact
zero (as is the back-projection's +0), and every depth-0 source pixel reaches the projection with z = 0: the waves that
hold them take the plain division.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_image_icp_step_order as SO
from align3d_amd import CameraIntrinsics, IcpParams, ImageIcp, MsIcpParams, RangeImageBuilder, Transform, _abi, synth
from gpu_util import gn_rel_err, small_pose, transform_diff

pytestmark = pytest.mark.gpu

ACC_TOL = 1e-6              # the project's own (tests/test_gpu_image_icp_projection.py)
ROT_TOL = TRANS_TOL = 1e-4  # the project's own (tests/test_gpu_image_icp.py)
STORED, FIVE_OPS = "A3D_ICP_DEPTH16", "A3D_ICP_SHORT_DIV"

_built = {}


def _level0(ctx, diag_ctx, w, h, cam=None):
    """Frames 0 and 2 of the synthetic stream at w x h built on both libraries (one level), with the host copy of the
    product's; once per size and camera."""
    cam = cam or SO._camera(w, h)
    key = (w, h, cam.fx, cam.cx)
    if key not in _built:
        frames = SO._frames(w, h)
        out = {}
        for name, c in (("product", ctx), ("diag", diag_ctx)):
            pyr = RangeImageBuilder(c).pyramid_levels(1).build_many(cam, list(frames), synth.DEPTH_SCALE)
            out[name] = (pyr[0][0], pyr[1][0])
        out["host"] = tuple(SO._frame_of(SO._host_copy([im])[0]) for im in out["product"])
        SO._assert_rebuilt_from_depth(diag_ctx, out["diag"][0])
        _built[key] = out
    return _built[key]


def _short_proven(diag_ctx, im):
    h, w = im.shape
    depth, bp, flag, ok = np.empty((h, w), np.uint16), (C.c_float * 5)(), C.c_int32(), C.c_int32()
    assert diag_ctx.lib.a3d_range_image_download_depth16(im.handle, _abi.ptr(depth), bp, C.byref(flag)) == 0
    assert diag_ctx.lib.a3d_backproject_short_division_proven(w, h, bp, C.byref(ok)) == 0
    return ok.value == 1


def _poses(ft):
    small = small_pose(3, rot=2.0 / ft.fx, trans=0.003)
    return [("identity", Transform.eye()), ("small", small), ("inverse", small.inverse())]


def _one_pass(ctx, diag_ctx, monkeypatch, built, what):
    ft, fs = built["host"]
    prm = IcpParams(max_iterations=1, max_distance=SO.MAX_DISTANCE, max_color_distance=SO.MAX_COLOR_DISTANCE)
    for name, T in _poses(ft):
        want = ImageIcp.new(ctx, prm, built["product"][0]).accumulate(built["product"][1], T)
        for knob, tag in ((STORED, "stored points"), (FIVE_OPS, "five operations"), (None, "diagnostics build")):
            if knob:
                monkeypatch.setenv(knob, "0")
            got = ImageIcp.new(diag_ctx, prm, built["diag"][0]).accumulate(built["diag"][1], T)
            if knob:
                monkeypatch.delenv(knob)
            SO._same_sums(got, want, (what, name, tag))
        st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, T.to_c(), accum_f64=True)
        assert st == 0, (what, name)
        g_ref, c_ref = g_ref.as_dict(), c_ref.as_dict()
        print(what, name, "counts", want[0]["count"], g_ref["count"], want[1]["count"], c_ref["count"])
        assert want[0]["count"] == g_ref["count"] and want[1]["count"] == c_ref["count"], (what, name)
        assert g_ref["count"] > 0, (what, name)
        for got, ref, tag in ((want[0], g_ref, "geometry"), (want[1], c_ref, "colour")):
            eh, eg, es = gn_rel_err(got, ref)
            print(what, name, tag, eh, eg, es)
            assert eh < ACC_TOL and eg < ACC_TOL and es < ACC_TOL, (what, name, tag, eh, eg, es)


def _axis_content(built, cam):
    """What the identity pose meets: depth-0 source pixels (z = 0 in the projection) and, where the principal point lies
    on an integer column of the image, valid source pixels on it (x is an exact zero: zero numerators).  Returns whether
    there is such a column."""
    fs = built["host"][1]
    mask = fs.mask.reshape(fs.h, fs.w) != 0
    assert (~mask).any() and mask.any()
    if not (float(cam.cx).is_integer() and 0 <= cam.cx < fs.w):
        return False
    on_col = mask[:, int(cam.cx)]
    assert (fs.points.reshape(fs.h, fs.w, 3)[:, int(cam.cx), 0][on_col] == 0).all()
    return bool(on_col.any())


@pytest.mark.parametrize("w,h,tiling", [(24, 16, 0), (256, 6, 0), (257, 5, 0), (300, 7, 0), (640, 4, 1), (640, 4, 3)],
                         ids=["24x16", "256x6", "257x5", "300x7", "640x4-tiles1", "640x4-tiles3"])
def test_one_pass(ctx, diag_ctx, monkeypatch, w, h, tiling):
    built = _level0(ctx, diag_ctx, w, h)
    assert _short_proven(diag_ctx, built["diag"][0])  # the three-operation instantiation is what the product runs here
    # (257 x 5: cx = 128.5, no zero numerator; 640 x 4: the four pixels of column 320 of the source frame are invalid)
    assert _axis_content(built, SO._camera(w, h)) or w in (257, 640)
    for c in (ctx, diag_ctx):
        c.set_tiling(tiling)
    try:
        _one_pass(ctx, diag_ctx, monkeypatch, built, (w, h, tiling))
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)


def test_camera_that_fails_the_short_division_sweep(ctx, diag_ctx, monkeypatch):
    """A batch whose images fail the sweep runs the five-operation instantiation and still matches.  No focal length that
    fails is known (2000 of 2000 random ones pass, tests/test_image_icp_pixel_step_cpu.py): the candidates below are
    asked through the hook, and without a failing one the case is skipped.  (The five-operation instantiation itself is
    compared in every case of test_one_pass, through the diagnostics build's A3D_ICP_SHORT_DIV=0.)"""
    w, h = 24, 16
    base = SO._camera(w, h)
    failing = None
    for k in range(24):
        f = float(np.float32(base.fx * (1.0 + 0.013 * k)))
        ok = C.c_int32()
        bp = (C.c_float * 5)(f, f, base.cx, base.cy, synth.DEPTH_SCALE)
        assert diag_ctx.lib.a3d_backproject_proven(w, h, bp, C.byref(ok)) == 0
        if not ok.value:
            continue
        assert diag_ctx.lib.a3d_backproject_short_division_proven(w, h, bp, C.byref(ok)) == 0
        if not ok.value:
            failing = f
            break
    if failing is None:
        pytest.skip("no focal length that fails the exhaustive short-division sweep is known")
    cam = CameraIntrinsics(failing, failing, base.cx, base.cy, w, h)
    built = _level0(ctx, diag_ctx, w, h, cam)
    assert not _short_proven(diag_ctx, built["diag"][0])
    _one_pass(ctx, diag_ctx, monkeypatch, built, ("failing sweep", failing))


@pytest.mark.parametrize("tiling", [0, 3], ids=["throughput", "tiles3"])
def test_batched_poses_all_levels(ctx, diag_ctx, monkeypatch, tiling):
    """64 x 48 pyramids, three levels, three iterations each, the four pairings of the two sizes in one batch."""
    pyr, dpyr, host = SO._pyramids(ctx, diag_ctx)
    prm = MsIcpParams.repeat(3, SO._gates(3, SO.BATCH_MAX_DISTANCE))
    tp, sp = [pyr[t][0] for t, _ in SO.KINDS], [pyr[s][1] for _, s in SO.KINDS]
    dtp, dsp = [dpyr[t][0] for t, _ in SO.KINDS], [dpyr[s][1] for _, s in SO.KINDS]
    assert _short_proven(diag_ctx, dpyr["big"][0][0]) and _short_proven(diag_ctx, dpyr["small"][0][0])
    for c in (ctx, diag_ctx):
        c.set_tiling(tiling)
    try:
        poses, want = SO._batch(ctx, prm, tp, sp)
        for knob, tag in ((STORED, "stored points"), (FIVE_OPS, "five operations"), (None, "diagnostics build")):
            if knob:
                monkeypatch.setenv(knob, "0")
            got = SO._batch(diag_ctx, prm, dtp, dsp)[1]
            if knob:
                monkeypatch.delenv(knob)
            SO._same(got, want, tag)
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)
    assert not want[:, -1].view(np.int32).any()
    for k, (t, s) in enumerate(SO.KINDS):
        st, T_ref = O.multiscale_align(prm.to_c_array(), 3, [SO._frame_of(lv) for lv in host[t][0]],
                                       [SO._frame_of(lv) for lv in host[s][1]], threads=4)
        ang, tr = transform_diff(poses[k], T_ref)
        print((t, s, tiling), "multiscale", ang, tr)
        assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (t, s, ang, tr)
