"""The pixel loop of image ICP requests the intensity-map cell of a pixel in stage B, beside the target gathers, and runs
stage B of pixel k+1 before pixel k is consumed (pixel_pass, image_icp.hip).  Nothing but the order of the loads and the
set of lanes that read a cell changes, so no sum and no pose may move by a single bit: the product build (new order)
against the diagnostics build with A3D_ICP_STEP_ORDER=classic (the earlier order: the cell requested by stage C, after
its gates), and both against the oracle with the project's tolerances (counts exact, sums within 1e-6 of its f64 sums,
poses within 1e-4 rad / 1e-4 m).

Shapes, the smallest at which the pipeline can go wrong: 24 x 16 (one block, two pixels per thread, one trip, lanes out
of range in the second pixel), 40 x 30 under pinned tilings 1 (three trips, ragged end) and 3 (two pixels per thread, a
partial last tile), 64 x 48 pyramids built on the device (level 0 rebuilt from the depth planes, level 2 = 16 x 12 a
single partial block) and the same frames uploaded (masks read), and pairs of unequal size.  Content: depth holes on
both sides, poses that send a band of pixels out of the target and others onto its border cells on all four sides, a
max_distance that rejects many pixels that are in bounds (the lanes whose cell is now read before the gate) and a
max_color_distance that rejects some colour terms."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (CameraIntrinsics, IcpParams, ImageIcp, MsIcpParams, MultiscaleAlignBatch, RangeImageBuilder,
                         Transform, _abi, synth)
from gpu_util import gn_rel_err, small_pose, to_range_image, transform_diff

pytestmark = pytest.mark.gpu

ACC_TOL = 1e-6              # the project's own (tests/test_gpu_image_icp_projection.py)
ROT_TOL = TRANS_TOL = 1e-4  # the project's own (tests/test_gpu_image_icp.py)
MAX_DISTANCE, MAX_COLOR_DISTANCE = 0.06, 0.1  # one pass: at level 0 of these frames 10 to 70 % of the in-bounds pixels fail the first
BATCH_MAX_DISTANCE = 0.15                     # the batch: every pairing still converges in the oracle
KNOB = "A3D_ICP_STEP_ORDER"

_cache = {}


def _camera(w, h):
    """The sample camera scaled to a w-wide image: the whole field of view, the principal point near the centre."""
    k = w / 640.0
    fx, fy, cx, cy = synth.SAMPLE_INTRINSICS
    return CameraIntrinsics(fx * k, fy * k, cx * k, cy * k, w, h)


def _frames(w, h):
    """Frames 0 and 2 of the synthetic stream seen whole at w x h (the renderer leaves 12 % of the pixels invalid), each
    with a rectangle of depth 0 of its own on top."""
    if (w, h) not in _cache:
        scene, cam, out = synth.Scene(31), _camera(w, h), []
        for k, (R, t) in enumerate(synth.trajectory(31, 3)):
            depth, rgb = scene.render(R, t, w, h, intr=(cam.fx, cam.fy, cam.cx, cam.cy), noise_seed=k)
            r0, c0 = (3 + 5 * k) % max(1, h // 2), (2 + 7 * k) % max(1, w // 2)
            depth[r0:r0 + max(2, h // 5), c0:c0 + max(2, w // 4)] = 0
            out.append((np.ascontiguousarray(depth), np.ascontiguousarray(rgb)))
        _cache[(w, h)] = (out[0], out[2])
    return _cache[(w, h)]


def _window(frame, cam, x0, y0, w, h):
    depth, rgb = frame
    return ((np.ascontiguousarray(depth[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w])),
            CameraIntrinsics(cam.fx, cam.fy, cam.cx - x0, cam.cy - y0, w, h))


def _oracle_frame(frame, cam):
    return O.build_frame(frame[0], frame[1], cam.fx, cam.fy, cam.cx, cam.cy, synth.DEPTH_SCALE)


def _frame_of(ri):
    k = ri.intrinsics
    return O.Frame(ri.points, ri.mask, k.fx, k.fy, k.cx, k.cy, ri.normals, ri.intensities, ri.intensity_map)


def _host_copy(pyr):
    host = [lv.download(colors=False) for lv in pyr]
    for lv in host:
        lv._device = None
    return host


def _poses(ft, fs):
    """A small pose that turns the view by two pixels of the target (and moves it by 3 mm), and its inverse: between them
    pixels leave the target through all four borders, and the depth along a ray hardly changes, so that the distance gate
    still decides pixel by pixel."""
    small = small_pose(3, rot=2.0 / ft.fx, trans=0.003)
    return [("small", small), ("inverse", small.inverse())]


def _bands(ft, fs, T):
    """How many valid source pixels project (in f64) onto the target's four border bands (left, right, top, bottom: the
    cells whose 2 x 2 neighbourhood reaches the map's border) and how many leave the image."""
    M = np.asarray(T.matrix(), np.float64)
    p = fs.points.reshape(-1, 3).astype(np.float64)[fs.mask.reshape(-1) != 0] @ M[:3, :3].T + M[:3, 3]
    u, v = p[:, 0] * ft.fx / p[:, 2] + ft.cx, p[:, 1] * ft.fy / p[:, 2] + ft.cy
    band = lambda x, lo: int(((x > lo - 1.0) & (x < lo)).sum())
    out = int(((u <= -1.5) | (u >= ft.w - 0.5) | (v <= -1.5) | (v >= ft.h - 0.5)).sum())
    return np.array([band(u, -0.5), band(u, ft.w - 0.5), band(v, -0.5), band(v, ft.h - 0.5)]), out


def _gates(iterations=1, max_distance=MAX_DISTANCE):
    return IcpParams(max_iterations=iterations, max_distance=max_distance, max_color_distance=MAX_COLOR_DISTANCE)


def _open_gates():
    return IcpParams(max_iterations=1, max_distance=float("inf"), max_color_distance=float("inf"))


def _same_sums(got, want, what):
    for a, b in zip(got, want):
        assert a["count"] == b["count"], (what, a["count"], b["count"])
        for key in ("H", "g", "ssq"):
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (what, key)


def _one_pass(ctx, diag_ctx, monkeypatch, ft, fs, images, diag_images, what, content=True, borders=True):
    """Both poses: the 58 sums of the product build, of the diagnostics build in the classic order and in its default
    (new) order, bit for bit; the product's against the oracle.  ft, fs: the oracle's frames of the arrays the kernels
    read; images / diag_images: (target, source) for the two builds."""
    prm, seen, left = _gates(), np.zeros(4, np.int64), 0
    for name, T in _poses(ft, fs):
        want = ImageIcp.new(ctx, prm, images[0]).accumulate(images[1], T)
        monkeypatch.setenv(KNOB, "classic")
        classic = ImageIcp.new(diag_ctx, prm, diag_images[0]).accumulate(diag_images[1], T)
        monkeypatch.delenv(KNOB)
        _same_sums(classic, want, (what, name, "classic order"))
        _same_sums(ImageIcp.new(diag_ctx, prm, diag_images[0]).accumulate(diag_images[1], T), want,
                   (what, name, "diagnostics build"))
        st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, T.to_c(), accum_f64=True)
        st_o, g_open, _ = O.image_icp_accumulate(_open_gates().to_c(), ft, fs, T.to_c(), accum_f64=True)
        assert st == 0 and st_o == 0, (what, name)
        g_ref, c_ref, n_open = g_ref.as_dict(), c_ref.as_dict(), g_open.as_dict()["count"]
        print(what, name, "counts", want[0]["count"], g_ref["count"], want[1]["count"], c_ref["count"], "open gates", n_open)
        assert want[0]["count"] == g_ref["count"] and want[1]["count"] == c_ref["count"], (what, name)
        for got, ref, tag in ((want[0], g_ref, "geometry"), (want[1], c_ref, "colour")):
            eh, eg, es = gn_rel_err(got, ref)
            print(what, name, tag, eh, eg, es)
            assert eh < ACC_TOL and eg < ACC_TOL and es < ACC_TOL, (what, name, tag, eh, eg, es)
        # the content: many in-bounds pixels fail the distance gate, some of the rest the colour gate
        if content:
            assert 0 < g_ref["count"] <= 0.95 * n_open and 0 < c_ref["count"] < g_ref["count"], (what, name)
        bands, out = _bands(ft, fs, T)
        seen, left = seen + bands, left + out
    if borders:  # every border band, and pixels outside the target
        assert (seen > 0).all() and left > 0, (what, seen, left)


def _upload_pair(ft, fs):
    return to_range_image(ft), to_range_image(fs)


# ---- (a) one pass -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,tiling", [(24, 16, 0), (40, 30, 1), (40, 30, 3)], ids=["24x16", "40x30-tiles1", "40x30-tiles3"])
def test_one_pass_uploaded(ctx, diag_ctx, monkeypatch, w, h, tiling):
    (t, s), cam = _frames(w, h), _camera(w, h)
    ft, fs = _oracle_frame(t, cam), _oracle_frame(s, cam)
    for c in (ctx, diag_ctx):
        c.set_tiling(tiling)
    try:
        _one_pass(ctx, diag_ctx, monkeypatch, ft, fs, _upload_pair(ft, fs), _upload_pair(ft, fs), (w, h, tiling))
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)


def _build(c, cam, frames):
    return RangeImageBuilder(c).build_many(cam, list(frames), synth.DEPTH_SCALE)


def _assert_rebuilt_from_depth(diag_ctx, lv):
    """The level carries its depth plane and passes the host proof behind DEPTH16: its points are rebuilt, not read."""
    h, w = lv.shape
    depth, bp, flag, proven = np.empty((h, w), np.uint16), (C.c_float * 5)(), C.c_int32(), C.c_int32()
    assert diag_ctx.lib.a3d_range_image_download_depth16(lv.handle, _abi.ptr(depth), bp, C.byref(flag)) == 0
    assert diag_ctx.lib.a3d_backproject_proven(w, h, bp, C.byref(proven)) == 0
    assert flag.value == 1 and proven.value == 1, (w, h)


_built = {}


def _pyramids(ctx, diag_ctx):
    """64 x 48 pyramids (three levels) of the two frames and 40 x 30 ones of a window of each, on both builds, with
    their host copies; built once for the module."""
    if not _built:
        frames, cam = _frames(64, 48), _camera(64, 48)
        wins = [_window(f, cam, 13, 9, 40, 30) for f in frames]
        for name, c in (("product", ctx), ("diag", diag_ctx)):
            _built[name] = {"big": _build(c, cam, frames), "small": _build(c, wins[0][1], [f for f, _ in wins])}
        _built["host"] = {k: [_host_copy(p) for p in v] for k, v in _built["product"].items()}
        for pyrs in _built["diag"].values():
            _assert_rebuilt_from_depth(diag_ctx, pyrs[0][0])
    return _built["product"], _built["diag"], _built["host"]


@pytest.mark.parametrize("level", [0, 1, 2], ids=["level0-depth16", "level1-zmask", "level2-16x12"])
def test_one_pass_device_built(ctx, diag_ctx, monkeypatch, level):
    pyr, dpyr, host = _pyramids(ctx, diag_ctx)
    ft, fs = _frame_of(host["big"][0][level]), _frame_of(host["big"][1][level])
    _one_pass(ctx, diag_ctx, monkeypatch, ft, fs, (pyr["big"][0][level], pyr["big"][1][level]),
              (dpyr["big"][0][level], dpyr["big"][1][level]), ("device-built", level), content=level == 0)


def test_one_pass_device_built_then_uploaded(ctx, diag_ctx, monkeypatch):
    """The same level-0 arrays uploaded from the host: never flagged, so the points and the masks are read."""
    _, _, host = _pyramids(ctx, diag_ctx)
    ft, fs = _frame_of(host["big"][0][0]), _frame_of(host["big"][1][0])
    _one_pass(ctx, diag_ctx, monkeypatch, ft, fs, _upload_pair(ft, fs), _upload_pair(ft, fs), "uploaded copies")


@pytest.mark.parametrize("kind", [("big", "small"), ("small", "big")], ids=lambda k: f"{k[0]}<-{k[1]}")
@pytest.mark.parametrize("built", [True, False], ids=["device-built", "uploaded"])
def test_one_pass_unequal_sizes(ctx, diag_ctx, monkeypatch, kind, built):
    pyr, dpyr, host = _pyramids(ctx, diag_ctx)
    t, s = kind
    ft, fs = _frame_of(host[t][0][0]), _frame_of(host[s][1][0])
    assert (ft.w, ft.h) != (fs.w, fs.h)
    images = (pyr[t][0][0], pyr[s][1][0]) if built else _upload_pair(ft, fs)
    diag_images = (dpyr[t][0][0], dpyr[s][1][0]) if built else _upload_pair(ft, fs)
    # (a smaller source inside a larger target reaches no border of it)
    _one_pass(ctx, diag_ctx, monkeypatch, ft, fs, images, diag_images, (kind, built), borders=t == "small")


# ---- (b) batched poses ------------------------------------------------------------------------------------------

def _batch(c, prm, tp, sp):
    """The poses, and the poses as float32 matrices with each pair's status appended."""
    b = MultiscaleAlignBatch(c, prm, tp, sp)
    poses, status = b.align()
    b.free()
    m = np.stack([p.matrix() for p in poses]).astype(np.float32).reshape(len(poses), -1)
    return poses, np.concatenate([m, status.view(np.float32)[:, None]], 1)


def _same(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, np.abs(a - b).max())


KINDS = [("big", "big"), ("small", "small"), ("big", "small"), ("small", "big")]  # (target, source): frame 0 <- frame 2


@pytest.mark.parametrize("tiling", [0, 1, 3], ids=["throughput", "tiles1", "tiles3"])
@pytest.mark.parametrize("built", [True, False], ids=["device-built", "uploaded"])
def test_batched_poses(ctx, diag_ctx, monkeypatch, built, tiling):
    """Three levels, three iterations each, the four pairings of the two sizes in one batch: poses and status."""
    pyr, dpyr, host = _pyramids(ctx, diag_ctx)
    prm = MsIcpParams.repeat(3, _gates(3, BATCH_MAX_DISTANCE))
    src = pyr if built else host
    dsrc = dpyr if built else host
    tp, sp = [src[t][0] for t, _ in KINDS], [src[s][1] for _, s in KINDS]
    dtp, dsp = [dsrc[t][0] for t, _ in KINDS], [dsrc[s][1] for _, s in KINDS]
    for c in (ctx, diag_ctx):
        c.set_tiling(tiling)
    try:
        poses, want = _batch(ctx, prm, tp, sp)
        monkeypatch.setenv(KNOB, "classic")
        _same(_batch(diag_ctx, prm, dtp, dsp)[1], want, "classic order")
        monkeypatch.delenv(KNOB)
        _same(_batch(diag_ctx, prm, dtp, dsp)[1], want, "diagnostics build")
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)
    assert not want[:, -1].view(np.int32).any()
    for k, (t, s) in enumerate(KINDS):
        st, T_ref = O.multiscale_align(prm.to_c_array(), 3, [_frame_of(lv) for lv in host[t][0]],
                                       [_frame_of(lv) for lv in host[s][1]], threads=4)
        ang, tr = transform_diff(poses[k], T_ref)
        print((t, s, built, tiling), "multiscale", ang, tr)
        assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (t, s, ang, tr)
