"""A level of a batched image ICP can run split (batch_enqueue, image_icp.hip): one solve launch per iteration and stream
group finishes the previous iteration once per pair (job_solve_head_kernel), and the pixel launch that follows reads
the pose it left instead of running the solve at the head of every block.  The partial loads, their order, the solve
and the tiles are the head form's, so nothing may move by a bit: every case runs on the diagnostics build with
A3D_ICP_SOLVE_SPLIT=0 (no level split), with the masks named (1: level 0, 7: every level), and on the product build with
its own rule; poses, status, trace rows and accumulate sums are compared on bits, and against the oracle with the
project's tolerances (poses 1e-4 rad / 1e-4 m, sums 1e-6) where the oracle runs the case.

Shapes, the smallest at which the hand-off can go wrong: one level of 24 x 16 with 1, 2 and 3 iterations (the first
solve launch has nothing to finish; the parity of the two state and partial buffers), 64 x 48 pyramids of three levels
built on the device (level 0 from the depth planes, level 2 a single partial block) and the same arrays uploaded
(masks read), pinned tilings of 1, 9, 24 and 40 on 96 x 64 (partial counts at and past the eight slices of the sum),
pairs of unequal size (surplus blocks store zeros), 13 pairs (three stream groups of 4 / 4 / 5), a pair that freezes
at its first solve beside a sound one, no iterations at level 0 (the finish kernel applies the pending level-1
iteration), and a one-level pyramid."""
import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (CameraIntrinsics, IcpParams, ImageIcp, MsIcpParams, MultiscaleAlignBatch, RangeImageBuilder,
                         _abi, synth)
from gpu_util import gn_rel_err, small_pose, to_range_image, transform_diff

pytestmark = pytest.mark.gpu

ACC_TOL = 1e-6              # the project's own (tests/test_gpu_image_icp_projection.py)
ROT_TOL = TRANS_TOL = 1e-4  # the project's own (tests/test_gpu_image_icp.py)
MAX_DISTANCE, MAX_COLOR_DISTANCE = 0.15, 0.1
KNOB = "A3D_ICP_SOLVE_SPLIT"

_frame_cache, _built, _oracle = {}, {}, {}


def _camera(w, h):
    k = w / 640.0
    fx, fy, cx, cy = synth.SAMPLE_INTRINSICS
    return CameraIntrinsics(fx * k, fy * k, cx * k, cy * k, w, h)


def _frames(w, h):
    """Frames 0, 1 and 2 of the synthetic stream at w x h, each with a rectangle of depth 0 of its own."""
    if (w, h) not in _frame_cache:
        scene, cam, out = synth.Scene(31), _camera(w, h), []
        for k, (R, t) in enumerate(synth.trajectory(31, 3)):
            depth, rgb = scene.render(R, t, w, h, intr=(cam.fx, cam.fy, cam.cx, cam.cy), noise_seed=k)
            r0, c0 = (3 + 5 * k) % max(1, h // 2), (2 + 7 * k) % max(1, w // 2)
            depth[r0:r0 + max(2, h // 5), c0:c0 + max(2, w // 4)] = 0
            out.append((np.ascontiguousarray(depth), np.ascontiguousarray(rgb)))
        _frame_cache[(w, h)] = out
    return _frame_cache[(w, h)]


def _window(frame, cam, x0, y0, w, h):
    depth, rgb = frame
    return ((np.ascontiguousarray(depth[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w])),
            CameraIntrinsics(cam.fx, cam.fy, cam.cx - x0, cam.cy - y0, w, h))


def _frame_of(ri):
    k = ri.intrinsics
    return O.Frame(ri.points, ri.mask, k.fx, k.fy, k.cx, k.cy, ri.normals, ri.intensities, ri.intensity_map)


def _host_copy(pyr):
    host = [lv.download(colors=False) for lv in pyr]
    for lv in host:
        lv._device = None
    return host


def _build(c, cam, frames):
    return RangeImageBuilder(c).build_many(cam, list(frames), synth.DEPTH_SCALE)


def _pyramids(ctx, diag_ctx, key):
    """Pyramids of the three frames on both builds and their host copies, built once per size: "big" 64 x 48, "small" a
    40 x 30 window of each, "wide" 96 x 64, "blank" 64 x 48 of depth 0 everywhere."""
    if key not in _built:
        if key == "small":
            cam = _camera(64, 48)
            wins = [_window(f, cam, 13, 9, 40, 30) for f in _frames(64, 48)]
            cam, frames = wins[0][1], [f for f, _ in wins]
        elif key == "blank":
            cam = _camera(64, 48)
            frames = [(np.zeros_like(d), rgb) for d, rgb in _frames(64, 48)[:1]]
        else:
            w, h = (96, 64) if key == "wide" else (64, 48)
            cam, frames = _camera(w, h), _frames(w, h)
        product = _build(ctx, cam, frames)
        _built[key] = {"product": product, "diag": _build(diag_ctx, cam, frames), "host": [_host_copy(p) for p in product]}
    return _built[key]


def _gates(iterations):
    return IcpParams(max_iterations=iterations, max_distance=MAX_DISTANCE, max_color_distance=MAX_COLOR_DISTANCE)


def _batch(c, prm, tp, sp):
    """(poses, the poses as float32 matrices with each pair's status appended, launches of the pass)."""
    b = MultiscaleAlignBatch(c, prm, tp, sp)
    poses, status = b.align()
    launches, groups = b.last_timing()[1], b.concurrency()
    b.free()
    m = np.stack([p.matrix() for p in poses]).astype(np.float32).reshape(len(poses), -1)
    return poses, np.concatenate([m, status.view(np.float32)[:, None]], 1), launches, groups


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, np.abs(a - b).max())


def _split_launches(prm, mask, groups):
    """Launches of one pass: one per iteration and group, one more where the level runs split."""
    return groups * sum(int(p.max_iterations) * (2 if (mask >> l) & 1 else 1) for l, p in enumerate(prm))


def _three_ways(ctx, diag_ctx, monkeypatch, prm, pairs, masks, what, levels=slice(None), source="built"):
    """pairs: [((target key, frame), (source key, frame))].  Runs the batch on the diagnostics build unsplit, under
    every mask, and on the product build; all on bits.  Returns the product's poses and bits."""
    def pyr(build, ref):
        key, k = ref
        built = _pyramids(ctx, diag_ctx, key)
        return (built["host"] if source == "uploaded" else built[build])[k][levels]
    lists = {bld: ([pyr(bld, t) for t, _ in pairs], [pyr(bld, s) for _, s in pairs]) for bld in ("product", "diag")}
    monkeypatch.setenv(KNOB, "0")
    _, want, launches, groups = _batch(diag_ctx, prm, *lists["diag"])
    assert launches == _split_launches(prm, 0, groups), (what, launches)
    for mask in masks:
        monkeypatch.setenv(KNOB, str(mask))
        _, got, launches, g = _batch(diag_ctx, prm, *lists["diag"])
        _same(got, want, (what, "mask", mask))
        assert g == groups and launches == _split_launches(prm, mask, groups), (what, mask, launches)
    monkeypatch.delenv(KNOB)
    poses, got, launches, g = _batch(ctx, prm, *lists["product"])
    _same(got, want, (what, "product"))
    # the product's rule: level 0 of a batch on three stream groups, nothing else
    assert launches == _split_launches(prm, 1 if g >= 3 else 0, g), (what, "product", launches, g)
    return poses, got


def _oracle_pose(ctx, diag_ctx, prm, pair, levels=slice(None)):
    (tk, tf), (sk, sf) = pair
    key = (tk, tf, sk, sf, tuple(int(p.max_iterations) for p in prm), levels.stop)
    if key not in _oracle:
        tp = [_frame_of(lv) for lv in _pyramids(ctx, diag_ctx, tk)["host"][tf][levels]]
        sp = [_frame_of(lv) for lv in _pyramids(ctx, diag_ctx, sk)["host"][sf][levels]]
        _oracle[key] = O.multiscale_align(prm.to_c_array(), len(prm), tp, sp, threads=4)
    return _oracle[key]


def _against_oracle(ctx, diag_ctx, prm, pairs, poses, what, levels=slice(None)):
    for k, pair in enumerate(pairs):
        st, T_ref = _oracle_pose(ctx, diag_ctx, prm, pair, levels)
        ang, tr = transform_diff(poses[k], T_ref)
        print(what, pair, "oracle", st, ang, tr)
        assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (what, pair, st, ang, tr)


PAIRS3 = [(("big", 0), ("big", 2)), (("big", 0), ("big", 1)), (("big", 1), ("big", 2))]


# ---- one level, one pair: the first solve launch has nothing to finish; buffer parity ---------------------------------

@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_one_level_one_pair(ctx, diag_ctx, monkeypatch, iterations):
    cam = _camera(24, 16)
    ft, fs = [O.build_frame(d, rgb, cam.fx, cam.fy, cam.cx, cam.cy, synth.DEPTH_SCALE) for d, rgb in _frames(24, 16)[:2]]
    prm = _gates(iterations)

    def run(c):
        T, trace = ImageIcp.new(c, prm, to_range_image(ft)).align(to_range_image(fs), trace=True)
        return T, np.concatenate([np.asarray(T.matrix(), np.float32).reshape(-1), trace.reshape(-1)])

    monkeypatch.setenv(KNOB, "0")
    _, want = run(diag_ctx)
    for mask in (1, 7):
        monkeypatch.setenv(KNOB, str(mask))
        _same(run(diag_ctx)[1], want, ("trace", iterations, mask))
    monkeypatch.delenv(KNOB)
    T, got = run(ctx)
    _same(got, want, ("trace", iterations, "product"))
    st, T_ref, trace_ref = O.image_icp_align(prm.to_c(), ft, fs, want_trace=True)
    ang, tr = transform_diff(T, T_ref)
    print("24x16", iterations, "oracle", st, ang, tr, np.abs(got[16:].reshape(-1, 8) - trace_ref).max())
    assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (iterations, st, ang, tr)


def test_one_pass_sums(ctx, diag_ctx, monkeypatch):
    """a3d_image_icp_accumulate through the split form (solve launch with nothing to finish, then the pixel launch)."""
    cam = _camera(24, 16)
    ft, fs = [O.build_frame(d, rgb, cam.fx, cam.fy, cam.cx, cam.cy, synth.DEPTH_SCALE) for d, rgb in _frames(24, 16)[:2]]
    prm, T = _gates(1), small_pose(3, rot=2.0 / ft.fx, trans=0.003)
    want = ImageIcp.new(ctx, prm, to_range_image(ft)).accumulate(to_range_image(fs), T)
    for mask in ("0", "1"):
        monkeypatch.setenv(KNOB, mask)
        got = ImageIcp.new(diag_ctx, prm, to_range_image(ft)).accumulate(to_range_image(fs), T)
        for a, b in zip(got, want):
            assert a["count"] == b["count"], (mask, a["count"], b["count"])
            for key in ("H", "g", "ssq"):
                x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (mask, key)
    st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, T.to_c(), accum_f64=True)
    assert st == 0
    for got, ref in ((want[0], g_ref.as_dict()), (want[1], c_ref.as_dict())):
        assert got["count"] == ref["count"] > 0
        eh, eg, es = gn_rel_err(got, ref)
        print("24x16 sums", eh, eg, es)
        assert eh < ACC_TOL and eg < ACC_TOL and es < ACC_TOL, (eh, eg, es)


# ---- three levels, a batch of three pairs ------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["built", "uploaded"])
def test_three_levels_three_pairs(ctx, diag_ctx, monkeypatch, source):
    prm = MsIcpParams.repeat(3, _gates(3))
    poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, PAIRS3, (1, 7), ("64x48", source), source=source)
    assert not bits[:, -1].view(np.int32).any()
    _against_oracle(ctx, diag_ctx, prm, PAIRS3, poses, ("64x48", source))


@pytest.mark.parametrize("tiling", [1, 9, 24, 40])
def test_pinned_tilings(ctx, diag_ctx, monkeypatch, tiling):
    prm = MsIcpParams.repeat(3, _gates(2))
    pairs = [(("wide", 0), ("wide", 2)), (("wide", 1), ("wide", 2))]
    for c in (ctx, diag_ctx):
        c.set_tiling(tiling)
    try:
        poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, pairs, (1, 7), ("96x64", tiling))
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)
    assert not bits[:, -1].view(np.int32).any()
    _against_oracle(ctx, diag_ctx, prm, pairs, poses, ("96x64", tiling))


def test_unequal_sizes(ctx, diag_ctx, monkeypatch):
    prm = MsIcpParams.repeat(3, _gates(3))
    pairs = [(("big", 0), ("big", 2)), (("small", 0), ("small", 2)), (("big", 0), ("small", 2))]
    poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, pairs, (1, 7), "unequal sizes")
    assert not bits[:, -1].view(np.int32).any()
    _against_oracle(ctx, diag_ctx, prm, pairs, poses, "unequal sizes")


def test_thirteen_pairs_three_stream_groups(ctx, diag_ctx, monkeypatch):
    prm = MsIcpParams.repeat(3, _gates(3))
    pairs = [PAIRS3[k % 3] for k in range(13)]
    poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, pairs, (1, 7), "13 pairs")
    assert not bits[:, -1].view(np.int32).any()
    for k in range(3, 13):  # a pair's result does not depend on its group
        _same(bits[k], bits[k % 3], ("13 pairs", k))
    _against_oracle(ctx, diag_ctx, prm, PAIRS3, poses[:3], "13 pairs")


def test_frozen_pair_beside_a_sound_one(ctx, diag_ctx, monkeypatch):
    """The first pair's source has no depth: its first solve finds no sample, the pair freezes with A3D_SOLVE_FAILED at
    its initial pose through every level; the sound pair beside it keeps the bits it has beside another sound pair."""
    prm = MsIcpParams.repeat(3, _gates(3))
    sound = (("big", 0), ("big", 2))
    _, ref = _three_ways(ctx, diag_ctx, monkeypatch, prm, [sound, sound], (1,), "two sound pairs")
    _, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, [(("big", 0), ("blank", 0)), sound], (1, 7), "frozen pair")
    assert list(bits[:, -1].view(np.int32)) == [_abi.A3D_SOLVE_FAILED, 0]
    _same(bits[0, :16], np.eye(4, dtype=np.float32).reshape(-1), "the frozen pair's pose")
    _same(bits[1], ref[1], "the sound pair")


def test_no_iterations_at_level_0(ctx, diag_ctx, monkeypatch):
    prm = MsIcpParams.repeat(3, _gates(3)).customize(lambda i, p: setattr(p, "max_iterations", 0 if i == 0 else 3))
    poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, PAIRS3, (1, 7), "no iterations at level 0")
    assert not bits[:, -1].view(np.int32).any()
    _against_oracle(ctx, diag_ctx, prm, PAIRS3, poses, "no iterations at level 0")


def test_one_level_pyramid(ctx, diag_ctx, monkeypatch):
    prm = MsIcpParams.repeat(1, _gates(3))
    poses, bits = _three_ways(ctx, diag_ctx, monkeypatch, prm, PAIRS3, (1,), "one level", levels=slice(0, 1))
    assert not bits[:, -1].view(np.int32).any()
    _against_oracle(ctx, diag_ctx, prm, PAIRS3, poses, "one level", levels=slice(0, 1))
