"""GPU parity of image ICP where a shifted intensity sample (u + 0.005, v) or (u, v + 0.005) falls into the next texel.

The pixel loop decides at the top of a step which lanes leave their cell, requests the column / row the held cell lacks
there, and stage D evaluates bilerp on the held and the requested texels (image_icp.hip: Shifted, request_shifted).  The
diagnostics build keeps the earlier form, in which stage D loads both shifted cells itself (A3D_ICP_RESAMPLE=late), and the
earlier step order with its own resample (A3D_ICP_STEP_ORDER=classic).  Every case here runs the product library against
both — sums and poses bit for bit (the sums of a pass are the block partials added in a fixed order, and under a pinned
tiling of 1 the one block's partial itself) — and against the oracle: counts exact, sums within 1e-6 of its f64 sums,
poses within 1e-4.

A wave's step covers one aligned run of 64 source pixels.  Every case asserts on the host, from the reference's u and v in
f32 (camera.rs:64-70 after transform.rs:138-153, restated in numpy) and before any alignment kernel runs, that its source
holds: a run no lane of which leaves; runs in which exactly one lane leaves — in u only, in v only, in both; a run every
lane of which leaves; leaving lanes whose shifted cell reaches the furthest column (ui + 2 == tw) and others the furthest
row (vi + 2 == th) a sample can touch (a lane that leaves has u + 0.005 < tw - 0.495, so the map's own last column,
tw + 1, is out of every sample's reach: tests/test_image_icp_resample_cpu.py); a live lane with u in (-0.005, 0), next to
the cut it cannot cross; a leaving lane that the distance gate rejects; a leaving lane whose colour term is rejected; a
leaving lane in a thread's first pixel and another in its last; and, where a thread has more than one trip (a case of one
trip cannot hold it), a leaving lane in the step directly after a trip in which its wave had no leaving lane.

Uploaded frames are crafted point by point, as tests/test_gpu_image_icp_projection.py crafts them (the masks are read).
Device-built pyramids are crafted through the depth plane: under a pure translation a pixel's depth sets how far it moves
in u and, 1.0025 times as far, in v, so each pixel picks one of {neither, u only, v only, both} by its depth; the level-0
pass runs the kernel that rebuilds the points from the depth planes, levels 1 and 2 the form that infers the masks."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (CameraIntrinsics, IcpParams, ImageIcp, MsIcpParams, MultiscaleAlign, RangeImageBuilder, Transform,
                         _abi, synth)
from gpu_util import gn_rel_err, to_range_image, transform_diff

pytestmark = pytest.mark.gpu

ROT_TOL = TRANS_TOL = 1e-4  # the project's own (tests/test_gpu_image_icp.py)
ACC_TOL = 1e-6
F32 = np.float32
H = F32(0.005)
FX = FY = 50.0
TARGETS = {(64, 48): (31.5, 23.25), (37, 29): (18.0, 13.75)}  # (w, h): (cx, cy)
SRC_K = (77.0, 71.0, 3.25, -2.5)  # a crafted source's own intrinsics: nothing may read them
MAX_DISTANCE, MAX_COLOR = 0.5, 0.3
NEITHER, U_ONLY, V_ONLY, BOTH = 0, 1, 2, 3
FRAC = {NEITHER: (0.5, 0.5), U_ONLY: (0.9975, 0.5), V_ONLY: (0.5, 0.9975), BOTH: (0.9975, 0.9975)}


def _gates(iterations=1):
    """The distance and colour gates decide; 4.0 > pi, so no angle is rejected."""
    return IcpParams(max_iterations=iterations, max_distance=MAX_DISTANCE, max_color_distance=MAX_COLOR, max_normal_angle=4.0)


def _tiling(n, pinned):
    """tiling_for (image_icp.hip) of a lone pair of n source pixels: (blocks, pixels per thread).  Unpinned, a lone small
    pair is cut into as many blocks of two pixels per thread as it fills."""
    most = max(1, -(-n // 512))
    want = most if pinned == 0 else max(1, min(pinned, most))
    p = -(-n // (256 * want))
    p = max(2, -(-p // 2) * 2)
    return max(1, -(-n // (256 * p))), p


def _usize(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(x, F32) > 0, np.trunc(x), 0).astype(np.int64)


def _project(pts, t, fx, fy, cx, cy):
    """transform_vector under a pure translation t (the identity rotation adds exact zeros: one rounding per coordinate)
    and CameraIntrinsics::project, in f32."""
    t = np.asarray(t, F32)
    p = (pts.reshape(-1, 3).astype(F32) + t[None, :]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = ((p[:, 0] * F32(fx)).astype(F32) / p[:, 2]).astype(F32) + F32(cx)
        v = ((p[:, 1] * F32(fy)).astype(F32) / p[:, 2]).astype(F32) + F32(cy)
    return p, u.astype(F32), v.astype(F32)


def _assert_holds_every_situation(ft, fs, t, pinned, what):
    """The module docstring's list, from the reference's u and v of source frame fs under the translation t against ft."""
    tw, th, n = ft.w, ft.h, fs.w * fs.h
    p, u, v = _project(fs.points, tuple(t), ft.fx, ft.fy, ft.cx, ft.cy)
    ur, vr = (u + F32(0.5)).astype(F32), (v + F32(0.5)).astype(F32)
    with np.errstate(invalid="ignore"):
        live = (fs.mask.reshape(-1) != 0) & ~((ur <= -1) | (ur >= tw) | (vr <= -1) | (vr >= th))
    ui, vi = _usize(u), _usize(v)
    lu = live & (_usize((u + H).astype(F32)) != ui)
    lv = live & (_usize((v + H).astype(F32)) != vi)
    leaves = lu | lv
    # the gates, in f64 with a margin either way: no lane this assertion counts on sits near a threshold
    col, row = np.trunc(np.where(live, ur, 0)).astype(np.int64), np.trunc(np.where(live, vr, 0)).astype(np.int64)
    tp = ft.points.reshape(th, tw, 3)[row, col].astype(np.float64)
    tvalid = ft.mask.reshape(th, tw)[row, col] == 1
    d2 = ((tp - p.astype(np.float64)) ** 2).sum(1)
    far, near = live & tvalid & (d2 > 2.0 * MAX_DISTANCE ** 2), live & tvalid & (d2 < 0.5 * MAX_DISTANCE ** 2)
    m = ft.intensity_map.astype(np.float64)
    a, b = np.where(live, ui, 0), np.where(live, vi, 0)
    uf, vf = np.where(live, u - ui, 0).astype(np.float64), np.where(live, v - vi, 0).astype(np.float64)
    value = (m[b, a] * (1 - uf) + m[b, a + 1] * uf) * (1 - vf) + (m[b + 1, a] * (1 - uf) + m[b + 1, a + 1] * uf) * vf
    rc = fs.intensities.reshape(-1).astype(np.float64) * 0.003921569 - value
    colour_out, colour_in = near & (rc ** 2 > 1.5 * MAX_COLOR ** 2), near & (rc ** 2 < 0.6 * MAX_COLOR ** 2)

    tiles, ppt = _tiling(n, pinned)
    runs = -(-n // 64)
    pad = runs * 64 - n
    per_run = lambda x: np.concatenate([x, np.zeros(pad, bool)]).reshape(runs, 64)
    n_leave, n_live = per_run(leaves).sum(1), per_run(live).sum(1)
    one = n_leave == 1
    found = {
        "a run no lane of which leaves": bool(((n_leave == 0) & (n_live > 0)).any()),
        "one lane leaves, in u only": bool((one & (per_run(lu & ~lv).sum(1) == 1)).any()),
        "one lane leaves, in v only": bool((one & (per_run(lv & ~lu).sum(1) == 1)).any()),
        "one lane leaves, in both": bool((one & (per_run(lu & lv).sum(1) == 1)).any()),
        "every lane leaves": bool((n_leave == 64).any()),
        "furthest column": bool((lu & (ui + 2 == tw)).any()),
        "furthest row": bool((lv & (vi + 2 == th)).any()),
        "u in (-0.005, 0)": bool((live & (u < 0) & (u > -0.005)).any()),
        "a leaving lane the distance gate rejects": bool((leaves & far).any()),
        "a leaving lane whose colour term is rejected": bool((leaves & colour_out).any()),
        "leaving lanes that count in both terms": bool((lu & colour_in).any() and (lv & colour_in).any()),
    }
    k_of = (np.arange(n) // 256) % ppt  # which of its thread's pixels a source pixel is
    found["a leaving lane in a thread's first pixel"] = bool((leaves & (k_of == 0)).any())
    found["a leaving lane in a thread's last pixel"] = bool((leaves & (k_of == k_of.max())).any())  # (the last in range)
    if ppt >= 4:
        quiet = np.concatenate([n_leave == 0, np.zeros(tiles * ppt * 4 - runs, bool)]).reshape(tiles, ppt, 4)  # [tile][step][wave]
        busy = np.concatenate([n_leave > 0, np.zeros(tiles * ppt * 4 - runs, bool)]).reshape(tiles, ppt, 4)
        found["a leaving lane directly after a trip without"] = bool(
            (quiet[:, 0:ppt - 2:2] & quiet[:, 1:ppt - 2:2] & busy[:, 2:ppt:2]).any())
    missing = [k for k, ok in found.items() if not ok]
    assert not missing, (what, missing, (tiles, ppt))
    print(what, "tiles, ppt", (tiles, ppt), "runs", runs, "leaving lanes", int(leaves.sum()), "of", int(live.sum()), "live")


# ---- uploaded frames, crafted point by point ---------------------------------------------------------------------

_targets = {}


def _target(w, h):
    """Points at the pixel centres with z = 1, normal (0, 0, 1); the intensity map of a seeded random luma."""
    if (w, h) not in _targets:
        cx, cy = TARGETS[(w, h)]
        vv, uu = np.mgrid[0:h, 0:w]
        pts = np.stack([(uu - cx) / FX, (vv - cy) / FY, np.ones(uu.shape)], -1).astype(F32)
        nrm = np.zeros((h, w, 3), F32)
        nrm[..., 2] = 1.0
        luma = np.random.default_rng(1000 + w).integers(0, 256, (h, w), dtype=np.uint8)
        _targets[(w, h)] = O.Frame(pts, np.ones((h, w), np.uint8), FX, FY, cx, cy, normals=nrm,
                                   intensities=luma.reshape(-1), intensity_map=O.intensity_map(luma))
    return _targets[(w, h)]


def _plan(n, ppt, rng):
    """A class per source pixel, and the lanes with a special role: {role: pixel}.  Run by run (64 pixels): 0 none leaves,
    1 / 2 / 3 one lane leaves (u only / v only / both), 4 every lane leaves; with more than one trip the third step of
    wave 0 (run 8) leaves after two silent steps (runs 0 and 4 — then run 5 takes the run every lane of which leaves);
    the last run of the thread's last pixel has a leaving lane; everything else is random with one lane in ten leaving."""
    runs = -(-n // 64)
    cls = np.where(rng.random(n) < 0.1, rng.integers(1, 4, n), NEITHER)
    full = 4 if ppt == 2 else 5
    silent = [0] if ppt == 2 else [0, 4]
    for r in silent + [1, 2, 3]:
        cls[64 * r:64 * r + 64] = NEITHER
    cls[64 * 1 + 5], cls[64 * 2 + 9], cls[64 * 3 + 13] = U_ONLY, V_ONLY, BOTH
    cls[64 * full:64 * full + 64] = np.tile([U_ONLY, V_ONLY, BOTH], 22)[:64]
    roles = {"full": full, "edge_u": 64 * full + 0, "edge_v": 64 * full + 1, "far": 64 * full + 3, "colour": 64 * full + 4,
             "negative_u": 7}
    if ppt >= 4:
        cls[64 * 8 + 21] = U_ONLY
    k_of = (np.arange(n) // 256) % ppt
    last = np.flatnonzero(k_of == k_of.max())  # a thread's last pixel that is in range
    cls[last[len(last) // 2]] = V_ONLY
    assert runs > full and n >= 64 * (full + 1)
    return cls, roles


def _crafted_source(size, shape, pinned, seed):
    """A source of `shape` whose points project, at the identity, to the planned (u, v) in the target of `size`."""
    w, h = size
    ft = _target(w, h)
    n = shape[0] * shape[1]
    rng = np.random.default_rng(seed)
    cls, roles = _plan(n, _tiling(n, pinned)[1], rng)
    fu = np.array([FRAC[c][0] for c in cls]) + np.where(cls == NEITHER, rng.uniform(-0.35, 0.35, n), 0)
    fv = np.array([FRAC[c][1] for c in cls]) + np.where(cls == NEITHER, rng.uniform(-0.35, 0.35, n), 0)
    fu = np.where(np.isin(cls, (V_ONLY,)), rng.uniform(0.1, 0.9, n), fu)
    fv = np.where(np.isin(cls, (U_ONLY,)), rng.uniform(0.1, 0.9, n), fv)
    u = rng.integers(1, w - 3, n) + fu
    v = rng.integers(1, h - 3, n) + fv
    u[roles["edge_u"]], v[roles["edge_v"]] = w - 2 + 0.9975, h - 2 + 0.9975  # (their classes: u only, v only)
    u[roles["negative_u"]] = -0.003
    z = np.ones(n)
    z[roles["far"]] = 3.0
    x, y = (u - ft.cx) / FX * z, (v - ft.cy) / FY * z
    pts = np.stack([x, y, z], -1).astype(F32).reshape(shape[0], shape[1], 3)
    inten = rng.integers(0, 256, n).astype(np.uint8)
    # the colour lane: as far from the target's value there as a byte can be
    _, pu, pv = _project(pts, (0, 0, 0), FX, FY, ft.cx, ft.cy)
    k = roles["colour"]
    a, b = int(pu[k]), int(pv[k])
    inten[k] = 255 if ft.intensity_map[b:b + 2, a:a + 2].mean() < 0.5 else 0
    return ft, O.Frame(pts, np.ones(shape, np.uint8), *SRC_K, intensities=inten)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _same_sums(got, want, what):
    for a, b, term in zip(got, want, ("geometry", "colour")):
        assert a["count"] == b["count"], (what, term)
        for key in ("H", "g", "ssq"):
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, term, key)


def _against_oracle(got, prm, ft, fs, T, what):
    st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, T.to_c(), accum_f64=True)
    assert st == 0, what
    for a, ref, term in zip(got, (g_ref.as_dict(), c_ref.as_dict()), ("geometry", "colour")):
        assert a["count"] == ref["count"] > 0, (what, term, a["count"], ref["count"])
        eh, eg, es = gn_rel_err(a, ref)
        print(what, term, a["count"], eh, eg, es)
        assert eh < ACC_TOL and eg < ACC_TOL and es < ACC_TOL, (what, term, eh, eg, es)


def _forms(monkeypatch, run):
    """run(context kind) for the diagnostics build as it is, with the earlier resample, with the earlier step order."""
    out = {"diagnostics build": run()}
    for knob, value in (("A3D_ICP_RESAMPLE", "late"), ("A3D_ICP_STEP_ORDER", "classic")):
        monkeypatch.setenv(knob, value)
        out[f"{knob}={value}"] = run()
        monkeypatch.delenv(knob)
    return out


CRAFTED = [((64, 48), (16, 24), 1), ((64, 48), (30, 40), 1), ((64, 48), (30, 40), 3), ((37, 29), (20, 31), 0)]


@pytest.mark.parametrize("size,shape,pinned", CRAFTED, ids=["24x16", "40x30-tiling1", "40x30-tiling3", "31x20-into-37x29"])
def test_crafted_uploaded_frames(ctx, diag_ctx, monkeypatch, size, shape, pinned):
    """24 x 16: one block, one trip, the second pixel's upper lanes out of range.  40 x 30: one block of three trips with a
    ragged end, and three blocks of one trip the last of which is partial.  31 x 20 into 37 x 29: unequal sizes, unpinned."""
    ft, fs = _crafted_source(size, shape, pinned, seed=shape[1])
    eye = Transform.eye()
    _assert_holds_every_situation(ft, fs, (0.0, 0.0, 0.0), pinned, (size, shape, pinned))
    rt, rs = to_range_image(ft), to_range_image(fs)
    prm, prm3 = _gates(), _gates(3)
    for c in (ctx, diag_ctx):
        c.set_tiling(pinned)
    try:
        sums = ImageIcp.new(ctx, prm, rt).accumulate(rs, eye)
        pose = np.asarray(ImageIcp.new(ctx, prm3, rt).align(rs).matrix(), F32)
        for name, got in _forms(monkeypatch, lambda: ImageIcp.new(diag_ctx, prm, rt).accumulate(rs, eye)).items():
            _same_sums(got, sums, (size, shape, pinned, name))
        for name, got in _forms(monkeypatch, lambda: np.asarray(ImageIcp.new(diag_ctx, prm3, rt).align(rs).matrix(), F32)).items():
            assert np.array_equal(got.view(np.uint32), pose.view(np.uint32)), (size, shape, pinned, name)
    finally:
        for c in (ctx, diag_ctx):
            c.set_tiling(0)
    _against_oracle(sums, prm, ft, fs, eye, (size, shape, pinned))
    st, T_ref, _ = O.image_icp_align(prm3.to_c(), ft, fs)
    ang, tr = transform_diff(ImageIcp.new(ctx, prm3, rt).align(rs), T_ref)
    print((size, shape, pinned), "align", ang, tr)
    assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (ang, tr)


# ---- device-built pyramids, crafted through the depth plane ------------------------------------------------------

W, HGT = 64, 48
CAM_T = (200.0, 200.0, 31.5, 23.5)
CAM_S = (200.0, 200.0, 32.5, 24.5)   # the principal point one pixel on: u = column - 1 + s, v = row - 1 + 1.0025 s
SCALE = 0.0002
Z0 = 1.6                             # metres, 8000 depth units: one unit moves s by 0.000125
RHO = 1.0025
SHIFT = (Z0 / CAM_T[0], RHO * Z0 / CAM_T[1], 0.0)   # s = SHIFT[0] fx / z = Z0 / z
S_OF = {NEITHER: 0.9915, U_ONLY: 0.99875, V_ONLY: 0.99376, BOTH: 0.99625}


def _depth_frames():
    """(target frame, source frame) as (depth u16, rgb u8): the source a pixel-by-pixel choice of four depths around Z0
    over a random texture, the target the same frame (its camera's principal point one pixel off) with one pixel far
    behind and one patch of the opposite colour."""
    rng = np.random.default_rng(77)
    n = W * HGT
    cls, roles = _plan(n, _tiling(n, 1)[1], rng)
    cls = cls.reshape(HGT, W)
    cls[HGT - 1, 10], cls[20, W - 1] = V_ONLY, U_ONLY  # v = th - 2 + 0.996..., u = tw - 2 + 0.998...
    cls[11, 0] = U_ONLY                                 # u = -1 + 0.99875: next to the cut, and it does not leave
    cls[roles["full"], 0] = V_ONLY                      # (so the first lane of the run that leaves whole leaves in v)
    depth_s = np.rint(Z0 / np.vectorize(S_OF.get)(cls) / SCALE).astype(np.uint16)
    depth_t = depth_s.copy()  # the same relief and, below, the same texture: under SHIFT the source lies on the target
    fr, fc = divmod(roles["far"], W)       # the source pixel (fr, fc) lands on target pixel (fr - 1 + 1, fc - 1 + 1)
    depth_t[fr, fc] = round(2 * Z0 / SCALE)
    def texture():  # random grey, 3 x 3 box mean: textured everywhere, without single-texel spikes
        g = np.pad(rng.integers(0, 256, (HGT, W)).astype(np.float64), 1, mode="edge")
        return (sum(g[i:i + HGT, j:j + W] for i in range(3) for j in range(3)) / 9.0).astype(np.uint8)[..., None]

    base = texture()
    rgb_t = np.repeat(base, 3, 2)
    rgb_s = rgb_t.copy()
    cr, cc = divmod(roles["colour"], W)
    rgb_s[cr, cc] = 255 if base[cr - 1:cr + 2, cc - 1:cc + 2].mean() < 128 else 0
    rgb_t[cr - 1:cr + 2, cc - 1:cc + 2] = 0 if rgb_s[cr, cc, 0] == 255 else 255
    return (depth_t, rgb_t), (depth_s, rgb_s)


def _host_copy(pyr):
    host = [lv.download(colors=False) for lv in pyr]
    for lv in host:
        lv._device = None
    return host


def _frame_of(ri):
    k = ri.intrinsics
    return O.Frame(ri.points, ri.mask, k.fx, k.fy, k.cx, k.cy, ri.normals, ri.intensities, ri.intensity_map)


def _build(c):
    ft, fs = _depth_frames()
    b = RangeImageBuilder(c)
    return (b.build_many(CameraIntrinsics(*CAM_T, W, HGT), [ft], SCALE)[0],
            b.build_many(CameraIntrinsics(*CAM_S, W, HGT), [fs], SCALE)[0])


def _assert_rebuilt_from_depth(diag_ctx, lv):
    h, w = lv.shape
    depth, bp, flag, proven = np.empty((h, w), np.uint16), (C.c_float * 5)(), C.c_int32(), C.c_int32()
    assert diag_ctx.lib.a3d_range_image_download_depth16(lv.handle, _abi.ptr(depth), bp, C.byref(flag)) == 0
    assert diag_ctx.lib.a3d_backproject_proven(w, h, bp, C.byref(proven)) == 0
    assert flag.value == 1 and proven.value == 1, (w, h)


def _poses(ctx, diag_ctx, monkeypatch, iterations, pyrs, dpyrs, frames, what, normal_angle=None):
    """MultiscaleAlign of the pair on the product library, bit for bit on the diagnostics build in its three forms, and
    (frames = the oracle's pyramids of the same arrays) within 1e-4 of the oracle."""
    def setup(i, p):
        p.max_iterations = iterations
        if normal_angle is not None:
            p.max_normal_angle = normal_angle

    ms = MsIcpParams.default().customize(setup)

    def lone(c, t, s):
        a = MultiscaleAlign.new(c, ms, t)
        T = a.align(s)
        a.free()
        return T

    T_gpu = lone(ctx, *pyrs)
    pose = np.asarray(T_gpu.matrix(), F32)
    for name, got in _forms(monkeypatch, lambda: np.asarray(lone(diag_ctx, *dpyrs).matrix(), F32)).items():
        assert np.array_equal(got.view(np.uint32), pose.view(np.uint32)), (what, iterations, name)
    if frames is not None:
        st, T_ref = O.multiscale_align(ms.to_c_array(), 3, frames[0], frames[1], threads=4)
        ang, tr = transform_diff(T_gpu, T_ref)
        print(what, iterations, "multiscale", ang, tr)
        assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (what, iterations, ang, tr)


@pytest.mark.parametrize("uploaded", [False, True], ids=["device-built", "uploaded-copies"])
def test_pyramids_crafted_through_the_depth_plane(ctx, diag_ctx, monkeypatch, uploaded):
    """64 x 48, three levels.  Device-built: level 0 is rebuilt from the depth planes, levels 1 and 2 infer the masks, level
    2 is a single partial block.  Uploaded copies of the same pyramids: the masks are read."""
    tgt, src = _build(ctx)
    dtgt, dsrc = _build(diag_ctx)
    for lv in (dtgt[0], dsrc[0]):
        _assert_rebuilt_from_depth(diag_ctx, lv)
    htgt, hsrc = _host_copy(tgt), _host_copy(src)
    ftp, fsp = [_frame_of(lv) for lv in htgt], [_frame_of(lv) for lv in hsrc]
    _assert_holds_every_situation(ftp[0], fsp[0], SHIFT, 1, ("depth plane, level 0", uploaded))
    if uploaded:
        tgt_u, src_u = ([lv.device(ctx) for lv in htgt], [lv.device(ctx) for lv in hsrc])
        dtgt_u, dsrc_u = ([lv.device(diag_ctx) for lv in _host_copy(dtgt)], [lv.device(diag_ctx) for lv in _host_copy(dsrc)])
    else:
        tgt_u, src_u, dtgt_u, dsrc_u = tgt, src, dtgt, dsrc
    prm = _gates()
    shift = Transform(t=SHIFT)
    for pinned in (1, 0):  # one block per level (level 0: six trips), and the throughput tiling (blocks of one trip)
        for c in (ctx, diag_ctx):
            c.set_tiling(pinned)
        try:
            for level in range(3):
                # (levels 1 and 2 from half and a quarter of the shift: the same scene, whatever leaves there)
                T = Transform(t=tuple(x / 2 ** level for x in SHIFT)) if level else shift
                sums = ImageIcp.new(ctx, prm, tgt_u[level]).accumulate(src_u[level], T)
                run = lambda: ImageIcp.new(diag_ctx, prm, dtgt_u[level]).accumulate(dsrc_u[level], T)
                for name, got in _forms(monkeypatch, run).items():
                    _same_sums(got, sums, (uploaded, pinned, level, name))
                if pinned == 1:
                    _against_oracle(sums, prm, ftp[level], fsp[level], T, ("depth plane", uploaded, level))
            # The default parameters for the bits.  Against the oracle the angle gate is open (4.0 > pi), as in the passes
            # above: the dimples' normals sit all around the default 0.314 rad, where a last-bit difference in p.n moves a
            # pixel in or out and the pose with it; the default gates meet the oracle on the rendered pair below.
            _poses(ctx, diag_ctx, monkeypatch, 3, (tgt_u, src_u), (dtgt_u, dsrc_u), None, ("depth plane", uploaded, pinned))
            _poses(ctx, diag_ctx, monkeypatch, 3, (tgt_u, src_u), (dtgt_u, dsrc_u), (ftp, fsp) if pinned == 1 else None,
                   ("depth plane", uploaded, pinned), normal_angle=4.0)
        finally:
            for c in (ctx, diag_ctx):
                c.set_tiling(0)
    for lv in list(tgt) + list(src) + list(dtgt) + list(dsrc):
        lv.free()


@pytest.mark.parametrize("uploaded", [False, True], ids=["device-built", "uploaded-copies"])
def test_rendered_pyramids(ctx, diag_ctx, monkeypatch, uploaded):
    """Two rendered 64 x 48 frames through the device builder, three levels, three iterations each: a well-conditioned pair
    for the pose against the oracle's, with whatever lanes leave (asserted: some do, at every level)."""
    frames, cam = synth.frame_stream(31, 2, W, HGT)[0], synth.camera(W, HGT)
    built = RangeImageBuilder(ctx).build_many(cam, frames, synth.DEPTH_SCALE)
    dbuilt = RangeImageBuilder(diag_ctx).build_many(cam, frames, synth.DEPTH_SCALE)
    _assert_rebuilt_from_depth(diag_ctx, dbuilt[0][0])
    host = [_host_copy(p) for p in built]
    ftp, fsp = [[_frame_of(lv) for lv in p] for p in host]
    for ft, fs in zip(ftp, fsp):
        _, u, v = _project(fs.points, (0, 0, 0), ft.fx, ft.fy, ft.cx, ft.cy)
        with np.errstate(invalid="ignore"):
            inside = (fs.mask.reshape(-1) != 0) & (u > 0) & (u < ft.w - 1) & (v > 0) & (v < ft.h - 1)
            leaves = inside & ((_usize((u + H).astype(F32)) != _usize(u)) | (_usize((v + H).astype(F32)) != _usize(v)))
        assert leaves.any(), (ft.w, ft.h)
    if uploaded:
        pyrs = [[lv.device(ctx) for lv in p] for p in host]
        dpyrs = [[lv.device(diag_ctx) for lv in _host_copy(p)] for p in dbuilt]
    else:
        pyrs, dpyrs = built, dbuilt
    for pinned in (1, 0):
        for c in (ctx, diag_ctx):
            c.set_tiling(pinned)
        try:
            _poses(ctx, diag_ctx, monkeypatch, 3, pyrs, dpyrs, (ftp, fsp) if pinned == 1 else None, ("rendered", uploaded, pinned))
        finally:
            for c in (ctx, diag_ctx):
                c.set_tiling(0)
    for lv in [lv for p in list(built) + list(dbuilt) for lv in p]:
        lv.free()
