"""GPU parity of image ICP where the projection decides, and for pairs whose two images differ in size.

A. Crafted sources step u and v a float at a time across every cut of the reference's rule (image_icp.rs:106-112:
   (u + 0.5) as i32 -> as usize -> get_point) and of IntensityMap::bilinear_grad at the raw u, v (intensity_map.rs:184-210:
   `u as usize` is 0 for a negative u, the sample at u + 0.005 may sit in the next texel, the last row and column read
   the map's border cells), over a steep random intensity map, with a lattice over the four border bands and corners.
B. One degenerate source point per call (u NaN, +-inf, beyond +-2^31, z outside the shared-reciprocal range) at chosen
   lanes, and masks other than 0 and 1 on both sides.
C. Uploaded pairs of unequal size: windows of rendered frames with their own intrinsics, either way round.
D. The same through device-built pyramids (ZMASK and DEPTH16 forms, batch, lone pair, pinned tiling), and a level-0
   pass from a pose that pushes a third of the source out through two adjacent borders.

The expected value is always the oracle's; counts are exact, H, g and the residual sum within 1e-6 of its f64 sums, poses
within 1e-4 rad / 1e-4 m, and what is called "the same bits" is compared on uint32 views."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import (BilateralFilter, CameraIntrinsics, IcpParams, ImageIcp, MsIcpParams, MultiscaleAlign,
                         MultiscaleAlignBatch, RangeImageBuilder, Transform, _abi, synth)
from gpu_util import gn_rel_err, small_pose, to_range_image, transform_diff

pytestmark = pytest.mark.gpu

ROT_TOL = TRANS_TOL = 1e-4  # the project's own (tests/test_gpu_image_icp.py)
ACC_TOL = 1e-6

F32 = np.float32
FX = FY = 50.0
TARGETS = {(64, 48): (31.5, 23.25), (37, 29): (18.0, 13.75)}  # (w, h): (cx, cy); the first is the gates tests' geometry
SRC_K = (77.0, 71.0, 3.25, -2.5)  # a crafted source's own intrinsics: nothing may read them


def _open_gates():
    """Only the projection (and the masks) decide: 4.0 > pi, so no angle is rejected."""
    return IcpParams(max_iterations=1, max_distance=float("inf"), max_color_distance=float("inf"), max_normal_angle=4.0)


def _next(x, k):
    """The float k steps above x (k < 0: below) in the total order of the floats (-0 and +0 count as one)."""
    u = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(u < 0, -(u & 0x7FFFFFFF), u) + k
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _around(x, k):
    return _next(np.full(2 * k, x, F32), np.arange(-k, k))


_targets = {}


def _target(w, h, mask=None):
    """Points at the pixel centres with z = 1, normal (0, 0, 1); the intensity map of a seeded random luma (steep texels,
    the border cells as IntensityMap::fill leaves them)."""
    if (w, h) not in _targets:
        cx, cy = TARGETS[(w, h)]
        vv, uu = np.mgrid[0:h, 0:w]
        pts = np.stack([(uu - cx) / FX, (vv - cy) / FY, np.ones(uu.shape)], -1).astype(F32)
        nrm = np.zeros((h, w, 3), F32)
        nrm[..., 2] = 1.0
        luma = np.random.default_rng(1000 + w).integers(0, 256, (h, w), dtype=np.uint8)
        _targets[(w, h)] = (pts, nrm, luma, O.intensity_map(luma))
    pts, nrm, luma, imap = _targets[(w, h)]
    cx, cy = TARGETS[(w, h)]
    m = np.ones((h, w), np.uint8) if mask is None else mask
    return O.Frame(pts, m, FX, FY, cx, cy, normals=nrm, intensities=luma.reshape(-1), intensity_map=imap)


def _source(x, y, shape, z=None, mask=None, seed=5):
    """A source of its own shape and intrinsics whose points are (x, y, z = 1), in row-major pixel order."""
    h, w = shape
    assert len(x) == len(y) == h * w
    pts = np.stack([x, y, np.ones(h * w, F32) if z is None else z], -1).astype(F32).reshape(h, w, 3)
    inten = np.random.default_rng(seed).integers(0, 256, h * w, dtype=np.uint8)
    m = np.ones((h, w), np.uint8) if mask is None else np.asarray(mask, np.uint8).reshape(h, w)
    return O.Frame(pts, m, *SRC_K, intensities=inten)


def _project(x, centre, focal):
    """CameraIntrinsics::project (camera.rs:64-70) at z = 1, in f32: fl(fl(fl(x f) / z) + c)."""
    return (np.asarray(x, F32) * F32(focal) / F32(1.0) + F32(centre)).astype(F32)


def _unproject(u, centre, focal):
    return ((np.asarray(u, np.float64) - centre) / focal).astype(F32)


def _interior(n, w, h, seed):
    """n source points that project well inside a w x h target, off the texel grid."""
    cx, cy = TARGETS[(w, h)]
    rng = np.random.default_rng(seed)
    return _unproject(rng.uniform(1.5, w - 2.5, n), cx, FX), _unproject(rng.uniform(1.5, h - 2.5, n), cy, FY)


def _cuts(dim):
    return [-1.5, -0.5, -0.005, 0.0, 0.995, 1.0, dim - 1.005, dim - 1.0, dim - 0.505, dim - 0.5]


def _sweeps(w, h, k=40):
    """One sweep per cut and axis: [(axis, cut, x, y)], 2k floats of the swept coordinate around the cut's pre-image, the
    other coordinate spread over the interior.  Asserts that each sweep straddles its cut."""
    cx, cy = TARGETS[(w, h)]
    out = []
    for axis, (dim, c0, f, odim, oc, of) in enumerate(((w, cx, FX, h, cy, FY), (h, cy, FY, w, cx, FX))):
        for c in _cuts(dim):
            a = _around(F32((c - c0) / f), k)
            ua = _project(a, c0, f)
            below, above = int((ua.astype(np.float64) < c).sum()), int((ua.astype(np.float64) >= c).sum())
            assert below >= 10 and above >= 10, (w, h, axis, c, below, above)
            assert len(np.unique(ua)) >= 20, (w, h, axis, c)
            b = _unproject(2.3 + (np.arange(2 * k) * 0.618034 * (odim - 5)) % (odim - 5), oc, of)
            out.append((axis, c, a, b) if axis == 0 else (axis, c, b, a))
    return out


def _axis_lattice(dim, step):
    """(fine, coarse) positions along one axis: 16 steps per texel over (-1.5, 1) and [dim - 2, dim - 0.5), and a walk
    over the interior in steps of `step` texels."""
    fine = np.concatenate([-1.5 + np.arange(1, 40) / 16.0, dim - 2 + np.arange(24) / 16.0])
    return fine, np.arange(1.37, dim - 2, step)


def _lattice(w, h, step):
    """The four border bands, 16 steps per texel across each band and, in the corners, along it too; `step` along the
    bands between the corners."""
    cx, cy = TARGETS[(w, h)]
    uf, uc = _axis_lattice(w, step)
    vf, vc = _axis_lattice(h, step)
    ua, va = np.meshgrid(uf, np.concatenate([vf, vc]))  # left and right bands with the four corners
    ub, vb = np.meshgrid(uc, vf)                          # top and bottom bands between them
    u, v = np.concatenate([ua.ravel(), ub.ravel()]), np.concatenate([va.ravel(), vb.ravel()])
    return _unproject(u, cx, FX), _unproject(v, cy, FY)


def _crafted(w, h, n_total=None, shuffle=False, step=5.3):
    """Every sweep, the lattice and at least 300 interior points; padded with interior points up to n_total."""
    parts = [(x, y) for _, _, x, y in _sweeps(w, h)] + [_lattice(w, h, step)]
    n = sum(len(x) for x, _ in parts)
    pad = 300 if n_total is None else n_total - n
    assert pad >= 300, (n, n_total)
    parts.append(_interior(pad, w, h, 11))
    x, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if shuffle:  # waves that mix lanes on a cut, border lanes and interior lanes
        order = np.random.default_rng(3).permutation(len(x))
        x, y = x[order], y[order]
    return x, y


def _finite(s):
    return bool(np.isfinite(s["H"]).all() and np.isfinite(s["g"]).all() and np.isfinite(s["ssq"]))


def _check(ctx, prm, ft, fs, T, what, diag_ctx=None, images=None):
    """One pass from T on the device against the oracle's f64-summed pass: counts exact, sums within ACC_TOL where the
    oracle's are finite and non-finite in the same places where they are not.  Returns the oracle's two counts."""
    st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, T.to_c(), accum_f64=True)
    assert st == 0, what
    g_ref, c_ref = g_ref.as_dict(), c_ref.as_dict()
    rt, rs = images if images is not None else (to_range_image(ft), to_range_image(fs))
    g_gpu, c_gpu = ImageIcp.new(ctx, prm, rt).accumulate(rs, T)
    print(what, "counts", g_gpu["count"], g_ref["count"], c_gpu["count"], c_ref["count"])
    assert g_gpu["count"] == g_ref["count"] and c_gpu["count"] == c_ref["count"], \
        (what, g_gpu["count"], g_ref["count"], c_gpu["count"], c_ref["count"])

    def compare(got, ref, tol, tag):
        if _finite(ref):
            eh, eg, es = gn_rel_err(got, ref)
            print(what, tag, eh, eg, es)
            assert eh < tol and eg < tol and es < tol, (what, tag, eh, eg, es)
        else:
            for key in ("H", "g", "ssq"):
                assert np.array_equal(np.isfinite(got[key]), np.isfinite(ref[key])), (what, tag, key)

    compare(g_gpu, g_ref, ACC_TOL, "geometry")
    compare(c_gpu, c_ref, ACC_TOL, "colour")
    if diag_ctx is not None:  # the cross-check kernel (the reference's unfused operations) between the two
        g_ex, c_ex = ImageIcp.new(diag_ctx, prm, to_range_image(ft)).accumulate_exact(to_range_image(fs), T)
        assert g_ex["count"] == g_ref["count"] and c_ex["count"] == c_ref["count"], (what, "exact kernel")
        compare(g_ex, g_ref, ACC_TOL, "exact kernel, geometry")
        compare(c_ex, c_ref, ACC_TOL, "exact kernel, colour")
        if _finite(g_ex) and _finite(c_ex):
            compare(g_gpu, g_ex, 5e-7, "fused vs exact kernel, geometry")
            compare(c_gpu, c_ex, 5e-7, "fused vs exact kernel, colour")
    return g_ref["count"], c_ref["count"]


POSES = [("eye", Transform.eye), ("pose3", lambda: small_pose(3))]


# ---- A. sweeps across every cut of the projection ----------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 63), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", list(TARGETS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_projection_cuts_one_sweep_per_call(ctx, diag_ctx, size, shape):
    """One wave (63 pixels) and one wave with a tail of one (65): each call holds one sweep, whose samples sit on
    neighbouring lanes, and one interior pixel."""
    w, h = size
    n = shape[0] * shape[1]
    k = (n - 1) // 2
    ft, prm = _target(w, h), _open_gates()
    kept = total = 0
    for axis, c, x, y in _sweeps(w, h, k):
        xi, yi = _interior(n - 2 * k, w, h, 17)
        fs = _source(np.concatenate([x, xi]), np.concatenate([y, yi]), shape)
        for name, pose in POSES:
            gc, cc = _check(ctx, prm, ft, fs, pose(), (size, shape, "uv"[axis], c, name), diag_ctx)
            assert gc == cc > 0
            if name == "eye":
                kept, total = kept + gc, total + n
    assert 0 < kept < total  # some sweeps leave the image


@pytest.mark.parametrize("shape,shuffle", [((8, 0), False), ((80, 96), True)], ids=["8xN", "96x80"])
@pytest.mark.parametrize("size", list(TARGETS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_projection_cuts_and_border_lattice(ctx, diag_ctx, size, shape, shuffle):
    """All twenty sweeps, the lattice over the border bands and corners and the interior pixels in one source: in order
    in 8 rows (whole waves on one cut), shuffled in 96 x 80 (every wave mixes lanes that resample with lanes that do not),
    several blocks each."""
    w, h = size
    if shape[1] == 0:  # as wide as it takes: the bands are walked at 0.37 texels, every row and column several times
        x, y = _crafted(w, h, step=0.37)
        x, y = _crafted(w, h, n_total=-(-len(x) // 8) * 8, step=0.37)
        shape = (8, len(x) // 8)
    else:
        x, y = _crafted(w, h, n_total=shape[0] * shape[1], shuffle=True)
    ft, fs, prm = _target(w, h), _source(x, y, shape), _open_gates()
    for name, pose in POSES:
        gc, cc = _check(ctx, prm, ft, fs, pose(), (size, shape, name), diag_ctx)
        assert 0 < gc < len(x) and cc == gc


# ---- B. degenerate projections and masks -------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
SPECIALS = [(0.0, 0.0, 0.0), (0.0, 0.0, -0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.1, 0.1, -1.0), (0.1, 0.1, 1e-30),
            (1e20, 0.1, 1e30), (NAN, 0.0, 1.0), (0.0, INF, 1.0), (3e9, 0.0, 1.0), (-3e9, 0.0, 1.0)]


@pytest.mark.parametrize("shape,at", [((1, 64), 0), ((1, 64), 31), ((1, 64), 63), ((8, 25), 130)],
                         ids=["64-lane0", "64-lane31", "64-lane63", "200-wave2"])
def test_one_degenerate_projection_per_call(ctx, shape, at):
    """u NaN (casts to pixel 0), +-inf and beyond +-2^31 (saturate out of range), a point behind the camera, and z or x fx
    outside the range of the shared reciprocal (the special's whole wave then takes the IEEE divide): one special among
    ordinary pixels, whose count says whether the reference keeps it."""
    prm = _open_gates()
    n = shape[0] * shape[1]
    in_geometry, in_colour = set(), set()
    for w, h in TARGETS:
        ft = _target(w, h)
        x, y = _interior(n, w, h, 23)
        mask = np.ones(n, np.uint8)
        mask[at] = 0
        for name, pose in POSES:
            T = pose()
            g0, c0 = _check(ctx, prm, ft, _source(x, y, shape, mask=mask), T, (w, h, shape, at, "without", name))
            assert g0 == c0 == n - 1
            for k, sp in enumerate(SPECIALS):
                xs, ys, zs = x.copy(), y.copy(), np.ones(n, F32)
                with np.errstate(over="ignore"):
                    xs[at], ys[at], zs[at] = sp
                gc, cc = _check(ctx, prm, ft, _source(xs, ys, shape, z=zs), T, (w, h, shape, at, sp, name))
                assert g0 <= gc <= g0 + 1 and c0 <= cc <= c0 + 1
                if name == "eye" and gc > g0:
                    in_geometry.add(k)
                if name == "eye" and cc > c0:
                    in_colour.add(k)
    assert 0 < len(in_geometry) < len(SPECIALS) and 0 < len(in_colour) < len(SPECIALS), (in_geometry, in_colour)


def test_masks_other_than_zero_and_one(ctx):
    """The source rule is mask != 0 (image_icp.rs:102), the target's mask == 1 (structure.rs:176)."""
    prm = _open_gates()
    values = np.array([0, 1, 2, 255], np.uint8)
    for w, h in TARGETS:
        tmask = values[np.random.default_rng(41).integers(0, 4, (h, w))]
        ft = _target(w, h, mask=tmask)
        x, y = _crafted(w, h)
        x, y = _crafted(w, h, n_total=-(-len(x) // 8) * 8)
        smask = values[(np.arange(len(x)) * 7 // 3) % 4]
        fs = _source(x, y, (8, len(x) // 8), mask=smask)
        for name, pose in POSES:
            gc, cc = _check(ctx, prm, ft, fs, pose(), (w, h, "masks", name))
            assert 0 < gc < int((smask != 0).sum()) and cc == gc
        # every pairing of the two mask values occurs among the pixels that project into the image
        ur, vr = _project(x, TARGETS[(w, h)][0], FX) + F32(0.5), _project(y, TARGETS[(w, h)][1], FY) + F32(0.5)
        u, v = np.trunc(ur).astype(np.int64), np.trunc(vr).astype(np.int64)
        inside = (ur > -1) & (u < w) & (vr > -1) & (v < h)
        seen = {(int(s), int(t)) for s, t in zip(smask[inside], tmask[v[inside], u[inside]])}
        assert len(seen) == 16


# ---- C. unequal sizes, uploaded images ---------------------------------------------------------------------------

_streams = {}


def _stream(w, h):
    if (w, h) not in _streams:
        _streams[(w, h)] = synth.frame_stream(31, 2, w, h)[0]
    return _streams[(w, h)]


def _window(frame, cam, x0, y0, w, h):
    """The w x h window of a rendered frame at (x0, y0), and the camera that sees it: the principal point moves."""
    depth, rgb = frame
    return ((np.ascontiguousarray(depth[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w])),
            CameraIntrinsics(cam.fx, cam.fy, cam.cx - x0, cam.cy - y0, w, h))


def _oracle_frame(frame, cam):
    return O.build_frame(frame[0], frame[1], cam.fx, cam.fy, cam.cx, cam.cy, synth.DEPTH_SCALE)


# (rendered size, window offset, window size, windowed side)
WINDOWS = [((300, 199), (40, 25), (211, 150), "source"), ((300, 199), (40, 25), (211, 150), "target"),
           ((160, 120), (17, 9), (101, 77), "source"), ((160, 120), (17, 9), (101, 77), "target")]
# a source wider than its target, and a source whose pixel count is no multiple of the wave
_SIZES = [(win, full) if side == "target" else (full, win) for full, _, win, side in WINDOWS]  # (target, source)
assert any(s[0] > t[0] for t, s in _SIZES) and any(s[0] * s[1] % 64 for _, s in _SIZES)


@pytest.mark.parametrize("full,offset,win,side", WINDOWS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_unequal_sizes_uploaded(ctx, full, offset, win, side):
    """Frame 0 is the target and frame 1 the source; one of the two is a window with its own intrinsics."""
    frames, cam = _stream(*full), synth.camera(*full)
    t, s = (frames[0], cam), (frames[1], cam)
    if side == "source":
        s = _window(frames[1], cam, *offset, *win)
    else:
        t = _window(frames[0], cam, *offset, *win)
    ft, fs = _oracle_frame(*t), _oracle_frame(*s)
    assert (ft.w, ft.h) != (fs.w, fs.h)
    prm = MsIcpParams.default()[0]
    images = (to_range_image(ft), to_range_image(fs))
    for name, pose in POSES:
        gc, _ = _check(ctx, prm, ft, fs, pose(), (full, win, side, name), images=images)
        assert gc > 20
    prm3 = MsIcpParams.default()[0]
    prm3.max_iterations = 3
    T_gpu = ImageIcp.new(ctx, prm3, images[0]).align(images[1])
    st, T_ref, _ = O.image_icp_align(prm3.to_c(), ft, fs)
    ang, tr = transform_diff(T_gpu, T_ref)
    print((full, win, side), "align", ang, tr)
    assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (ang, tr)


# ---- D. unequal sizes through device-built pyramids --------------------------------------------------------------

BIG, SMALL, SMALL_AT = (160, 120), (128, 96), (20, 14)
KINDS = [("big", "small"), ("small", "big"), ("big", "big"), ("small", "small")]  # (target, source): frame 0 <- frame 1


def _build(c, filt):
    """{"big" | "small": [pyramid of frame 0, pyramid of frame 1]}, three levels each, built on context c."""
    frames, cam = _stream(*BIG), synth.camera(*BIG)
    small = [_window(f, cam, *SMALL_AT, *SMALL) for f in frames]
    b = RangeImageBuilder(c)
    if filt:
        b = b.with_bilateral_filter(BilateralFilter.default())
    return {"big": b.build_many(cam, frames, synth.DEPTH_SCALE),
            "small": b.build_many(small[0][1], [f for f, _ in small], synth.DEPTH_SCALE)}


def _free(built):
    for lv in (lv for pyrs in built.values() for p in pyrs for lv in p):
        lv.free()


def _host_copy(pyr):
    host = [lv.download(colors=False) for lv in pyr]
    for lv in host:
        lv._device = None
    return host


def _frame_of(ri):
    k = ri.intrinsics
    return O.Frame(ri.points, ri.mask, k.fx, k.fy, k.cx, k.cy, ri.normals, ri.intensities, ri.intensity_map)


def _batch(c, prm, tp, sp):
    """The poses as float32 matrices with each pair's status appended."""
    b = MultiscaleAlignBatch(c, prm, tp, sp)
    poses, status = b.align()
    b.free()
    m = np.stack([p.matrix() for p in poses]).astype(np.float32).reshape(len(poses), -1)
    return poses, np.concatenate([m, status.view(np.float32)[:, None]], 1)


def _lone(c, prm, t, s):
    a = MultiscaleAlign.new(c, prm, t)
    m = a.align(s).matrix()
    a.free()
    return np.asarray(m, np.float32).reshape(-1)


def _same(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, np.abs(a - b).max())


def _assert_rebuilt_from_depth(diag_ctx, built):
    """Both sizes pass the host proof behind DEPTH16 and carry their planes: the level-0 points are rebuilt, not read."""
    for pyrs in built.values():
        lv = pyrs[0][0]
        h, w = lv.shape
        depth, bp, flag = np.empty((h, w), np.uint16), (C.c_float * 5)(), C.c_int32()
        assert diag_ctx.lib.a3d_range_image_download_depth16(lv.handle, _abi.ptr(depth), bp, C.byref(flag)) == 0
        proven = C.c_int32()
        assert diag_ctx.lib.a3d_backproject_proven(w, h, bp, C.byref(proven)) == 0
        assert flag.value == 1 and proven.value == 1, (w, h)


@pytest.mark.parametrize("filt", [False, True], ids=["plain", "bilateral"])
def test_unequal_sizes_through_device_built_pyramids(ctx, diag_ctx, monkeypatch, filt):
    pyr, dpyr = _build(ctx, filt), _build(diag_ctx, filt)
    _assert_rebuilt_from_depth(diag_ctx, dpyr)
    host = {k: [_host_copy(p) for p in v] for k, v in pyr.items()}
    prm = MsIcpParams.default()
    kinds = KINDS * 3  # 12 pairs: three stream groups
    tp, sp = [pyr[t][0] for t, _ in kinds], [pyr[s][1] for _, s in kinds]
    dtp, dsp = [dpyr[t][0] for t, _ in kinds], [dpyr[s][1] for _, s in kinds]
    htp, hsp = [host[t][0] for t, _ in kinds], [host[s][1] for _, s in kinds]
    poses, fast = _batch(ctx, prm, tp, sp)
    assert not fast[:, -1].view(np.int32).any()
    _same(fast, _batch(diag_ctx, prm, dtp, dsp)[1], "diagnostics build")
    monkeypatch.setenv("A3D_ICP_DEPTH16", "0")
    _same(fast, _batch(diag_ctx, prm, dtp, dsp)[1], "points read")
    monkeypatch.delenv("A3D_ICP_DEPTH16")
    monkeypatch.setenv("A3D_ICP_ZMASK", "0")
    _same(fast, _batch(diag_ctx, prm, dtp, dsp)[1], "masks read")
    monkeypatch.delenv("A3D_ICP_ZMASK")
    _same(fast, _batch(ctx, prm, htp, hsp)[1], "uploaded copies")
    for k in range(4, 12):  # equal inputs give equal outputs wherever the pair sits
        _same(fast[k], fast[k % 4], ("position", k))
    # a lone pair: rebuilt from depth against uploaded, as a lone pair is cut into blocks by its own rule
    for k, (t, s) in enumerate(KINDS):
        _same(_lone(ctx, prm, pyr[t][0], pyr[s][1]),
              _lone(ctx, prm, [lv.device(ctx) for lv in host[t][0]], [lv.device(ctx) for lv in host[s][1]]), ("lone", t, s))
    # pinned tiling: the batch against its uploaded copy, and each pair alone against its row of the batch
    ctx.set_tiling(24)
    try:
        pinned = _batch(ctx, prm, tp, sp)[1]
        _same(pinned, _batch(ctx, prm, htp, hsp)[1], "pinned tiling, uploaded copies")
        for k, (t, s) in enumerate(KINDS):
            _same(pinned[k, :16], _lone(ctx, prm, pyr[t][0], pyr[s][1]), ("pinned tiling, lone", t, s))
    finally:
        ctx.set_tiling(0)
    # each distinct pair against the oracle on the arrays the kernels read
    for k, (t, s) in enumerate(KINDS):
        st, T_ref = O.multiscale_align(prm.to_c_array(), 3, [_frame_of(lv) for lv in host[t][0]],
                                       [_frame_of(lv) for lv in host[s][1]], threads=4)
        ang, tr = transform_diff(poses[k], T_ref)
        print((t, s, filt), "multiscale", ang, tr)
        assert st == 0 and ang <= ROT_TOL and tr <= TRANS_TOL, (t, s, ang, tr)
    _free(pyr), _free(dpyr)


@pytest.mark.parametrize("kind", KINDS[:2], ids=lambda k: f"{k[0]}<-{k[1]}")
def test_level0_rebuilt_from_depth_at_two_borders(ctx, diag_ctx, monkeypatch, kind):
    """Level 0 of an unequal device-built pair (points rebuilt from the depth planes, each side with its own constants)
    from a pose that moves the source by a third of the target's width and height at the scene's mean depth: a large
    share of the source leaves through the right and the bottom border."""
    pyr, dpyr = _build(ctx, True), _build(diag_ctx, True)
    _assert_rebuilt_from_depth(diag_ctx, dpyr)
    t, s = kind
    tgt, src = pyr[t][0][0], pyr[s][1][0]
    ht, hs = _host_copy([tgt])[0], _host_copy([src])[0]
    ft, fs = _frame_of(ht), _frame_of(hs)
    z = float(hs.points[..., 2][hs.mask == 1].mean())
    push = Transform(t=(ft.w / 3.0 / ft.fx * z, ft.h / 3.0 / ft.fy * z, 0.0)) * small_pose(3)
    prm = _open_gates()
    at_eye, _ = _check(ctx, prm, ft, fs, Transform.eye(), (kind, "eye"), images=(tgt, src))
    pushed, _ = _check(ctx, prm, ft, fs, push, (kind, "pushed"), images=(tgt, src))
    print(kind, "share of the source that left the image:", 1.0 - pushed / at_eye, pushed, at_eye)
    assert 0 < pushed <= 0.75 * at_eye
    # the three kernel forms give the same sums
    dt, dsrc = dpyr[t][0][0], dpyr[s][1][0]
    for T in (Transform.eye(), push):
        want = ImageIcp.new(ctx, prm, tgt).accumulate(src, T)
        forms = [ImageIcp.new(diag_ctx, prm, dt).accumulate(dsrc, T)]
        for knob in ("A3D_ICP_DEPTH16", "A3D_ICP_ZMASK"):
            monkeypatch.setenv(knob, "0")
            forms.append(ImageIcp.new(diag_ctx, prm, dt).accumulate(dsrc, T))
            monkeypatch.delenv(knob)
        for got in forms:
            for a, b in zip(got, want):
                assert a["count"] == b["count"]
                for key in ("H", "g", "ssq"):
                    assert np.array_equal(np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)), key
    _free(pyr), _free(dpyr)
