"""GPU parity of the ICP correspondence gates at their thresholds.

Crafted inputs put hundreds of correspondences within a few floats of each cut: the normal-angle gate (|acos(d)| >
max_normal_angle, strict, in point-cloud ICP; >= on the point p in image ICP: the kernels compare d with a host-bisected
cut instead), the distance gate (d2 > max_distance^2) and the colour gate (rc^2 <= max_color_distance^2).  Counts must
be the oracle's exactly; H, g and the residual sum within the usual 1e-6 of the f64-summed oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import CameraIntrinsics, Icp, IcpParams, ImageIcp, MsIcpParams, PointCloud, RangeImage, Transform, _abi
from gpu_util import gn_rel_err

pytestmark = pytest.mark.gpu

F32 = np.float32
PI = F32(np.pi)
DEFAULT_ANGLE = F32(IcpParams.default().max_normal_angle)
DEFAULT_DISTANCE = F32(IcpParams.default().max_distance)


def _next(x, k):
    """The float k steps above x (k < 0: below) in the total order of the floats (-0 and +0 count as one)."""
    u = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(u < 0, -(u & 0x7FFFFFFF), u) + k
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _around(x, k):
    return _next(np.full(2 * k, x, F32), np.arange(-k, k))


ANGLES = [F32(0.0), F32(-0.0), F32(1e-30), F32(1e-6), F32(0.1), DEFAULT_ANGLE, F32(MsIcpParams.default()[0].max_normal_angle),
          F32(np.pi / 4), F32(np.pi / 2), F32(3.0), _next(PI, -1)[()], PI, _next(PI, 1)[()], F32(4.0), F32(-0.5),
          F32(np.nan), F32(np.inf)]
DISTANCES = [F32(0.0), F32(1e-3), DEFAULT_DISTANCE, F32(1e3), F32(np.inf), F32(np.nan)]


def _cut(thr, strict):
    out = C.c_float()
    assert _abi.load_library(_abi.DIAG_LIB_PATH).a3d_acos_gate_threshold(F32(thr), int(strict), C.byref(out)) == 0
    return F32(out.value)


NONFINITE_DOTS = np.array([np.nan, np.inf, -np.inf], F32)


def _dot_sweep(thr, k=100, finite=False):
    """Dot products around both cuts and fl(cos thr), near +-1, and the values whose acos is NaN (kept by the reference):
    1 + ulp, -1 - ulp and (unless `finite`) NaN, +-inf."""
    parts = [_around(_cut(thr, True), k), _around(_cut(thr, False), k), _around(F32(1.0), 20), _around(F32(-1.0), 20),
             np.array([0.0, -0.0, _next(F32(1.0), 1), _next(F32(-1.0), 1)], F32)] + ([] if finite else [NONFINITE_DOTS])
    if np.isfinite(thr):
        parts.append(_around(F32(np.cos(thr)), k))
    return np.concatenate(parts)


# ---- point-cloud ICP ---------------------------------------------------------------------------------------------

def _pcl_case(dots, md, k_off=201):
    """Target point k at (G k, -2 k, 2 ((37 k) mod 4099) + 0.5), normal (1, 0, 0): every coordinate distinct, so the
    descent of a query that differs from a target point by 0 <= delta < G in x only follows that point's path (split
    values are points' coordinates, a point equal to the split goes right) and its leaf scan finds it at squared distance
    fl(delta^2).  Source point k: its partner + (delta_k, 0, 0), normal (c_k, s_k, 0), so sn . tn == c_k exactly at the
    identity.  The first k_off points sweep delta over the floats x_k + md + j ulp (j = 0, 1, -1, 2, ...; point 0 at
    x = 0 has delta = md exactly): exact differences whose squares fall below, on and above fl(md^2).  The angle-sweep
    points get small distinct offsets (distinct residuals); every point has a distinct Jacobian (0, z, -y) part."""
    base = md if np.isfinite(md) else DEFAULT_DISTANCE  # (inf / NaN: every offset passes; the default's sweep stands in)
    n = k_off + len(dots)
    assert n < 4099
    gap = F32(2.0 ** np.ceil(np.log2(4.0 * max(float(base), 1.0))))
    k = np.arange(n)
    x = (k * gap).astype(F32)
    y = (-2.0 * k).astype(F32)
    z = (2.0 * ((37 * k) % 4099) + 0.5).astype(F32)
    j = np.array([(i + 1) // 2 * (1 if i % 2 else -1) for i in range(k_off)])
    if base == 0:
        j = np.abs(j)  # (delta >= 0: the partner stays the nearest)
    sx = np.concatenate([_next((x[:k_off] + base).astype(F32), j),
                         (x[k_off:] + (np.arange(len(dots)) + 1).astype(F32) * F32(2.0 ** -16)).astype(F32)])
    c = np.concatenate([np.ones(k_off, F32), dots])
    c[1:k_off:2] = _next(F32(1.0), 1)  # (acos NaN: kept whatever the angle)
    tgt = PointCloud(np.stack([x, y, z], 1), np.tile(np.array([[1, 0, 0]], F32), (n, 1)))
    with np.errstate(invalid="ignore"):
        s = np.where(np.abs(c) <= 1, np.sqrt(np.maximum(0.0, 1.0 - c.astype(np.float64) ** 2)), 0).astype(F32)
    src = PointCloud(np.stack([sx, y, z], 1), np.stack([c, s, np.zeros(n, F32)], 1))
    return tgt, src


def _pcl_check(ctx, thr, md):
    tgt, src = _pcl_case(_dot_sweep(thr), md)
    prm = IcpParams(max_iterations=1, max_normal_angle=float(thr), max_distance=float(md))
    tree = O.KdTree(tgt.points)
    g = O.GnStateC()
    tv, sv = O.pcl_view(tgt.points, tgt.normals), O.pcl_view(src.points, src.normals)
    p, t = prm.to_c(), Transform.eye().to_c()
    assert O.load().orc_pcl_icp_accumulate(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(t), 1, C.byref(g)) == 0
    ref = g.as_dict()
    gpu = Icp.new(ctx, prm, tgt).accumulate(src, Transform.eye())
    assert gpu["count"] == ref["count"] and ref["count"] > 0, (thr, md, gpu["count"], ref["count"])
    eh, eg, es = gn_rel_err(gpu, ref)
    assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (thr, md, eh, eg, es)
    return ref["count"], src.len()


@pytest.mark.parametrize("thr", ANGLES, ids=lambda t: repr(float(t)) + ("-" if np.signbit(t) else ""))
def test_pcl_icp_normal_gate_at_the_cut(ctx, thr):
    kept, n = _pcl_check(ctx, thr, DEFAULT_DISTANCE)
    if np.isfinite(thr) and 0.0 < thr < 3.0:
        assert 0 < kept < n  # the sweep straddles the cut


@pytest.mark.parametrize("md", DISTANCES, ids=lambda v: repr(float(v)))
def test_pcl_icp_distance_gate_at_the_cut(ctx, md):
    kept, n = _pcl_check(ctx, DEFAULT_ANGLE, md)
    if np.isfinite(md):
        assert 0 < kept < n


# ---- image ICP ---------------------------------------------------------------------------------------------------

W, H = 64, 48
FX = FY = 50.0
CX, CY = 31.5, 23.25


def _image_pair(dots, offsets, intensities=None, tc=0.5):
    """Source: z = 1 at every pixel centre (mask 1), so each pixel associates with its own target pixel at the identity.
    Target: the same points moved by (0, 0, delta), normal (0, 0, c) so that p . n == c exactly."""
    n = W * H
    vv, uu = np.mgrid[0:H, 0:W]
    pts = np.stack([((uu - CX) / FX), ((vv - CY) / FY), np.ones(uu.shape)], -1).astype(F32)
    c = np.ones(n, F32)
    c[:len(dots)] = dots
    delta = np.zeros(n, F32)
    delta[len(dots):len(dots) + len(offsets)] = offsets
    assert len(dots) + len(offsets) <= n
    tpts = pts.copy()
    tpts[..., 2] = (F32(1.0) + delta.reshape(H, W)).astype(F32)
    nrm = np.zeros((H, W, 3), F32)
    nrm[..., 2] = c.reshape(H, W)
    mask = np.ones((H, W), np.uint8)
    inten = (np.arange(n) % 256).astype(np.uint8) if intensities is None else intensities
    imap = np.full((H + 2, W + 2), F32(tc), F32)
    ft = O.Frame(tpts, mask, FX, FY, CX, CY, normals=nrm, intensities=inten, intensity_map=imap)
    fs = O.Frame(pts, mask, FX, FY, CX, CY, normals=nrm, intensities=inten, intensity_map=imap)
    k = CameraIntrinsics(FX, FY, CX, CY, W, H)
    rt = RangeImage(tpts, mask, k, normals=nrm, intensities=inten, intensity_map=imap)
    rs = RangeImage(pts, mask, k, normals=nrm, intensities=inten, intensity_map=imap)
    return ft, fs, rt, rs


def _image_offsets(md, k=60):
    """Target z = fl(1 + delta): z - 1 on the grid of the floats near 1, around md (exactly md for 0.5, 1e3, 0)."""
    base = DEFAULT_DISTANCE if not np.isfinite(md) else md
    z = _around(F32(1.0) + base, k) if base > 0 else _around(F32(1.0), k)
    return (z - F32(1.0)).astype(F32)  # (one sign: offsets of +-1e3 would cancel in g down to the f32 summation error)


def _image_check(ctx, prm, ft, fs, rt, rs, what):
    st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, Transform.eye().to_c(), accum_f64=True)
    assert st == 0
    g_ref, c_ref = g_ref.as_dict(), c_ref.as_dict()
    g_gpu, c_gpu = ImageIcp.new(ctx, prm, rt).accumulate(rs, Transform.eye())
    assert g_gpu["count"] == g_ref["count"] and c_gpu["count"] == c_ref["count"], \
        (what, g_gpu["count"], g_ref["count"], c_gpu["count"], c_ref["count"])
    for gpu, ref in ((g_gpu, g_ref), (c_gpu, c_ref)):
        eh, eg, es = gn_rel_err(gpu, ref)
        assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (what, eh, eg, es)
    return g_ref["count"], c_ref["count"]


@pytest.mark.parametrize("thr", ANGLES, ids=lambda t: repr(float(t)) + ("-" if np.signbit(t) else ""))
def test_image_icp_normal_gate_at_the_cut(ctx, thr):
    dots = _dot_sweep(thr, k=80, finite=True)  # (a non-finite target normal enters the Jacobian: below)
    ft, fs, rt, rs = _image_pair(dots, _image_offsets(DEFAULT_DISTANCE))
    prm = IcpParams(max_iterations=1, max_normal_angle=float(thr), max_distance=float(DEFAULT_DISTANCE))
    kept, _ = _image_check(ctx, prm, ft, fs, rt, rs, ("angle", thr))
    if np.isfinite(thr) and 0.0 < thr < 3.0:
        assert 0 < kept < W * H


@pytest.mark.parametrize("thr", [F32(0.0), DEFAULT_ANGLE, PI, F32(-0.5)], ids=lambda t: repr(float(t)))
def test_image_icp_keeps_non_finite_normal_dots(ctx, thr):
    """p . n NaN or +-inf: acos is NaN and the reference keeps the pixel, whose Jacobian then holds the non-finite
    normal: the counts must match, and H and g be non-finite exactly where the oracle's are."""
    dots = np.concatenate([NONFINITE_DOTS, _dot_sweep(thr, k=20, finite=True)])
    ft, fs, rt, rs = _image_pair(dots, np.zeros(0, F32))
    prm = IcpParams(max_iterations=1, max_normal_angle=float(thr))
    st, g_ref, _ = O.image_icp_accumulate(prm.to_c(), ft, fs, Transform.eye().to_c(), accum_f64=True)
    assert st == 0
    g_ref = g_ref.as_dict()
    g_gpu, _ = ImageIcp.new(ctx, prm, rt).accumulate(rs, Transform.eye())
    assert g_gpu["count"] == g_ref["count"], (g_gpu["count"], g_ref["count"])
    for key in ("H", "g"):
        assert np.array_equal(np.isfinite(g_gpu[key]), np.isfinite(g_ref[key])), key


@pytest.mark.parametrize("md", DISTANCES, ids=lambda v: repr(float(v)))
def test_image_icp_distance_gate_at_the_cut(ctx, md):
    ft, fs, rt, rs = _image_pair(np.zeros(0, F32), _image_offsets(md))
    prm = IcpParams(max_iterations=1, max_normal_angle=float(DEFAULT_ANGLE), max_distance=float(md))
    kept, _ = _image_check(ctx, prm, ft, fs, rt, rs, ("distance", md))
    if np.isfinite(md):
        assert 0 < kept < W * H


def test_image_icp_colour_gate_at_every_residual(ctx):
    """A constant intensity map and all 256 source intensities: max_color_distance at every distinct |rc| (in the
    oracle's own f32 arithmetic) and the floats either side of it."""
    tc = F32(0.5)
    ft, fs, rt, rs = _image_pair(np.zeros(0, F32), np.zeros(0, F32), tc=tc)
    rc = np.abs(np.arange(256).astype(F32) * F32(0.003921569) - tc).astype(F32)
    icp = ImageIcp.new(ctx, IcpParams(max_iterations=1), rt)
    d_src = rs.device(ctx)
    checked = 0
    for r in np.unique(rc):
        for mc in (_next(r, -1), r, _next(r, 1)):
            prm = IcpParams(max_iterations=1, max_color_distance=float(mc))
            st, g_ref, c_ref = O.image_icp_accumulate(prm.to_c(), ft, fs, Transform.eye().to_c(), accum_f64=True)
            assert st == 0
            icp.params = prm
            g_gpu, c_gpu = icp.accumulate(d_src, Transform.eye())
            assert g_gpu["count"] == g_ref.count == W * H
            assert c_gpu["count"] == c_ref.count, (float(mc), c_gpu["count"], c_ref.count)
            eh, eg, es = gn_rel_err(c_gpu, c_ref.as_dict())
            assert es < 1e-6, (float(mc), es)
            checked += 1
    assert checked >= 3 * 200
