"""The host cut that replaces the reference's normal-angle gate (no GPU needed).

Neither ICP kernel calls acos: acos_gate_threshold (csrc/context.hip) bisects the float line once per launch for the
largest dot product d with |acos(d)| > max_normal_angle (point-cloud ICP, strict: pcl_icp.rs) or >= (image ICP, on the
point p: image_icp.rs), and the kernels reject iff -1 <= d <= cut.  That decision must be the reference's for every
float d, whatever the threshold: here it is compared with the oracle's own expression on every float near the cut, near
both ends of [-1, 1] and on the special values, through the diagnostics build's export of the same host function."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import IcpParams, MsIcpParams, _abi

F32 = np.float32
PI = F32(np.pi)


def _next(x, k):
    """The float k steps above x (k < 0: below) in the total order of the floats (through +-0, on to +-inf)."""
    u = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(u < 0, -(u & 0x7FFFFFFF), u) + k  # signed magnitude -> a line on which -0 and +0 coincide
    b = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)
    return b.view(F32)


def _around(x, k):
    """The 2k floats nearest to x: k below it and k from it upwards."""
    return _next(np.full(2 * k, x, F32), np.arange(-k, k))


def _thresholds():
    return [F32(0.0), F32(-0.0), F32(1e-30), F32(1e-6), F32(0.1), F32(IcpParams.default().max_normal_angle),
            F32(MsIcpParams.default()[0].max_normal_angle),
            F32(np.pi / 4), F32(np.pi / 2), F32(3.0), _next(PI, -1)[()], PI, _next(PI, 1)[()], F32(4.0), F32(-0.5),
            F32(np.nan), F32(np.inf)]


def _cut(lib, thr, strict):
    out = C.c_float()
    assert lib.a3d_acos_gate_threshold(F32(thr), int(strict), C.byref(out)) == 0
    return F32(out.value)


@pytest.fixture(scope="module")
def diag_lib():
    return _abi.load_library(_abi.DIAG_LIB_PATH)


def _probe_values(thr):
    one = F32(1.0)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.nan, -np.nan, np.inf, -np.inf], F32)
    parts = [special, _next(np.array([one, one, -one, -one], F32), np.array([1, -1, 1, -1])),
             _around(one, 1 << 16), _around(-one, 1 << 16)]
    if np.isfinite(thr):
        parts.append(_around(F32(np.cos(thr)), 1 << 20))
    return np.concatenate(parts)


@pytest.mark.parametrize("strict", [1, 0], ids=["strict_pcl", "nonstrict_image"])
@pytest.mark.parametrize("thr", _thresholds(), ids=lambda t: repr(float(t)) + ("-" if np.signbit(t) else ""))
def test_dot_product_cut_decides_as_the_reference_gate(diag_lib, thr, strict):
    cut = _cut(diag_lib, thr, strict)
    d = _probe_values(thr)
    with np.errstate(invalid="ignore"):
        product = (d >= F32(-1.0)) & (d <= cut)  # kdtree.hip pcl_point_loop, image_icp.hip stage_c
    ref = O.acos_gate_rejects(d, thr, strict)
    bad = np.flatnonzero(product != ref)
    assert bad.size == 0, (f"thr={thr!r} strict={strict} cut={cut!r}: {bad.size} floats decided differently, e.g. "
                           f"{d[bad[:4]].tolist()} (reference rejects: {ref[bad[:4]].tolist()})")


def test_probe_helpers_walk_the_float_line():
    assert _next(F32(1.0), 1) == np.nextafter(F32(1.0), F32(2.0))
    assert _next(F32(1.0), -1) == np.nextafter(F32(1.0), F32(0.0))
    assert _next(F32(0.0), -1) == -np.nextafter(F32(0.0), F32(1.0))
    assert _next(F32(-0.0), 1) == np.nextafter(F32(0.0), F32(1.0))
    a = _around(F32(1.0), 8)
    assert len(a) == 16 and np.all(np.diff(a.astype(np.float64)) > 0) and a[8] == F32(1.0)
