"""Host side of the level-0 pixel step of image ICP (image_icp.hip, devmath.hpp), checked without a GPU.

1. The carried row and column.  A thread's source pixels are 256 apart; the kernel divides the first index by the width
   (row = trunc((i + 0.5) RN(1 / w)) in f32, col = i - row w) and then steps `col += 256 % w; row += 256 / w; if col >= w:
   col -= w, row += 1` in f32 (src_advance).  Restated here in numpy float32 and compared with divmod of the index for
   every in-range pixel of every thread, for every width 1..700 at a few heights, with the tile bases and pixels per
   thread the product's tiling gives (tiling_for, restated: pinned tilings 1 and 3 and the 24 blocks per pair of the
   benchmark's batch), including the two records a thread requests past its own pixels.
2. The verdict behind the three-operation division by the focal lengths (a3d_backproject_short_division_proven: the
   back-projection proof and the exhaustive sweep for fx and fy).
3. The sweep itself where it runs, in C++: tests/cpp/short_division_sweep.hip, host code built here with hipcc, compares
   q = a y, r = fma(-f, q, a), q + r y with `/` over all 2^23 mantissas for the sample focal lengths (and 2^20 numerators
   over the whole admitted range) and for random ones.  Recorded once with 2000 random focal lengths (log-uniform in
   1e-2..1e5, either sign): 2000 of 2000 pass — no focal length that fails has been found; the test runs 40 and does
   not gate on that count."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from align3d_amd import _abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _tiling_for(n, want):
    """tiling_for (image_icp.hip) with one pixel per pipeline step: pixels per thread (even) and blocks."""
    want = max(1, min(want, max(1, (n + 511) // 512)))
    p = (n + 256 * want - 1) // (256 * want)
    p = max(2, ((p + 1) // 2) * 2)
    return max(1, (n + 256 * p - 1) // (256 * p)), p


def _carried(w, n, tiles, ppt):
    """Row and column of every (tile, thread, step) as the kernel derives them, steps 0..ppt+1; with the indices."""
    base = (np.arange(tiles, dtype=np.uint32)[:, None] * np.uint32(256 * ppt) + np.arange(256, dtype=np.uint32)[None, :])
    inv_w = F32(1.0) / F32(w)
    r0 = ((base.astype(F32) + F32(0.5)) * inv_w).astype(np.uint32)  # (v_cvt_u32_f32 truncates)
    row, col = r0.astype(F32), (base - r0 * np.uint32(w)).astype(F32)
    q, r, wf = F32(256 // w), F32(256 % w), F32(w)
    rows, cols, idx = [row], [col], [base]
    for k in range(1, ppt + 2):
        c = col + r
        wrap = c >= wf
        col = np.where(wrap, c - wf, c).astype(F32)
        row = (row + np.where(wrap, q + F32(1.0), q)).astype(F32)
        rows.append(row), cols.append(col), idx.append(base + np.uint32(256 * k))
    return np.stack(rows), np.stack(cols), np.stack(idx)


def _check(w, h, want):
    n = w * h
    tiles, ppt = _tiling_for(n, want)
    rows, cols, idx = _carried(w, n, tiles, ppt)
    live = idx < n
    assert (idx[:ppt] < n).sum() == n, (w, h, want)  # every pixel belongs to one (tile, thread, step < ppt)
    qr, rr = np.divmod(idx[live].astype(np.int64), w)
    assert np.array_equal(rows[live].astype(np.int64), qr) and np.array_equal(cols[live].astype(np.int64), rr), (w, h, want)


@pytest.mark.parametrize("want", [1, 3, 24], ids=["tiles1", "tiles3", "tiles24"])
def test_carried_row_and_column_every_width(want):
    for w in range(1, 701):
        for h in (1, 4, 7, 48):
            _check(w, h, want)


@pytest.mark.parametrize("w,h,want", [(640, 480, 24), (640, 480, 1), (640, 4, 3), (257, 5, 1), (300, 7, 3), (256, 6, 1),
                                      (24, 16, 1), (2048, 2048, 24)])
def test_carried_row_and_column_at_the_product_sizes(w, h, want):
    """The benchmark's level 0, the GPU test's shapes, and the largest image level 0 rebuilds (2^22 pixels)."""
    _check(w, h, want)


@pytest.fixture(scope="module")
def diag():
    return _abi.load_library(_abi.DIAG_LIB_PATH)


def _short(lib, w, h, bp):
    k = (C.c_float * 5)(*[float(F32(v)) for v in bp])
    out = C.c_int32(-1)
    assert lib.a3d_backproject_short_division_proven(w, h, k, C.byref(out)) == _abi.A3D_OK
    return out.value


def test_short_division_verdict(diag):
    fx, fy, cx, cy = synth.SAMPLE_INTRINSICS
    assert _short(diag, 640, 480, (fx, fy, cx, cy, synth.DEPTH_SCALE)) == 1
    k = 24 / 640.0
    assert _short(diag, 24, 16, (fx * k, fy * k, cx * k, cy * k, synth.DEPTH_SCALE)) == 1
    assert _short(diag, 7, 5, (5.0, 4.0, 3.0, 2.0, 0.001)) == 1
    assert _short(diag, 7, 5, (-5.0, -4.0, 3.5, 2.5, 0.001)) == 1       # negative focal lengths, no zero numerator
    assert _short(diag, 7, 5, (-5.0, 4.0, 3.0, 2.0, 0.001)) == 0        # negative fx and a column on cx: +0 / f is -0
    assert _short(diag, 7, 5, (5.0, -4.0, 3.5, 2.0, 0.001)) == 0
    for bad in (1e-10, 2e9, -1e-10, -2e9, 0.0, float("nan"), float("inf")):  # outside div_den_ok
        assert _short(diag, 7, 5, (bad, 4.0, 3.5, 2.5, 0.001)) == 0, bad
        assert _short(diag, 7, 5, (5.0, bad, 3.5, 2.5, 0.001)) == 0, bad
    assert _short(diag, 0, 5, (5.0, 4.0, 3.5, 2.5, 0.001)) == 0


def test_short_division_sweep_program(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "short_division_sweep")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "align3d_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "short_division_sweep.hip")])
    out = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": 0 of 8388608 mantissas differ, 0 random numerators over the range differ, +0 ok, library verdict 1") == 4
    assert "0 verdicts disagree" in out.stdout
