"""The host proof behind the straight-line back-projection of the image ICP kernel (backproject_proven, devmath.hpp):
for one image's size and constants it must say yes exactly when every depth unit d in [1, 65535] at every row and
column gives z = d scale finite and > 0, both focal lengths inside div_by's range, both numerators (col - cx) z and
(row - cy) z inside it (0, or 1e-20 < |a| < 1e9), and a zero numerator only as +0 over a positive focal length (where
div_by(+0) is the +0 that backproject_px selects).  Checked against brute force over every d, in numpy's IEEE f32."""
import ctypes as C

import numpy as np
import pytest

from align3d_amd import _abi

D = np.arange(1, 65536, dtype=np.float32)


@pytest.fixture(scope="module")
def diag():
    return _abi.load_library(_abi.DIAG_LIB_PATH)


def _proven(lib, w, h, bp):
    k = (C.c_float * 5)(*[float(np.float32(v)) for v in bp])
    out = C.c_int32(-1)
    assert lib.a3d_backproject_proven(w, h, k, C.byref(out)) == _abi.A3D_OK
    return out.value


def _axis_brute(n, f, c, scale):
    f, c, scale = np.float32(f), np.float32(c), np.float32(scale)
    if not (abs(f) > np.float32(1e-9) and abs(f) < np.float32(1e9)):
        return False
    with np.errstate(all="ignore"):
        z = D * scale
        if not (np.isfinite(z).all() and (z > 0).all()):
            return False
        k = np.arange(n, dtype=np.float32) - c
        for a in np.array_split(k, max(1, n // 64)):
            ax = a[None, :] * z[:, None]
            zero = ax == 0
            if not (zero | ((np.abs(ax) > np.float32(1e-20)) & (np.abs(ax) < np.float32(1e9)))).all():
                return False
            if zero.any() and (np.signbit(ax[zero]).any() or not f > 0):
                return False
    return True


def _brute(w, h, bp):
    fx, fy, cx, cy, scale = bp
    return int(_axis_brute(w, fx, cx, scale) and _axis_brute(h, fy, cy, scale))


CASES = [  # (w, h, (fx, fy, cx, cy, scale)), expected
    ((7, 5, (5.0, 4.0, 3.0, 2.0, 0.001)), 1),           # integer cx, cy: zero numerators over positive focal lengths
    ((7, 5, (5.0, 4.0, 3.5, 2.25, 0.001)), 1),          # non-integer
    ((8, 6, (5.0, 4.0, 3.3, 2.7, 1e-4)), 1),
    ((8, 6, (5.0, 4.0, -20.25, 40.5, 0.001)), 1),       # principal point outside the image
    ((8, 6, (5.0, 4.0, 1e4, -3e3, 0.001)), 1),
    ((7, 5, (-5.0, 4.0, 3.0, 2.0, 0.001)), 0),          # negative fx and a column at cx: div_by(+0) = -0
    ((7, 5, (-5.0, -4.0, 3.5, 2.5, 0.001)), 1),         # negative focal lengths, no zero numerator
    ((7, 5, (5.0, -4.0, 3.5, 2.0, 0.001)), 0),
    ((7, 5, (5.0, 4.0, 3.0, 2.0, 1e35)), 0),            # 65535 scale leaves the f32 range
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 1e5)), 0),             # |a| reaches 1e9
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 2e3)), 1),
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 1e-21)), 0),           # tiny scale: |a| below 1e-20
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 1e-19)), 1),
    ((7, 5, (5.0, 4.0, 3.0001, 2.5, 1e-17)), 0),        # a column next to cx: its small |col - cx| times scale
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 1e-40)), 0),           # subnormal scale
    ((7, 5, (5.0, 4.0, 3.5, 2.5, 0.0)), 0),
    ((7, 5, (5.0, 4.0, 3.5, 2.5, -0.001)), 0),
    ((7, 5, (1e-10, 4.0, 3.5, 2.5, 0.001)), 0),         # focal length outside div_by's range
    ((7, 5, (2e9, 4.0, 3.5, 2.5, 0.001)), 0),
    ((7, 5, (5.0, 4.0, float("nan"), 2.5, 0.001)), 0),
    ((1, 1, (5.0, 4.0, 0.0, 0.0, 0.001)), 1),
    ((1, 1, (5.0, 4.0, 0.5, 0.5, 0.001)), 1),
    ((640, 480, (525.0, 525.0, 319.5, 239.5, 0.001)), 1),  # the benchmark's size
    ((640, 480, (525.0, 525.0, 320.0, 240.0, 0.0002)), 1),
]


@pytest.mark.parametrize("case,expected", CASES)
def test_proof_matches_brute_force(diag, case, expected):
    w, h, bp = case
    assert _brute(w, h, bp) == expected
    assert _proven(diag, w, h, bp) == expected


def test_proof_random_constants(diag):
    """Random small images around the boundaries: integer and half-integer principal points, scales spanning the range."""
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(60):
        w, h = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        cx = float(rng.choice([rng.integers(-3, 15), rng.integers(-3, 15) + 0.5, rng.uniform(-5, 15)]))
        cy = float(rng.choice([rng.integers(-3, 15), rng.uniform(-5, 15)]))
        fx = float(rng.choice([1.0, -1.0]) * 10 ** rng.uniform(-10, 10))
        fy = float(10 ** rng.uniform(-10, 10))
        scale = float(10 ** rng.uniform(-25, 8))
        bp = (fx, fy, cx, cy, scale)
        want = _brute(w, h, bp)
        assert _proven(diag, w, h, bp) == want, (w, h, bp)
        seen.add(want)
    assert seen == {0, 1}


def test_proof_rejects_empty_images(diag):
    assert _proven(diag, 0, 5, (5.0, 4.0, 3.5, 2.5, 0.001)) == 0
    assert _proven(diag, 5, 0, (5.0, 4.0, 3.5, 2.5, 0.001)) == 0
