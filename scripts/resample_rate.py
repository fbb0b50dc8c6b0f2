"""How often the image-ICP pixel loop takes its resample branch on the benchmark's own frames (CPU only, numpy).

A lane leaves its intensity-map cell when the sample at u + 0.005 (or v + 0.005) falls into the next texel; a wave takes the
branch when any of its 64 lanes does (image_icp.hip: request_shifted).  For the synthetic stream bench.py aligns (seed 1000,
frames 0-2, 640 x 480) this prints, per level, the share of live lanes that leave and the share of aligned 64-pixel runs with
a live lane that hold one — at the ground-truth relative pose, at its inverse and from the identity.

Method: f64 back-projection of the source depth, rounded to the f32 points that are resident, then in f64 the rigid
transform, the projection and the bounds test -1 < u + 0.5 < w; u and v are rounded to f32 before the two casts.  The distance and angle gates are left out (the kernel decides before them too), and
levels 1 and 2 are approximated by taking every 2nd / 4th pixel with the intrinsics halved / quartered.

    python scripts/resample_rate.py > profiles/resample_branch_rate.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from align3d_amd import synth  # noqa: E402

SEED, FRAMES, W, H = 1000, 3, 640, 480
F32 = np.float32


def usize(x):
    return np.where(x > 0, np.trunc(x), 0).astype(np.int64)


def rates(depth, k, R, t, level):
    s = 2 ** level
    fx, fy, cx, cy = k.fx / s, k.fy / s, k.cx / s, k.cy / s
    d = depth[::s, ::s].astype(np.float64) * synth.DEPTH_SCALE
    h, w = d.shape
    vv, uu = np.mgrid[0:h, 0:w]
    p = np.stack([(uu - cx) * d / fx, (vv - cy) * d / fy, d], -1).reshape(-1, 3)
    p = p.astype(F32).astype(np.float64) @ R.T + t  # (the resident points are f32: from the identity that rounding decides)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (p[:, 0] * fx / p[:, 2] + cx).astype(F32)
        v = (p[:, 1] * fy / p[:, 2] + cy).astype(F32)
        live = (d.reshape(-1) > 0) & ~((u + F32(0.5) <= -1) | (u + F32(0.5) >= w) | (v + F32(0.5) <= -1) | (v + F32(0.5) >= h))
        leaves = live & ((usize(u + F32(0.005)) != usize(u)) | (usize(v + F32(0.005)) != usize(v)))
    n = len(u) // 64 * 64
    runs_live, runs_leave = live[:n].reshape(-1, 64).any(1), leaves[:n].reshape(-1, 64).any(1)
    return leaves.sum() / max(1, live.sum()), runs_leave.sum() / max(1, runs_live.sum())


def main():
    frames, poses = synth.frame_stream(SEED, FRAMES, W, H)
    k = synth.camera(W, H)
    print(f"# scripts/resample_rate.py: synth.frame_stream({SEED}, {FRAMES}, {W}, {H}); source frame -> target frame")
    print("# pose | pair | level | lanes that leave, % of live lanes | 64-pixel runs that take the branch, % of runs with a live lane")
    for a, b in ((1, 0), (2, 1), (0, 1), (1, 2)):  # (source, target): the ground-truth pose of a pair, and its inverse
        (Ra, ta), (Rb, tb) = poses[a], poses[b]
        R = np.asarray(Rb, np.float64).T @ np.asarray(Ra, np.float64)
        t = np.asarray(Rb, np.float64).T @ (np.asarray(ta, np.float64) - np.asarray(tb, np.float64))
        for name, (RR, tt) in (("ground truth", (R, t)), ("identity", (np.eye(3), np.zeros(3)))):
            for level in range(3):
                lanes, runs = rates(frames[a][0], k, RR, tt, level)
                print(f"{name} | {a} -> {b} | {level} | {100 * lanes:.2f} | {100 * runs:.1f}")


if __name__ == "__main__":
    main()
