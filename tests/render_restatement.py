"""A numpy restatement of the render rule (a3d_point_cloud_render_device), written from the reference:
PinholeCamera::project_to_image (src/camera.rs:177-202), CameraIntrinsics::project (camera.rs:64-70) and
Transform::transform_vector / transform_normal (src/transform.rs:138-153), never from the kernel.

All arithmetic is f32 with every operation rounded on its own (numpy float32 arrays do exactly that).  For each row k:
  p = q * points[k] + t (or points[k] verbatim), z = p.z; dropped unless 0 < z < inf;
  u = p.x * fx / z + cx, v = p.y * fy / z + cy; ui = round(u), vi = round(v) with halves AWAY from zero (Rust f32::round;
  np.round is half-to-even and wrong here); dropped unless 0 <= ui < width and 0 <= vi < height as f32;
  half-widths 0 for radius == 0, else min(floor(radius * fx / z), 8), min(floor(radius * fy / z), 8);
  every pixel of [ui - hx, ui + hx] x [vi - hy, vi + hy] inside the image is offered bits(z) << 32 | k, the minimum wins."""
import numpy as np

from numpy_restatement import _rotate

F = np.float32
MAX_HALF = 8
NO_ROW = 0xFFFFFFFF


def round_half_away(x):
    """Rust's f32::round on a float32 array: trunc plus the fractional part, which is exactly representable (|x| < 2^23
    has frac = x - trunc(x) exact; larger values are integers already).  NaN and infinities pass through."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        frac = x - t  # exact
        step = np.where(np.abs(frac) >= F(0.5), np.copysign(F(1), x), F(0)).astype(F)
        out = (t + step).astype(F)
    # -0.3 -> -0.0 like the reference (trunc keeps the sign); inf - inf above is NaN: put the infinities back
    return np.where(np.isinf(x), x, out).astype(F)


def camera_points(points, pose):
    """Step 1: (p [n, 3]) in the camera's frame; pose = (t_xyz, q_ijkw) or None (verbatim)."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    if pose is None:
        return points.copy()
    t, q = np.asarray(pose[0], F), np.asarray(pose[1], F)
    with np.errstate(all="ignore"):
        return (_rotate(q, points) + t).astype(F)


def camera_normals(normals, pose):
    normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    if pose is None:
        return normals.copy()
    with np.errstate(all="ignore"):
        return _rotate(np.asarray(pose[1], F), normals).astype(F)


def project(p, fx, fy, cx, cy):
    """CameraIntrinsics::project on rows whose z is positive and finite: (u, v) f32."""
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    with np.errstate(all="ignore"):
        z = p[:, 2]
        return (p[:, 0] * fx / z + cx).astype(F), (p[:, 1] * fy / z + cy).astype(F)


def footprints(p, fx, fy, cx, cy, width, height, radius):
    """Steps 2-6 for camera-frame rows p: (rows kept, ui, vi, hx, hy) as int64 arrays over the kept rows."""
    z = p[:, 2]
    with np.errstate(all="ignore"):
        alive = (z > F(0)) & (z < F(np.inf))
        u, v = project(p, fx, fy, cx, cy)
        ui, vi = round_half_away(u), round_half_away(v)
        inside = (ui >= F(0)) & (ui < F(width)) & (vi >= F(0)) & (vi < F(height))
        keep = np.nonzero(alive & inside)[0]
        zk = z[keep]
        if F(radius) == F(0):
            hx = hy = np.zeros(len(keep), np.int64)
        else:
            hx = np.minimum(np.floor((F(radius) * F(fx)).astype(F) / zk), F(MAX_HALF)).astype(np.int64)
            hy = np.minimum(np.floor((F(radius) * F(fy)).astype(F) / zk), F(MAX_HALF)).astype(np.int64)
    return keep, ui[keep].astype(np.int64), vi[keep].astype(np.int64), hx, hy


def render(points, normals, colors, pose, fx, fy, cx, cy, width, height, radius):
    """The whole rule.  Returns a dict: points [h, w, 3] f32, mask [h, w] u8, normals or None, colors or None,
    index [h, w] u32."""
    p = camera_points(points, pose)
    keep, ui, vi, hx, hy = footprints(p, fx, fy, cx, cy, width, height, radius)
    zbits = p[:, 2].copy().view(np.uint32).astype(np.uint64)
    best = np.full(width * height, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    # one (dy, dx) offset of the footprint at a time, over every row at once: at most 17 x 17 passes
    for dy in range(-MAX_HALF, MAX_HALF + 1):
        for dx in range(-MAX_HALF, MAX_HALF + 1):
            sel = (np.abs(dx) <= hx) & (np.abs(dy) <= hy)
            if not sel.any():
                continue
            c, r = ui[sel] + dx, vi[sel] + dy
            ok = (c >= 0) & (c < width) & (r >= 0) & (r < height)
            k = keep[sel][ok].astype(np.uint64)
            key = zbits[keep[sel][ok]] << np.uint64(32) | k
            np.minimum.at(best, (r[ok] * width + c[ok]), key)
    won = best != np.uint64(0xFFFFFFFFFFFFFFFF)
    index = np.where(won, best & np.uint64(0xFFFFFFFF), np.uint64(NO_ROW)).astype(np.uint32)
    rows = index[won].astype(np.int64)
    out_points = np.zeros((width * height, 3), F)
    out_points[won] = p[rows]
    out = {"points": out_points.reshape(height, width, 3), "mask": won.astype(np.uint8).reshape(height, width),
           "index": index.reshape(height, width), "normals": None, "colors": None}
    if normals is not None:
        n = np.zeros((width * height, 3), F)
        n[won] = camera_normals(normals, pose)[rows]
        out["normals"] = n.reshape(height, width, 3)
    if colors is not None:
        c = np.zeros((width * height, 3), np.uint8)
        c[won] = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)[rows]
        out["colors"] = c.reshape(height, width, 3)
    return out
