"""The dense TSDF volume (a3d_tsdf_volume_integrate / a3d_tsdf_volume_raycast) timed in one job.
    python scripts/tsdf_probe.py [profiles/tsdf_probe.json] [--parent-library PATH] [--no-track]
Prints one JSON line (and writes it to the path given).  Shapes: the sample1 sequence (640 x 480), its odometry poses, a
256^3 volume at v = 0.02 (truncation 4 v) that holds the scene in front of frame 0.
(a) integrate of one frame, without and with colours, beside a device-to-device copy of the volume's bytes (8 and 12 per
    voxel: the copy reads and writes them once, the integrate reads them once and writes the voxels it touched);
(b) integrate_many of 8 frames in one call beside the same 8 frames as 8 calls: the in-thread frame loop against 8 passes
    over the volume;
(c) raycast at 640 x 480 (samples every 2 v from 0.3 m to the far side of the volume) beside DeviceVoxelMap.render of the
    same scene, the nearest-point map of the whole sequence at the same voxel size, radius v / 2, from the same pose; with
    it, untimed, the pixels each model image covers;
(d) with --parent-library (libalign3d_hip.so of the parent commit): DevicePointCloud render of a frame, one voxel-map insert
    and voxel_downsample of a frame on this build and on the parent's, in alternating windows (and alternating order);
    `within_parent_range` says whether this build's median lies inside the parent's own min-max range, `at_most_parent_max`
    whether it is at least not above it;
(e) unless --no-track: examples/pcl_map.py --tsdf-track 0.02 on sample1 in a child process, its trajectory-error line.
Every timed call is a raw, host-synchronous library call between two device events on the context's stream, averaged over
a window of calls; the windows of the variants of a group alternate; median and extremes over the windows are kept."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import (Context, DevicePointCloud, DeviceTsdfVolume, DeviceVoxelMap, RangeImageBuilder,  # noqa: E402
                         SlamTbDataset, _abi)
from voxel_downsample_probe import odometry_poses, spread  # noqa: E402

WINDOWS = 7
WARMUP = 3
VOXEL = 0.02
DIMS = (256, 256, 256)
ORIGIN = (-2.56, -2.56, 0.0)
Z_NEAR = 0.3
NEW_SYMBOLS = tuple(name for name in _abi.SIGNATURES if name.startswith("a3d_tsdf_volume_"))


def measure(ctx, variants, calls):
    for _, fn in variants:
        for _ in range(WARMUP):
            fn()
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ctx.timer_start()
            for _ in range(calls):
                fn()
            ms[name].append(ctx.timer_stop() / calls)
    return {name: dict(spread(v), calls_per_window=calls) for name, v in ms.items()}


def load_frames(ctx):
    """(camera, level-0 images with colours, their clouds with normals and colours) of the sample1 sequence."""
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).build_many(cam, [(f[1], f[2]) for f in frames], depth_scale)
    images = [p[0] for p in built]
    return cam, images, DevicePointCloud.from_range_images(images, colors=True)


def parent_context(path):
    """A context on a library that predates the volume's entries: loaded without asking for them."""
    held = {name: _abi.SIGNATURES.pop(name) for name in NEW_SYMBOLS}
    try:
        _abi.load_library(path)
    finally:
        _abi.SIGNATURES.update(held)
    return Context(0, library=path)


def shared_calls(ctx, cam, clouds, poses):
    """(d): entries the parent build has too, as raw calls on preallocated outputs."""
    lib, frame = ctx.lib, clouds[-1]
    view, views = frame.view(), (_abi.PointCloudViewC * 1)(frame.view())
    handle = C.c_void_p()
    m = DeviceVoxelMap(ctx, VOXEL, normals=True, colors=True)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    pose, colors, dropped = (_abi.PoseC * 1)(poses[-1].to_c()), (C.c_void_p * 1)(frame.d_colors), (C.c_uint64 * 1)()
    out = DevicePointCloud._allocate(ctx, frame.len(), True)
    out_p, out_n = (C.c_void_p * 1)(out.d_points), (C.c_void_p * 1)(out.d_normals)
    caps, lens, drops = (C.c_uint64 * 1)(frame.len()), (C.c_uint64 * 1)(), (C.c_uint64 * 1)()

    def render():
        st = lib.a3d_point_cloud_render_device(ctx.handle, C.byref(view), frame.d_colors, None, cam.fx, cam.fy, cam.cx, cam.cy,
                                               640, 480, 0.0, None, C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    def insert():
        assert lib.a3d_voxel_map_insert_rgb(m.handle, views, colors, pose, 1, dropped, None) == 0

    def downsample():
        st = lib.a3d_point_clouds_voxel_downsample_device(ctx.handle, views, 1, VOXEL, None, out_p, out_n, None, caps, lens, drops)
        assert st == 0, st

    return [("render_frame_640x480", render), ("voxel_map_insert_frame", insert), ("voxel_downsample_frame", downsample)], (m, out)


def main():
    args = sys.argv[1:]
    parent_path = None
    if "--parent-library" in args:
        k = args.index("--parent-library")
        parent_path = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    track = "--no-track" not in args
    out_path = next((a for a in args if not a.startswith("--")), None)
    ctx = Context(0)
    lib = ctx.lib
    cam, images, clouds = load_frames(ctx)
    assert (cam.width, cam.height) == (640, 480)
    poses = odometry_poses(ctx, clouds)
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    out = {"probe": "tsdf", "windows": WINDOWS, "voxel": VOXEL, "dims": DIMS, "origin": ORIGIN, "frames": len(images),
           "one_job_on_one_box": True}

    # ---- (a), (b): integrate
    plain = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN)
    rgb = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN, colors=True)
    src, dst = ctx.malloc(voxels * 12), ctx.malloc(voxels * 12)
    w2c = (_abi.PoseC * 8)(*[p.inverse().to_c() for p in poses[:8]])
    handles = (C.c_void_p * 8)(*[im.handle for im in images[:8]])

    def integrate(volume, n):
        def call():
            assert lib.a3d_tsdf_volume_integrate(volume.handle, handles, w2c, n) == 0
        return call

    def one_by_one(volume):
        def call():
            for f in range(8):
                one = (C.c_void_p * 1)(images[f].handle)
                assert lib.a3d_tsdf_volume_integrate(volume.handle, one, C.byref(w2c[f]), 1) == 0
        return call

    def copy_of(nbytes):
        def call():
            _abi.check(lib.a3d_memcpy_d2d(ctx.handle, dst, src, nbytes), "a3d_memcpy_d2d")
            ctx.synchronize()  # (the entries under test are host-synchronous: the copy is timed the same way)
        return call

    ms = measure(ctx, [("integrate_1_frame", integrate(plain, 1)), ("integrate_1_frame_colours", integrate(rgb, 1)),
                       ("copy_volume_bytes_8_per_voxel", copy_of(voxels * 8)),
                       ("copy_volume_bytes_12_per_voxel", copy_of(voxels * 12))], calls=20)
    out["integrate_ms"] = ms
    out["integrate_over_copy"] = {
        "plain": round(ms["integrate_1_frame"]["median"] / ms["copy_volume_bytes_8_per_voxel"]["median"], 2),
        "colours": round(ms["integrate_1_frame_colours"]["median"] / ms["copy_volume_bytes_12_per_voxel"]["median"], 2)}
    ms = measure(ctx, [("integrate_many_8_frames", integrate(plain, 8)), ("integrate_8_single_calls", one_by_one(plain)),
                       ("integrate_many_8_frames_colours", integrate(rgb, 8)),
                       ("integrate_8_single_calls_colours", one_by_one(rgb))], calls=10)
    out["integrate_many_ms"] = ms
    out["single_calls_over_integrate_many"] = {
        "plain": round(ms["integrate_8_single_calls"]["median"] / ms["integrate_many_8_frames"]["median"], 2),
        "colours": round(ms["integrate_8_single_calls_colours"]["median"] / ms["integrate_many_8_frames_colours"]["median"], 2)}
    ctx.free(src), ctx.free(dst)
    plain.free()

    # ---- (c): raycast beside the voxel map's render of the same scene
    rgb.clear()
    rgb.integrate_many(images, poses)
    D, W, _ = rgb.download()
    out["voxels_observed"] = int((W > 0).sum())
    del D, W
    m = DeviceVoxelMap(ctx, VOXEL, normals=True, colors=True)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    out["map_cells"] = m.cells()
    pose = poses[-1]
    c2w, inv = pose.to_c(), pose.inverse().to_c()
    z_far = ORIGIN[2] + DIMS[2] * VOXEL
    step = 2 * VOXEL
    handle = C.c_void_p()

    def raycast():
        st = lib.a3d_tsdf_volume_raycast(rgb.handle, C.byref(c2w), cam.fx, cam.fy, cam.cx, cam.cy, 640, 480, Z_NEAR, z_far, step,
                                         C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    def map_render():
        st = lib.a3d_voxel_map_render(m.handle, C.byref(inv), cam.fx, cam.fy, cam.cx, cam.cy, 640, 480, VOXEL / 2, None,
                                      C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    ms = measure(ctx, [("raycast_640x480", raycast), ("voxel_map_render_640x480", map_render)], calls=10)
    out["raycast_ms"] = ms
    out["raycast_samples_per_ray"] = int(np.floor((np.float32(z_far) - np.float32(Z_NEAR)) / np.float32(step))) + 1
    out["raycast_over_map_render"] = round(ms["raycast_640x480"]["median"] / ms["voxel_map_render_640x480"]["median"], 2)
    model = rgb.raycast(cam, pose, Z_NEAR, z_far, step)
    host = model.download(intensity=False)
    out["raycast_pixels_covered"] = int(host.mask.sum())
    out["raycast_pixels_with_normal"] = int(np.any(host.normals != 0, axis=-1).sum())
    model.free()
    model = m.render(cam, pose, VOXEL / 2)
    out["map_render_pixels_covered"] = int(model.download(intensity=False).mask.sum())
    model.free()
    m.free(), rgb.free()

    # ---- (d): entries the parent build has, on both builds
    if parent_path:
        pctx = parent_context(parent_path)
        _, pimages, pclouds = load_frames(pctx)
        this_calls, this_keep = shared_calls(ctx, cam, clouds, poses)
        parent_calls, parent_keep = shared_calls(pctx, cam, pclouds, poses)
        for _, fn in this_calls + parent_calls:
            for _ in range(WARMUP):
                fn()
        rows = {}
        for (name, fn), (_, pfn) in zip(this_calls, parent_calls):
            this_ms, parent_ms = [], []
            for window in range(WINDOWS):
                sides = ((pctx, pfn, parent_ms), (ctx, fn, this_ms))
                for side_ctx, side_fn, acc in (sides if window % 2 == 0 else sides[::-1]):  # (neither build always goes second)
                    side_ctx.timer_start()
                    for _ in range(20):
                        side_fn()
                    acc.append(side_ctx.timer_stop() / 20)
            t, p = spread(this_ms), spread(parent_ms)
            rows[name] = {"this": t, "parent": p, "within_parent_range": bool(p["min"] <= t["median"] <= p["max"]),
                          "at_most_parent_max": bool(t["median"] <= p["max"])}
        out["against_parent_ms"] = rows
        for keep in (this_keep, parent_keep):
            for x in keep:
                x.free()
        for x in pimages + pclouds:
            x.free()
        pctx.close()
    for x in images + clouds:
        x.free()
    ctx.close()

    # ---- (e): the tracking record, in a process of its own
    if track:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pcl_map.py"), "--tsdf-track", str(VOXEL)],
                             capture_output=True, text=True, timeout=600)
        found = re.search(r"mean trajectory error over (\d+) frames: odometry alone ([0-9.e+-]+) m, corrected against the "
                          r"raycast volume ([0-9.e+-]+) m", run.stdout)
        if found:
            out["tsdf_track"] = {"frames": int(found.group(1)), "odometry_alone_m": float(found.group(2)),
                                 "tsdf_track_m": float(found.group(3)),
                                 "recorded_before_m": {"odometry_alone": 0.0271, "render_track_nearest_point_map": 0.0576,
                                                       "render_track_map_of_means": 0.0456}}
        else:
            out["tsdf_track_error"] = (run.stdout + run.stderr)[-600:]
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
