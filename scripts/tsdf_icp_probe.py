"""Point-to-SDF ICP against the TSDF volume (DeviceTsdfVolume.align / sample, a3d_tsdf_volume_icp_align_device /
a3d_tsdf_volume_sample_device) beside what it replaces, in one job.
    python scripts/tsdf_icp_probe.py [profiles/tsdf_icp_probe.json] [--parent-library PATH] [--no-track]
Prints one JSON line (and writes it to the path given).  Shapes: the sample1 sequence (640 x 480) under its odometry poses,
fused into a 256^3 volume at v = 0.02 (truncation 4 v, with colours); the frame is the last frame's cloud in its own
coordinates, the pose its odometry pose, the parameters IcpParams.default().
(a) align of that frame cloud against the volume, from the pose: a raw, host-synchronous library call;
(b) the route it replaces for the same frame and pose, as examples/pcl_map.py --tsdf-track runs it: raycast at 640 x 480 +
    pyramid(3) + MultiscaleAlign.new + align of the frame's pyramid + the frees;
(c) DeviceVoxelMap.align of the same frame against the nearest-point map of the sequence at the same voxel size, and
    Icp.align of the frame moved by its pose on a kept tree over that map's extract: with (a), the device time of the
    iteration launches (last_device_ms) per iteration;
(d) sample of the frame's points beside a device-to-device copy of its output bytes (16 per point), and how many points
    have a value and a direction;
(e) with --parent-library (libalign3d_hip.so of the parent commit): integrate of one frame and raycast at 640 x 480 on this
    build and on the parent's, in alternating windows (and alternating order); `within_parent_range` says whether this
    build's median lies inside the parent's own min-max range;
(f) unless --no-track: examples/pcl_map.py --tsdf-track 0.02 without and with --tsdf-direct on sample1, each in a child
    process, their trajectory-error lines.
Every timed span lies between two device events on the context's stream around host-synchronous calls, averaged over a
window of calls; the windows of the variants of a group alternate; median and extremes over the windows are kept."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import (Context, DevicePointCloud, DeviceTsdfVolume, DeviceVoxelMap, Icp, IcpParams, MsIcpParams,  # noqa: E402
                         MultiscaleAlign, RangeImageBuilder, SlamTbDataset, _abi)
from voxel_downsample_probe import odometry_poses, spread  # noqa: E402

WINDOWS = 5
CALLS = 10
WARMUP = 3
VOXEL = 0.02
DIMS = (256, 256, 256)
ORIGIN = (-2.56, -2.56, 0.0)
Z_NEAR = 0.3
Z_FAR = ORIGIN[2] + DIMS[2] * VOXEL
NEW_SYMBOLS = ("a3d_tsdf_volume_sample_device", "a3d_tsdf_volume_icp_align_device", "a3d_tsdf_volume_icp_accumulate_device",
               "a3d_tsdf_volume_icp_last_device_ms")


def measure(ctx, variants, calls=CALLS):
    """{name: spread of the per-call ms over the windows}, and per variant the median of what its call returns."""
    for _, fn in variants:
        for _ in range(WARMUP):
            fn()
    ms = {name: [] for name, _ in variants}
    inner = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ctx.timer_start()
            for _ in range(calls):
                r = fn()
                if r is not None:
                    inner[name].append(r)
            ms[name].append(ctx.timer_stop() / calls)
    return ({name: dict(spread(v), calls_per_window=calls) for name, v in ms.items()},
            {name: round(statistics.median(v), 4) for name, v in inner.items() if v})


def load_frames(ctx, levels):
    """(camera, the frames' pyramids with colours) of the sample1 sequence."""
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    return cam, RangeImageBuilder(ctx).pyramid_levels(levels).build_many(cam, [(f[1], f[2]) for f in frames], depth_scale)


def parent_context(path):
    """A context on a library that predates this pull request's entries: loaded without asking for them."""
    held = {name: _abi.SIGNATURES.pop(name) for name in NEW_SYMBOLS}
    try:
        _abi.load_library(path)
    finally:
        _abi.SIGNATURES.update(held)
    return Context(0, library=path)


def volume_calls(ctx, cam, images, poses):
    """(e): integrate of one frame and a raycast, as raw calls, on a volume of this context that holds the sequence."""
    lib = ctx.lib
    vol = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN, colors=True)
    vol.integrate_many(images, poses)
    one, w2c, c2w = (C.c_void_p * 1)(images[-1].handle), poses[-1].inverse().to_c(), poses[-1].to_c()
    handle = C.c_void_p()

    def integrate():
        assert lib.a3d_tsdf_volume_integrate(vol.handle, one, C.byref(w2c), 1) == 0

    def raycast():
        st = lib.a3d_tsdf_volume_raycast(vol.handle, C.byref(c2w), cam.fx, cam.fy, cam.cx, cam.cy, 640, 480, Z_NEAR, Z_FAR,
                                         2 * VOXEL, C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    return [("integrate_1_frame_colours", integrate), ("raycast_640x480", raycast)], vol


def track_line(extra):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pcl_map.py"), "--tsdf-track", str(VOXEL)] + extra,
                         capture_output=True, text=True, timeout=600)
    found = re.search(r"mean trajectory error over (\d+) frames: odometry alone ([0-9.e+-]+) m, corrected against the "
                      r"(raycast volume|volume's field) ([0-9.e+-]+) m", run.stdout)
    if not found:
        return {"error": (run.stdout + run.stderr)[-600:]}
    return {"frames": int(found.group(1)), "odometry_alone_m": float(found.group(2)), "route": found.group(3),
            "corrected_m": float(found.group(4))}


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
    cam, built = load_frames(ctx, 3)
    assert (cam.width, cam.height) == (640, 480)
    images = [p[0] for p in built]
    clouds = DevicePointCloud.from_range_images(images, colors=True)
    poses = odometry_poses(ctx, clouds)
    frame, pose = clouds[-1], poses[-1]
    prm = IcpParams.default()
    iterations = int(prm.max_iterations)
    volume = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN, colors=True)
    volume.integrate_many(images, poses)
    out = {"probe": "tsdf_icp", "windows": WINDOWS, "voxel": VOXEL, "dims": DIMS, "origin": ORIGIN, "frames": len(images),
           "frame_points": frame.len(), "iterations": iterations, "one_job_on_one_box": True}
    print(f"[probe] volume fused, frame of {frame.len()} points", file=sys.stderr, flush=True)

    # ---- (a), (b), (c)
    prm_c, pose_c, frame_view = prm.to_c(), pose.to_c(), frame.view()
    out_pose, device_ms = _abi.PoseC(), C.c_float()

    def volume_align():
        st = lib.a3d_tsdf_volume_icp_align_device(volume.handle, C.byref(prm_c), C.byref(frame_view), C.byref(pose_c),
                                                  C.byref(out_pose))
        assert st == 0, st
        assert lib.a3d_tsdf_volume_icp_last_device_ms(volume.handle, C.byref(device_ms)) == 0
        return device_ms.value

    ms_prm = MsIcpParams.default()

    def raycast_route():
        model = volume.raycast(cam, pose, Z_NEAR, Z_FAR).pyramid(3)
        aligner = MultiscaleAlign.new(ctx, ms_prm, model)
        aligner.align(built[-1])
        aligner.free()
        for level in model:
            level.free()

    vmap = DeviceVoxelMap(ctx, VOXEL)
    for c, t in zip(clouds, poses):
        vmap.insert(c, t)

    def map_align():
        st = lib.a3d_voxel_map_icp_align_device(vmap.handle, C.byref(prm_c), C.byref(frame_view), C.byref(pose_c),
                                                C.byref(out_pose))
        assert st == 0, st
        assert lib.a3d_voxel_map_icp_last_device_ms(vmap.handle, C.byref(device_ms)) == 0
        return device_ms.value

    kept_world, kept_moved = vmap.extract(), pose * frame
    kept = Icp(ctx, prm, kept_world)

    def tree_align():
        kept.align(kept_moved)
        return kept.last_device_ms()

    per_frame, device = measure(ctx, [("volume_align", volume_align), ("raycast_pyramid_multiscale_align", raycast_route),
                                      ("voxel_map_align", map_align), ("icp_align_on_a_kept_tree", tree_align)])
    out["per_frame_ms"] = per_frame
    out["iteration_launches_device_ms"] = device
    out["per_iteration_device_us"] = {k: round(1e3 * v / iterations, 2) for k, v in device.items()}
    a, b = per_frame["volume_align"]["median"], per_frame["raycast_pyramid_multiscale_align"]["median"]
    out["raycast_route_over_volume_align"] = round(b / a, 2)
    out["map_cells"] = vmap.cells()
    via_volume = volume.align(frame, prm, initial=pose) * pose.inverse()
    via_map = vmap.align(frame, prm, initial=pose) * pose.inverse()
    via_tree = kept.align(kept_moved)
    out["correction"] = {name: {"angle": float(t.angle()), "translation": float(np.linalg.norm(t.t))}
                         for name, t in (("volume_align", via_volume), ("voxel_map_align", via_map),
                                         ("icp_on_extract", via_tree))}
    state = volume.accumulate(frame, prm, pose)
    out["points_accumulated_at_the_pose"] = int(state["count"])
    print("[probe] align routes measured", file=sys.stderr, flush=True)
    kept.free(), kept_world.free(), kept_moved.free(), vmap.free()

    # ---- (d): the field query beside a copy of its output bytes
    n = frame.len()
    d_dist, d_nrm = ctx.malloc(n * 4), ctx.malloc(n * 12)
    src, dst = ctx.malloc(n * 16), ctx.malloc(n * 16)

    def sample():
        st = lib.a3d_tsdf_volume_sample_device(volume.handle, frame.d_points, n, C.byref(pose_c), d_dist, d_nrm)
        assert st == 0, st

    def copy():
        _abi.check(lib.a3d_memcpy_d2d(ctx.handle, dst, src, n * 16), "a3d_memcpy_d2d")
        ctx.synchronize()  # (the entry under test is host-synchronous: the copy is timed the same way)

    ms, _ = measure(ctx, [("sample_frame_points", sample), ("copy_output_bytes_16_per_point", copy)], calls=20)
    out["sample_ms"] = ms
    out["sample_over_copy"] = round(ms["sample_frame_points"]["median"] / ms["copy_output_bytes_16_per_point"]["median"], 2)
    sample()
    dist, nrm = ctx.to_host(d_dist, np.empty(n, np.float32)), ctx.to_host(d_nrm, np.empty((n, 3), np.float32))
    out["sample_points_with_a_value"] = int((~np.isnan(dist)).sum())
    out["sample_points_with_a_direction"] = int(np.any(nrm != 0, axis=1).sum())
    for p in (d_dist, d_nrm, src, dst):
        ctx.free(p)
    volume.free()
    print("[probe] sample measured", file=sys.stderr, flush=True)

    # ---- (e): integrate and raycast on both builds
    if parent_path:
        pctx = parent_context(parent_path)
        _, pbuilt = load_frames(pctx, 1)
        pimages = [p[0] for p in pbuilt]
        this_calls, this_vol = volume_calls(ctx, cam, images, poses)
        parent_calls, parent_vol = volume_calls(pctx, cam, pimages, poses)
        for _, fn in this_calls + parent_calls:
            for _ in range(WARMUP):
                fn()
        rows = {}
        for (name, fn), (_, pfn) in zip(this_calls, parent_calls):
            this_ms, parent_ms = [], []
            for window in range(WINDOWS + 2):
                sides = ((pctx, pfn, parent_ms), (ctx, fn, this_ms))
                for side_ctx, side_fn, acc in (sides if window % 2 == 0 else sides[::-1]):  # (neither build always goes second)
                    side_ctx.timer_start()
                    for _ in range(CALLS):
                        side_fn()
                    acc.append(side_ctx.timer_stop() / CALLS)
            t, p = spread(this_ms), spread(parent_ms)
            rows[name] = {"this": t, "parent": p, "within_parent_range": bool(p["min"] <= t["median"] <= p["max"]),
                          "at_most_parent_max": bool(t["median"] <= p["max"])}
        out["against_parent_ms"] = rows
        this_vol.free(), parent_vol.free()
        for x in pimages:
            x.free()
        pctx.close()
        print("[probe] parent comparison measured", file=sys.stderr, flush=True)
    for x in [level for p in built for level in p] + clouds:
        x.free()
    ctx.close()

    # ---- (f): the tracking record, each route in a process of its own
    if track:
        out["tsdf_track"] = {"raycast_route": track_line([]), "direct_route": track_line(["--tsdf-direct"]),
                             "recorded_before_m": {"odometry_alone": 0.0271, "render_track_nearest_point_map": 0.0576,
                                                   "render_track_map_of_means": 0.0456, "tsdf_track_raycast": 0.0136}}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
