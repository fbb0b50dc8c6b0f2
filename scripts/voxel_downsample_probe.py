"""Voxel-grid downsampling of resident clouds (a3d_point_clouds_voxel_downsample_device) against the things it is judged
by: a device-to-device copy of the input bytes in the same run (the floor), the host round trip it replaces (download, the
numpy restatement of tests/voxel_restatement.py, upload), and what a thinned map buys Icp.new + align.  Prints one JSON
line (and writes it to argv[1] if given: profiles/voxel_downsample_probe.json).  `--trace N` runs only five calls on N
single-frame clouds, for `rocprofv3 --kernel-trace --stats -- python scripts/voxel_downsample_probe.py --trace N`: the
launches of one call at N = 1 and at N = 64 must be equal in number.

Shapes: the merged map of every frame of tests/golden/rgbd/sample1 under its IcpBatch odometry pose (examples/pcl_map.py)
at v = 0.01, 0.02 and 0.05, and a batch of 64 single-frame clouds at v = 0.02.  A figure is the time of a window of
back-to-back host-synchronous calls between two device events on the context's stream, divided by the calls in it (so it
includes each call's table upload, the fill of the hash tables and the synchronise, which is what a caller pays); the
windows of the call and of the copy alternate, and the median and the extremes over the windows are kept."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_restatement as V  # noqa: E402
from align3d_amd import (Context, DevicePointCloud, Icp, IcpBatch, IcpParams, PointCloud, RangeImageBuilder,  # noqa: E402
                         SlamTbDataset, Transform, TrajectoryBuilder, _abi)

WINDOWS = 5
WINDOW_S = 0.25  # a window is sized to about this long from a first estimate


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sample1_clouds(ctx, n_frames=None):
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(min(ds.len(), n_frames or ds.len()))]
    cam, _, _, depth_scale = frames[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(cam, [(f[1], f[2]) for f in frames],
                                                                                      depth_scale)
    images = [pyramid[0] for pyramid in built]
    clouds = DevicePointCloud.from_range_images(images)
    for im in images:
        im.free()
    return clouds


def odometry_poses(ctx, clouds):
    batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
    poses, status = batch.align(clouds[1:])
    batch.free()
    traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
    out = [traj.current_camera_to_world()]
    for k, (now_to_previous, st) in enumerate(zip(poses, status)):
        if st == 0:
            traj.accumulate(now_to_previous, float(k + 1))
        out.append(traj.current_camera_to_world())
    return out


class Case:
    """P clouds on one context with preallocated outputs: the raw call, so that no allocation is timed."""

    def __init__(self, ctx, clouds):
        self.ctx, self.clouds, self.n = ctx, clouds, len(clouds)
        self.points = sum(c.len() for c in clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        self.outs = [DevicePointCloud._allocate(ctx, c.len(), True) for c in clouds]
        self.out_p = (C.c_void_p * self.n)(*[o.d_points for o in self.outs])
        self.out_n = (C.c_void_p * self.n)(*[o.d_normals for o in self.outs])
        self.caps = (C.c_uint64 * self.n)(*[c.len() for c in clouds])
        self.lens, self.dropped = (C.c_uint64 * self.n)(), (C.c_uint64 * self.n)()
        # the copy of the input bytes: 24 B per point (points and normals), as two plain buffers
        self.copy_src, self.copy_dst = ctx.malloc(self.points * 24), ctx.malloc(self.points * 24)

    def downsample(self, voxel):
        st = self.ctx.lib.a3d_point_clouds_voxel_downsample_device(self.ctx.handle, self.views, self.n, voxel, None, self.out_p,
                                                                   self.out_n, None, self.caps, self.lens, self.dropped)
        assert st == 0, st

    def copy(self):
        _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, self.copy_dst, self.copy_src, self.points * 24))
        self.ctx.synchronize()  # (the entry under test is host-synchronous: the copy is timed the same way)

    def free(self):
        for o in self.outs:
            o.free()
        self.ctx.free(self.copy_src), self.ctx.free(self.copy_dst)


def window_ms(ctx, fn, calls):
    ctx.timer_start()
    for _ in range(calls):
        fn()
    return ctx.timer_stop() / calls


def measure(ctx, variants):
    """variants: [(name, fn)] -> {name: spread of ms per call}; the windows of the variants alternate."""
    calls = {}
    for name, fn in variants:
        for _ in range(3):
            fn()  # warm-up of this shape (grows the context's scratch region once)
        calls[name] = max(5, int(WINDOW_S * 1e3 / max(window_ms(ctx, fn, 5), 1e-3)))
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ms[name].append(window_ms(ctx, fn, calls[name]))
    return {name: dict(spread(v), calls_per_window=calls[name]) for name, v in ms.items()}


def host_round_trip(ctx, cloud, voxel):
    """What a caller does without the entry: download, the numpy restatement, upload; ms by the host clock, ending in a
    device synchronise."""
    t0 = time.perf_counter()
    pts, nrm = cloud.download()
    t1 = time.perf_counter()
    out_p, out_n, _, _ = V.voxel_downsample_cloud(pts, nrm, voxel)
    t2 = time.perf_counter()
    dc = DevicePointCloud(ctx, PointCloud(out_p, out_n))
    ctx.synchronize()
    t3 = time.perf_counter()
    dc.free()
    return {"download": round((t1 - t0) * 1e3, 2), "numpy_restatement": round((t2 - t1) * 1e3, 2),
            "upload": round((t3 - t2) * 1e3, 2), "total": round((t3 - t0) * 1e3, 2)}


def icp_new_and_align_ms(ctx, target, source, repeats=3):
    """Icp.new (the kd-tree build over the target) + align of one frame, ms by the host clock (both host-synchronous)."""
    out = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        icp = Icp.new(ctx, IcpParams.default(), target)
        t1 = time.perf_counter()
        icp.align(source)
        t2 = time.perf_counter()
        icp.free()
        out.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    out = out[1:]  # (the first builds the context's kd-tree scratch)
    return {"new_ms": spread([a for a, _ in out]), "align_ms": spread([b for _, b in out])}


def main():
    args = sys.argv[1:]
    ctx = Context(0)
    if "--trace" in args:
        n = int(args[args.index("--trace") + 1])
        first = sample1_clouds(ctx, 1)[0]
        clouds = [first] + [DevicePointCloud.merge([first]) for _ in range(n - 1)]
        case = Case(ctx, clouds)
        for _ in range(5):
            case.downsample(0.02)
        print(json.dumps({"trace_clouds": n, "calls": 5, "kept_per_cloud": int(case.lens[0])}))
        ctx.close()
        return
    out_path = next((a for a in args if not a.startswith("--")), None)
    out = {"probe": "voxel_downsample", "windows": WINDOWS, "copy_bytes_per_point": 24}
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    world_map = DevicePointCloud.merge(clouds, poses)
    out["map"] = {"frames": len(clouds), "points": world_map.len()}
    case = Case(ctx, [world_map])
    for voxel in (0.01, 0.02, 0.05):
        res = measure(ctx, [("voxel_downsample", lambda: case.downsample(voxel)), ("memcpy_d2d_input_bytes", case.copy)])
        res["kept"], res["dropped"] = int(case.lens[0]), int(case.dropped[0])
        res["times_the_copy"] = round(res["voxel_downsample"]["median"] / res["memcpy_d2d_input_bytes"]["median"], 2)
        res["host_round_trip_ms"] = host_round_trip(ctx, world_map, voxel)
        out["map"][f"v{voxel}"] = res
    case.free()
    # a batch of 64 single-frame clouds
    batch = [clouds[0]] + [DevicePointCloud.merge([clouds[0]]) for _ in range(63)]
    case = Case(ctx, batch)
    res = measure(ctx, [("voxel_downsample", lambda: case.downsample(0.02)), ("memcpy_d2d_input_bytes", case.copy)])
    res["clouds"], res["points"], res["kept_per_cloud"] = 64, case.points, int(case.lens[0])
    res["times_the_copy"] = round(res["voxel_downsample"]["median"] / res["memcpy_d2d_input_bytes"]["median"], 2)
    rt = host_round_trip(ctx, clouds[0], 0.02)
    res["host_round_trip_ms_one_cloud"] = rt
    res["host_round_trip_ms_64_clouds"] = round(64 * rt["total"], 1)
    out["batch64_v0.02"] = res
    case.free()
    for c in batch[1:]:
        c.free()
    # frame to map: the last frame under its odometry pose against the full map and against the thinned one
    source = poses[-1] * clouds[-1]
    out["icp_last_frame_against_full_map"] = dict(icp_new_and_align_ms(ctx, world_map, source), target_points=world_map.len())
    for voxel in (0.01, 0.02, 0.05):
        thin = world_map.voxel_downsample(voxel)
        out[f"icp_last_frame_against_map_v{voxel}"] = dict(icp_new_and_align_ms(ctx, thin, source), target_points=thin.len())
        thin.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
