"""Voxel-grid downsampling by cell mean (a3d_point_clouds_voxel_mean_device) beside the two things it is judged by, in the
same job and on the same inputs: the nearest-point downsample (a3d_point_clouds_voxel_downsample_device) and a
device-to-device copy of the input's bytes.  Prints one JSON line (and writes it to argv[1] if given:
profiles/voxel_mean_probe.json).  The protocol is that of scripts/voxel_downsample_probe.py: a figure is the time of a
window of back-to-back host-synchronous calls between two device events on the context's stream, divided by the calls in
it; the windows of the variants alternate, and the median and the extremes over the windows are kept.

Shapes: the merged map of every frame of tests/golden/rgbd/sample1 under its IcpBatch odometry pose at v = 0.02, one
frame cloud, 64 frame clouds in one call, and 270 213 uniform points that all fall in one cell (v = 1e3).  Clouds carry
points and normals (24 bytes per point, which is what the copy moves).  The host round trip a caller would make without
the entry (download, the numpy restatement, upload) is timed by the host clock.  `scratch_bytes` is the call's part of
the context's scratch region, by the layout of voxel_mean.hip and of voxel_downsample.hip.  The last entry holds the
figures of examples/pcl_map.py --voxel 0.02 --mean on sample1 for both maps: there is no gate on them."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import voxel_mean_restatement as M  # noqa: E402
from align3d_amd import Context, DevicePointCloud, Icp, IcpParams, PointCloud, _abi  # noqa: E402
from voxel_downsample_probe import WINDOWS, measure, odometry_poses, sample1_clouds  # noqa: E402


def pad256(x):
    return (x + 255) // 256 * 256


def scratch_bytes(lens):
    """(mean, nearest): bytes of scratch region 3 one call takes for clouds of these lengths."""
    mean = nearest = 0
    tiles = 0
    for n in lens:
        slots = 2
        while slots < 2 * n:
            slots <<= 1
        groups = (n + 63) // 64
        chunks = (n + 1023) // 1024
        per = (chunks + 4095) // 4096
        tiles += (chunks + per - 1) // per
        nearest += pad256(groups * 8) + slots * 16
        mean += pad256(groups * 8) + slots * 16 + pad256(4 * n) + pad256(16 * n) + pad256(96 * groups)
    k = len(lens)
    return (mean + pad256(136 * k) + pad256(8 * (3 * k + 1)) + pad256(4 * tiles),
            nearest + pad256(104 * k) + pad256(8 * (2 * k + 1)) + pad256(4 * tiles))


class Case:
    """Clouds on one context with preallocated outputs: the raw calls, so that no allocation is timed."""

    def __init__(self, ctx, clouds):
        self.ctx, self.clouds, self.n = ctx, clouds, len(clouds)
        self.points = sum(c.len() for c in clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        self.outs = [DevicePointCloud._allocate(ctx, c.len(), True) for c in clouds]
        self.out_p = (C.c_void_p * self.n)(*[o.d_points for o in self.outs])
        self.out_n = (C.c_void_p * self.n)(*[o.d_normals for o in self.outs])
        self.caps = (C.c_uint64 * self.n)(*[c.len() for c in clouds])
        self.lens, self.dropped = (C.c_uint64 * self.n)(), (C.c_uint64 * self.n)()
        self.copy_src, self.copy_dst = ctx.malloc(self.points * 24), ctx.malloc(self.points * 24)

    def mean(self, voxel):
        st = self.ctx.lib.a3d_point_clouds_voxel_mean_device(self.ctx.handle, self.views, None, self.n, voxel, None, self.out_p,
                                                             self.out_n, None, None, None, self.caps, self.lens, self.dropped)
        assert st == 0, st

    def nearest(self, voxel):
        st = self.ctx.lib.a3d_point_clouds_voxel_downsample_device(self.ctx.handle, self.views, self.n, voxel, None, self.out_p,
                                                                   self.out_n, None, self.caps, self.lens, self.dropped)
        assert st == 0, st

    def copy(self):
        _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, self.copy_dst, self.copy_src, self.points * 24))
        self.ctx.synchronize()  # (the entries under test are host-synchronous: the copy is timed the same way)

    def free(self):
        for o in self.outs:
            o.free()
        self.ctx.free(self.copy_src), self.ctx.free(self.copy_dst)


def host_round_trip(ctx, cloud, voxel):
    t0 = time.perf_counter()
    pts, nrm = cloud.download()
    t1 = time.perf_counter()
    out_p, out_n, _, _, _, _ = M.voxel_mean(pts, nrm, None, voxel)
    t2 = time.perf_counter()
    dc = DevicePointCloud(ctx, PointCloud(out_p, out_n))
    ctx.synchronize()
    t3 = time.perf_counter()
    dc.free()
    return {"download": round((t1 - t0) * 1e3, 2), "numpy_restatement": round((t2 - t1) * 1e3, 2),
            "upload": round((t3 - t2) * 1e3, 2), "total": round((t3 - t0) * 1e3, 2)}


def run_case(ctx, clouds, voxel, round_trip_of=None):
    case = Case(ctx, clouds)
    res = measure(ctx, [("voxel_mean", lambda: case.mean(voxel)), ("voxel_nearest", lambda: case.nearest(voxel)),
                        ("memcpy_d2d_input_bytes", case.copy)])
    case.mean(voxel)
    res["clouds"], res["points"], res["voxel"] = case.n, case.points, voxel
    res["rows_first_cloud"], res["dropped_first_cloud"] = int(case.lens[0]), int(case.dropped[0])
    res["mean_over_nearest"] = round(res["voxel_mean"]["median"] / res["voxel_nearest"]["median"], 2)
    res["mean_over_copy"] = round(res["voxel_mean"]["median"] / res["memcpy_d2d_input_bytes"]["median"], 2)
    mean_b, near_b = scratch_bytes([c.len() for c in clouds])
    res["scratch_bytes"] = {"voxel_mean": mean_b, "voxel_nearest": near_b,
                            "growth_bytes_per_point": round((mean_b - near_b) / max(1, case.points), 2)}
    if round_trip_of is not None:
        rt = host_round_trip(ctx, round_trip_of, voxel)
        res["host_round_trip_ms"] = rt
        res["mean_slower_than_host_round_trip"] = bool(res["voxel_mean"]["median"] > rt["total"])
    case.free()
    return res


def example_figures(ctx, clouds, poses, world_map, voxel):
    """What examples/pcl_map.py --voxel V --mean prints, for both maps."""
    out = {"voxel": voxel, "offered": world_map.len()}
    last = poses[-1] * clouds[-1]
    near = world_map.voxel_downsample(voxel)
    mean = world_map.voxel_downsample(voxel, mode="mean")
    for name, target in (("nearest", near), ("mean", mean)):
        icp = Icp(ctx, IcpParams.default(), target)
        correction = icp.align(last)
        icp.free()
        out[name] = {"points": target.len(), "correction_angle_rad": float(correction.angle()),
                     "correction_translation": float(np.linalg.norm(correction.t))}
    for x in (last, near, mean):
        x.free()
    return out


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    out = {"probe": "voxel_mean", "windows": WINDOWS, "copy_bytes_per_point": 24,
           "designs_built": "(b) counting sort by cell + run reduction; (a) per-row atomic sums was not built"}
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    world_map = DevicePointCloud.merge(clouds, poses)
    out["map_v0.02"] = dict(run_case(ctx, [world_map], 0.02, world_map), frames=len(clouds))
    out["one_frame_v0.02"] = run_case(ctx, [clouds[0]], 0.02, clouds[0])
    batch = [clouds[0]] + [DevicePointCloud.merge([clouds[0]]) for _ in range(63)]
    res = run_case(ctx, batch, 0.02)
    res["host_round_trip_ms_64_clouds"] = round(64 * out["one_frame_v0.02"]["host_round_trip_ms"]["total"], 1)
    res["mean_slower_than_host_round_trip"] = bool(res["voxel_mean"]["median"] > res["host_round_trip_ms_64_clouds"])
    out["batch64_v0.02"] = res
    for c in batch[1:]:
        c.free()
    rng = np.random.default_rng(1)
    cube = rng.uniform(0.25, 3.25, size=(270213, 3)).astype(np.float32)
    one_cell = DevicePointCloud(ctx, PointCloud(cube, rng.normal(size=cube.shape).astype(np.float32)))
    out["one_cell_270k_v1000"] = run_case(ctx, [one_cell], 1e3, one_cell)
    one_cell.free()
    out["pcl_map_mean_sample1"] = example_figures(ctx, clouds, poses, world_map, 0.02)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
