"""Normals of resident clouds from their own neighbourhoods (a3d_point_clouds_estimate_normals_device) against the things
it is judged by: a device-to-device copy of the output's bytes in the same run (the project's yardstick) and
compute_normals on the range image of the same frame (what a cloud WITH a pixel grid pays).  Prints one JSON line (and
writes it to argv[1] if given: profiles/cloud_normals_probe.json).

Shapes, all from tests/golden/rgbd/sample1: (a) one frame's cloud at r = 0.01; (b) the same frame thinned at v = 0.02, at
r = 0.06; (c) the extract of the v = 0.02 voxel map of every frame under its odometry pose, at r = 0.06, oriented by the
normals it has; (d) 64 frame clouds in one call at r = 0.01.  For (a) also the median angle between estimated and image
normals (quality, not a gate) and the estimate kernel's product form (threads in cell order, four candidates loaded per
trip, no LDS) against the forms the diagnostics build keeps (A3D_NORMALS_ORDER=input, A3D_NORMALS_AHEAD=1,
A3D_NORMALS_LDS=1: LDS staging on), all timed on the diagnostics build in alternating windows.

A figure is the time of a window of back-to-back host-synchronous calls between two device events on the context's stream,
divided by the calls in it (so it includes each call's table upload, the fill of the hash tables and the synchronise,
which is what a caller pays); the windows of the variants alternate, and the median and the extremes over the windows are
kept."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from align3d_amd import (Context, DevicePointCloud, DeviceVoxelMap, IcpBatch, IcpParams, RangeImageBuilder,  # noqa: E402
                         SlamTbDataset, Transform, TrajectoryBuilder, _abi)

WINDOWS = 5
WINDOW_S = 0.25  # a window is sized to about this long from a first estimate


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


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


def sample1(ctx):
    """(frame clouds, frame images kept for compute_normals, camera-to-world odometry poses)."""
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(cam, [(f[1], f[2]) for f in frames],
                                                                                      depth_scale)
    images = [pyramid[0] for pyramid in built]
    clouds = DevicePointCloud.from_range_images(images)
    batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
    poses, status = batch.align(clouds[1:])
    batch.free()
    traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
    out = [traj.current_camera_to_world()]
    for k, (now_to_previous, st) in enumerate(zip(poses, status)):
        if st == 0:
            traj.accumulate(now_to_previous, float(k + 1))
        out.append(traj.current_camera_to_world())
    return clouds, images, out


class Case:
    """P clouds on one context with preallocated outputs: the raw call, so that no allocation is timed."""

    def __init__(self, ctx, clouds, orient=0):
        self.ctx, self.n, self.orient = ctx, len(clouds), orient
        self.points = sum(c.len() for c in clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        self.outs = [ctx.malloc(max(1, c.len()) * 12) for c in clouds]
        self.out_n = (C.c_void_p * self.n)(*self.outs)
        self.valid, self.dropped = (C.c_uint64 * self.n)(), (C.c_uint64 * self.n)()
        # the copy of the output's bytes: 12 B per point
        self.copy_src, self.copy_dst = ctx.malloc(self.points * 12), ctx.malloc(self.points * 12)

    def estimate(self, radius):
        st = self.ctx.lib.a3d_point_clouds_estimate_normals_device(self.ctx.handle, self.views, self.n, radius, 3, None,
                                                                   self.orient, self.out_n, None, None, self.valid,
                                                                   self.dropped)
        assert st == 0, st

    def copy(self):
        _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, self.copy_dst, self.copy_src, self.points * 12))
        self.ctx.synchronize()  # (the entry under test is host-synchronous: the copy is timed the same way)

    def normals(self, k=0, n=None):
        return self.ctx.to_host(self.outs[k], np.empty((n, 3), np.float32))

    def free(self):
        for o in self.outs + [self.copy_src, self.copy_dst]:
            self.ctx.free(o)


def run_case(ctx, clouds, radius, image=None, orient=0):
    case = Case(ctx, clouds, orient)
    variants = [("estimate_normals", lambda: case.estimate(radius)), ("memcpy_d2d_output_bytes", case.copy)]
    if image is not None:
        def image_normals():
            image.compute_normals()
            ctx.synchronize()
        variants.append(("compute_normals_on_the_range_image", image_normals))
    res = measure(ctx, variants)
    res.update(clouds=len(clouds), points=case.points, radius=radius, valid=int(sum(case.valid)), dropped=int(sum(case.dropped)))
    res["times_the_copy"] = round(res["estimate_normals"]["median"] / res["memcpy_d2d_output_bytes"]["median"], 2)
    if image is not None:
        res["times_compute_normals"] = round(res["estimate_normals"]["median"]
                                             / res["compute_normals_on_the_range_image"]["median"], 2)
    return res, case


def median_angle_deg(estimated, reference):
    ok = (np.linalg.norm(estimated, axis=1) > 0.5) & (np.linalg.norm(reference, axis=1) > 0.5)
    cos = np.clip((estimated[ok] * reference[ok]).sum(axis=1), -1.0, 1.0)
    return round(float(np.degrees(np.median(np.arccos(cos)))), 3), int(ok.sum())


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    out = {"probe": "cloud_normals", "windows": WINDOWS, "copy_bytes_per_point": 12, "min_neighbors": 3}
    clouds, images, poses = sample1(ctx)
    frame, image = clouds[0], images[0]
    # (a) one frame's cloud
    res, case = run_case(ctx, [frame], 0.01, image)
    angle, rows = median_angle_deg(case.normals(0, frame.len()), frame.download()[1])
    res["median_angle_to_image_normals_deg"], res["rows_compared"] = angle, rows
    case.free()
    out["a_frame_r0.01"] = res
    # (b) the same frame thinned
    thin = frame.voxel_downsample(0.02)
    res, case = run_case(ctx, [thin], 0.06, image)
    angle, rows = median_angle_deg(case.normals(0, thin.len()), thin.download()[1])
    res["median_angle_to_image_normals_deg"], res["rows_compared"] = angle, rows
    case.free()
    out["b_frame_thinned_v0.02_r0.06"] = res
    # (c) the map's extract, oriented by the normals it has
    vmap = DeviceVoxelMap(ctx, 0.02, normals=True)
    vmap.insert_many(clouds, poses)
    extract = vmap.extract()
    res, case = run_case(ctx, [extract], 0.06, image, orient=1)
    angle, rows = median_angle_deg(case.normals(0, extract.len()), extract.download()[1])
    res["median_angle_to_the_cells_sensor_normals_deg"], res["rows_compared"] = angle, rows
    case.free()
    out["c_map_extract_v0.02_r0.06"] = res
    # (d) 64 frame clouds in one call
    batch = [frame] + [DevicePointCloud.merge([frame]) for _ in range(63)]
    res, case = run_case(ctx, batch, 0.01, image)
    case.free()
    out["d_64_frames_r0.01"] = res
    for c in batch[1:] + [thin, extract]:
        c.free()
    vmap.free()
    pts, _ = frame.download()
    ctx.close()
    # (a) again on the diagnostics build: the estimate kernel in cell order against input order
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    from align3d_amd import PointCloud  # noqa: E402

    dframe = DevicePointCloud(diag, PointCloud(pts))
    case = Case(diag, [dframe])

    def form(name=None, value=None):
        def fn():
            for knob in ("A3D_NORMALS_ORDER", "A3D_NORMALS_AHEAD", "A3D_NORMALS_LDS"):
                os.environ.pop(knob, None)
            if name:
                os.environ[name] = value
            case.estimate(0.01)
        return fn
    res = measure(diag, [("product_form", form()), ("input_order", form("A3D_NORMALS_ORDER", "input")),
                         ("one_candidate_per_trip", form("A3D_NORMALS_AHEAD", "1")),
                         ("lds_staging", form("A3D_NORMALS_LDS", "1"))])
    form()()
    res["input_order_over_product_form"] = round(res["input_order"]["median"] / res["product_form"]["median"], 3)
    res["one_candidate_per_trip_over_product_form"] = round(res["one_candidate_per_trip"]["median"]
                                                            / res["product_form"]["median"], 3)
    res["lds_staging_over_product_form"] = round(res["lds_staging"]["median"] / res["product_form"]["median"], 3)
    res["note"] = ("whole calls on the diagnostics build, count / place / scatter included in all; the candidates are read from "
                   "the cell-ordered copy in all; product form: threads in cell order, four candidates loaded per trip, no LDS; lds_staging: a wave loads the "
                   "runs its lanes share into LDS, 64 records per coalesced load, and the lanes read them back")
    out["a_frame_r0.01_estimate_kernel_forms"] = res
    case.free(), dframe.free()
    diag.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
