"""Transform * PointCloud on resident clouds (a3d_point_clouds_transform_device / a3d_point_clouds_merge_device) against
the two things it is judged by: the host round trip a caller needs without it (download, the oracle's one-thread loop,
upload) and a device-to-device copy of the same bytes in the same run.  Prints one JSON line (and writes it to argv[1] if
given).  `--trace` runs only a short series of calls on the 64-cloud shape, for
`rocprofv3 --kernel-trace --stats -- python scripts/cloud_transform_probe.py --trace`.

Shapes: P = 1, 8, 64 clouds of the sample1 frame-0 size (270 213 points, with normals) and one cloud of 500 000 points.
A figure is the time of a window of back-to-back host-synchronous calls between two device events on the context's
stream, divided by the calls in it (so it includes each call's job-table upload and synchronise, which is what a caller
pays); windows of the variants alternate in the same run, and the median and the extremes over the windows are kept.
Bytes are the kernel's algorithmic traffic, 48 B per point with normals (24 read, 24 written): the bound is HBM
bandwidth.  The points-per-thread variants (A3D_CLOUD_TRANSFORM_PPT = 1, 2, 4) exist in the diagnostics build only; the
product library is timed beside them."""
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
import oracle_lib as O  # noqa: E402
from align3d_amd import (Context, DevicePointCloud, PointCloud, RangeImageBuilder, SlamTbDataset, Transform,  # noqa: E402
                         _abi)

HBM_BYTES_PER_S = 8e12
WINDOWS = 5
WINDOW_S = 0.25  # a window is sized to about this long from a first estimate


def spread(xs):
    return {"median": round(statistics.median(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}


def poses_for(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = rng.normal(size=4).astype(np.float32)
        out.append(Transform(rng.uniform(-1, 1, size=3), q / np.float32(np.linalg.norm(q))))
    return out


class Case:
    """P clouds on one context with preallocated outputs: the raw calls, so that no allocation is timed."""

    def __init__(self, ctx, clouds):
        self.ctx, self.clouds, self.n = ctx, clouds, len(clouds)
        self.points = sum(c.len() for c in clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        self.poses = (_abi.PoseC * self.n)(*[t.to_c() for t in poses_for(self.n)])
        self.outs = [DevicePointCloud._allocate(ctx, c.len(), True) for c in clouds]
        self.out_p = (C.c_void_p * self.n)(*[o.d_points for o in self.outs])
        self.out_n = (C.c_void_p * self.n)(*[o.d_normals for o in self.outs])
        self.merged = DevicePointCloud._allocate(ctx, self.points, True)
        self.len = C.c_uint64()
        # the copy of the same bytes: 24 B per point read and 24 B written, as two plain buffers
        self.copy_src, self.copy_dst = ctx.malloc(self.points * 24), ctx.malloc(self.points * 24)

    def transform_many(self):
        st = self.ctx.lib.a3d_point_clouds_transform_device(self.ctx.handle, self.views, self.poses, self.n, self.out_p,
                                                            self.out_n)
        assert st == 0, st

    def merge(self):
        st = self.ctx.lib.a3d_point_clouds_merge_device(self.ctx.handle, self.views, self.poses, self.n, self.merged.d_points,
                                                        self.merged.d_normals, self.points, C.byref(self.len))
        assert st == 0, st

    def copy(self):
        _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, self.copy_dst, self.copy_src, self.points * 24))
        self.ctx.synchronize()  # (the entries under test are host-synchronous: the copy is timed the same way)

    def free(self):
        for o in self.outs + [self.merged]:
            o.free()
        self.ctx.free(self.copy_src), self.ctx.free(self.copy_dst)


def window_ms(ctx, fn, calls):
    ctx.timer_start()
    for _ in range(calls):
        fn()
    return ctx.timer_stop() / calls


def measure(variants):
    """variants: [(name, ctx, fn, setup)] -> {name: spread of ms per call}; the windows of the variants alternate."""
    calls = {}
    for name, ctx, fn, setup in variants:
        setup()
        for _ in range(3):
            fn()  # warm-up of this shape
        calls[name] = max(10, int(WINDOW_S * 1e3 / max(window_ms(ctx, fn, 10), 1e-3)))
    ms = {name: [] for name, *_ in variants}
    for _ in range(WINDOWS):
        for name, ctx, fn, setup in variants:
            setup()
            ms[name].append(window_ms(ctx, fn, calls[name]))
    return {name: dict(spread(v), calls_per_window=calls[name]) for name, v in ms.items()}


def set_ppt(v):
    def setup():
        if v is None:
            os.environ.pop("A3D_CLOUD_TRANSFORM_PPT", None)
        else:
            os.environ["A3D_CLOUD_TRANSFORM_PPT"] = str(v)
    return setup


def rates(entry, points):
    nbytes = 48 * points
    entry["algorithmic_bytes"] = nbytes
    entry["GBps"] = round(nbytes / (entry["median"] * 1e-3) / 1e9, 1)
    entry["fraction_of_8TBs"] = round(nbytes / (entry["median"] * 1e-3) / HBM_BYTES_PER_S, 3)
    return entry


def host_round_trip(ctx, cloud, pose):
    """What a caller does without the entries: download, the oracle's loop on one thread, upload; ms, by the host clock,
    ending in a device synchronise."""
    t0 = time.perf_counter()
    pts, nrm = cloud.download()
    t1 = time.perf_counter()
    out_p = O.transform_points(pose, pts)
    out_n = np.empty_like(nrm)
    O.load().orc_transform_normals(C.byref(pose), _abi.ptr(nrm), nrm.size // 3, _abi.ptr(out_n))
    t2 = time.perf_counter()
    dc = DevicePointCloud(ctx, PointCloud(out_p, out_n))
    ctx.synchronize()
    t3 = time.perf_counter()
    dc.free()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3


def frame0_cloud(ctx):
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    cam, depth, rgb, depth_scale = ds.get(0)
    lv = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build(cam, depth, rgb, depth_scale)[0]
    dc = DevicePointCloud.from_range_image(lv)
    lv.free()
    return dc


def synthetic_cloud(ctx, n, seed=9):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return DevicePointCloud(ctx, PointCloud(rng.uniform(-2, 2, size=(n, 3)).astype(np.float32), nrm))


def main():
    trace = "--trace" in sys.argv[1:]
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    product, diag = Context(0), Context(0, library=_abi.DIAG_LIB_PATH, pair=False)
    out = {"probe": "cloud_transform", "bytes_per_point": 48, "bound": "HBM bandwidth", "windows": WINDOWS}
    shapes = [("P1_270213", 1, None), ("P8_270213", 8, None), ("P64_270213", 64, None), ("P1_500000", 1, 500000)]
    if trace:  # one shape, so that a kernel's statistics are not an average over shapes
        shapes = shapes[2:3]
    for name, p, synthetic in shapes:
        per_ctx = {}
        for ctx in (product, diag):
            first = synthetic_cloud(ctx, synthetic) if synthetic else frame0_cloud(ctx)
            per_ctx[ctx] = [first] + [DevicePointCloud.merge([first]) for _ in range(p - 1)]  # resident copies
        cp, cd = Case(product, per_ctx[product]), Case(diag, per_ctx[diag])
        if trace:  # a short series per variant for the kernel trace: the kernel names carry the variant
            for _ in range(20):
                cp.transform_many(), cp.merge()
            for v in (1, 2, 4):
                set_ppt(v)()
                for _ in range(20):
                    cd.transform_many(), cd.merge()
            set_ppt(None)()
        else:
            none = set_ppt(None)
            res = measure([("transform_many", product, cp.transform_many, none), ("merge", product, cp.merge, none),
                           ("memcpy_d2d_same_bytes", product, cp.copy, none)]
                          + [(f"diag_transform_many_ppt{v}", diag, cd.transform_many, set_ppt(v)) for v in (1, 2, 4)]
                          + [(f"diag_merge_ppt{v}", diag, cd.merge, set_ppt(v)) for v in (1, 2, 4)])
            set_ppt(None)()
            res = {k: rates(v, cp.points) for k, v in res.items()}
            copy_rate = res["memcpy_d2d_same_bytes"]["GBps"]
            for k, v in res.items():
                v["share_of_copy_rate"] = round(v["GBps"] / copy_rate, 3)
            res["clouds"], res["points"] = p, cp.points
            if p == 1:
                res["note"] = "one cloud: launch- and synchronise-bound, not a bandwidth figure"
            out[name] = res
        cp.free(), cd.free()
        for clouds in per_ctx.values():
            for c in clouds:
                c.free()
    if not trace:
        first = frame0_cloud(product)
        pose = poses_for(1)[0].to_c()
        host_round_trip(product, first, pose)
        rt = [host_round_trip(product, first, pose) for _ in range(8)]
        out["host_round_trip_ms_per_270213_point_cloud"] = {
            "download": spread([r[0] for r in rt]), "oracle_loop_one_thread": spread([r[1] for r in rt]),
            "upload": spread([r[2] for r in rt]), "total": spread([r[3] for r in rt])}
        # the Python call a user makes, allocation of the result included
        t = []
        T = poses_for(1)[0]
        for _ in range(10):
            t0 = time.perf_counter()
            moved = T * first
            t.append((time.perf_counter() - t0) * 1e3)
            moved.free()
        out["transform_times_cloud_wall_ms_incl_alloc"] = spread(t)
        first.free()
    product.close(), diag.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
