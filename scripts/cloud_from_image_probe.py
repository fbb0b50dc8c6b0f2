"""PointCloud::from(&RangeImage) on the device (a3d_range_image_to_point_clouds) against the host round trip it replaces
(download, numpy compaction, upload), and the benches/bench_icp.rs pipeline (builder -> clouds -> Icp::new + align) both
ways with the pose bits compared.  Prints one JSON line (and writes it to argv[1] if given).

Device times are hipEvent brackets on the context's stream around one host-synchronous call (they include the call's
small job-table upload and length read-back); bytes are the kernels' algorithmic traffic: mask read twice (count pass and
rank pass) plus the 12-byte point and 12-byte normal of every pixel (26 B/px), or on builder level 0 the mask, the 2-byte
depth plane and the normal (15 B/px), plus 24 B written per kept point."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from align3d_amd import Context, DevicePointCloud, Icp, IcpParams, PointCloud, RangeImageBuilder, SlamTbDataset  # noqa: E402
from align3d_amd.range_image import DeviceRangeImage  # noqa: E402

HBM_BYTES_PER_S = 8e12


def med(xs):
    return round(statistics.median(xs), 4)


def convert(ctx, images, outs, caps, lens):
    n = len(images)
    st = ctx.lib.a3d_range_image_to_point_clouds((C.c_void_p * n)(*[im.handle for im in images]), n,
                                                 (C.c_void_p * n)(*[o[0] for o in outs]),
                                                 (C.c_void_p * n)(*[o[1] for o in outs]), caps, lens)
    assert st == 0, st


def device_time(ctx, images, reps):
    n = len(images)
    outs = [(ctx.malloc(im.shape[0] * im.shape[1] * 12), ctx.malloc(im.shape[0] * im.shape[1] * 12)) for im in images]
    caps = (C.c_uint64 * n)(*[im.shape[0] * im.shape[1] for im in images])
    lens = (C.c_uint64 * n)()
    convert(ctx, images, outs, caps, lens)  # warm-up
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.timer_start()
        convert(ctx, images, outs, caps, lens)
        ms.append(ctx.timer_stop())
        wall.append((time.perf_counter() - t0) * 1e3)
    for p, q in outs:
        ctx.free(p), ctx.free(q)
    return med(ms), med(wall), [int(x) for x in lens]


def host_round_trip(ctx, lv):
    t0 = time.perf_counter()
    host = lv.download(intensity=False)
    t1 = time.perf_counter()
    pc = PointCloud.from_range_image(host)
    t2 = time.perf_counter()
    dc = DevicePointCloud(ctx, pc)
    ctx.synchronize()
    t3 = time.perf_counter()
    dc.free()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3


def main():
    ctx = Context(0)
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    builder = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False)
    out = {"probe": "cloud_from_image", "shape": [480, 640]}

    # one frame: builder level 0 (depth-plane path) and the same image uploaded (plain path)
    lv = builder.build(cam, frames[0][1], frames[0][2], depth_scale)[0]
    up = DeviceRangeImage(ctx, lv.download(intensity=False))
    ms_d, wall_d, lens = device_time(ctx, [lv], 50)
    ms_p, wall_p, _ = device_time(ctx, [up], 50)
    out["one_frame"] = {"points": lens[0], "device_ms_depth16": ms_d, "device_ms_plain": ms_p,
                        "call_wall_ms_depth16": wall_d, "call_wall_ms_plain": wall_p}
    rt = [host_round_trip(ctx, lv) for _ in range(10)]
    out["one_frame"]["host_round_trip_ms"] = {"download": med([r[0] for r in rt]), "numpy_compaction": med([r[1] for r in rt]),
                                              "upload": med([r[2] for r in rt]), "total": med([r[3] for r in rt])}
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dc = DevicePointCloud.from_range_image(lv)
        t.append((time.perf_counter() - t0) * 1e3)
        dc.free()
    out["one_frame"]["from_range_image_wall_ms_incl_alloc"] = med(t)

    # a 64-frame batch, both paths
    picks = [frames[i % len(frames)] for i in range(64)]
    built = [p[0] for p in builder.build_many(cam, [(f[1], f[2]) for f in picks], depth_scale)]
    uploaded = [DeviceRangeImage(ctx, b.download(intensity=False)) for b in built]
    px = 64 * 480 * 640
    for name, imgs, rd in (("batch64_depth16", built, 15), ("batch64_plain", uploaded, 26)):
        ms, wall, lens = device_time(ctx, imgs, 20)
        nbytes = rd * px + 24 * sum(lens)
        out[name] = {"device_ms": ms, "call_wall_ms": wall, "points": sum(lens), "bytes": nbytes,
                     "fraction_of_8TBs": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}
    rt = [host_round_trip(ctx, b) for b in built[:16]]
    out["batch64_host_round_trip_ms_per_frame"] = med([r[3] for r in rt])
    for b in built + uploaded:
        b.free()

    # benches/bench_icp.rs: frames 0 (target) and 5 (source), builder -> clouds -> Icp::new + align, both ways
    prm = IcpParams(max_iterations=10)

    def host_way(levels):
        ht, hs = (PointCloud.from_range_image(x.download(intensity=False)) for x in levels)
        dt, dsrc = DevicePointCloud(ctx, ht), DevicePointCloud(ctx, hs)
        icp = Icp.new(ctx, prm, dt)
        T = icp.align(dsrc)
        icp.free(), dt.free(), dsrc.free()
        return T

    def device_way(levels):
        dt, dsrc = DevicePointCloud.from_range_images(levels)
        icp = Icp.new(ctx, prm, dt)
        T = icp.align(dsrc)
        icp.free(), dt.free(), dsrc.free()
        return T

    levels = [builder.build(cam, frames[i][1], frames[i][2], depth_scale)[0] for i in (0, 5)]
    res = {}
    for name, fn in (("host_round_trip", host_way), ("device", device_way)):
        fn(levels)
        t = []
        for _ in range(9):
            t0 = time.perf_counter()
            T = fn(levels)
            t.append((time.perf_counter() - t0) * 1e3)
        res[name] = (med(t), T.to_c())
    bits = [np.asarray(list(p.t) + list(p.q), np.float32).view(np.uint32).tolist() for _, p in res.values()]
    out["bench_icp_shape"] = {"clouds_new_align_wall_ms_host_round_trip": res["host_round_trip"][0],
                              "clouds_new_align_wall_ms_device": res["device"][0],
                              "pose_bits_identical": bits[0] == bits[1]}
    for x in levels + [lv, up]:
        x.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
