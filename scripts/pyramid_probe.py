"""RangeImage::pyramid on the device (a3d_range_image_pyramids: 3 levels, normals, colours, intensity on every level) for 1
and 64 resident 640x480 images, against the host round trip it replaces (download level 0, the oracle's pyr_down twice
on the CPU, upload_pyramid), and the frame builder's own pyramid stages.  Prints one JSON line (and writes it to argv[1]
if given).

Device times are hipEvent brackets on the context's stream around one host-synchronous call (they include the call's
table upload; the coarser levels' arenas come from the context's pool after the warm-up).  Bytes are the algorithmic
traffic counted from the shapes (pyramid_bytes).  The builder's pyramid stages are the difference between its kernel
time for 3-level and 1-level pyramids of the same 64 frames (a3d_context_set_build_profiling)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from align3d_amd import Context, RangeImage, RangeImageBuilder, SlamTbDataset, pyramids  # noqa: E402
from align3d_amd.range_image import CameraIntrinsics, upload_pyramid  # noqa: E402

HBM_BYTES_PER_S = 8e12


def med(xs):
    return round(statistics.median(xs), 4)


def pyramid_bytes(w, h, levels=3):
    """Bytes one image's pyramid moves: level 0 read once (points 12, mask 1, normals 12, colours 3) plus its colours
    again for the luma, its intensities (1) and map (4) written; every coarser level written (28 + 5) and its colours
    read back for the luma and (but the last) for the next blur."""
    n = [(w >> l) * (h >> l) for l in range(levels)]
    total = n[0] * (28 + 3 + 5)
    for l in range(1, levels):
        total += n[l] * (28 + 5 + 3 + (3 if l < levels - 1 else 0))
    return total


def device_time(ctx, images, reps):
    out = pyramids(images, 3)  # warm-up: code objects, tap tables, pooled arenas
    for p in out:
        for lv in p[1:]:
            lv.free()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.timer_start()
        out = pyramids(images, 3)
        ms.append(ctx.timer_stop())
        wall.append((time.perf_counter() - t0) * 1e3)
        for p in out:
            for lv in p[1:]:
                lv.free()
    return med(ms), med(wall)


def host_round_trip(ctx, lv):
    t0 = time.perf_counter()
    host = lv.download()
    t1 = time.perf_counter()
    k = host.intrinsics
    pyr = [O.Frame(host.points, host.mask, k.fx, k.fy, k.cx, k.cy, host.normals, host.intensities, host.intensity_map,
                   colors=host.colors)]
    for _ in range(2):
        pyr.append(O.pyr_down(pyr[-1], 1.0))
    t2 = time.perf_counter()
    levels = [RangeImage(f.points, f.mask, CameraIntrinsics(f.fx, f.fy, f.cx, f.cy, f.w, f.h), normals=f.normals,
                         intensities=f.intensities, intensity_map=f.intensity_map) for f in pyr[1:]]
    devs = upload_pyramid(ctx, levels)
    t3 = time.perf_counter()
    for d in devs:
        d.free()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3


def builder_kernel_ms(ctx, builder, cam, frames, depth_scale, levels):
    b = builder.pyramid_levels(levels)
    for _ in range(2):
        for p in b.build_many(cam, frames, depth_scale):
            for lv in p:
                lv.free()
    ms = []
    for _ in range(5):
        out = b.build_many(cam, frames, depth_scale)
        v = C.c_float()
        ctx.lib.a3d_context_last_build_kernel_ms(ctx.handle, C.byref(v))
        ms.append(v.value)
        for p in out:
            for lv in p:
                lv.free()
    return med(ms)


def main():
    ctx = Context(0)
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    builder = RangeImageBuilder(ctx).pyramid_levels(1)
    picks = [(frames[i % len(frames)][1], frames[i % len(frames)][2]) for i in range(64)]
    level0 = [p[0] for p in builder.build_many(cam, picks, depth_scale)]
    per_image = pyramid_bytes(640, 480)
    out = {"probe": "pyramid", "shape": [480, 640], "levels": 3, "bytes_per_image": per_image}
    for n, reps in ((1, 50), (64, 20)):
        ms, wall = device_time(ctx, level0[:n], reps)
        out[f"batch{n}"] = {"device_ms": ms, "call_wall_ms": wall, "device_us_per_image": round(ms * 1e3 / n, 2),
                            "fraction_of_8TBs": round(per_image * n / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}
    rt = [host_round_trip(ctx, level0[0]) for _ in range(5)]
    out["host_round_trip_ms"] = {"download": med([r[0] for r in rt]), "oracle_pyr_down_cpu": med([r[1] for r in rt]),
                                 "upload_pyramid": med([r[2] for r in rt]), "total": med([r[3] for r in rt])}
    ctx.lib.a3d_context_set_build_profiling(ctx.handle, 1)
    k1 = builder_kernel_ms(ctx, builder, cam, picks, depth_scale, 1)
    k3 = builder_kernel_ms(ctx, builder, cam, picks, depth_scale, 3)
    ctx.lib.a3d_context_set_build_profiling(ctx.handle, 0)
    out["builder_64"] = {"kernel_ms_1_level": k1, "kernel_ms_3_levels": k3,
                         "pyramid_stages_us_per_frame": round((k3 - k1) * 1e3 / 64, 2)}
    for lv in level0:
        lv.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
