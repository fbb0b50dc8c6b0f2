"""The persistent voxel map (a3d_voxel_map_*, DeviceVoxelMap) against what it replaces, in one job.  Prints one JSON line
(and writes it to argv[1] if given: profiles/voxel_map_probe.json).

(a) per frame, online: one sample1 frame (with normals, under its odometry pose) into a map at v = 0.02 that was built
    the way a live caller builds it, one insert per frame of the sequence (so its table has the size the reservation
    rule gives such a caller), against the same step without the map: merge([map cloud, frame], [eye, pose]) +
    voxel_downsample of the result.  Both as raw calls into preallocated buffers, timed between two device events on the
    context's stream over a window of back-to-back host-synchronous calls (so a figure includes the call's upload and
    its wait), and both through the Python wrappers by the host clock (allocations included: what a caller pays).
(b) extract of that map against a device-to-device copy of its output bytes, timed BEFORE the insert windows: every
    offered point lengthens extract's bitmap, and the map must be the sequence's, not the timing loop's.
(c) 64 single-frame clouds in one insert_many into a cleared map (clear + insert + extract) against merge +
    voxel_downsample of the same clouds.
(d) the two forms of pass B (re-probe / slot stored by pass A) on the diagnostics build, where both exist.
Windows of the variants alternate; the median and the extremes over the windows are kept."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceVoxelMap, Transform, _abi  # noqa: E402
from voxel_downsample_probe import odometry_poses, sample1_clouds, spread, window_ms  # noqa: E402

WINDOWS = 5
VOXEL = 0.02


def measure(ctx, variants, calls, warmup=3):
    """variants: [(name, fn)] -> {name: spread of device ms per call}; `calls` per window, the windows alternate."""
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ms[name].append(window_ms(ctx, fn, calls))
    return {name: dict(spread(v), calls_per_window=calls) for name, v in ms.items()}


def host_ms(fn, repeats=20, warmup=3):
    out = []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def raw_insert(ctx, m, clouds, poses):
    n = len(clouds)
    views = DevicePointCloud._views(clouds)
    poses_c = (_abi.PoseC * n)(*[t.to_c() for t in poses])
    dropped = (C.c_uint64 * n)()

    def call():
        st = ctx.lib.a3d_voxel_map_insert(m.handle, views, poses_c, n, dropped, None)
        assert st == 0, st
    return call


def raw_merge_downsample(ctx, clouds, poses):
    """merge + voxel_downsample as raw calls into preallocated buffers."""
    n, total = len(clouds), sum(c.len() for c in clouds)
    views = DevicePointCloud._views(clouds)
    poses_c = (_abi.PoseC * n)(*[t.to_c() for t in poses])
    merged, out = DevicePointCloud._allocate(ctx, total, True), DevicePointCloud._allocate(ctx, total, True)
    n_out, lens = C.c_uint64(), (C.c_uint64 * 1)()
    out_p, out_n, caps = (C.c_void_p * 1)(out.d_points), (C.c_void_p * 1)(out.d_normals), (C.c_uint64 * 1)(total)

    def call():
        st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, views, poses_c, n, merged.d_points, merged.d_normals, total,
                                                   C.byref(n_out))
        assert st == 0, st
        view = merged.view()
        st = ctx.lib.a3d_point_clouds_voxel_downsample_device(ctx.handle, C.byref(view), 1, VOXEL, None, out_p, out_n, None,
                                                              caps, lens, None)
        assert st == 0, st
    return call, lens, (merged, out)


def online_map(ctx, clouds, poses):
    """The map of the sequence as a live caller builds it: one insert per frame."""
    m = DeviceVoxelMap(ctx, VOXEL)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    return m


def per_frame(ctx, clouds, poses):
    """(b), then (a): the map of every frame, then the last frame once more."""
    res = {}
    m = online_map(ctx, clouds, poses)
    map_cloud = m.extract()
    frame, pose = clouds[-1], poses[-1]
    cells = m.cells()
    res["map_cells"], res["frame_points"], res["map_slots"] = cells, frame.len(), m.stats()["slots"]
    # (b) extract against a device-to-device copy of its output (24 B per cell: points and normals)
    out = DevicePointCloud._allocate(ctx, cells, True)
    src = ctx.malloc(cells * 24)
    dst = ctx.malloc(cells * 24)
    n_out = C.c_uint64()

    def extract():
        st = ctx.lib.a3d_voxel_map_extract(m.handle, out.d_points, out.d_normals, None, cells, C.byref(n_out))
        assert st == 0, st

    def copy():
        _abi.check(ctx.lib.a3d_memcpy_d2d(ctx.handle, dst, src, cells * 24))
        ctx.synchronize()
    ex = measure(ctx, [("voxel_map_extract", extract), ("memcpy_d2d_output_bytes", copy)], calls=100)
    ex["total_offered"] = m.total()
    ex["times_the_copy"] = round(ex["voxel_map_extract"]["median"] / ex["memcpy_d2d_output_bytes"]["median"], 2)
    res["extract"] = ex
    ctx.free(src), ctx.free(dst)
    # (a)
    insert = raw_insert(ctx, m, [frame], [pose])
    baseline, lens, buffers = raw_merge_downsample(ctx, [map_cloud, frame], [Transform.eye(), pose])
    res["device_ms"] = measure(ctx, [("voxel_map_insert", insert), ("merge_then_voxel_downsample", baseline)], calls=100)
    assert int(lens[0]) == m.cells() == cells  # the same step: the frame was in the map already
    res["baseline_over_insert"] = round(res["device_ms"]["merge_then_voxel_downsample"]["median"] /
                                        res["device_ms"]["voxel_map_insert"]["median"], 2)

    def python_baseline():
        merged = DevicePointCloud.merge([map_cloud, frame], [Transform.eye(), pose])
        thin = merged.voxel_downsample(VOXEL)
        merged.free(), thin.free()
    res["host_clock_ms"] = {"DeviceVoxelMap.insert": host_ms(lambda: m.insert(frame, pose)),
                            "merge + voxel_downsample": host_ms(python_baseline)}
    res["map_slots_after"], res["growths"] = m.stats()["slots"], m.stats()["growths"]
    for x in (out, map_cloud, m, *buffers):
        x.free()
    return res


def batch64(ctx, frame, pose):
    """(c): 64 clouds of one frame's size in one call."""
    batch = [frame] + [DevicePointCloud.merge([frame]) for _ in range(63)]
    poses = [pose] * 64
    m = DeviceVoxelMap(ctx, VOXEL, reserve_cells=64 * frame.len())
    insert = raw_insert(ctx, m, batch, poses)
    cells_room = frame.len()
    out = DevicePointCloud._allocate(ctx, cells_room, True)
    n_out = C.c_uint64()

    def online():
        m.clear()
        insert()
        st = ctx.lib.a3d_voxel_map_extract(m.handle, out.d_points, out.d_normals, None, cells_room, C.byref(n_out))
        assert st == 0, st
    baseline, lens, buffers = raw_merge_downsample(ctx, batch, poses)
    res = {"device_ms": measure(ctx, [("clear_insert_many_extract", online), ("merge_then_voxel_downsample", baseline)],
                                calls=4, warmup=2)}
    assert int(lens[0]) == int(n_out.value)
    res.update(clouds=64, points=64 * frame.len(), cells=int(n_out.value), map_slots=m.stats()["slots"])
    res["baseline_over_online"] = round(res["device_ms"]["merge_then_voxel_downsample"]["median"] /
                                        res["device_ms"]["clear_insert_many_extract"]["median"], 2)
    for x in (out, m, *buffers, *batch[1:]):
        x.free()
    return res


def pass_b_forms(clouds_host, poses):
    """(d): the same per-frame insert on the diagnostics build, pass B re-probing against pass B reading stored slots."""
    ctx = Context(0, library=_abi.DIAG_LIB_PATH)
    clouds = [DevicePointCloud(ctx, c) for c in clouds_host]
    m = online_map(ctx, clouds, poses)
    insert = raw_insert(ctx, m, [clouds[-1]], [poses[-1]])

    def with_knob(value):
        def call():
            os.environ["A3D_VOXEL_MAP_STORED_SLOT"] = value
            insert()
        return call
    res = measure(ctx, [("pass_b_re_probe", with_knob("0")), ("pass_b_stored_slot", with_knob("1"))], calls=100)
    os.environ.pop("A3D_VOXEL_MAP_STORED_SLOT", None)
    m.free()
    for c in clouds:
        c.free()
    ctx.close()
    return res


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    out = {"probe": "voxel_map", "windows": WINDOWS, "voxel": VOXEL, "frames": len(clouds),
           "points": sum(c.len() for c in clouds)}
    out["per_frame"] = per_frame(ctx, clouds, poses)
    out["batch64"] = batch64(ctx, clouds[-1], poses[-1])
    from align3d_amd import PointCloud  # noqa: E402

    hosts = [PointCloud(*c.download()) for c in clouds]
    for c in clouds:
        c.free()
    ctx.close()
    out["pass_b_forms_diag_build"] = pass_b_forms(hosts, poses)
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
