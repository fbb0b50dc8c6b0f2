"""Frame-to-map ICP against the live voxel map (DeviceVoxelMap.align, a3d_voxel_map_icp_align_device) beside what it
replaces, in one job.  Prints one JSON line (and writes it to argv[1] if given: profiles/voxel_map_icp_probe.json).

The map is the sample1 sequence at v = 0.02, built the way a live caller builds it (one insert per frame under its
odometry pose); the frame is the last frame's cloud in its own coordinates; 15 iterations.
(a) per frame: a3d_voxel_map_icp_align_device(frame, initial = pose)  against what it replaces, the frame moved by its
    pose + extract + Icp.new + align + free of the Icp, in two forms: on the raw ABI into PREALLOCATED outputs
    (a3d_point_clouds_transform_device, a3d_voxel_map_extract, a3d_pcl_icp_new_device / _align_device / _free: a caller
    that reuses its buffers; the tree's memory comes from the context's block pool), which is the figure the comparison
    rests on, and through the Python wrappers (pose * frame, extract(), Icp(...), align, and the free() of all three:
    four hipMalloc and four hipFree per frame, each a device-wide synchronisation, all inside the span), which is what
    examples/pcl_map.py paid.  Also align alone on a tree that is kept (a map that did not change; the frame already
    moved).  Each variant is timed between two device events of its own on the context's stream (every call is
    host-synchronous, so the span holds its uploads and its waits), averaged over a window of calls; the windows of the
    variants alternate; the median and the extremes over the windows are kept.
    The map's align is also timed on the same map after a compaction (2 * cells slots: a caller that retains per frame),
    whose table is a sixteenth of the one the last insert reserved.
(b) per iteration: the device time of the iteration launches of each, from last_device_ms, over the same calls.
(c) the association alone: DeviceVoxelMap nearest for the frame's points against a3d_kdtree_nearest_device on the
    extracted map (resident queries and results on both sides).
The two ICPs do not associate alike (27 cells against one kd-tree leaf), so their poses differ; both are reported."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceVoxelMap, Icp, IcpParams, _abi  # noqa: E402
from voxel_downsample_probe import odometry_poses, sample1_clouds, spread  # noqa: E402

WINDOWS = 5
CALLS = 10
WARMUP = 3
VOXEL = 0.02
ITERATIONS = 15


def measure(ctx, variants):
    """{name: spread of the per-call ms over the windows}, and per variant the values its call returns (device ms)."""
    for _, fn in variants:
        for _ in range(WARMUP):
            fn()
    ms = {name: [] for name, _ in variants}
    inner = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            total = 0.0
            for _ in range(CALLS):
                ctx.timer_start()
                r = fn()
                total += ctx.timer_stop()
                if r is not None:
                    inner[name].append(r)
            ms[name].append(total / CALLS)
    return ({name: dict(spread(v), calls_per_window=CALLS) for name, v in ms.items()},
            {name: round(statistics.median(v), 4) for name, v in inner.items() if v})


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    m = DeviceVoxelMap(ctx, VOXEL)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    frame, pose = clouds[-1], poses[-1]
    prm = IcpParams(max_iterations=ITERATIONS)
    out = {"probe": "voxel_map_icp", "windows": WINDOWS, "voxel": VOXEL, "frames": len(clouds), "map_cells": m.cells(),
           "map_slots": m.stats()["slots"], "points_offered": m.total(), "frame_points": frame.len(), "iterations": ITERATIONS}

    lib = ctx.lib
    prm_c, pose_c, frame_view = prm.to_c(), pose.to_c(), frame.view()
    out_pose, device_ms = _abi.PoseC(), C.c_float()

    def raw_map_align(handle):
        st = lib.a3d_voxel_map_icp_align_device(handle, C.byref(prm_c), C.byref(frame_view), C.byref(pose_c), C.byref(out_pose))
        assert st == 0, st
        assert lib.a3d_voxel_map_icp_last_device_ms(handle, C.byref(device_ms)) == 0
        return device_ms.value

    def map_align():
        return raw_map_align(m.handle)

    # the replaced path on the raw ABI: every output preallocated once, outside the spans
    cells = m.cells()
    moved_buf = DevicePointCloud._allocate(ctx, frame.len(), True)
    world_buf = DevicePointCloud._allocate(ctx, cells, True)
    frame_views, poses_c = (_abi.PointCloudViewC * 1)(frame_view), (_abi.PoseC * 1)(pose_c)
    moved_points, moved_normals = (C.c_void_p * 1)(moved_buf.d_points), (C.c_void_p * 1)(moved_buf.d_normals)
    moved_view = moved_buf.view()
    n_world = C.c_uint64()

    def raw_extract_build_align():
        st = lib.a3d_point_clouds_transform_device(ctx.handle, frame_views, poses_c, 1, moved_points, moved_normals)
        assert st == 0, st
        st = lib.a3d_voxel_map_extract(m.handle, world_buf.d_points, world_buf.d_normals, None, cells, C.byref(n_world))
        assert st == 0 and n_world.value == cells, st
        world_view = world_buf.view()
        icp = C.c_void_p()
        st = lib.a3d_pcl_icp_new_device(ctx.handle, C.byref(prm_c), C.byref(world_view), C.byref(icp))
        assert st == 0, st
        st = lib.a3d_pcl_icp_align_device(icp, C.byref(moved_view), C.byref(out_pose))
        assert st == 0, st
        assert lib.a3d_pcl_icp_last_device_ms(icp, C.byref(device_ms)) == 0
        ms = device_ms.value
        lib.a3d_pcl_icp_free(icp)  # (its blocks go back to the context's pool: the next frame's tree takes them)
        return ms

    def wrappers_extract_build_align():
        moved = pose * frame
        world = m.extract()
        icp = Icp(ctx, prm, world)
        icp.align(moved)
        ms = icp.last_device_ms()
        icp.free(), world.free(), moved.free()  # (counted: see the docstring)
        return ms

    # the same map after a compaction (a caller that retains per frame): 2 * cells slots instead of the 2 * (cells + frame)
    # that the last insert reserved
    small = DeviceVoxelMap(ctx, VOXEL)
    for c, t in zip(clouds, poses):
        small.insert(c, t)
    small.compact()
    out["compacted_map_slots"] = small.stats()["slots"]

    def compacted_map_align():
        return raw_map_align(small.handle)

    kept_world, kept_moved = m.extract(), pose * frame
    kept = Icp(ctx, prm, kept_world)

    def tree_reused_align():
        kept.align(kept_moved)
        return kept.last_device_ms()

    per_frame, device = measure(ctx, [("map_align", map_align), ("raw_transform_extract_icp_new_align", raw_extract_build_align),
                                      ("wrappers_transform_extract_icp_new_align", wrappers_extract_build_align),
                                      ("align_on_a_kept_tree", tree_reused_align),
                                      ("map_align_after_compaction", compacted_map_align)])
    out["per_frame_ms"] = per_frame
    out["iteration_launches_device_ms"] = device
    out["per_iteration_device_us"] = {k: round(1e3 * v / ITERATIONS, 2) for k, v in device.items()}
    a, b, w, c = (per_frame[k]["median"] for k in ("map_align", "raw_transform_extract_icp_new_align",
                                                   "wrappers_transform_extract_icp_new_align", "align_on_a_kept_tree"))
    out["raw_replaced_path_over_map_align"] = round(b / a, 2)
    out["wrappers_replaced_path_over_map_align"] = round(w / a, 2)
    out["kept_tree_over_map_align"] = round(c / a, 2)
    # what surrounds the iterations, per frame, and the iteration count at which the raw replaced path and the map's align
    # cost the same (below it the map wins; None: the map's iteration is not the slower one)
    it_map, it_tree = device["map_align"] / ITERATIONS, device["raw_transform_extract_icp_new_align"] / ITERATIONS
    fixed_map, fixed_raw = a - device["map_align"], b - device["raw_transform_extract_icp_new_align"]
    out["fixed_cost_ms"] = {"map_align": round(fixed_map, 4), "raw_transform_extract_icp_new_align": round(fixed_raw, 4),
                            "wrappers_transform_extract_icp_new_align":
                                round(w - device["wrappers_transform_extract_icp_new_align"], 4)}
    out["break_even_iterations_against_raw"] = (None if it_map <= it_tree
                                                else round((fixed_raw - fixed_map) / (it_map - it_tree), 1))
    # the poses: the correction each path asks of the odometry pose
    via_map = m.align(frame, prm, initial=pose) * pose.inverse()
    via_tree = kept.align(kept_moved)
    out["correction"] = {"map_align": {"angle": float(via_map.angle()), "translation": float(np.linalg.norm(via_map.t))},
                         "icp_on_extract": {"angle": float(via_tree.angle()), "translation": float(np.linalg.norm(via_tree.t))}}
    # (c) the association alone, resident on both sides
    n = kept_moved.len()
    d_idx, d_d2 = ctx.malloc(n * 4), ctx.malloc(n * 4)
    tree = C.c_void_p()
    _abi.check(ctx.lib.a3d_kdtree_new_device(ctx.handle, kept_world.d_points, kept_world.len(), C.byref(tree)))

    def map_nearest():
        st = ctx.lib.a3d_voxel_map_nearest_device(m.handle, kept_moved.d_points, n, None, d_idx, d_d2)
        assert st == 0, st

    def compacted_map_nearest():
        st = ctx.lib.a3d_voxel_map_nearest_device(small.handle, kept_moved.d_points, n, None, d_idx, d_d2)
        assert st == 0, st

    def tree_nearest():
        st = ctx.lib.a3d_kdtree_nearest_device(tree, kept_moved.d_points, n, d_idx, d_d2)
        assert st == 0, st
        ctx.synchronize()  # (enqueue-only: the map's call waits by itself)

    out["nearest_ms"], _ = measure(ctx, [("voxel_map_nearest", map_nearest), ("kdtree_nearest_on_extract", tree_nearest),
                                         ("voxel_map_nearest_after_compaction", compacted_map_nearest)])
    out["nearest_queries"] = n
    map_nearest()
    found = ctx.to_host(d_idx, np.empty(n, np.uint32))
    out["nearest_queries_with_a_row_in_reach"] = int((found != 0xFFFFFFFF).sum())
    ctx.lib.a3d_kdtree_free(tree)
    ctx.free(d_idx), ctx.free(d_d2)
    kept.free()
    for x in (kept_world, kept_moved, moved_buf, world_buf, m, small, *clouds):
        x.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
