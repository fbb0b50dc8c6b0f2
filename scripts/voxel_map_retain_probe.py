"""DeviceVoxelMap.retain (a3d_voxel_map_retain) against what reaches the same state without it, in one job.  Prints one
JSON line (and writes it to argv[1] if given: profiles/voxel_map_retain_probe.json).

The map is the sample1 sequence at v = 0.02, built the way a live caller builds it (one insert per frame, the frame
boundaries recorded as total()).
(a) extract of that long-lived map (a table sized by the reservation rule for a whole frame on top of the cells, a bitmap
    of every point ever offered) before and after one compaction.
(b) retain in three forms — a compaction, a one-sided box that keeps about half of the cells, a min_seq that keeps the
    cells of the last W frames — beside the three calls that compact a map without it: extract into preallocated buffers,
    clear, insert of the extracted rows.  Every timed call starts from the same state, the compacted map (cells = total),
    which an untimed clear + insert of its rows restores before it; each call is timed between two device events of its
    own on the context's stream (a call is host-synchronous, so the span holds its uploads and its wait), averaged over a
    window of calls.  The windows of the variants alternate; the median and the extremes over the windows are kept."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceVoxelMap  # noqa: E402
from voxel_downsample_probe import odometry_poses, sample1_clouds, spread  # noqa: E402

WINDOWS = 5
CALLS = 20
VOXEL = 0.02
LAST_FRAMES = 5
INF = float("inf")


def window_ms(ctx, fn, before=None, calls=CALLS):
    ms = 0.0
    for _ in range(calls):
        if before:
            before()
        ctx.timer_start()
        fn()
        ms += ctx.timer_stop()
    return ms / calls


def measure(ctx, variants, before=None):
    for _, fn in variants:
        for _ in range(3):
            if before:
                before()
            fn()
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ms[name].append(window_ms(ctx, fn, before))
    return {name: dict(spread(v), calls_per_window=CALLS) for name, v in ms.items()}


def raw_retain(ctx, m, box=None, min_seq=0):
    lo = hi = None
    if box is not None:
        lo, hi = (C.c_float * 3)(*box[0]), (C.c_float * 3)(*box[1])
    removed = C.c_uint64()

    def call():
        st = ctx.lib.a3d_voxel_map_retain(m.handle, lo, hi, min_seq, None, 0, None, C.byref(removed))
        assert st == 0, st
    return call, removed


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    m = DeviceVoxelMap(ctx, VOXEL)
    starts = []
    for c, t in zip(clouds, poses):
        starts.append(m.total())
        m.insert(c, t)
    cells = m.cells()
    out = {"probe": "voxel_map_retain", "windows": WINDOWS, "voxel": VOXEL, "frames": len(clouds), "map_cells": cells}
    buf = DevicePointCloud._allocate(ctx, cells, True)
    n_out = C.c_uint64()

    def extract():
        st = ctx.lib.a3d_voxel_map_extract(m.handle, buf.d_points, buf.d_normals, None, cells, C.byref(n_out))
        assert st == 0, st
    # (a)
    before = dict(measure(ctx, [("voxel_map_extract", extract)])["voxel_map_extract"], slots=m.stats()["slots"], total=m.total())
    removed, marks = m.retain(marks=np.asarray(starts, np.uint64))
    assert removed == 0 and m.cells() == m.total() == cells
    after = dict(measure(ctx, [("voxel_map_extract", extract)])["voxel_map_extract"], slots=m.stats()["slots"], total=m.total())
    out["extract_of_the_long_lived_map"] = {"before_compaction": before, "after_compaction": after,
                                            "before_over_after": round(before["median"] / after["median"], 2)}
    # (b)
    rows = m.extract()
    x_median = float(np.median(rows.download()[0][:, 0]))
    half_box = ((-INF, -INF, -INF), (x_median, INF, INF))
    last = int(marks[-LAST_FRAMES])

    def restore():
        m.clear()
        m.insert(rows)
    restore()
    assert m.cells() == m.total() == cells
    compaction, removed_c = raw_retain(ctx, m)
    box_half, removed_b = raw_retain(ctx, m, box=half_box)
    last_frames, removed_f = raw_retain(ctx, m, min_seq=last)
    view = (type(buf.view()) * 1)(buf.view())
    dropped = (C.c_uint64 * 1)()

    def three_calls():
        extract()
        m.clear()
        st = ctx.lib.a3d_voxel_map_insert(m.handle, view, None, 1, dropped, None)
        assert st == 0 and m.cells() == cells, st
    out["device_ms"] = measure(ctx, [("retain_compaction", compaction), ("retain_box_keeping_half", box_half),
                                     (f"retain_min_seq_last_{LAST_FRAMES}_frames", last_frames),
                                     ("extract_clear_insert", three_calls)], before=restore)
    out["state_before_each_call"] = dict(cells=cells, total=cells, slots=m.stats()["slots"])
    out["removed"] = {"retain_compaction": int(removed_c.value), "retain_box_keeping_half": int(removed_b.value),
                      f"retain_min_seq_last_{LAST_FRAMES}_frames": int(removed_f.value)}
    out["three_calls_over_compaction"] = round(out["device_ms"]["extract_clear_insert"]["median"] /
                                               out["device_ms"]["retain_compaction"]["median"], 2)
    for x in (rows, buf, m, *clouds):
        x.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
