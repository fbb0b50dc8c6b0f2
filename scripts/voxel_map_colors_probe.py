"""What colours cost in the persistent voxel map, and what they cost a caller who does not use them, in one job.  Prints
one JSON line (and writes it to argv[1] if given: profiles/voxel_map_colors_probe.json).

The shapes are those of profiles/voxel_map_probe.json: the map of the sample1 sequence at v = 0.02 built the way a live
caller builds it (one insert per frame), and the sequence's last frame.  Three calls are timed as raw calls into
preallocated buffers, each between two device events on the context's stream (a call is host-synchronous, so the span
holds its upload and its wait):
  insert   the last frame once more under its pose;
  extract  the whole map (timed before the insert windows: every offered point lengthens extract's bitmap);
  retain   a pure compaction of the compacted map (an untimed clear + insert of its rows restores the state before each).
Each is timed on a map without colours and on a map with colours, and, with --parent-library PATH (libalign3d_hip.so
built from the commit before colours existed), on that library too, without colours.  A repetition is one window of
back-to-back calls; the windows of the sides alternate, so all sides see the same minutes of the same box.  The median
and the extremes over the windows are kept.  `gate`: whether this build's median WITHOUT colours lies inside the parent's
own min-max range, per call: what an existing caller pays for the feature."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceVoxelMap, RangeImageBuilder, SlamTbDataset, _abi  # noqa: E402
from voxel_downsample_probe import odometry_poses, sample1_clouds, spread  # noqa: E402

WINDOWS = 9
CALLS = {"insert": 50, "extract": 50, "retain": 10}
VOXEL = 0.02
NEW_SYMBOLS = ("a3d_range_image_has_colors", "a3d_range_image_to_point_clouds_rgb", "a3d_point_clouds_merge_rgb_device",
               "a3d_point_clouds_voxel_downsample_rgb_device", "a3d_voxel_map_new_rgb", "a3d_voxel_map_insert_rgb",
               "a3d_voxel_map_extract_rgb")


def parent_context(path):
    """A context on a library that predates the colour entries: loaded without asking for them."""
    held = {name: _abi.SIGNATURES.pop(name) for name in NEW_SYMBOLS}
    try:
        _abi.load_library(path)
    finally:
        _abi.SIGNATURES.update(held)
    return Context(0, library=path)


class Side:
    """One library and one kind of map: its clouds, the sequence's map, and the three timed calls."""

    def __init__(self, name, ctx, clouds, poses, colors):
        self.name, self.ctx, self.colors = name, ctx, colors
        lib = ctx.lib
        m = self.map = DeviceVoxelMap(ctx, VOXEL, colors=True) if colors else DeviceVoxelMap(ctx, VOXEL)
        for c, t in zip(clouds, poses):
            m.insert(c, t)
        self.cells, self.slots = m.cells(), m.stats()["slots"]
        cells = self.cells
        frame, pose = clouds[-1], (_abi.PoseC * 1)(poses[-1].to_c())
        self.frame_points = frame.len()
        view, dropped = (_abi.PointCloudViewC * 1)(frame.view()), (C.c_uint64 * 1)()
        out = self.out = DevicePointCloud._allocate(ctx, cells, True, colors)
        n_out, removed = C.c_uint64(), C.c_uint64()
        if colors:
            frame_colors = (C.c_void_p * 1)(frame.d_colors)

            def insert():
                assert lib.a3d_voxel_map_insert_rgb(m.handle, view, frame_colors, pose, 1, dropped, None) == 0

            def extract():
                assert lib.a3d_voxel_map_extract_rgb(m.handle, out.d_points, out.d_normals, out.d_colors, None, cells,
                                                     C.byref(n_out)) == 0
        else:
            def insert():
                assert lib.a3d_voxel_map_insert(m.handle, view, pose, 1, dropped, None) == 0

            def extract():
                assert lib.a3d_voxel_map_extract(m.handle, out.d_points, out.d_normals, None, cells, C.byref(n_out)) == 0

        def retain():
            assert lib.a3d_voxel_map_retain(m.handle, None, None, 0, None, 0, None, C.byref(removed)) == 0

        self.calls = {"insert": insert, "extract": extract, "retain": retain}
        self.rows = None

    def prepare_retain(self):
        """The compacted map's rows, kept for the restore."""
        self.map.compact()
        self.rows = self.map.extract()
        assert self.map.cells() == self.map.total() == self.cells

    def restore(self):
        self.map.clear()
        self.map.insert(self.rows)

    def window(self, call):
        fn, ctx, ms = self.calls[call], self.ctx, 0.0
        if call != "retain":
            ctx.timer_start()
            for _ in range(CALLS[call]):
                fn()
            return ctx.timer_stop() / CALLS[call]
        for _ in range(CALLS[call]):
            self.restore()
            ctx.timer_start()
            fn()
            ms += ctx.timer_stop()
        return ms / CALLS[call]

    def free(self):
        for x in (self.rows, self.out, self.map):
            if x is not None:
                x.free()


def main():
    args = sys.argv[1:]
    parent_path = None
    if "--parent-library" in args:
        k = args.index("--parent-library")
        parent_path = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    out_path = args[0] if args else None
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    # the same frames with their colours (the clouds above came through the entry without them)
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(frames[0][0], [(f[1], f[2]) for f in frames],
                                                                                      frames[0][3])
    coloured = DevicePointCloud.from_range_images([p[0] for p in built], colors=True)
    for p in built:
        p[0].free()
    sides = [Side("without_colours", ctx, clouds, poses, False), Side("with_colours", ctx, coloured, poses, True)]
    everything = [*clouds, *coloured]
    if parent_path:
        pctx = parent_context(parent_path)
        pclouds = sample1_clouds(pctx)
        sides.insert(0, Side("parent_without_colours", pctx, pclouds, poses, False))
        everything += pclouds
    assert len({s.cells for s in sides}) == 1 and len({s.slots for s in sides}) == 1
    out = {"probe": "voxel_map_colors", "windows": WINDOWS, "calls_per_window": CALLS, "voxel": VOXEL, "frames": len(clouds),
           "map_cells": sides[0].cells, "map_slots": sides[0].slots, "frame_points": sides[0].frame_points,
           "parent_library": bool(parent_path), "device_ms": {}}
    for call in ("extract", "insert", "retain"):
        if call == "retain":
            for s in sides:
                s.prepare_retain()
        for s in sides:  # warm-up of this shape on every side
            for _ in range(3):
                if call == "retain":
                    s.restore()
                s.calls[call]()
        ms = {s.name: [] for s in sides}
        for _ in range(WINDOWS):
            for s in sides:
                ms[s.name].append(s.window(call))
        out["device_ms"][call] = {name: spread(v) for name, v in ms.items()}
    # bytes a call moves per row beyond the table's probes: 12 + 12 of point and normal, + 3 of colour read or written
    # by row and + 4 of the packed colour by slot
    out["payload_bytes_per_row"] = {"without_colours": 24, "with_colours_by_row": 27, "with_colours_by_slot": 28}
    ratios, gate = {}, {}
    for call, by_side in out["device_ms"].items():
        ratios[call] = round(by_side["with_colours"]["median"] / by_side["without_colours"]["median"], 3)
        if parent_path:
            p, n = by_side["parent_without_colours"], by_side["without_colours"]
            gate[call] = {"median": n["median"], "parent_min": p["min"], "parent_max": p["max"],
                          "within_parent_range": bool(p["min"] <= n["median"] <= p["max"])}
    out["with_over_without_colours"] = ratios
    if parent_path:
        out["gate"] = gate
    for s in sides:
        s.free()
    for c in everything:
        c.free()
    if parent_path:
        pctx.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
