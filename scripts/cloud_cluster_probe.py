"""Clustering of resident clouds (a3d_point_clouds_cluster_device) against the thing it is judged by.  Prints one JSON
line (and writes it to argv[1] if given: profiles/cloud_cluster_probe.json).
    python scripts/cloud_cluster_probe.py [out.json] [--parent DIR [--gate-only]]

Shapes, all from tests/golden/rgbd/sample1: (a) one frame's cloud at r = 0.01; (b) the same frame thinned at v = 0.02, at
r = 0.06; (c) the extract of the v = 0.02 voxel map of every frame under its odometry pose, at r = 0.06; (d) 64 frame
clouds in one call at r = 0.01 (the dataset's frames, repeated); (e) the frame of (a) at r = 1e3: every row in one cell,
every union on one root.  Per shape:
  - cluster at min_points = 1 and 8 beside the yardstick, neighbor_distances(radius, 0) on the same cloud in the same run:
    that call does one of the two neighbourhood walks clustering needs, so the ratio says what the rest costs;
  - the wrappers remove_small_clusters and largest_cluster end to end (allocation and the result included);
  - per kernel, the median time of the cluster call's and the k = 0 call's kernels on (b) and (a), from a kernel trace of a
    child process; and the mapping record (examples/pcl_map.py --render-track with --clusters 0.02 1 50), a child as well;
  - on the diagnostics build, the product form beside the forms that build keeps (A3D_CLUSTER_LINK=all: union with every
    core neighbour, not the lower-indexed half; A3D_CLUSTER_HALVING=0: no path halving in the link pass).
--parent DIR (a directory that holds the align3d_amd package of the parent commit, built): every entry that walks the
cell sort of cell_sort.hpp (neighbor_distances at k = 0, 8 and 32, estimate_normals counts only and in full, cluster at
min_points 1 and 8) and two that do not (select, voxel_downsample) are timed on shapes (a) to (d) in child processes, this
build and the parent's in turn, three times each (this, parent, parent, this, this, parent).  The gate: for every entry and
shape, this build's median is at or below the parent's maximum (all_at_or_below_parent_max); whether it also lies inside
the parent's own min-max range is recorded beside it.  --gate-only: nothing but the gate (profiles/cell_sort_gate.json).

A figure is the time of a window of back-to-back host-synchronous calls between two device events on the context's stream,
divided by the calls in it (so it includes each call's table upload, the fill and the synchronise, which is what a caller
pays); the windows of the variants alternate, and the median and the extremes over the windows are kept."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = os.environ.get("A3D_PROBE_PACKAGE_ROOT", ROOT)  # (a child of the gate imports the parent's package)
sys.path.insert(0, PACKAGE_ROOT)
from align3d_amd import (Context, DevicePointCloud, DeviceVoxelMap, IcpBatch, IcpParams, PointCloud,  # noqa: E402
                         RangeImageBuilder, SlamTbDataset, Transform, TrajectoryBuilder, _abi)

WINDOWS = 5
WINDOW_S = 0.2  # a window is sized to about this long from a first estimate
SHAPES = (("a_frame_r0.01", 0.01), ("b_frame_thinned_v0.02_r0.06", 0.06), ("c_map_extract_v0.02_r0.06", 0.06))
KNOBS = ("A3D_CLUSTER_LINK", "A3D_CLUSTER_HALVING")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def window_ms(ctx, fn, calls):
    ctx.timer_start()
    for _ in range(calls):
        fn()
    return ctx.timer_stop() / calls


def measure(ctx, variants, light=False):
    """variants: [(name, fn)] -> {name: spread of ms per call}; the windows of the variants alternate.  light (a shape whose
    call takes seconds): one warm-up call, windows of one call, three of them, or one if a call takes more than 4 s."""
    calls, windows = {}, 3 if light else WINDOWS
    for name, fn in variants:
        for _ in range(1 if light else 3):
            fn()  # warm-up of this shape (grows the context's scratch region once)
        first = window_ms(ctx, fn, 1 if light else 3)
        calls[name] = 1 if light else max(3, int(WINDOW_S * 1e3 / max(first, 1e-3)))
        if light and first > 4e3:
            windows = 1
        print(f"  {name}: about {first:.3f} ms a call", file=sys.stderr, flush=True)
    ms = {name: [] for name, _ in variants}
    for _ in range(windows):
        for name, fn in variants:
            ms[name].append(window_ms(ctx, fn, calls[name]))
    return {name: dict(spread(v), calls_per_window=calls[name], windows=windows) for name, v in ms.items()}


def sample1_shapes(ctx):
    """(the three clouds, resident: a frame, the frame thinned, the map's extract; every frame's cloud)."""
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(cam, [(f[1], f[2]) for f in frames],
                                                                                      depth_scale)
    clouds = DevicePointCloud.from_range_images([pyramid[0] for pyramid in built])
    batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
    poses, status = batch.align(clouds[1:])
    batch.free()
    traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
    world = [traj.current_camera_to_world()]
    for k, (now_to_previous, st) in enumerate(zip(poses, status)):
        if st == 0:
            traj.accumulate(now_to_previous, float(k + 1))
        world.append(traj.current_camera_to_world())
    vmap = DeviceVoxelMap(ctx, 0.02, normals=True)
    vmap.insert_many(clouds, world)
    shapes = [clouds[0], clouds[0].voxel_downsample(0.02), vmap.extract()]
    vmap.free()
    return shapes, clouds


class Case:
    """A batch of clouds with preallocated outputs: the raw calls, so that no allocation is timed."""

    def __init__(self, ctx, clouds, cluster=True):
        self.ctx, self.clouds, self.n = ctx, clouds, len(clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        names = ("counts", "qsum", "curvature", "normals", "out_points", "out_normals", "mask") + (("labels", "row_sizes", "sizes", "roots") if cluster else ())
        wide = ("normals", "out_points", "out_normals")
        self.bufs = {name: [ctx.malloc(max(4, (12 if name in wide else 4) * c.len())) for c in clouds] for name in names}
        for c, d in zip(clouds, self.bufs["mask"]):
            mask = np.ascontiguousarray(np.arange(c.len()) % 2, np.uint32)  # every other row
            _abi.check(ctx.lib.a3d_memcpy_h2d(ctx.handle, d, _abi.ptr(mask), 4 * c.len()))
        self.tables = {name: (C.c_void_p * self.n)(*ptrs) for name, ptrs in self.bufs.items()}
        self.words = (C.c_uint64 * (4 * self.n))()
        self.found = (C.c_uint64 * self.n)()
        self.noise = (C.c_uint64 * self.n)()

    def knn_k0(self, radius):
        st = self.ctx.lib.a3d_point_clouds_knn_distance_device(self.ctx.handle, self.views, self.n, radius, 0, self.tables["counts"],
                                                               None, self.words, None)
        assert st == 0, st

    def knn(self, radius, k):
        st = self.ctx.lib.a3d_point_clouds_knn_distance_device(self.ctx.handle, self.views, self.n, radius, k, self.tables["counts"],
                                                               self.tables["qsum"], self.words, None)
        assert st == 0, st

    def cluster(self, radius, m, row_sizes=True):
        st = self.ctx.lib.a3d_point_clouds_cluster_device(self.ctx.handle, self.views, self.n, radius, m, self.tables["labels"],
                                                          self.tables["row_sizes"] if row_sizes else None, self.tables["sizes"],
                                                          self.tables["roots"], self.found, self.noise, None)
        assert st == 0, st

    def estimate_counts(self, radius):
        st = self.ctx.lib.a3d_point_clouds_estimate_normals_device(self.ctx.handle, self.views, self.n, radius, 3, None, 0,
                                                                   self.tables["normals"], None, self.tables["counts"],
                                                                   self.words, None)
        assert st == 0, st

    def estimate_full(self, radius):
        st = self.ctx.lib.a3d_point_clouds_estimate_normals_device(self.ctx.handle, self.views, self.n, radius, 3, None, 0,
                                                                   self.tables["normals"], self.tables["curvature"],
                                                                   self.tables["counts"], self.words, None)
        assert st == 0, st

    def downsample(self, voxel):
        st = self.ctx.lib.a3d_point_clouds_voxel_downsample_device(self.ctx.handle, self.views, self.n, voxel, None,
                                                                   self.tables["out_points"], self.tables["out_normals"], None,
                                                                   (C.c_uint64 * self.n)(*[c.len() for c in self.clouds]),
                                                                   self.words, None)
        assert st == 0, st

    def select_half(self):
        ones = (C.c_uint32 * self.n)(*[1] * self.n)
        st = self.ctx.lib.a3d_point_clouds_select_device(self.ctx.handle, self.views, None, self.n, self.tables["mask"], ones, ones,
                                                         self.tables["out_points"], None, None, None,
                                                         (C.c_uint64 * self.n)(*[c.len() for c in self.clouds]), self.words)
        assert st == 0, st

    def free(self):
        for ptrs in self.bufs.values():
            for p in ptrs:
                self.ctx.free(p)


def existing_entries(ctx):
    """What a child of the gate measures: entries the parent build has too."""
    out = {}
    shapes, frames = sample1_shapes(ctx)
    batches = [[cloud] for cloud in shapes] + [[frames[i % len(frames)] for i in range(64)]]
    for (name, radius), clouds in zip(GATE_SHAPES, batches):
        print(name, file=sys.stderr, flush=True)
        case = Case(ctx, clouds)
        out[name] = dict(measure(ctx, [("neighbor_distances_k0", lambda: case.knn_k0(radius)),
                                       ("neighbor_distances_k8", lambda: case.knn(radius, 8)),
                                       ("neighbor_distances_k32", lambda: case.knn(radius, 32)),
                                       ("estimate_normals_counts", lambda: case.estimate_counts(radius)),
                                       ("estimate_normals_full", lambda: case.estimate_full(radius)),
                                       ("cluster_m1", lambda: case.cluster(radius, 1)),
                                       ("cluster_m8", lambda: case.cluster(radius, 8)),
                                       ("select_half", case.select_half),
                                       ("voxel_downsample_v0.02", lambda: case.downsample(0.02))]),
                         points=sum(c.len() for c in clouds))
        case.free()
    return out


# (shape (e), every row in one cell, takes seconds a call: not gated, as the light path above)
GATE_SHAPES = SHAPES + (("d_64_frames_one_call_r0.01", 0.01),)
ENTRIES = ("neighbor_distances_k0", "neighbor_distances_k8", "neighbor_distances_k32", "estimate_normals_counts",
           "estimate_normals_full", "cluster_m1", "cluster_m8", "select_half", "voxel_downsample_v0.02")


def gate(parent):
    """This build and the parent's in turn, three child processes each, in the order this, parent, parent, this, this,
    parent (so that neither build always runs on the device the other has just warmed up)."""
    runs = {"this": [], "parent": []}
    builds = (("this", ROOT), ("parent", os.path.abspath(parent)))
    for order in (builds, builds[::-1], builds):
        for who, root in order:
            env = dict(os.environ, A3D_PROBE_PACKAGE_ROOT=root)
            env.pop("A3D_LIBRARY", None)
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True,
                                  stdout=subprocess.PIPE, text=True, timeout=480).stdout.strip().splitlines()[-1]
            runs[who].append(json.loads(line))
    out = {"all_at_or_below_parent_max": True, "all_inside": True}
    for shape, _ in GATE_SHAPES:
        res = {"points": runs["this"][0][shape]["points"]}
        for entry in ENTRIES:
            t_med = statistics.median(r[shape][entry]["median"] for r in runs["this"])
            p_min = min(r[shape][entry]["min"] for r in runs["parent"])
            p_max = max(r[shape][entry]["max"] for r in runs["parent"])
            p_med = statistics.median(r[shape][entry]["median"] for r in runs["parent"])
            res[entry] = {"this_median": round(t_med, 4), "parent_median": round(p_med, 4), "parent_min": p_min,
                          "parent_max": p_max, "inside": p_min <= t_med <= p_max, "at_or_below_parent_max": t_med <= p_max}
            out["all_at_or_below_parent_max"] &= res[entry]["at_or_below_parent_max"]
            out["all_inside"] &= res[entry]["inside"]
        out[shape] = res
    return out


def cluster_figures(ctx, case, radius, light=False):
    variants = [("neighbor_distances_k0", lambda: case.knn_k0(radius)), ("cluster_m1", lambda: case.cluster(radius, 1)),
                ("cluster_m8", lambda: case.cluster(radius, 8))]
    if not light:
        variants.append(("cluster_m1_labels_only", lambda: case.cluster(radius, 1, row_sizes=False)))
    res = measure(ctx, variants, light)
    for m in (1, 8):
        case.cluster(radius, m)
        res[f"clusters_m{m}"] = sum(int(v) for v in case.found)
        res[f"noise_rows_m{m}"] = sum(int(v) for v in case.noise)
        res[f"cluster_m{m}_over_neighbor_distances_k0"] = round(res[f"cluster_m{m}"]["median"] / res["neighbor_distances_k0"]["median"], 3)
    res.update(points=sum(c.len() for c in case.clouds), clouds=case.n, radius=radius)
    return res


TRACE_CALLS = 30


def trace_child():
    """What the kernel trace runs: TRACE_CALLS cluster calls (m = 1) and as many k = 0 calls, on shape (b), then on (a)."""
    ctx = Context(0)
    shapes, _ = sample1_shapes(ctx)
    for cloud, radius in ((shapes[1], 0.06), (shapes[0], 0.01)):
        case = Case(ctx, [cloud])
        for _ in range(TRACE_CALLS):
            case.cluster(radius, 1)
            case.knn_k0(radius)
        case.free()
    ctx.close()


def kernel_times():
    """Median kernel times in microseconds of the cluster call's and the k = 0 call's kernels on shapes (b) and (a), from a
    kernel trace of a child process (rocprofv3 --kernel-trace --stats; the kernels run one after the other on one stream, and the
    first half of a kernel's dispatches are shape (b)'s)."""
    import shutil
    import sqlite3
    import tempfile

    if shutil.which("rocprofv3") is None:
        return {"skipped": "no rocprofv3 on the path"}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__),
                        "--trace-child"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
        found = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
        if not found:
            return {"skipped": "the trace left no database"}
        rows = sqlite3.connect(found[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = {}
    for name, start, end in rows:
        # (the sort's kernels are templates of cell_sort.hpp: a3d::cell_count_kernel<(anonymous namespace)::KnnJob>(...))
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("a3d::", "").split("(")[0]
        if short.startswith(("knn_", "cluster_", "cell_")):
            per.setdefault(short, []).append((end - start) / 1e3)
    out = {"calls_per_shape": TRACE_CALLS}
    for short, us in per.items():
        half = len(us) // 2
        out[short] = {"b_frame_thinned_us": round(statistics.median(us[:half]), 1),
                      "a_frame_us": round(statistics.median(us[half:]), 1), "dispatches": len(us)}
    return out


def mapping_record():
    """examples/pcl_map.py --voxel 0.02 --online --render-track on sample1, 20 frames, with --clusters 0.02 1 50: what the
    filter removes and the two trajectory errors it prints.  A record, not a gate."""
    import re

    cmd = [sys.executable, os.path.join(ROOT, "examples", "pcl_map.py"), "--max-frames", "20", "--voxel", "0.02", "--online",
           "--render-track", "--clusters", "0.02", "1", "50"]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240).stdout
    rows = re.search(r"cluster outlier filter .*: (\d+) rows -> (\d+)", text)
    err = re.search(r"odometry alone ([0-9.e+-]+) m, corrected against the rendered map ([0-9.e+-]+) m", text)
    cells = re.search(r"map of (\d+) points", text)
    return {"command": " ".join(["examples/pcl_map.py"] + cmd[2:]), "rows_in": int(rows.group(1)), "rows_kept": int(rows.group(2)),
            "odometry_alone_m": float(err.group(1)), "corrected_against_the_rendered_map_m": float(err.group(2)),
            "cells": int(cells.group(1))}


def main():
    args = sys.argv[1:]
    if "--trace-child" in args:
        trace_child()
        return
    if "--child" in args:
        ctx = Context(0)
        print(json.dumps(existing_entries(ctx)))
        ctx.close()
        return
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    out_path = next((a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")), None)
    if "--gate-only" in args:
        assert parent, "--gate-only needs --parent DIR"
        line = json.dumps({"probe": "cloud_cluster", "gate_against_the_parent_build": gate(parent)})
        print(line)
        if out_path:
            with open(out_path, "w") as f:
                f.write(line + "\n")
        return
    ctx = Context(0)
    out = {"probe": "cloud_cluster", "launches_per_call": 8}  # (every figure carries its own number of windows)
    shapes, frames = sample1_shapes(ctx)
    hosts = []
    for (name, radius), cloud in zip(SHAPES, shapes):
        print(name, file=sys.stderr, flush=True)
        case = Case(ctx, [cloud])
        res = cluster_figures(ctx, case, radius)
        case.free()

        def small():
            cloud.remove_small_clusters(radius, 1, 10).free()

        def largest():
            cloud.largest_cluster(radius, 1).free()
        res.update(measure(ctx, [("remove_small_clusters_m1_s10", small), ("largest_cluster_m1", largest)]))
        kept_s, kept_l = cloud.remove_small_clusters(radius, 1, 10), cloud.largest_cluster(radius, 1)
        res.update(kept_by_remove_small_clusters=kept_s.len(), rows_of_largest_cluster=kept_l.len())
        kept_s.free(), kept_l.free()
        out[name] = res
        hosts.append(cloud.download()[0])
    many = [frames[i % len(frames)] for i in range(64)]
    case = Case(ctx, many)
    out["d_64_frames_one_call_r0.01"] = cluster_figures(ctx, case, 0.01)
    case.free()
    case = Case(ctx, [shapes[0]])
    out["e_frame_in_one_cell_r1e3"] = cluster_figures(ctx, case, 1e3, light=True)
    case.free()
    ctx.close()
    # the forms of the link pass, on the diagnostics build
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    cases = [(n, r, p, False) for (n, r), p in zip(SHAPES, hosts)] + [("e_frame_in_one_cell_r1e3", 1e3, hosts[0], True)]
    for key, radius, pts, light in cases:
        print(key + " (diagnostics build)", file=sys.stderr, flush=True)
        cloud = DevicePointCloud(diag, PointCloud(pts))
        case = Case(diag, [cloud])

        def form(m, knob=None, value=None):
            def fn():
                for k in KNOBS:
                    os.environ.pop(k, None)
                if knob:
                    os.environ[knob] = value
                case.cluster(radius, m)
            return fn
        forms = {}
        for m in (1,) if light else (1, 8):
            res = measure(diag, [("product_form", form(m)), ("link_all", form(m, "A3D_CLUSTER_LINK", "all")),
                                 ("no_halving", form(m, "A3D_CLUSTER_HALVING", "0"))], light)
            form(m)()
            for other in ("link_all", "no_halving"):
                res[f"{other}_over_product_form"] = round(res[other]["median"] / res["product_form"]["median"], 3)
            forms[f"m{m}"] = res
        out[key]["link_pass_forms_diagnostics_build"] = forms
        case.free(), cloud.free()
    diag.close()
    print("kernel trace", file=sys.stderr, flush=True)
    out["kernel_times_m1"] = kernel_times()
    print("mapping record", file=sys.stderr, flush=True)
    out["mapping_record_clusters_0.02_1_50"] = mapping_record()
    if parent:
        print("gate", file=sys.stderr, flush=True)
        out["gate_against_the_parent_build"] = gate(parent)
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
