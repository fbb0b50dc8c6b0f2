"""Plane segmentation of resident clouds (a3d_point_clouds_segment_plane_device) against the things it is judged by.
Prints one JSON line (and writes it to argv[1] if given: profiles/cloud_plane_probe.json).
    python scripts/cloud_plane_probe.py [out.json] [--parent DIR]

Shapes, all from tests/golden/rgbd/sample1 (those of scripts/cloud_cluster_probe.py): (a) one frame's cloud; (b) the same
frame thinned at v = 0.02; (c) the extract of the v = 0.02 voxel map of every frame under its odometry pose; (d) 64 frame
clouds in one call (the dataset's frames, repeated).  The threshold is 0.02 m, the candidates a3d_plane_hypotheses(seed 0).
Per shape:
  - the raw call at H = 100 / 1000 / 4096 candidates and R = 0 / 2 refinement rounds, into preallocated buffers, beside a
    device-to-device copy of the input points and neighbor_distances(radius, 0) on the same cloud in the same run;
  - split_plane through the wrappers end to end (H = 1000; allocation, both selects and the results included).
On shape (a):
  - the score kernel's own time at H = 1000 from a kernel trace of a child process, against its VALU bound: the rows x
    candidates x VALU instructions per row and candidate of the compiled loop (VALU_PER_TEST, read from the ISA) at one
    wave64 instruction per two cycles per SIMD, 1024 SIMDs, 2.4 GHz;
  - on the diagnostics build, the product form beside the forms that build keeps: A3D_PLANE_ROWS (rows per thread and
    pass: 1, 2, 8 beside the product's 4), A3D_PLANE_SPLIT (blocks per tile over the candidates: 1 to 16 beside the
    product's choice) and A3D_PLANE_COUNTERS=global (a global atomic per wave and candidate, no LDS counters).
The mapping record is examples/pcl_map.py --render-track with and without --remove-plane, two children.
--parent DIR (a directory that holds the align3d_amd package of the parent commit, built): voxel_downsample,
estimate_normals(counts), neighbor_distances(k = 0) and cluster(m = 1) on the frame are timed in child processes, this
build and the parent's in turn, three times each (this, parent, parent, this, this, parent); this build's medians must lie
inside the parent's own min-max range, and the JSON says how many of the entries did.

A figure is measured as in scripts/cloud_cluster_probe.py: windows of back-to-back host-synchronous calls between two
device events, the windows of the variants alternating, median and extremes over the windows."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_cluster_probe as P  # noqa: E402  (measure, the shapes, the raw calls of the entries the parent has too)
from align3d_amd import Context, DevicePointCloud, PointCloud, _abi  # noqa: E402  (the package P chose: the gate's children)

T = 0.02
SHAPES = (("a_frame", 0.01), ("b_frame_thinned_v0.02", 0.06), ("c_map_extract_v0.02", 0.06))
KNOBS = ("A3D_PLANE_ROWS", "A3D_PLANE_SPLIT", "A3D_PLANE_COUNTERS")
VALU_PER_TEST = 9  # the score loop per row and candidate: 3 v_subrev, 3 v_mul, 2 v_add, 1 v_cmp (cloud_plane.hip, -O3, gfx950)
SIMDS, CLOCK_HZ, CYCLES_PER_WAVE_INSTRUCTION = 1024, 2.4e9, 2
GATE_ENTRIES = ("voxel_downsample_v0.02", "estimate_normals_counts", "neighbor_distances_k0", "cluster_m1")


def hypotheses(n, H):
    out = np.zeros((H, 3), np.uint32)
    _abi.check(_abi.load_library().a3d_plane_hypotheses(0, n, H, out.ctypes.data_as(C.POINTER(C.c_uint32))), "hypotheses")
    return out


class PlaneCase:
    """A batch of clouds with preallocated outputs and candidates for every H: the raw call, so that no allocation is timed."""

    def __init__(self, ctx, clouds):
        self.ctx, self.clouds, self.n = ctx, clouds, len(clouds)
        self.views = (_abi.PointCloudViewC * self.n)(*[c.view() for c in clouds])
        self.flags = [ctx.malloc(max(4, 4 * c.len())) for c in clouds]
        self.copies = [ctx.malloc(max(4, 12 * c.len())) for c in clouds]
        self.d_flags = (C.c_void_p * self.n)(*self.flags)
        self.triples = {H: [hypotheses(c.len(), H) for c in clouds] for H in (100, 1000, 4096)}
        self.planes = (C.c_double * (4 * self.n))()
        self.inliers, self.best = (C.c_uint64 * self.n)(), (C.c_uint64 * self.n)()

    def segment(self, H, refine):
        tr = self.triples[H]
        st = self.ctx.lib.a3d_point_clouds_segment_plane_device(
            self.ctx.handle, self.views, self.n, T, refine, (C.c_void_p * self.n)(*[t.ctypes.data for t in tr]),
            (C.c_uint32 * self.n)(*[H] * self.n), self.d_flags, None, self.planes, self.best, self.inliers, None)
        assert st == 0, st

    def copy_points(self):
        for c, d in zip(self.clouds, self.copies):
            _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, d, c.d_points, 12 * c.len()))

    def free(self):
        for p in self.flags + self.copies:
            self.ctx.free(p)


def plane_figures(ctx, clouds, radius, light=False):
    case, knn = PlaneCase(ctx, clouds), P.Case(ctx, clouds, cluster=False)
    variants = [("copy_of_the_points_d2d", case.copy_points), ("neighbor_distances_k0", lambda: knn.knn_k0(radius))]
    for H in (100, 1000, 4096):
        for refine in (0, 2):
            variants.append((f"segment_plane_H{H}_R{refine}", lambda H=H, refine=refine: case.segment(H, refine)))
    res = P.measure(ctx, variants, light)
    case.segment(1000, 0)
    points = sum(c.len() for c in clouds)
    res.update(points=points, clouds=len(clouds), t=T, radius_of_neighbor_distances=radius,
               inliers_H1000_R0=sum(int(v) for v in case.inliers))
    for H in (100, 1000, 4096):
        res[f"segment_plane_H{H}_R0_over_neighbor_distances_k0"] = round(
            res[f"segment_plane_H{H}_R0"]["median"] / res["neighbor_distances_k0"]["median"], 3)
    case.free(), knn.free()
    return res


def valu_bound_ms(points, H):
    return points * H * VALU_PER_TEST / 64 * CYCLES_PER_WAVE_INSTRUCTION / SIMDS / CLOCK_HZ * 1e3


TRACE_CALLS = 30


def trace_child():
    ctx = Context(0)
    shapes, _ = P.sample1_shapes(ctx)
    case = PlaneCase(ctx, [shapes[0]])
    for _ in range(TRACE_CALLS):
        case.segment(1000, 0)
    case.free()
    ctx.close()


def kernel_times(points):
    """Median kernel times in microseconds of the call's kernels on shape (a) at H = 1000, R = 0, from a kernel trace of a
    child process, and the score kernel's time over its VALU bound."""
    import shutil
    import sqlite3
    import tempfile

    if shutil.which("rocprofv3") is None:
        return {"skipped": "no rocprofv3 on the path"}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--", sys.executable,
                        os.path.abspath(__file__), "--trace-child"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=240)
        found = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
        if not found:
            return {"skipped": "the trace left no database"}
        rows = sqlite3.connect(found[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = {}
    for name, start, end in rows:
        short = name.replace("(anonymous namespace)::", "").replace("a3d::", "").replace("void ", "").split("(")[0].split("<")[0]
        if short.startswith("plane_"):
            per.setdefault(short, []).append((end - start) / 1e3)
    out = {"calls": TRACE_CALLS, "H": 1000, "points": points}
    for short, us in per.items():
        out[short] = {"median_us": round(statistics.median(us), 1), "dispatches": len(us)}
    if "plane_score_kernel" in out:
        bound = valu_bound_ms(points, 1000) * 1e3
        out["score_valu_bound_us"] = round(bound, 1)
        out["score_time_over_valu_bound"] = round(out["plane_score_kernel"]["median_us"] / bound, 2)
        out["valu_instructions_per_row_and_candidate"] = VALU_PER_TEST
    return out


def mapping_record():
    """examples/pcl_map.py --voxel 0.02 --online --render-track on sample1, 20 frames, without and with --remove-plane 0.02:
    what the removal takes out and the two trajectory errors each run prints.  A record, not a gate."""
    out = {}
    base = [sys.executable, os.path.join(ROOT, "examples", "pcl_map.py"), "--max-frames", "20", "--voxel", "0.02", "--online",
            "--render-track"]
    for name, extra in (("without", []), ("with_remove_plane_0.02", ["--remove-plane", "0.02"])):
        text = subprocess.run(base + extra, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              timeout=240).stdout
        err = re.search(r"odometry alone ([0-9.e+-]+) m, corrected against the rendered map ([0-9.e+-]+) m", text)
        cells = re.search(r"map of (\d+) points", text)
        rec = {"command": " ".join(["examples/pcl_map.py"] + base[2:] + extra), "odometry_alone_m": float(err.group(1)),
               "corrected_against_the_rendered_map_m": float(err.group(2)), "cells": int(cells.group(1))}
        rows = re.search(r"plane removal .*: (\d+) rows -> (\d+)", text)
        if rows:
            rec.update(rows_in=int(rows.group(1)), rows_kept=int(rows.group(2)))
        out[name] = rec
    return out


def gate_child():
    """What a child of the gate measures: entries the parent build has too, on the frame."""
    ctx = Context(0)
    shapes, _ = P.sample1_shapes(ctx)
    case = P.Case(ctx, [shapes[0]])
    res = P.measure(ctx, [("voxel_downsample_v0.02", lambda: case.downsample(0.02)),
                          ("estimate_normals_counts", lambda: case.estimate_counts(0.01)),
                          ("neighbor_distances_k0", lambda: case.knn_k0(0.01)),
                          ("cluster_m1", lambda: case.cluster(0.01, 1))])
    case.free()
    print(json.dumps(res))
    ctx.close()


def gate(parent):
    """This build and the parent's in turn, three child processes each, in the order this, parent, parent, this, this,
    parent (so that neither build always runs on the device the other has just warmed up)."""
    runs = {"this": [], "parent": []}
    builds = (("this", ROOT), ("parent", os.path.abspath(parent)))
    for order in (builds, builds[::-1], builds):
        for who, root in order:
            env = dict(os.environ, A3D_PROBE_PACKAGE_ROOT=root)
            env.pop("A3D_LIBRARY", None)
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--gate-child"], env=env, check=True,
                                  stdout=subprocess.PIPE, text=True, timeout=240).stdout.strip().splitlines()[-1]
            runs[who].append(json.loads(line))
    out = {"shape": "a_frame", "entries": len(GATE_ENTRIES), "inside": 0}
    for entry in GATE_ENTRIES:
        t_med = statistics.median(r[entry]["median"] for r in runs["this"])
        p_min = min(r[entry]["min"] for r in runs["parent"])
        p_max = max(r[entry]["max"] for r in runs["parent"])
        p_med = statistics.median(r[entry]["median"] for r in runs["parent"])
        out[entry] = {"this_median": round(t_med, 4), "parent_median": round(p_med, 4), "parent_min": p_min, "parent_max": p_max,
                      "inside": p_min <= t_med <= p_max, "at_or_below_parent_max": t_med <= p_max}
        out["inside"] += out[entry]["inside"]
    return out


def forms(points_host):
    """The product form beside the forms the diagnostics build keeps, on shape (a) at H = 1000, R = 0."""
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    cloud = DevicePointCloud(diag, PointCloud(points_host))
    case = PlaneCase(diag, [cloud])

    def form(knob=None, value=None):
        def fn():
            for k in KNOBS:
                os.environ.pop(k, None)
            if knob:
                os.environ[knob] = value
            case.segment(1000, 0)
        return fn
    variants = [("product_form_rows4_split8", form())]
    variants += [(f"rows{r}", form("A3D_PLANE_ROWS", str(r))) for r in (1, 2, 8)]
    variants += [(f"split{s}", form("A3D_PLANE_SPLIT", str(s))) for s in (1, 2, 4, 16)]
    variants += [("global_counters", form("A3D_PLANE_COUNTERS", "global"))]
    res = P.measure(diag, variants)
    form()()
    for name, _ in variants[1:]:
        res[f"{name}_over_product_form"] = round(res[name]["median"] / res[variants[0][0]]["median"], 3)
    case.free(), cloud.free()
    diag.close()
    return res


def main():
    args = sys.argv[1:]
    if "--trace-child" in args:
        return trace_child()
    if "--gate-child" in args:
        return gate_child()
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    out_path = next((a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")), None)
    ctx = Context(0)
    out = {"probe": "cloud_plane", "launches_per_call": "4 + 1 per refinement round"}
    shapes, frames = P.sample1_shapes(ctx)
    for (name, radius), cloud in zip(SHAPES, shapes):
        print(name, file=sys.stderr, flush=True)
        res = plane_figures(ctx, [cloud], radius)

        def split():
            _, on, off = cloud.split_plane(T, 1000)
            on.free(), off.free()
        res.update(P.measure(ctx, [("split_plane_H1000_wrappers", split)]))
        for H in (100, 1000, 4096):
            res[f"score_valu_bound_ms_H{H}"] = round(valu_bound_ms(cloud.len(), H), 4)
        out[name] = res
    frame_host = shapes[0].download()[0]
    print("d_64_frames_one_call", file=sys.stderr, flush=True)
    out["d_64_frames_one_call"] = plane_figures(ctx, [frames[i % len(frames)] for i in range(64)], 0.01)
    ctx.close()
    print("forms (diagnostics build)", file=sys.stderr, flush=True)
    out["a_frame"]["score_forms_diagnostics_build_H1000"] = forms(frame_host)
    print("kernel trace", file=sys.stderr, flush=True)
    out["kernel_times_a_frame_H1000"] = kernel_times(len(frame_host))
    print("mapping record", file=sys.stderr, flush=True)
    out["mapping_record_render_track"] = mapping_record()
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
