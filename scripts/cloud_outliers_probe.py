"""Outlier removal for resident clouds (a3d_point_clouds_knn_distance_device, a3d_point_clouds_select_device) against the
things it is judged by.  Prints one JSON line (and writes it to argv[1] if given: profiles/cloud_outliers_probe.json).
    python scripts/cloud_outliers_probe.py [out.json] [--parent DIR]

Shapes, all from tests/golden/rgbd/sample1: (a) one frame's cloud at r = 0.01; (b) the same frame thinned at v = 0.02, at
r = 0.06; (c) the extract of the v = 0.02 voxel map of every frame under its odometry pose, at r = 0.06.  Per shape:
  - the k = 0 call beside estimate_normals(counts=True) at the same radius (it does strictly less: no moments, no Jacobi),
    and the k = 8 / 16 / 32 calls, the price of the selection;
  - select keeping every other row (points, normals, index) beside a device-to-device copy of its output bytes;
  - both filters end to end through the Python wrappers (allocation and the index-free result included);
  - on the diagnostics build, the product form of the k = 8 call beside the forms that build keeps (A3D_OUTLIERS_K=32: the
    widest register array for every k; A3D_OUTLIERS_SELECT=t: select on the lattice distance of every candidate).
--parent DIR (a directory that holds the align3d_amd package of the parent commit, built): estimate_normals(counts=True),
voxel_downsample and, where the build has it, the k = 0 call are timed in child processes, this build and the parent's in
turn, twice each (this, parent, parent, this); the k = 0 call's range must lie at or below the parent's estimate_normals range, and this build's medians
of the two existing entries inside the parent's own range.

A figure is the time of a window of back-to-back host-synchronous calls between two device events on the context's stream,
divided by the calls in it (so it includes each call's table upload, the fill of the hash tables and the synchronise,
which is what a caller pays); the windows of the variants alternate, and the median and the extremes over the windows are
kept."""
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
        calls[name] = max(3, int(WINDOW_S * 1e3 / max(window_ms(ctx, fn, 3), 1e-3)))
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ms[name].append(window_ms(ctx, fn, calls[name]))
    return {name: dict(spread(v), calls_per_window=calls[name]) for name, v in ms.items()}


def sample1_shapes(ctx):
    """The three clouds, resident: a frame, the frame thinned, the map's extract."""
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
    return shapes


class Case:
    """One cloud with preallocated outputs: the raw calls, so that no allocation is timed."""

    def __init__(self, ctx, cloud, new_entries=True):
        self.ctx, self.cloud, self.n = ctx, cloud, cloud.len()
        self.view = (_abi.PointCloudViewC * 1)(cloud.view())
        sizes = {"normals": 12 * self.n, "counts": 4 * self.n, "out_points": 12 * self.n, "out_normals": 12 * self.n}
        if new_entries:
            sizes.update(qsum=4 * self.n, out_index=4 * self.n, mask=4 * self.n, copy_src=28 * (self.n // 2),
                         copy_dst=28 * (self.n // 2))
        self.bufs = {name: ctx.malloc(max(4, size)) for name, size in sizes.items()}
        if new_entries:
            mask = np.ascontiguousarray(np.arange(self.n) % 2, np.uint32)  # every other row
            _abi.check(ctx.lib.a3d_memcpy_h2d(ctx.handle, self.bufs["mask"], _abi.ptr(mask), 4 * self.n))
        self.words = (C.c_uint64 * 4)()
        self.one = {name: (C.c_void_p * 1)(p) for name, p in self.bufs.items()}

    def estimate_counts(self, radius):
        st = self.ctx.lib.a3d_point_clouds_estimate_normals_device(self.ctx.handle, self.view, 1, radius, 3, None, 0,
                                                                   self.one["normals"], None, self.one["counts"], self.words,
                                                                   None)
        assert st == 0, st

    def downsample(self, voxel):
        st = self.ctx.lib.a3d_point_clouds_voxel_downsample_device(self.ctx.handle, self.view, 1, voxel, None,
                                                                   self.one["out_points"], self.one["out_normals"], None,
                                                                   (C.c_uint64 * 1)(self.n), self.words, None)
        assert st == 0, st

    def knn(self, radius, k):
        st = self.ctx.lib.a3d_point_clouds_knn_distance_device(self.ctx.handle, self.view, 1, radius, k, self.one["counts"],
                                                               self.one["qsum"] if k else None, self.words, None)
        assert st == 0, st

    def select_half(self):
        st = self.ctx.lib.a3d_point_clouds_select_device(self.ctx.handle, self.view, None, 1, self.one["mask"],
                                                         (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(1), self.one["out_points"],
                                                         self.one["out_normals"], None, self.one["out_index"],
                                                         (C.c_uint64 * 1)(self.n), self.words)
        assert st == 0 and self.words[0] == self.n // 2, (st, self.words[0])

    def copy_half(self):  # what select_half writes: 12 + 12 + 4 bytes for every other row
        _abi.check(self.ctx.lib.a3d_memcpy_d2d(self.ctx.handle, self.bufs["copy_dst"], self.bufs["copy_src"],
                                               28 * (self.n // 2)))
        self.ctx.synchronize()  # (the entry under test is host-synchronous: the copy is timed the same way)

    def free(self):
        for p in self.bufs.values():
            self.ctx.free(p)


def existing_entries(ctx):
    """What a child of the gate measures: the entries the parent build has too (and the k = 0 call where there is one)."""
    out = {}
    has_knn = hasattr(ctx.lib, "a3d_point_clouds_knn_distance_device")
    for (name, radius), cloud in zip(SHAPES, sample1_shapes(ctx)):
        case = Case(ctx, cloud, new_entries=has_knn)
        variants = [("estimate_normals_counts", lambda: case.estimate_counts(radius)),
                    ("voxel_downsample_v0.02", lambda: case.downsample(0.02))]
        if has_knn:
            variants.append(("knn_k0", lambda: case.knn(radius, 0)))
        out[name] = dict(measure(ctx, variants), points=case.n, radius=radius)
        case.free()
    return out


def gate(parent):
    """This build and the parent's in turn, two child processes each, in the order this, parent, parent, this (so that
    neither build always runs on the device the other has just warmed up)."""
    runs = {"this": [], "parent": []}
    builds = (("this", ROOT), ("parent", os.path.abspath(parent)))
    for order in (builds, builds[::-1]):
        for who, root in order:
            env = dict(os.environ, A3D_PROBE_PACKAGE_ROOT=root)
            env.pop("A3D_LIBRARY", None)
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True,
                                  stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1]
            runs[who].append(json.loads(line))
    out = {}
    for shape, _ in SHAPES:
        res = {}

        def rng(who, entry):
            return (min(r[shape][entry]["min"] for r in runs[who]), max(r[shape][entry]["max"] for r in runs[who]),
                    statistics.median(r[shape][entry]["median"] for r in runs[who]))
        for entry in ("estimate_normals_counts", "voxel_downsample_v0.02"):
            t_min, t_max, t_med = rng("this", entry)
            p_min, p_max, p_med = rng("parent", entry)
            res[entry] = {"this_median": round(t_med, 4), "this_min": t_min, "this_max": t_max, "parent_median": round(p_med, 4),
                          "parent_min": p_min, "parent_max": p_max, "inside": p_min <= t_med <= p_max}
        k_min, k_max, k_med = rng("this", "knn_k0")
        p_min, p_max, p_med = rng("parent", "estimate_normals_counts")
        res["knn_k0_vs_parent_estimate_normals_counts"] = {
            "knn_k0_median": round(k_med, 4), "knn_k0_min": k_min, "knn_k0_max": k_max, "parent_median": round(p_med, 4),
            "parent_min": p_min, "parent_max": p_max, "at_or_below": k_max <= p_max and k_min <= p_min}
        res["points"] = runs["this"][0][shape]["points"]
        out[shape] = res
    return out


def main():
    args = sys.argv[1:]
    if "--child" in args:
        ctx = Context(0)
        print(json.dumps(existing_entries(ctx)))
        ctx.close()
        return
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    out_path = next((a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")), None)
    ctx = Context(0)
    out = {"probe": "cloud_outliers", "windows": WINDOWS}
    shapes = sample1_shapes(ctx)
    hosts = []
    for (name, radius), cloud in zip(SHAPES, shapes):
        case = Case(ctx, cloud)
        res = measure(ctx, [("estimate_normals_counts", lambda: case.estimate_counts(radius)),
                            ("knn_k0", lambda: case.knn(radius, 0)), ("knn_k8", lambda: case.knn(radius, 8)),
                            ("knn_k16", lambda: case.knn(radius, 16)), ("knn_k32", lambda: case.knn(radius, 32)),
                            ("select_half", case.select_half), ("memcpy_d2d_select_output_bytes", case.copy_half)])
        case.knn(radius, 8)
        res["rows_with_8_others"] = int(case.words[0])
        res["k0_over_estimate_normals_counts"] = round(res["knn_k0"]["median"] / res["estimate_normals_counts"]["median"], 3)
        for k in (8, 16, 32):
            res[f"k{k}_over_k0"] = round(res[f"knn_k{k}"]["median"] / res["knn_k0"]["median"], 3)
        res["select_times_the_copy"] = round(res["select_half"]["median"] / res["memcpy_d2d_select_output_bytes"]["median"], 2)
        case.free()

        def radius_filter():
            cloud.remove_radius_outliers(radius, 8).free()

        def statistical_filter():
            cloud.remove_statistical_outliers(radius, 8, 2.0).free()
        res.update(measure(ctx, [("remove_radius_outliers_n8", radius_filter),
                                 ("remove_statistical_outliers_k8_a2", statistical_filter)]))
        kept_r, kept_s = cloud.remove_radius_outliers(radius, 8), cloud.remove_statistical_outliers(radius, 8, 2.0)
        res.update(points=cloud.len(), radius=radius, kept_by_radius_filter=kept_r.len(), kept_by_statistical_filter=kept_s.len())
        kept_r.free(), kept_s.free()
        out[name] = res
        hosts.append(cloud.download()[0])
    ctx.close()
    # the k = 8 call's forms, on the diagnostics build
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    for (name, radius), pts in zip(SHAPES, hosts):
        cloud = DevicePointCloud(diag, PointCloud(pts))
        case = Case(diag, cloud)

        def form(knob=None, value=None):
            def fn():
                for k in ("A3D_OUTLIERS_K", "A3D_OUTLIERS_SELECT"):
                    os.environ.pop(k, None)
                if knob:
                    os.environ[knob] = value
                case.knn(radius, 8)
            return fn
        res = measure(diag, [("product_form", form()), ("widest_array_K32", form("A3D_OUTLIERS_K", "32")),
                             ("select_on_t", form("A3D_OUTLIERS_SELECT", "t"))])
        form()()
        for other in ("widest_array_K32", "select_on_t"):
            res[f"{other}_over_product_form"] = round(res[other]["median"] / res["product_form"]["median"], 3)
        out[name]["k8_kernel_forms_diagnostics_build"] = res
        case.free(), cloud.free()
    diag.close()
    if parent:
        out["gate_against_the_parent_build"] = gate(parent)
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
