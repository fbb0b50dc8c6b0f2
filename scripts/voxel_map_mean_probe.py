"""The voxel map of cell means (DeviceVoxelMap(mode="mean")) beside the nearest-point map and beside the batch route it
replaces, in one job.  Prints one JSON line (and writes it to argv[1] if given: profiles/voxel_map_mean_probe.json).

    python scripts/voxel_map_mean_probe.py [out.json] [--parent DIR] [--no-tracking]

The inputs are those of the other map probes: the 20 frames of sample1 (5.4 M points) under their odometry poses, v = 0.02.
(a) insert of the last frame (270 k points) into the map of the 19 frames before it, a map of means beside a
    nearest-point map; each timed insert starts from the same state, which an untimed clear + insert of the map's rows
    restores.
(b) extract of the whole map and (c) a compaction of it, both kinds.
(d) the route the mean map replaces: merge(all 20 frames).voxel_downsample(mode="mean"), which a caller without the map
    repeats for every frame added.
(e) 270 k points into ONE cell, the worst case for the atomics, both kinds.
(f) the mean insert of (a) with and without run combining, both in the diagnostics build (the knob lives only there).
(g) bytes per slot of every configuration.
The gate (--parent DIR: a directory that holds the align3d_amd package of the parent commit, built): the figures of the
NEAREST-point map for insert, extract and compaction are taken in child processes, this build and the parent's in turn,
and this build's median must not exceed the largest window the parent showed.  The mean map's own times are recorded,
not gated.  Tracking (unless --no-tracking): examples/pcl_map.py --voxel 0.02 --online --render-track on sample1 with and
without --mean; the mean trajectory error of each run and of the odometry alone."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = os.environ.get("A3D_PROBE_PACKAGE_ROOT", ROOT)  # (a child of the gate imports the parent's package)
sys.path.insert(0, PACKAGE_ROOT)
sys.path.insert(1, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceVoxelMap, PointCloud, _abi  # noqa: E402
from voxel_downsample_probe import odometry_poses, sample1_clouds, spread  # noqa: E402

WINDOWS = 5
CALLS = 10
VOXEL = 0.02


def measure(ctx, variants):
    """variants: [(name, fn, before or None)] -> {name: spread of ms per call}: every call between two device events of
    its own (a call is host-synchronous), `before` untimed; the windows of the variants alternate."""
    def window(fn, before):
        ms = 0.0
        for _ in range(CALLS):
            if before:
                before()
            ctx.timer_start()
            fn()
            ms += ctx.timer_stop()
        return ms / CALLS
    for _, fn, before in variants:
        for _ in range(2):
            if before:
                before()
            fn()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(WINDOWS):
        for name, fn, before in variants:
            ms[name].append(window(fn, before))
    return {name: dict(spread(v), calls_per_window=CALLS) for name, v in ms.items()}


class Filled:
    """A map of the first 19 frames, and the calls on it that are timed."""

    def __init__(self, ctx, clouds, poses, **kw):
        self.ctx, self.m = ctx, DeviceVoxelMap(ctx, VOXEL, **kw)
        for c, t in zip(clouds[:-1], poses[:-1]):
            self.m.insert(c, t)
        self.cells = self.m.cells()
        self.rows = self.m.extract()
        self.restore()
        self.last, self.pose = clouds[-1], poses[-1]
        self.buf = DevicePointCloud._allocate(ctx, 2 * self.cells, True)
        self.n_out = C.c_uint64()

    def insert(self):
        self.m.insert(self.last, self.pose)

    def restore(self):
        """Back to the cells of the 19 frames, as voxel_map_retain_probe.py restores its state: clear, then the map's
        rows go in as one cloud (cells = total; the allocation stays).  (In a map of means every cell then holds one
        point: the cells that the next insert finds and opens are the same, and so is its work.)"""
        self.m.clear()
        self.m.insert(self.rows)
        assert abs(self.m.cells() - self.cells) <= self.cells // 100  # (a mean may have rounded onto its cell's face)

    def extract(self):
        st = self.ctx.lib.a3d_voxel_map_extract(self.m.handle, self.buf.d_points, self.buf.d_normals, None, 2 * self.cells,
                                                C.byref(self.n_out))
        assert st == 0, st

    def compact(self):
        assert self.m.compact() == 0

    def variants(self, tag):
        return [(f"insert_frame_{tag}", self.insert, self.restore), (f"extract_{tag}", self.extract, None),
                (f"compaction_{tag}", self.compact, None)]

    def free(self):
        self.buf.free(), self.rows.free(), self.m.free()


def nearest_only():
    """The gate's child: the nearest-point map's three figures with whatever package PACKAGE_ROOT holds."""
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    f = Filled(ctx, clouds, poses)
    out = measure(ctx, f.variants("nearest"))
    out["map_cells"] = f.cells
    f.free()
    for c in clouds:
        c.free()
    ctx.close()
    print("NEAREST_ONLY " + json.dumps(out))


def gate(parent):
    """This build and the parent's in turn, two child processes each."""
    runs = {"this": [], "parent": []}
    for _ in range(2):
        for who, root in (("this", ROOT), ("parent", os.path.abspath(parent))):
            env = dict(os.environ, A3D_PROBE_PACKAGE_ROOT=root)
            env.pop("A3D_LIBRARY", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--nearest-only"], env=env, capture_output=True,
                               text=True, timeout=300)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("NEAREST_ONLY ")), None)
            assert p.returncode == 0 and line, (who, p.returncode, p.stderr[-2000:])
            runs[who].append(json.loads(line[len("NEAREST_ONLY "):]))
    out = {"runs": runs, "holds": True}
    for name in ("insert_frame_nearest", "extract_nearest", "compaction_nearest"):
        this = float(np.median([r[name]["median"] for r in runs["this"]]))
        parent_max = max(r[name]["max"] for r in runs["parent"])
        parent_min = min(r[name]["min"] for r in runs["parent"])
        ok = this <= parent_max
        out[name] = {"this_median": round(this, 4), "parent_min": parent_min, "parent_max": parent_max, "inside": ok}
        out["holds"] = out["holds"] and ok
    return out


def tracking():
    """Mean trajectory errors (m) of examples/pcl_map.py --voxel 0.02 --online --render-track, nearest and mean."""
    out = {}
    for name, extra in (("nearest", []), ("mean", ["--mean"])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pcl_map.py"), "--voxel", str(VOXEL), "--online",
                            "--render-track"] + extra, capture_output=True, text=True, timeout=600)
        m = re.search(r"mean trajectory error over (\d+) frames: odometry alone (\S+) m, corrected against the rendered map (\S+) m",
                      p.stdout)
        assert p.returncode == 0 and m, (name, p.returncode, p.stdout[-1000:], p.stderr[-2000:])
        out[name] = {"frames": int(m.group(1)), "odometry_alone_m": float(m.group(2)), "corrected_m": float(m.group(3))}
    return out


def main():
    args = sys.argv[1:]
    if "--nearest-only" in args:
        return nearest_only()
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    out_path = next((a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")), None)
    ctx = Context(0)
    clouds = sample1_clouds(ctx)
    poses = odometry_poses(ctx, clouds)
    out = {"probe": "voxel_map_mean", "windows": WINDOWS, "voxel": VOXEL, "frames": len(clouds),
           "points": sum(c.len() for c in clouds), "frame_points": clouds[-1].len()}
    nearest, mean = Filled(ctx, clouds, poses), Filled(ctx, clouds, poses, mode="mean")
    assert nearest.cells == mean.cells
    out["map_cells_before_the_frame"] = mean.cells
    out["device_ms"] = measure(ctx, nearest.variants("nearest") + mean.variants("mean"))
    out["slots"] = mean.m.stats()["slots"]
    nearest.free(), mean.free()

    # (d) the batch route, per frame added
    def batch_route():
        full = DevicePointCloud.merge(clouds, poses)
        thin = full.voxel_downsample(VOXEL, mode="mean")
        full.free(), thin.free()
    out["device_ms"].update(measure(ctx, [("merge_all_frames_then_voxel_mean", batch_route, None)]))
    # (e) one cell
    n = clouds[-1].len()
    rng = np.random.default_rng(1)
    one = DevicePointCloud(ctx, PointCloud((3.0 + rng.uniform(0.05, 0.95, size=(n, 3))).astype(np.float32) * np.float32(VOXEL),
                                           np.tile(np.float32([0.0, 0.0, 1.0]), (n, 1))))
    singles = {mode: DeviceVoxelMap(ctx, VOXEL, mode=mode, reserve_cells=n) for mode in ("nearest", "mean")}
    out["device_ms"].update(measure(ctx, [(f"insert_{n}_points_into_one_cell_{mode}", (lambda m=m: m.insert(one)), m.clear)
                                          for mode, m in singles.items()]))
    assert all(m.cells() == 1 for m in singles.values())
    for m in singles.values():
        m.free()
    one.free()
    # (g) (a new map allocates nothing on the device)
    out["bytes_per_slot"] = {}
    for mode in ("nearest", "mean"):
        for normals in (False, True):
            for colors in (False, True):
                m = DeviceVoxelMap(ctx, VOXEL, normals=normals, colors=colors, mode=mode)
                out["bytes_per_slot"][f"{mode}{', normals' if normals else ''}{', colours' if colors else ''}"] = m.bytes_per_slot()
                m.free()
    for c in clouds:
        c.free()
    ctx.close()
    # (f) run combining, in the diagnostics build
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    clouds = sample1_clouds(diag)
    f = Filled(diag, clouds, poses, mode="mean")

    def knob(value):
        def set_it():
            os.environ["A3D_VOXEL_MAP_MEAN_NO_COMBINE"] = value
            f.restore()
        return set_it
    out["device_ms_diagnostics_build"] = measure(diag, [("insert_frame_mean_runs_combined", f.insert, knob("0")),
                                                        ("insert_frame_mean_not_combined", f.insert, knob("1"))])
    os.environ.pop("A3D_VOXEL_MAP_MEAN_NO_COMBINE", None)
    f.free()
    for c in clouds:
        c.free()
    diag.close()
    if parent:
        out["nearest_point_gate"] = gate(parent)
    if "--no-tracking" not in args:
        out["tracking_sample1"] = tracking()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
