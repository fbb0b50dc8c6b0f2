"""IcpBatch (a3d_pcl_icp_batch_*) against the loop it replaces — a3d_pcl_icp_new_device + a3d_pcl_icp_align_device per
pair — on resident clouds: P = 8, 32, 64 pairs of 640x480 range-image clouds (align3d_amd/synth.py frame_stream, seeded,
built on the device and converted with from_range_images) and P = 4 pairs of 500 k x 500 k uniform points (the
benches/bench_icp.rs shape), 15 iterations.  After a warm-up the two forms alternate REPS times.  Prints one JSON line
(and writes it to argv[1] if given).

Per form and P: "new + align" is a host clock round the whole of it (the loop's ends in its last host-synchronous align,
the batch's in its result read); "align only" is device time, the sum of a3d_pcl_icp_last_device_ms over the loop's
pairs and a3d_pcl_icp_batch_last_device_ms.  spread = (max - min) / median over the repetitions.

Bytes per iteration of a pair, from shapes as DESIGN.md counts the one-pair iteration (252 B per source
point = 12 + 12 point and normal, 204 of the query, 12 + 12 target point and normal; 126 MB at 500 k x 500 k); the
split table is read from LDS / L2 and not counted.

With --sweep (the diagnostics library: the geometry knobs exist only there) the batch's align device time is also
measured for the alternatives of the blocks-per-pair / LDS-levels rule at P = 32."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from align3d_amd import (Context, DevicePointCloud, Icp, IcpBatch, IcpParams, PointCloud, RangeImageBuilder,  # noqa: E402
                         _abi)
from align3d_amd import synth  # noqa: E402

HBM_BYTES_PER_S = 8e12
REPS = 5
ITERATIONS = 15


def stats(xs):
    m = statistics.median(xs)
    return {"median": round(m, 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round((max(xs) - min(xs)) / m, 4)}


def uniform_cloud(seed, n):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3), dtype=np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return PointCloud(pts, nrm)


def loop_form(ctx, prm, targets, sources):
    t0 = time.perf_counter()
    dev_ms, poses = 0.0, []
    for t, s in zip(targets, sources):
        icp = Icp.new(ctx, prm, t)
        try:
            poses.append(icp.align(s))
        except _abi.A3dError as e:  # a pair whose solve fails still did its work
            if e.status != _abi.A3D_SOLVE_FAILED:
                raise
            poses.append(None)
        dev_ms += icp.last_device_ms()
        icp.free()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, dev_ms, poses


def batch_form(ctx, prm, targets, sources):
    t0 = time.perf_counter()
    batch = IcpBatch(ctx, prm, targets)
    poses, status = batch.align(sources)
    dev_ms = batch.last_device_ms()
    batch.free()  # inside the clock, as the loop's frees are
    wall = (time.perf_counter() - t0) * 1e3
    return wall, dev_ms, poses, status


def compare(ctx, prm, targets, sources):
    P = len(targets)
    loop_form(ctx, prm, targets, sources), batch_form(ctx, prm, targets, sources)  # warm-up
    lw, ld, bw, bd = [], [], [], []
    for _ in range(REPS):
        w, d, lposes = loop_form(ctx, prm, targets, sources)
        lw.append(w), ld.append(d)
        w, d, bposes, status = batch_form(ctx, prm, targets, sources)
        bw.append(w), bd.append(d)
    worst = 0.0
    for a, b in zip(lposes, bposes):
        if a is not None:
            worst = max(worst, float(np.max(np.abs(np.asarray(list(a.to_c().t) + list(a.to_c().q)) -
                                                   np.asarray(list(b.to_c().t) + list(b.to_c().q))))))
    nbytes = sum(252 * s.len() for s in sources)
    bdm, ldm = statistics.median(bd), statistics.median(ld)
    return {
        "pairs": P, "source_points": sum(s.len() for s in sources), "target_points": sum(t.len() for t in targets),
        "failed_pairs": int(np.count_nonzero(status)),
        "loop_new_align_wall_ms": stats(lw), "batch_new_align_wall_ms": stats(bw),
        "loop_align_device_ms": stats(ld), "batch_align_device_ms": stats(bd),
        "loop_pairs_per_s": round(P / (statistics.median(lw) * 1e-3), 1),
        "batch_pairs_per_s": round(P / (statistics.median(bw) * 1e-3), 1),
        "speedup_new_align": round(statistics.median(lw) / statistics.median(bw), 3),
        "speedup_align_only": round(ldm / bdm, 3),
        "bytes_per_iteration": nbytes,
        "batch_fraction_of_8TBs": round(nbytes * ITERATIONS / (bdm * 1e-3) / HBM_BYTES_PER_S, 4),
        "loop_fraction_of_8TBs": round(nbytes * ITERATIONS / (ldm * 1e-3) / HBM_BYTES_PER_S, 4),
        "max_abs_pose_component_difference_loop_vs_batch": worst,
    }


def image_clouds(ctx, n_frames):
    frames, _ = synth.frame_stream(7, n_frames)
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(synth.camera(), frames,
                                                                                      synth.DEPTH_SCALE)
    images = [p[0] for p in built]
    clouds = DevicePointCloud.from_range_images(images)
    for im in images:
        im.free()
    return clouds


def sweep_child(p_pairs):
    """Runs in a child process on the diagnostics library with the geometry knobs in its environment."""
    ctx = Context(0, library=_abi.DIAG_LIB_PATH)
    clouds = image_clouds(ctx, 17)
    targets = [clouds[i % 16] for i in range(p_pairs)]
    sources = [clouds[i % 16 + 1] for i in range(p_pairs)]
    prm = IcpParams(max_iterations=ITERATIONS)
    batch = IcpBatch(ctx, prm, targets)
    batch.align(sources)
    ms = []
    for _ in range(REPS):
        batch.align(sources)
        ms.append(batch.last_device_ms())
    batch.free()
    ctx.close()
    print(json.dumps(stats(ms)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--sweep-child":
        return sweep_child(int(sys.argv[2]))
    out = {"probe": "pcl_icp_batch", "iterations": ITERATIONS, "reps": REPS}
    ctx = Context(0)
    prm = IcpParams(max_iterations=ITERATIONS)
    clouds = image_clouds(ctx, 17)
    out["image_cloud_points"] = [c.len() for c in clouds[:4]]
    for P in (8, 32, 64):
        targets = [clouds[i % 16] for i in range(P)]
        sources = [clouds[i % 16 + 1] for i in range(P)]
        out[f"image_clouds_P{P}"] = compare(ctx, prm, targets, sources)
    for c in clouds:
        c.free()
    big = [DevicePointCloud(ctx, uniform_cloud(100 + i, 500000)) for i in range(8)]
    out["uniform_500k_P4"] = compare(ctx, prm, big[:4], big[4:])
    for c in big:
        c.free()
    ctx.close()
    if "--sweep" in sys.argv:  # fresh processes: the knobs are read when a batch is created, the library is another
        sweep = {}
        for name, env in (("block1024_levels15_1perCU (the rule)", {}),
                          ("block1024_levels15_2perCU", {"A3D_PCLB_BLOCKS_PER_CU": "2"}),
                          ("block512_levels14_2perCU", {"A3D_PCLB_BLOCK": "512", "A3D_PCLB_LDS_LEVELS": "14", "A3D_PCLB_BLOCKS_PER_CU": "2"}),
                          ("block512_levels13_4perCU", {"A3D_PCLB_BLOCK": "512", "A3D_PCLB_LDS_LEVELS": "13", "A3D_PCLB_BLOCKS_PER_CU": "4"}),
                          ("block256_levels12_8perCU", {"A3D_PCLB_BLOCK": "256", "A3D_PCLB_LDS_LEVELS": "12", "A3D_PCLB_BLOCKS_PER_CU": "8"})):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-child", "32"], env={**os.environ, **env},
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:  # a failed variant ends the sweep: nothing more is started on the GPU
                sweep[name] = {"error": r.returncode, "stderr": r.stderr[-400:]}
                break
            sweep[name] = json.loads(r.stdout.strip().splitlines()[-1])
        out["geometry_sweep_P32_batch_align_device_ms"] = sweep
    line = json.dumps(out)
    print(line)
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    if paths:
        with open(paths[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
