"""Why so few points of a real frame pass the gates of DeviceTsdfVolume.align: per frame of sample1 (frames 1, 10 and 19
under their odometry poses, against the 256^3 volume at v = 0.02 fused from the whole sequence), how many points have a
direction, how many lie within max_distance, how many pass the angle gate, and the quantiles of the dot product between
the frame's image normals and the field's gradient, and of |d|.
    python scripts/tsdf_icp_gate_stats.py [profiles/tsdf_icp_gate_stats.json]
Prints one JSON line (and writes it to the path given).  Nothing is timed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceTsdfVolume, IcpParams  # noqa: E402
from tsdf_icp_probe import DIMS, ORIGIN, VOXEL, load_frames  # noqa: E402
from voxel_downsample_probe import odometry_poses  # noqa: E402


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    cam, built = load_frames(ctx, 1)
    images = [p[0] for p in built]
    clouds = DevicePointCloud.from_range_images(images, colors=True)
    poses = odometry_poses(ctx, clouds)
    vol = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN, colors=True)
    vol.integrate_many(images, poses)
    prm = IcpParams.default()
    out = {"max_distance": prm.max_distance, "max_normal_angle": prm.max_normal_angle}
    for k in (1, 10, 19):
        frame, pose = clouds[k], poses[k]
        d, n = vol.sample(frame, pose)
        world = pose * frame
        sn = world.download()[1]
        world.free()
        has = np.any(n != 0, axis=1)
        dot = (sn * n).sum(axis=1)[has]
        dd = d[has]
        out[k] = {"points": len(d), "direction": int(has.sum()),
                  "within_distance": int((dd * dd <= prm.max_distance ** 2).sum()),
                  "dot_above_cos_angle": int((dot > np.cos(prm.max_normal_angle)).sum()),
                  "dot_quantiles": np.quantile(dot, [0.05, 0.25, 0.5, 0.75, 0.95]).round(3).tolist(),
                  "abs_d_quantiles": np.quantile(np.abs(dd), [0.25, 0.5, 0.75, 0.95]).round(4).tolist(),
                  "finite_source_normals": int(np.isfinite(sn).all(axis=1).sum()),
                  "count": vol.accumulate(frame, prm, pose)["count"]}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
