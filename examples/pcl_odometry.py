#!/usr/bin/env python3
"""Point-cloud odometry over a recorded sequence without leaving the device:
    python examples/pcl_odometry.py [tests/golden/rgbd/sample1] [--max-frames N]
frames -> RangeImageBuilder (one batched build) -> DevicePointCloud.from_range_images (one pass) -> IcpBatch over the
consecutive pairs (one launch per iteration for all of them) -> TrajectoryBuilder.  Prints the pairs that failed, the
device time of the alignment and the last camera-to-world pose."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from align3d_amd import (Context, DevicePointCloud, IcpBatch, IcpParams, RangeImageBuilder, SlamTbDataset,  # noqa: E402
                         TrajectoryBuilder)

ap = argparse.ArgumentParser()
ap.add_argument("dataset", nargs="?", default=os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
ap.add_argument("--max-frames", type=int, default=None)
args = ap.parse_args()

ctx = Context(0)
ds = SlamTbDataset.load(args.dataset)
frames = [ds.get(i) for i in range(min(ds.len(), args.max_frames or ds.len()))]
cam, _, _, depth_scale = frames[0]
built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(cam, [(f[1], f[2]) for f in frames],
                                                                                  depth_scale)
images = [pyramid[0] for pyramid in built]
clouds = DevicePointCloud.from_range_images(images)  # frame k's cloud, resident
# pair k: frame k + 1 (source) onto frame k (target)
batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
poses, status = batch.align(clouds[1:])
traj = TrajectoryBuilder()
for k, (now_to_previous, st) in enumerate(zip(poses, status)):
    if st != 0:
        print(f"pair {k} <- {k + 1}: solve failed (status {st}); its transform is left out")
        continue
    traj.accumulate(now_to_previous, float(k + 1))
print(f"{len(poses)} pairs, {sum(c.len() for c in clouds)} points, alignment {batch.last_device_ms():.3f} ms on the device")
print("last camera-to-world:", traj.current_camera_to_world())
batch.free()
for x in clouds + images:
    x.free()
ctx.close()
