#!/usr/bin/env python3
"""A map from a recorded sequence without leaving the device:
    python examples/pcl_map.py [tests/golden/rgbd/sample1] [--max-frames N]
        [--voxel V [--mean] [--online [--check-batch | --window-box R | --window-frames W] [--render-track]]] [--colors]
        [--estimate-normals R] [--remove-plane T] [--radius-outliers R N] [--stat-outliers R K A] [--clusters R M S]
        [--tsdf-track V [--tsdf-direct] [--tsdf-mesh FILE]] [--out map.npy]
examples/pcl_odometry.py plus the last step: frames -> RangeImageBuilder (one batched build) ->
DevicePointCloud.from_range_images (one pass) -> IcpBatch over the consecutive pairs -> TrajectoryBuilder, and then the
camera-to-world poses go into DevicePointCloud.merge(clouds, poses): every frame's cloud in world coordinates, back to
back in one resident cloud (one launch).  With --voxel V the map is then thinned to one point per V-sized cell
(DevicePointCloud.voxel_downsample: still on the device) and the last frame is aligned against the thinned map with Icp,
frame to map.  With --mean on the offline route (merge -> voxel_downsample(mode="mean")) a second map is made from the
same merged cloud, the centroid of each cell with its mean normal and mean colour instead of one picked sample, and the
figures printed for the nearest-point map are printed for it as well, side by side.  With --online the thinned map is built the way a live caller would, frame by frame into a persistent
DeviceVoxelMap (insert per frame, one extract at the end) instead of merge + voxel_downsample of everything: no merged
cloud exists at any time, and the lines it prints are the same; the last frame is then corrected against the live map
itself (DeviceVoxelMap.align from its odometry pose: no extract, no kd-tree build, the frame in its own coordinates), and
the correction printed is that alignment relative to the odometry pose (the map's association is not the kd-tree's, so
its figures differ from the batch path's).  --online --mean makes the live map a map of cell means
(DeviceVoxelMap(mode="mean"): running integer sums per cell; everything else, the windows and --render-track included, runs
unchanged on it, and a window then keeps a cell by its mean row and by the age of its FIRST point).  --check-batch runs the
batch path as well, only to assert that the two maps are the same bits (with --mean: the bits of
voxel_downsample(mode="mean")).  --window-box R and --window-frames W keep the online map LOCAL, the way
an odometry loop that runs for hours must: after each insert DeviceVoxelMap.retain drops the cells outside the box of
half-side R (metres) around the current camera position, or the cells whose point is older than the last W frames
(frame boundaries are recorded as total() and carried through every retain by its `marks`).  A retain also renumbers the
cells, so total(), printed per frame beside the cell count, stays bounded instead of running towards 2^32.  --colors carries
every point's RGB colour from the frames through whichever of these paths is selected (merge, voxel_downsample, the online
map and its retains: a colour follows its point and decides nothing), and --out then also writes <out>_colors.npy ([N, 3]
u8) beside the points.  --render-track (with --online; it carries the colours too) is frame-to-model tracking the way
KinectFusion does it: before frame k goes in, the live map is rendered (DeviceVoxelMap.render, radius V / 2, the frame's
intrinsics and size) at the pose the odometry predicts, the corrected pose of frame k - 1 times the pair's alignment;
pyramid(3) of that image is the target of a MultiscaleAlign, point-to-plane and intensity terms, whose source is the
frame's own pyramid; the frame is inserted under the corrected pose, and the mean distance of the camera positions from
the dataset's trajectory is printed with and without the correction.  --estimate-normals R treats the frames as clouds
from a sensor without a pixel grid: every frame's cloud drops its image normals and takes normals estimated from its own
points within R metres (DevicePointCloud.estimate_normals_many, the viewpoint at the frame's camera) before anything is
aligned; with --render-track the model that is rendered is then the map's extract with its normals refreshed from the
map's own neighbourhood (estimate_normals(3 V, orient="normals"): one raw sensor normal per cell otherwise), and the
trajectory errors printed are those of this variant.  --radius-outliers R N and --stat-outliers R K A clean each frame's
cloud before it goes into the map, whichever route builds it (the odometry still aligns the full clouds): the first drops
the rows with fewer than N rows within R metres, themselves counted (DevicePointCloud.remove_radius_outliers_many), the
second the rows whose mean distance to their K nearest others within R lies more than A standard deviations above the
frame's mean (remove_statistical_outliers_many); with both, the radius filter runs first.  The flying pixels at depth edges
and isolated returns then never own a cell of the map.  --clusters R M S runs after them and drops what they keep, the
floating clumps: the rows that are noise or belong to a cluster of fewer than S rows under DBSCAN with radius R and
min_points M (DevicePointCloud.remove_small_clusters_many; M = 1 is PCL's Euclidean cluster extraction with a minimum size).
--remove-plane T runs before all of them: each frame's dominant plane (the floor, a wall or a table top: the rows within T
metres of the best of 1000 candidate planes, DevicePointCloud.remove_plane_many, one segment call and one select call for
all frames) stays out of the map, and the cluster filter then sees objects instead of one connected room.  --tsdf-track V
runs the --render-track loop against a dense model instead, on its own (no --voxel needed): every frame is fused into a
DeviceTsdfVolume of voxel size V (truncation 4 V, with colours) that encloses the first frame's cloud with half a metre to
spare, the model image is raycast from it at the predicted pose (samples every 2 V), and the same mean-trajectory-error
line is printed; the map that follows is built from the odometry poses as without it.  --tsdf-direct replaces the
correction step by DeviceTsdfVolume.align(clouds[k], IcpParams.default(), initial=pose), the frame's cloud against the
distance field itself: no raycast, no pyramid and no MultiscaleAlign, and the same line is printed for this route.
--tsdf-mesh FILE then takes the
fused volume's surface out as a triangle mesh (DeviceTsdfVolume.extract_triangle_mesh, observed at least twice) and as a
point cloud (extract_point_cloud), prints their counts and saves points, normals, colors and faces to FILE as an .npz (file
formats such as PLY are out of scope).  The map is downloaded once, for its bounding box; prints the point count and the box, and --out writes the points ([N, 3] f32)."""
import argparse
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from align3d_amd import (A3dError, Context, DevicePointCloud, DeviceTsdfVolume, DeviceVoxelMap, Icp, IcpBatch,  # noqa: E402
                         IcpParams, MsIcpParams, MultiscaleAlign, RangeImageBuilder, SlamTbDataset, Transform, TrajectoryBuilder)

ap = argparse.ArgumentParser()
ap.add_argument("dataset", nargs="?", default=os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
ap.add_argument("--max-frames", type=int, default=None)
ap.add_argument("--voxel", type=float, default=None, help="thin the map to one point per cell of this size (metres)")
ap.add_argument("--mean", action="store_true",
                help="with --voxel: also thin the merged cloud to each cell's mean and print both maps' figures; with --online: "
                     "the live map is a map of cell means")
ap.add_argument("--online", action="store_true", help="with --voxel: build the thinned map by inserting frame by frame")
ap.add_argument("--check-batch", action="store_true",
                help="with --online: also run merge + voxel_downsample and assert that the online map is the same bits")
ap.add_argument("--window-box", type=float, default=None, metavar="R",
                help="with --online: after each insert keep only the cells within R metres (per axis) of the camera")
ap.add_argument("--window-frames", type=int, default=None, metavar="W",
                help="with --online: after each insert keep only the cells whose point came with the last W frames")
ap.add_argument("--render-track", action="store_true",
                help="with --online: correct each frame's pose against a rendering of the live map before it is inserted")
ap.add_argument("--colors", action="store_true", help="carry the frames' RGB colours into the map")
ap.add_argument("--estimate-normals", type=float, default=None, metavar="R",
                help="replace every frame's image normals by normals estimated from the cloud itself within R metres "
                     "(with --render-track the rendered model's normals are refreshed too, within 3 V whatever R is)")
ap.add_argument("--remove-plane", type=float, default=None, metavar="T",
                help="before a frame's cloud goes into the map (and before the filters below), drop its dominant plane: the rows "
                     "within T metres of the best of 1000 candidate planes")
ap.add_argument("--radius-outliers", nargs=2, type=float, default=None, metavar=("R", "N"),
                help="before a frame's cloud goes into the map, drop its rows with fewer than N rows within R metres")
ap.add_argument("--stat-outliers", nargs=3, type=float, default=None, metavar=("R", "K", "A"),
                help="before a frame's cloud goes into the map, drop its rows whose mean distance to their K nearest others "
                     "within R metres is more than A standard deviations above the frame's mean")
ap.add_argument("--clusters", nargs=3, type=float, default=None, metavar=("R", "M", "S"),
                help="before a frame's cloud goes into the map, drop the noise and the clusters of fewer than S rows of DBSCAN "
                     "with radius R metres and min_points M")
ap.add_argument("--tsdf-track", type=float, default=None, metavar="V",
                help="correct each frame's pose against a raycast of a TSDF volume of voxel size V that the frames are fused into")
ap.add_argument("--tsdf-direct", action="store_true",
                help="with --tsdf-track: align each frame's cloud against the volume's distance field itself, without a raycast")
ap.add_argument("--tsdf-mesh", default=None, metavar="FILE",
                help="with --tsdf-track: save the fused volume's surface (points, normals, colors, faces) to this .npz file")
ap.add_argument("--out", default=None, help="write the map's points to this .npy file (with --colors: and <out>_colors.npy)")
args = ap.parse_args()
if args.online and not args.voxel:
    ap.error("--online needs --voxel")
if args.mean and not args.voxel:
    ap.error("--mean needs --voxel")
if args.check_batch and not args.online:
    ap.error("--check-batch needs --online")
windowed = args.window_box is not None or args.window_frames is not None
if windowed and not args.online:
    ap.error("--window-box and --window-frames need --online")
if windowed and args.check_batch:
    ap.error("--check-batch compares whole maps: not with --window-box or --window-frames")
if args.window_frames is not None and args.window_frames < 1:
    ap.error("--window-frames keeps at least one frame")
if args.render_track and not args.online:
    ap.error("--render-track needs --online")
if args.render_track and args.check_batch:
    ap.error("--check-batch compares maps built under the same poses: not with --render-track")
if args.tsdf_mesh and args.tsdf_track is None:
    ap.error("--tsdf-mesh needs --tsdf-track")
if args.tsdf_direct and args.tsdf_track is None:
    ap.error("--tsdf-direct needs --tsdf-track")
args.colors = args.colors or args.render_track  # (the intensity term reads the map's colours)

ctx = Context(0)
ds = SlamTbDataset.load(args.dataset)
frames = [ds.get(i) for i in range(min(ds.len(), args.max_frames or ds.len()))]
cam, _, _, depth_scale = frames[0]
builder = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False)
if args.render_track or args.tsdf_track is not None:  # the frames are also the sources of the frame-to-model alignment: three levels, with intensities
    builder = RangeImageBuilder(ctx).pyramid_levels(3)
built = builder.build_many(cam, [(f[1], f[2]) for f in frames], depth_scale)
images = [pyramid[0] for pyramid in built]
coarser = [level for pyramid in built for level in pyramid[1:]]
clouds = DevicePointCloud.from_range_images(images, colors=args.colors)  # frame k's cloud, resident
if args.estimate_normals is not None:  # in each camera's own frame: the viewpoint is the origin
    valid = DevicePointCloud.estimate_normals_many(clouds, args.estimate_normals)
    print(f"estimated normals within {args.estimate_normals} m: {sum(valid)} of {sum(c.len() for c in clouds)} rows valid")
# pair k: frame k + 1 (source) onto frame k (target)
batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
poses, status = batch.align(clouds[1:])
traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)  # frame 0 is the world
camera_to_world = [traj.current_camera_to_world()]
for k, (now_to_previous, st) in enumerate(zip(poses, status)):
    if st != 0:
        print(f"pair {k} <- {k + 1}: solve failed (status {st}); frame {k + 1} keeps frame {k}'s pose")
    else:
        traj.accumulate(now_to_previous, float(k + 1))
    camera_to_world.append(traj.current_camera_to_world())



def mean_error(truth, estimate):
    """Mean distance of the estimated camera positions from the dataset's trajectory, frame 0 as the world."""
    origin = truth.camera_to_world[0].inverse()
    return float(np.mean([np.linalg.norm(e.t - (origin * truth.camera_to_world[i]).t) for i, e in enumerate(estimate)]))


if args.tsdf_track is not None:  # frame-to-model tracking against a dense model: fuse, raycast, align, fuse
    first = clouds[0].download()[0]
    first = first[np.isfinite(first).all(axis=1)]
    lo, hi = first.min(axis=0) - 0.5, first.max(axis=0) + 0.5  # frame 0 is the world
    dims = np.clip(np.ceil((hi - lo) / args.tsdf_track).astype(np.int64) + 1, 2, 1024)
    volume = DeviceTsdfVolume(ctx, dims, args.tsdf_track, lo, colors=True)
    z_far = float(hi[2])
    corrected = []
    for k, image in enumerate(images):
        pose = camera_to_world[0]
        if k > 0:
            pose = corrected[-1] * poses[k - 1] if status[k - 1] == 0 else corrected[-1]  # the odometry's prediction
        if k > 0 and args.tsdf_direct:  # the frame's cloud against the field itself, from the predicted pose
            try:
                pose = volume.align(clouds[k], IcpParams.default(), initial=pose)
            except A3dError as e:
                print(f"frame {k}: no correction against the volume's field ({e})")
        elif k > 0:
            model = volume.raycast(cam, pose, 0.3, z_far).pyramid(3)
            try:
                aligner = MultiscaleAlign.new(ctx, MsIcpParams.default(), model)
                pose = pose * aligner.align(built[k])
                aligner.free()
            except A3dError as e:
                print(f"frame {k}: no correction against the raycast volume ({e})")
            for level in model:
                level.free()
        corrected.append(pose)
        volume.integrate(image, pose)
    print(f"tsdf volume {tuple(int(d) for d in dims)} voxels of {args.tsdf_track} m")
    truth = ds.trajectory()
    if truth is not None:
        route = "the volume's field" if args.tsdf_direct else "the raycast volume"
        print(f"mean trajectory error over {len(corrected)} frames: odometry alone {mean_error(truth, camera_to_world):.4e} m, "
              f"corrected against {route} {mean_error(truth, corrected):.4e} m")
    if args.tsdf_mesh:  # the surface of what was fused, independent of any viewpoint
        mesh, surface = volume.extract_triangle_mesh(min_weight=2), volume.extract_point_cloud(min_weight=2)
        print(f"tsdf surface (observed at least twice): mesh of {mesh.len_vertices} vertices and {mesh.len_faces} triangles, "
              f"point cloud of {surface.len()} points")
        np.savez(args.tsdf_mesh, **mesh.download())
        mesh.free(), surface.free()
    volume.free()

# what goes into the map: the frames' clouds, cleaned if asked for (one plane, knn or cluster call and one select call per filter,
# all frames)
map_clouds = clouds
for name, spec in (("plane", args.remove_plane), ("radius", args.radius_outliers), ("statistical", args.stat_outliers),
                   ("cluster", args.clusters)):
    if spec is None:
        continue
    if name == "plane":
        cleaned = DevicePointCloud.remove_plane_many(map_clouds, spec)
    elif name == "radius":
        cleaned = DevicePointCloud.remove_radius_outliers_many(map_clouds, spec[0], int(spec[1]))
    elif name == "statistical":
        cleaned = DevicePointCloud.remove_statistical_outliers_many(map_clouds, spec[0], int(spec[1]), spec[2])
    else:
        cleaned = DevicePointCloud.remove_small_clusters_many(map_clouds, spec[0], int(spec[1]), int(spec[2]))
    print(f"{name} {'removal' if name == 'plane' else 'outlier filter'} {spec}: {sum(c.len() for c in map_clouds)} rows -> "
          f"{sum(c.len() for c in cleaned)}")
    if map_clouds is not clouds:
        for c in map_clouds:
            c.free()
    map_clouds = cleaned


mean_map = None  # --mean: the map of cell means, beside the nearest-point map


def thinned_by_batch():
    """(points offered, thinned map): all frames in one coordinate system, then one point per cell."""
    global mean_map
    full = DevicePointCloud.merge(map_clouds, camera_to_world)
    if args.online and args.mean:  # --check-batch of a live map of means: the batch call it must equal
        thin = full.voxel_downsample(args.voxel, mode="mean")
    else:
        thin = full.voxel_downsample(args.voxel)
        if args.mean:
            mean_map = full.voxel_downsample(args.voxel, mode="mean")
    offered = full.len()
    full.free()
    return offered, thin


if args.online:
    online = DeviceVoxelMap(ctx, args.voxel, normals=map_clouds[0].d_normals is not None, colors=args.colors,
                            mode="mean" if args.mean else "nearest")
    offered = 0
    starts = collections.deque()  # --window-frames: the first sequence number of each kept frame, in the map's numbering
    corrected = []  # --render-track: the poses the frames went in under
    for k, (cloud, pose) in enumerate(zip(map_clouds, camera_to_world)):  # what a live caller does as each frame arrives
        if args.render_track:
            if k > 0:
                pose = corrected[-1] * poses[k - 1] if status[k - 1] == 0 else corrected[-1]  # the odometry's prediction
                if args.estimate_normals is not None:
                    snapshot = online.extract()  # the model's normals from the model's own neighbourhood
                    snapshot.estimate_normals(3 * args.voxel, orient="normals")
                    model = snapshot.render(cam, pose, radius=args.voxel / 2).pyramid(3)
                    snapshot.free()
                else:
                    model = online.render(cam, pose, radius=args.voxel / 2).pyramid(3)
                try:
                    aligner = MultiscaleAlign.new(ctx, MsIcpParams.default(), model)
                    pose = pose * aligner.align(built[k])  # (the frame in the rendered camera's frame, then in the world)
                    aligner.free()
                except A3dError as e:
                    print(f"frame {k}: no correction against the rendered map ({e})")
                for level in model:
                    level.free()
            corrected.append(pose)
        if args.window_frames is not None:
            starts.append(online.total())
        online.insert(cloud, pose)
        offered += cloud.len()
        if args.window_box is not None:
            centre = pose.translation()
            _, marks = online.retain(box=(centre - np.float32(args.window_box), centre + np.float32(args.window_box)),
                                     marks=np.asarray(starts, np.uint64))
            starts = collections.deque(marks.tolist())
        if args.window_frames is not None:
            while len(starts) > args.window_frames:
                starts.popleft()
            _, marks = online.retain(min_seq=starts[0], marks=np.asarray(starts, np.uint64))  # starts[0] becomes 0
            starts = collections.deque(marks.tolist())
        if windowed:
            print(f"frame {k}: {online.cells()} cells, total {online.total()} (offered so far: {offered})")
    if args.render_track:
        truth = ds.trajectory()
        if truth is not None:
            print(f"mean trajectory error over {len(corrected)} frames: odometry alone {mean_error(truth, camera_to_world):.4e} m, "
                  f"corrected against the rendered map {mean_error(truth, corrected):.4e} m")
    # frame to map against the LIVE map: no extract, no kd-tree, and the frame stays in its own coordinates: the map's
    # association (DeviceVoxelMap.nearest) takes the tree's place and the alignment starts from the odometry pose
    aligned = online.align(clouds[-1], IcpParams.default(), initial=camera_to_world[-1])
    correction = aligned * camera_to_world[-1].inverse()
    world_map = online.extract()
    online.free()
    if args.check_batch:  # the batch path, for this comparison only
        _, batch_map = thinned_by_batch()
        same = batch_map.len() == world_map.len() and all(
            a is None and b is None or np.array_equal(a.view(np.uint32), b.view(np.uint32))
            for a, b in zip(batch_map.download(), world_map.download()))
        assert same, "the online map differs from merge + voxel_downsample" + (' (mode="mean")' if args.mean else "")
        if args.colors:
            assert np.array_equal(batch_map.download_colors(), world_map.download_colors()), "the maps' colours differ"
        batch_map.free()
elif args.voxel:
    offered, world_map = thinned_by_batch()
else:
    world_map = DevicePointCloud.merge(map_clouds, camera_to_world)  # the last step: all frames in one coordinate system
if args.voxel:
    print(f"voxel {args.voxel}{' (a live map of cell means)' if args.online and args.mean else ''}: {offered} points -> "
          f"{world_map.len()}")
    if not args.online:
        # frame to map: the last frame, brought to the world by its odometry pose, against the thinned map; what Icp
        # returns is the correction the map asks of that pose
        last = camera_to_world[-1] * clouds[-1]
        icp = Icp(ctx, IcpParams.default(), world_map)
        correction = icp.align(last)
        icp.free(), last.free()
    print(f"last frame against the thinned map: correction angle {correction.angle():.3e} rad, "
          f"translation {float(np.linalg.norm(correction.t)):.3e}")
    if mean_map is not None:  # the same figures for the map of cell means
        last = camera_to_world[-1] * clouds[-1]
        icp = Icp(ctx, IcpParams.default(), mean_map)
        mean_correction = icp.align(last)
        icp.free(), last.free()
        print(f"voxel {args.voxel} (cell means): {offered} points -> {mean_map.len()}")
        print(f"last frame against the map of cell means: correction angle {mean_correction.angle():.3e} rad, "
              f"translation {float(np.linalg.norm(mean_correction.t)):.3e}")
points, _ = world_map.download()
finite = points[np.isfinite(points).all(axis=1)]
print(f"{len(clouds)} frames, map of {world_map.len()} points" + (" with normals" if world_map.d_normals is not None else "")
      + (" and colours" if world_map.has_colors() else ""))
if len(finite):
    print("bounding box: min", finite.min(axis=0).tolist(), "max", finite.max(axis=0).tolist())
if args.out:
    np.save(args.out, points)
    print("wrote", args.out)
    if args.colors:
        colors_out = os.path.splitext(args.out)[0] + "_colors.npy"
        np.save(colors_out, world_map.download_colors())
        print("wrote", colors_out)
batch.free()
for x in [world_map] + ([mean_map] if mean_map is not None else []) + clouds + images + coarser + (
        map_clouds if map_clouds is not clouds else []):
    x.free()
ctx.close()
