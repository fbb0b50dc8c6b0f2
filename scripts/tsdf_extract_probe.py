"""The TSDF surface extraction (a3d_tsdf_volume_extract_surface) timed in one job.
    python scripts/tsdf_extract_probe.py [profiles/tsdf_extract_probe.json] [--parent-library PATH]
Prints one JSON line (and writes it to the path given).  Shapes: the sample1 sequence (640 x 480) fused at its odometry
poses into a 256^3 volume with colours at v = 0.02 (truncation 4 v), the volume of scripts/tsdf_probe.py.
(a) raw calls on preallocated outputs: count-only (mesh and cloud forms), the cloud form and the mesh form with normals and
    colours, beside a device-to-device copy of the volume's bytes (8 per voxel: the count pass reads the records once; and
    12, with the colour plane);
(b) the wrappers a user calls: extract_point_cloud() (count, allocate, extract) beside raycast() + from_range_image() from
    the last pose: the two ways from a fused volume to a cloud with normals and colours;
(c) the vertex and triangle counts;
(d) with --parent-library (libalign3d_hip.so of the parent commit): integrate of one frame, raycast at 640 x 480 and
    DeviceVoxelMap.render on this build and on the parent's, in alternating windows (and alternating order);
    `within_parent_range` says whether this build's median lies inside the parent's own min-max range,
    `at_most_parent_max` whether it is at least not above it.
Every timed call is host-synchronous and lies between two device events on the context's stream, averaged over a window of
calls; the windows of the variants of a group alternate; median and extremes over the windows are kept."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import Context, DevicePointCloud, DeviceTsdfVolume, DeviceVoxelMap, _abi  # noqa: E402
from tsdf_probe import DIMS, ORIGIN, VOXEL, WARMUP, WINDOWS, Z_NEAR, load_frames, measure  # noqa: E402
from voxel_downsample_probe import odometry_poses, spread  # noqa: E402

NEW_SYMBOLS = ("a3d_tsdf_volume_extract_surface", "a3d_tsdf_volume_upload")


def parent_context(path):
    """A context on a library that predates the new entries: loaded without asking for them."""
    held = {name: _abi.SIGNATURES.pop(name) for name in NEW_SYMBOLS}
    try:
        _abi.load_library(path)
    finally:
        _abi.SIGNATURES.update(held)
    return Context(0, library=path)


def fused_volume(ctx, images, poses):
    volume = DeviceTsdfVolume(ctx, DIMS, VOXEL, ORIGIN, colors=True)
    volume.integrate_many(images, poses)
    return volume


def shared_calls(ctx, cam, images, clouds, poses):
    """(d): entries the parent build has too, as raw calls."""
    lib = ctx.lib
    volume = fused_volume(ctx, images, poses)
    m = DeviceVoxelMap(ctx, VOXEL, normals=True, colors=True)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    pose = poses[-1]
    c2w, inv = pose.to_c(), pose.inverse().to_c()
    one = (C.c_void_p * 1)(images[-1].handle)
    z_far, step = ORIGIN[2] + DIMS[2] * VOXEL, 2 * VOXEL
    handle = C.c_void_p()

    def integrate():
        assert lib.a3d_tsdf_volume_integrate(volume.handle, one, C.byref(inv), 1) == 0

    def raycast():
        st = lib.a3d_tsdf_volume_raycast(volume.handle, C.byref(c2w), cam.fx, cam.fy, cam.cx, cam.cy, 640, 480, Z_NEAR, z_far, step,
                                         C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    def map_render():
        st = lib.a3d_voxel_map_render(m.handle, C.byref(inv), cam.fx, cam.fy, cam.cx, cam.cy, 640, 480, VOXEL / 2, None,
                                      C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    return [("integrate_1_frame_colours", integrate), ("raycast_640x480", raycast), ("voxel_map_render_640x480", map_render)], \
        (volume, m)


def main():
    args = sys.argv[1:]
    parent_path = None
    if "--parent-library" in args:
        k = args.index("--parent-library")
        parent_path = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    out_path = next((a for a in args if not a.startswith("--")), None)
    ctx = Context(0)
    lib = ctx.lib
    cam, images, clouds = load_frames(ctx)
    poses = odometry_poses(ctx, clouds)
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    out = {"probe": "tsdf_extract", "windows": WINDOWS, "voxel": VOXEL, "dims": DIMS, "origin": ORIGIN, "frames": len(images),
           "one_job_on_one_box": True}

    volume = fused_volume(ctx, images, poses)
    nv, nf = C.c_uint64(), C.c_uint64()

    def counts(want_faces):
        assert lib.a3d_tsdf_volume_extract_surface(volume.handle, 1, want_faces, None, None, None, 0, None, 0, C.byref(nv),
                                                   C.byref(nf)) == 0
        return int(nv.value), int(nf.value)

    mesh_vertices, mesh_faces = counts(1)
    cloud_vertices, _ = counts(0)
    out["counts"] = {"mesh_vertices": mesh_vertices, "mesh_triangles": mesh_faces, "cloud_points": cloud_vertices}
    D, W, _ = volume.download()
    out["voxels_observed"] = int((W > 0).sum())
    del D, W

    # ---- (a): raw calls
    vertices = DevicePointCloud._allocate(ctx, mesh_vertices, True, True)
    d_faces = ctx.malloc(max(1, mesh_faces) * 12)
    src, dst = ctx.malloc(voxels * 12), ctx.malloc(voxels * 12)

    def extract(want_faces, vcap, fcap):
        def call():
            st = lib.a3d_tsdf_volume_extract_surface(volume.handle, 1, want_faces, vertices.d_points, vertices.d_normals,
                                                     vertices.d_colors, vcap, d_faces if want_faces else None, fcap, C.byref(nv),
                                                     C.byref(nf))
            assert st == 0, st
        return call

    def copy_of(nbytes):
        def call():
            _abi.check(lib.a3d_memcpy_d2d(ctx.handle, dst, src, nbytes), "a3d_memcpy_d2d")
            ctx.synchronize()  # (the entries under test are host-synchronous: the copy is timed the same way)
        return call

    ms = measure(ctx, [("count_only_mesh", lambda: counts(1)), ("count_only_cloud", lambda: counts(0)),
                       ("extract_cloud", extract(0, cloud_vertices, 0)), ("extract_mesh", extract(1, mesh_vertices, mesh_faces)),
                       ("copy_volume_bytes_8_per_voxel", copy_of(voxels * 8)),
                       ("copy_volume_bytes_12_per_voxel", copy_of(voxels * 12))], calls=10)
    out["extract_ms"] = ms
    copy8 = ms["copy_volume_bytes_8_per_voxel"]["median"]
    out["over_copy_of_the_records"] = {name: round(ms[name]["median"] / copy8, 2)
                                       for name in ("count_only_mesh", "count_only_cloud", "extract_cloud", "extract_mesh")}
    ctx.free(src), ctx.free(dst), ctx.free(d_faces)
    vertices.free()

    # ---- (b): the wrappers
    pose = poses[-1]
    z_far, step = ORIGIN[2] + DIMS[2] * VOXEL, 2 * VOXEL
    seen = {}

    def wrapper_cloud():
        cloud = volume.extract_point_cloud()
        seen["extract_point_cloud"] = cloud.len()
        cloud.free()

    def wrapper_mesh():
        mesh = volume.extract_triangle_mesh()
        mesh.free()

    def raycast_cloud():
        image = volume.raycast(cam, pose, Z_NEAR, z_far, step)
        cloud = DevicePointCloud.from_range_image(image, colors=True)
        seen["raycast_from_range_image"] = cloud.len()
        cloud.free(), image.free()

    ms = measure(ctx, [("extract_point_cloud", wrapper_cloud), ("extract_triangle_mesh", wrapper_mesh),
                       ("raycast_plus_from_range_image", raycast_cloud)], calls=10)
    out["wrapper_ms"] = ms
    out["wrapper_points"] = seen
    out["extract_point_cloud_over_raycast_cloud"] = round(
        ms["extract_point_cloud"]["median"] / ms["raycast_plus_from_range_image"]["median"], 2)
    volume.free()

    # ---- (d): entries the parent build has, on both builds
    if parent_path:
        pctx = parent_context(parent_path)
        _, pimages, pclouds = load_frames(pctx)
        this_calls, this_keep = shared_calls(ctx, cam, images, clouds, poses)
        parent_calls, parent_keep = shared_calls(pctx, cam, pimages, pclouds, poses)
        for _, fn in this_calls + parent_calls:
            for _ in range(WARMUP):
                fn()
        rows = {}
        for (name, fn), (_, pfn) in zip(this_calls, parent_calls):
            this_ms, parent_ms = [], []
            for window in range(WINDOWS):
                sides = ((pctx, pfn, parent_ms), (ctx, fn, this_ms))
                for side_ctx, side_fn, acc in (sides if window % 2 == 0 else sides[::-1]):  # (neither build always goes second)
                    side_ctx.timer_start()
                    for _ in range(20):
                        side_fn()
                    acc.append(side_ctx.timer_stop() / 20)
            t, p = spread(this_ms), spread(parent_ms)
            rows[name] = {"this": t, "parent": p, "within_parent_range": bool(p["min"] <= t["median"] <= p["max"]),
                          "at_most_parent_max": bool(t["median"] <= p["max"]),
                          "this_over_parent_median": round(t["median"] / p["median"], 4)}
        out["against_parent_ms"] = rows
        for keep in (this_keep, parent_keep):
            for x in keep:
                x.free()
        for x in pimages + pclouds:
            x.free()
        pctx.close()
    for x in images + clouds:
        x.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
