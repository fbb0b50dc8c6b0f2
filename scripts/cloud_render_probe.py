"""Rendering resident clouds and the voxel map into range images (a3d_point_cloud_render_device, a3d_voxel_map_render),
timed in one job.  Prints one JSON line (and writes it to argv[1] if given: profiles/cloud_render_probe.json).

The shapes are those of the other voxel-map probes: the sample1 sequence, its last frame's cloud (with normals and
colours) and the map of the whole sequence at v = 0.02 built one insert per frame under the odometry poses.
(a) the frame cloud into 640 x 480 under its own camera, radius 0;
(b) the map at the last frame's pose into 640 x 480 at radius 0.01, and into 160 x 120 with the intrinsics scaled by 0.25;
(c) (a) and (b) with both splat forms, on the diagnostics build (A3D_CLOUD_RENDER_SPLAT: 0 the atomic alone, 1 the load
    that skips it);
(d) the whole frame-to-model step, map.render + pyramid(3) + MultiscaleAlign.new + align of the frame's own builder
    pyramid, beside DeviceVoxelMap.align of the same frame's cloud (15 iterations, started from the same pose); with it,
    untimed, what that aligner is given (the rendered model against the frame's own image, pixel by pixel) and the
    correction each route returns.
Every render is a raw call whose image is freed inside the span (its arena goes back to the context's pool: no hipMalloc
in a steady stream).  Each variant is timed between two device events on the context's stream (a call is
host-synchronous, so the span holds its waits), averaged over a window of calls; the windows of the variants alternate;
median and extremes over the windows are kept.  Each render is also given as a multiple of a device-to-device copy of its
output image's bytes (28 per pixel with normals and colours), timed in the same windows."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from align3d_amd import (Context, DevicePointCloud, DeviceVoxelMap, IcpParams, ImageIcp, MsIcpParams,  # noqa: E402
                         MultiscaleAlign, RangeImageBuilder, SlamTbDataset, Transform, _abi)
from voxel_downsample_probe import odometry_poses, spread  # noqa: E402

WINDOWS = 7
CALLS = 20
WARMUP = 3
VOXEL = 0.02
RADIUS = 0.01
BYTES_PER_PIXEL = 12 + 1 + 12 + 3


def load_frames(ctx):
    """(camera, depth scale, [(depth, rgb)], clouds with normals and colours) of the sample1 sequence."""
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    frames = [ds.get(i) for i in range(ds.len())]
    cam, _, _, depth_scale = frames[0]
    pairs = [(f[1], f[2]) for f in frames]
    built = RangeImageBuilder(ctx).pyramid_levels(1).build_many(cam, pairs, depth_scale)
    images = [p[0] for p in built]
    clouds = DevicePointCloud.from_range_images(images, colors=True)
    for im in images:
        im.free()
    return cam, depth_scale, pairs, clouds


def build_map(ctx, clouds, poses):
    m = DeviceVoxelMap(ctx, VOXEL, normals=True, colors=True)
    for c, t in zip(clouds, poses):
        m.insert(c, t)
    return m


def measure(ctx, variants, calls=CALLS):
    for _, fn in variants:
        for _ in range(WARMUP):
            fn()
    ms = {name: [] for name, _ in variants}
    for _ in range(WINDOWS):
        for name, fn in variants:
            ctx.timer_start()
            for _ in range(calls):
                fn()
            ms[name].append(ctx.timer_stop() / calls)
    return {name: dict(spread(v), calls_per_window=calls) for name, v in ms.items()}


def render_calls(ctx, cam, frame, m, pose):
    """The three timed renders of (a) and (b) as raw calls, and the copies they are measured against."""
    lib = ctx.lib
    view, w2c = frame.view(), pose.inverse().to_c()
    small = cam.scale(0.25)
    handle = C.c_void_p()

    def frame_640():
        st = lib.a3d_point_cloud_render_device(ctx.handle, C.byref(view), frame.d_colors, None, cam.fx, cam.fy, cam.cx, cam.cy,
                                               640, 480, 0.0, None, C.byref(handle))
        assert st == 0, st
        lib.a3d_range_image_free(handle)

    def map_at(k, w, h):
        def call():
            st = lib.a3d_voxel_map_render(m.handle, C.byref(w2c), k.fx, k.fy, k.cx, k.cy, w, h, RADIUS, None, C.byref(handle))
            assert st == 0, st
            lib.a3d_range_image_free(handle)
        return call

    return [("frame_cloud_640x480_radius_0", frame_640), ("map_640x480_radius_0.01", map_at(cam, 640, 480)),
            ("map_160x120_radius_0.01", map_at(small, 160, 120))]


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    ctx = Context(0)
    cam, depth_scale, pairs, clouds = load_frames(ctx)
    assert (cam.width, cam.height) == (640, 480)
    poses = odometry_poses(ctx, clouds)
    m = build_map(ctx, clouds, poses)
    frame, pose = clouds[-1], poses[-1]
    out = {"probe": "cloud_render", "windows": WINDOWS, "voxel": VOXEL, "radius": RADIUS, "frames": len(clouds),
           "map_cells": m.cells(), "frame_points": frame.len(), "bytes_per_pixel": BYTES_PER_PIXEL}

    # ---- (a), (b): the product library, beside the copies of the outputs' bytes
    big, small = 640 * 480 * BYTES_PER_PIXEL, 160 * 120 * BYTES_PER_PIXEL
    src, dst = ctx.malloc(big), ctx.malloc(big)

    def copy_of(nbytes):
        def call():
            _abi.check(ctx.lib.a3d_memcpy_d2d(ctx.handle, dst, src, nbytes), "a3d_memcpy_d2d")
        return call

    renders = render_calls(ctx, cam, frame, m, pose)
    ms = measure(ctx, renders + [("copy_640x480_image_bytes", copy_of(big)), ("copy_160x120_image_bytes", copy_of(small))])
    out["render_ms"] = ms
    out["render_over_copy"] = {
        name: round(ms[name]["median"] / ms["copy_160x120_image_bytes" if "160x120" in name else "copy_640x480_image_bytes"]["median"], 2)
        for name, _ in renders}
    image, index = m.render(cam, pose, RADIUS, return_index=True)
    out["map_640x480_pixels_covered"] = int((index != 0xFFFFFFFF).sum())
    image.free()
    image, index = frame.render(cam, None, 0.0, return_index=True)
    out["frame_640x480_pixels_covered"] = int((index != 0xFFFFFFFF).sum())
    image.free()

    def splat_forms():
        # ---- (c): both splat forms, diagnostics build, its own context and its own copies of the inputs
        diag = Context(0, library=_abi.DIAG_LIB_PATH)
        _, _, _, dclouds = load_frames(diag)
        dm = build_map(diag, dclouds, poses)
        variants = []
        for form, name in (("0", "atomic"), ("1", "checked")):
            for label, fn in render_calls(diag, cam, dclouds[-1], dm, pose):
                def call(fn=fn, form=form):
                    os.environ["A3D_CLOUD_RENDER_SPLAT"] = form
                    fn()
                variants.append((f"{label}/{name}", call))
        out["splat_forms_ms"] = measure(diag, variants)
        os.environ.pop("A3D_CLOUD_RENDER_SPLAT", None)
        dm.free()
        for c in dclouds:
            c.free()
        diag.close()

    def frame_to_model():
        # ---- (d): the frame-to-model step beside the map's own align
        builder = RangeImageBuilder(ctx).pyramid_levels(3)
        src_pyr = builder.build(cam, *pairs[-1], depth_scale)
        ms_prm, icp_prm = MsIcpParams.default(), IcpParams(max_iterations=15)
        last = {}

        def render_track():
            model = m.render(cam, pose, RADIUS)
            pyr = model.pyramid(3)
            aligner = MultiscaleAlign.new(ctx, ms_prm, pyr)
            last["render_track"] = aligner.align(src_pyr)
            aligner.free()
            for lv in pyr:
                lv.free()

        def map_align():
            last["map_align"] = m.align(frame, icp_prm, initial=pose)

        step = measure(ctx, [("render_pyramid_multiscale_align", render_track), ("voxel_map_align", map_align)], calls=10)
        out["frame_to_model_ms"] = step
        out["render_track_over_map_align"] = round(step["render_pyramid_multiscale_align"]["median"] / step["voxel_map_align"]["median"], 2)
        # the correction each asks of the odometry pose (the render route aligns in the camera's frame: its pose IS the correction)
        via_map = last["map_align"] * pose.inverse()
        # what the aligner is given: the rendered model beside the frame's own image, pixel by pixel, at the pose the frame
        # went into the map with, and the pixels each term accepts at level 0 from the identity
        model = m.render(cam, pose, RADIUS)
        mh, fh = model.download(intensity=False), src_pyr[0].download()
        both = (mh.mask != 0) & (fh.mask != 0)
        dots = np.sum(mh.normals * fh.normals, -1)[both]
        g, c = ImageIcp(ctx, ms_prm.pyramid[0], model.compute_intensity()).accumulate(src_pyr[0], Transform.eye())
        g_self, _ = ImageIcp(ctx, ms_prm.pyramid[0], src_pyr[0]).accumulate(src_pyr[0], Transform.eye())
        out["model_against_frame"] = {
            "pixels_valid_in_both": int(both.sum()),
            "median_abs_depth_difference_m": round(float(np.median(np.abs(mh.points[..., 2] - fh.points[..., 2])[both])), 5),
            "fraction_normals_within_18_degrees": round(float((dots > np.cos(np.pi / 10)).mean()), 4),
            "level0_accepted_geometric": int(g["count"]), "level0_accepted_colour": int(c["count"]),
            "level0_accepted_geometric_frame_on_itself": int(g_self["count"])}
        model.free()
        # the same step without the intensity term (colour weight 0), once, for its pose only: the rendered model is a mosaic
        # of footprints, each of one colour, so what the intensity term sees of it is worth knowing apart
        try:
            model = m.render(cam, pose, RADIUS).pyramid(3)
            aligner = MultiscaleAlign.new(ctx, MsIcpParams.default().customize(lambda i, p: setattr(p, "color_weight", 0.0)), model)
            geometry_only = aligner.align(src_pyr)
            aligner.free()
            for lv in model:
                lv.free()
            out["correction_geometry_only"] = {"angle": float(geometry_only.angle()),
                                               "translation": float(np.linalg.norm(geometry_only.t))}
        except Exception as e:  # noqa: BLE001
            out["correction_geometry_only"] = f"{type(e).__name__}: {e}"
        out["correction"] = {
            "render_track": {"angle": float(last["render_track"].angle()), "translation": float(np.linalg.norm(last["render_track"].t))},
            "map_align": {"angle": float(via_map.angle()), "translation": float(np.linalg.norm(via_map.t))}}

        for lv in src_pyr:
            lv.free()

    for part in (splat_forms, frame_to_model):  # (a part that raises is named in the output; the others still count)
        try:
            part()
        except Exception as e:  # noqa: BLE001
            out[part.__name__ + "_error"] = f"{type(e).__name__}: {e}"
    ctx.free(src), ctx.free(dst)
    m.free()
    for c in clouds:
        c.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
