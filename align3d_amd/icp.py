"""ImageIcp, MultiscaleAlign, Icp — the reference's alignment API (src/icp/*.rs) over the C ABI."""
import ctypes as C
import types

import numpy as np

from . import _abi
from .icp_params import IcpParams, MsIcpParams
from .range_image import CameraIntrinsics, DeviceRangeImage, RangeImage, upload_pyramid
from .transform import Transform


def _dev(ctx, image):
    if isinstance(image, DeviceRangeImage):
        return image
    if isinstance(image, RangeImage):
        return image.device(ctx)
    raise TypeError("expected a RangeImage or DeviceRangeImage")


def _dev_pyramid(ctx, images):
    """Device copies of a pyramid; host RangeImages that are not resident yet go up in ONE call sharing one arena."""
    images = list(images)
    missing = [im for im in images if isinstance(im, RangeImage) and (im._device is None or im._device.ctx is not ctx)]
    if len(missing) > 1:
        upload_pyramid(ctx, missing)
    return [_dev(ctx, im) for im in images]


def _handle_array(images):
    arr = (C.c_void_p * max(1, len(images)))()
    for i, im in enumerate(images):
        arr[i] = im.handle
    return arr


class ImageIcp:
    """ImageIcp (src/icp/image_icp.rs:19-165)."""

    def __init__(self, ctx, params, target):
        self.ctx = ctx
        self.params = params
        self.target = _dev(ctx, target)
        self.initial_transform = Transform.eye()

    @staticmethod
    def new(ctx, params, target):
        return ImageIcp(ctx, params, target)

    def align(self, source, trace=False):
        src = _dev(self.ctx, source)
        p = self.params.to_c()
        init = self.initial_transform.to_c()
        out = _abi.PoseC()
        if trace:
            tr = np.zeros((int(self.params.max_iterations), 8), np.float32)
            _abi.check(
                self.ctx.lib.a3d_image_icp_align_trace(self.ctx.handle, C.byref(p), self.target.handle, src.handle,
                                                       C.byref(init), C.byref(out), _abi.ptr(tr)),
                "ImageIcp::align",
            )
            return Transform.from_c(out), tr
        _abi.check(
            self.ctx.lib.a3d_image_icp_align(self.ctx.handle, C.byref(p), self.target.handle, src.handle,
                                             C.byref(init), C.byref(out)),
            "ImageIcp::align",
        )
        return Transform.from_c(out)

    def accumulate(self, source, transform):
        """One pass of the pixel loop from `transform`: (geom, colour) accumulators (test hook)."""
        src = _dev(self.ctx, source)
        p = self.params.to_c()
        t = transform.to_c()
        g, c = _abi.GnStateC(), _abi.GnStateC()
        _abi.check(
            self.ctx.lib.a3d_image_icp_accumulate(self.ctx.handle, C.byref(p), self.target.handle, src.handle,
                                                  C.byref(t), C.byref(g), C.byref(c)),
            "ImageIcp accumulate",
        )
        return g.as_dict(), c.as_dict()

    def accumulate_exact(self, source, transform):
        """The same pass through the cross-check kernel whose per-pixel arithmetic is the reference's operation for
        operation (a3d_image_icp_accumulate_exact, test hook)."""
        src = _dev(self.ctx, source)
        p, t = self.params.to_c(), transform.to_c()
        g, c = _abi.GnStateC(), _abi.GnStateC()
        _abi.check(
            self.ctx.lib.a3d_image_icp_accumulate_exact(self.ctx.handle, C.byref(p), self.target.handle, src.handle,
                                                        C.byref(t), C.byref(g), C.byref(c)),
            "ImageIcp accumulate_exact",
        )
        return g.as_dict(), c.as_dict()

    def accumulate_weighted(self, source, transform):
        """One pass of the opt-in merged accumulation (A3D_ICP_ACCUM=merged: a thread sums geom.add_weighted(color, w,
        cw) directly): the merged accumulator H, g, weighted residual sum, combined count (test hook)."""
        src = _dev(self.ctx, source)
        p, t, g = self.params.to_c(), transform.to_c(), _abi.GnStateC()
        _abi.check(
            self.ctx.lib.a3d_image_icp_accumulate_weighted(self.ctx.handle, C.byref(p), self.target.handle, src.handle,
                                                           C.byref(t), C.byref(g)),
            "ImageIcp accumulate_weighted",
        )
        return g.as_dict()


class MultiscaleAlign:
    """MultiscaleAlign (src/icp/multiscale.rs:7-68)."""

    def __init__(self, ctx, params, target_pyramid):
        self.ctx = ctx
        self.params = params
        self.targets = _dev_pyramid(ctx, target_pyramid)
        self.handle = C.c_void_p()
        parr = params.to_c_array()
        tarr = _handle_array(self.targets)
        st = ctx.lib.a3d_multiscale_new(ctx.handle, parr, len(params), tarr, len(self.targets), C.byref(self.handle))
        if st == _abi.A3D_INVALID_PARAMETER:
            # Err(A3dError::InvalidParameter(..)) (multiscale.rs:30-34)
            raise _abi.InvalidParameter(ctx.lib.a3d_last_error().decode())
        _abi.check(st, "MultiscaleAlign::new")

    @staticmethod
    def new(ctx, params, target_pyramid):
        return MultiscaleAlign(ctx, params, target_pyramid)

    def align(self, source_pyramid):
        source_pyramid = list(source_pyramid)
        out = _abi.PoseC()
        if source_pyramid and all(isinstance(im, RangeImage) and im._device is None for im in source_pyramid):
            # the reference's literal call: `&[RangeImage]` in host memory.  Uploaded and aligned in ONE call, the coarse
            # levels iterating under the upload of the fine ones (a3d_multiscale_align_host); nothing stays resident
            views = (_abi.RangeImageViewC * len(source_pyramid))(*[im.view() for im in source_pyramid])
            _abi.check(self.ctx.lib.a3d_multiscale_align_host(self.handle, views, len(source_pyramid), C.byref(out)),
                       "MultiscaleAlign::align")
            return Transform.from_c(out)
        srcs = _dev_pyramid(self.ctx, source_pyramid)
        _abi.check(self.ctx.lib.a3d_multiscale_align(self.handle, _handle_array(srcs), len(srcs), C.byref(out)),
                   "MultiscaleAlign::align")
        return Transform.from_c(out)

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.a3d_multiscale_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiscaleAlignBatch:
    """P independent MultiscaleAlign::new(params, target_p).align(source_p) in one launch sequence."""

    def __init__(self, ctx, params, target_pyramids, source_pyramids):
        assert len(target_pyramids) == len(source_pyramids) and len(target_pyramids) > 0
        self.ctx = ctx
        self.n_pairs = len(target_pyramids)
        self.n_levels = len(target_pyramids[0])
        self._keep = []
        t_flat, s_flat = [], []
        for tp, sp in zip(target_pyramids, source_pyramids):
            assert len(tp) == self.n_levels and len(sp) == self.n_levels
            t_flat += [_dev(ctx, t) for t in tp]
            s_flat += [_dev(ctx, s) for s in sp]
        self._keep = (t_flat, s_flat)
        self.handle = C.c_void_p()
        st = ctx.lib.a3d_multiscale_batch_new(ctx.handle, params.to_c_array(), len(params), self.n_pairs,
                                              self.n_levels, _handle_array(t_flat), _handle_array(s_flat),
                                              C.byref(self.handle))
        if st == _abi.A3D_INVALID_PARAMETER:
            raise _abi.InvalidParameter(ctx.lib.a3d_last_error().decode())
        _abi.check(st, "a3d_multiscale_batch_new")

    def rebind(self, target_pyramids, source_pyramids):
        """The same batch object on other pyramids (same pair / level counts): nothing is allocated or freed."""
        assert len(target_pyramids) == self.n_pairs and len(source_pyramids) == self.n_pairs
        t_flat, s_flat = [], []
        for tp, sp in zip(target_pyramids, source_pyramids):
            assert len(tp) == self.n_levels and len(sp) == self.n_levels
            t_flat += [_dev(self.ctx, t) for t in tp]
            s_flat += [_dev(self.ctx, s) for s in sp]
        _abi.check(self.ctx.lib.a3d_multiscale_batch_rebind(self.handle, _handle_array(t_flat), _handle_array(s_flat)),
                   "a3d_multiscale_batch_rebind")
        self._keep = (t_flat, s_flat)
        return self

    def align(self, matrices_device=None):
        """Runs all pairs; returns (list of Transform, int32 status array)."""
        poses = (_abi.PoseC * self.n_pairs)()
        status = np.zeros(self.n_pairs, np.int32)
        _abi.check(
            self.ctx.lib.a3d_multiscale_batch_align(self.handle, poses, matrices_device,
                                                    status.ctypes.data_as(C.POINTER(C.c_int32))),
            "a3d_multiscale_batch_align",
        )
        return [Transform.from_c(p) for p in poses], status

    def enqueue(self, matrices_device=None):
        """Enqueues one pass without synchronising the host."""
        _abi.check(self.ctx.lib.a3d_multiscale_batch_align(self.handle, None, matrices_device, None))

    def results(self):
        """(list of Transform, int32 status array) of the most recent pass: waits for that pass only, not for what
        was enqueued on the context since (another batch's pass)."""
        poses = (_abi.PoseC * self.n_pairs)()
        status = np.zeros(self.n_pairs, np.int32)
        _abi.check(self.ctx.lib.a3d_multiscale_batch_results(self.handle, poses,
                                                             status.ctypes.data_as(C.POINTER(C.c_int32))),
                   "a3d_multiscale_batch_results")
        return [Transform.from_c(p) for p in poses], status

    def set_profiling(self, on):
        _abi.check(self.ctx.lib.a3d_multiscale_batch_set_profiling(self.handle, 1 if on else 0))

    def last_timing(self):
        ms, n = C.c_float(), C.c_uint64()
        _abi.check(self.ctx.lib.a3d_multiscale_batch_last_timing(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def persistent_levels(self):
        """Bit mask of the levels the most recent align ran inside the persistent kernel."""
        m = C.c_uint32()
        _abi.check(self.ctx.lib.a3d_multiscale_batch_persistent_levels(self.handle, C.byref(m)))
        return int(m.value)

    def concurrency(self):
        """Number of pair groups whose launches run on separate streams at the same time."""
        n = C.c_uint32()
        _abi.check(self.ctx.lib.a3d_multiscale_batch_concurrency(self.handle, C.byref(n)))
        return n.value

    def last_kernel_ms(self):
        ms = C.c_float()
        _abi.check(self.ctx.lib.a3d_multiscale_batch_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def last_level_ms(self, level):
        """(sum of the per-pixel kernel's launch durations at `level` in the last pass, number of launches); profiling on."""
        ms, n = C.c_float(), C.c_uint32()
        _abi.check(self.ctx.lib.a3d_multiscale_batch_last_level_ms(self.handle, int(level), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def free(self):
        if self.handle and self.ctx.handle:  # a handle must not outlive its context
            self.ctx.lib.a3d_multiscale_batch_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PointCloud:
    """PointCloud (src/pointcloud.rs:8-12): points [N,3], optional normals, optional colours [N,3] u8 (RGB)."""

    def __init__(self, points, normals=None, colors=None):
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        if self.colors is not None and len(self.colors) != len(self.points):
            raise _abi.InvalidParameter(f"PointCloud: {len(self.points)} points but {len(self.colors)} colours")

    @staticmethod
    def from_range_image(im):
        """From<&RangeImage> for PointCloud (src/range_image/structure.rs:375-406): mask != 0, row-major; the colours
        pass the same mask when the image has them (structure.rs:392-398)."""
        m = im.mask.reshape(-1) != 0
        normals = None if im.normals is None else im.normals.reshape(-1, 3)[m]
        colors = getattr(im, "colors", None)
        colors = None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3)[m]
        return PointCloud(im.points.reshape(-1, 3)[m], normals, colors)

    def len(self):
        return len(self.points)

    def view(self):
        v = _abi.PointCloudViewC()
        v.points = _abi.ptr(self.points)
        v.normals = _abi.ptr(self.normals)
        v.len = len(self.points)
        return v


def _render(ctx, what, camera, camera_to_world, radius, return_index, call, name):
    """The part DevicePointCloud.render and DeviceVoxelMap.render share: argument types, the pose's inverse, the index
    plane's buffer and the new image's handle.  call(pose, camera, radius, d_index, out_handle) is the ABI entry."""
    if not isinstance(camera, CameraIntrinsics):
        raise TypeError(f"{what} takes a CameraIntrinsics (got {type(camera).__name__})")
    if camera_to_world is not None and not isinstance(camera_to_world, Transform):
        raise TypeError(f"{what}: camera_to_world is a Transform or None (got {type(camera_to_world).__name__})")
    w, h = camera.width, camera.height
    if w < 0 or h < 0:
        raise _abi.InvalidParameter(f"{what}: the camera's width and height are the image's size (got {w} x {h})")
    pose = None if camera_to_world is None else C.byref(camera_to_world.inverse().to_c())
    handle = C.c_void_p()
    d_index = None
    try:
        if return_index and 0 < w * h < 1 << 31:
            d_index = ctx.malloc(w * h * 4)
        _abi.check(call(pose, camera, float(radius), d_index, C.byref(handle)), name)
        image = DeviceRangeImage(ctx, handle=handle)
        if not return_index:
            return image
        try:
            return image, ctx.to_host(d_index, np.empty((h, w), np.uint32))
        except BaseException:
            image.free()
            raise
    finally:
        if d_index is not None:
            ctx.free(d_index)


class DevicePointCloud:
    """A PointCloud (src/pointcloud.rs:8-12) resident in HBM: points / normals [len][3] f32 on the context's GPU, for
    the device-pointer forms a3d_pcl_icp_new_device / a3d_pcl_icp_align_device (no PCIe traffic per call).  Colours, when
    the cloud has them, are [len][3] u8 in a buffer of their own (d_colors): a payload that merge, voxel_downsample and
    DeviceVoxelMap carry beside the point it belongs to; no ICP reads them."""

    d_colors = None  # (a cloud assembled field by field has no colours until it is given some)

    def __init__(self, ctx, cloud):
        self.ctx = ctx
        self.n = cloud.len()
        self.d_points = self.d_normals = self.d_colors = None
        try:
            self.d_points = ctx.to_device(cloud.points)
            self.d_normals = None if cloud.normals is None else ctx.to_device(cloud.normals)
            colors = getattr(cloud, "colors", None)
            if colors is not None:
                self.d_colors = ctx.to_device(colors) if self.n else ctx.malloc(1)
        except BaseException:
            self.free()
            raise

    @staticmethod
    def from_range_image(device_image, colors=False):
        """PointCloud::from(&RangeImage) (src/range_image/structure.rs:375-406) without leaving the device: the kept
        pixels (mask != 0) of a resident image, row-major, bit for bit (a3d_range_image_to_point_cloud).  The cloud has
        normals iff the image has them; it owns its buffers (`free()`).  colors=True also carries the kept pixels'
        colours (see from_range_images)."""
        return DevicePointCloud.from_range_images([device_image], colors=colors)[0]

    @staticmethod
    def from_range_images(images, colors=False):
        """from_range_image for resident images of one context in one pass (a3d_range_image_to_point_clouds).
        colors=True: every cloud also gets the colours of its kept pixels (a3d_range_image_to_point_clouds_rgb; an image
        without colours raises A3D_MISSING_FIELD).  The reference always copies the colours; here they are opt-in, so
        that callers who only align pay neither memory nor time for a field no ICP reads."""
        images = list(images)
        if not images:
            return []
        ctx = images[0].ctx
        n = len(images)
        clouds = []
        try:
            for im in images:
                h, w = im.shape
                c = DevicePointCloud.__new__(DevicePointCloud)
                c.ctx, c.n = ctx, 0
                c.d_points, c.d_normals, c.d_colors = None, None, None
                clouds.append(c)
                c.d_points = ctx.malloc(w * h * 12)
                c.d_normals = ctx.malloc(w * h * 12) if im.has_normals() else None
                c.d_colors = ctx.malloc(w * h * 3) if colors else None
            caps = (C.c_uint64 * n)(*[im.shape[0] * im.shape[1] for im in images])
            lens = (C.c_uint64 * n)()
            if colors:
                _abi.check(
                    ctx.lib.a3d_range_image_to_point_clouds_rgb(_handle_array(images), n,
                                                                (C.c_void_p * n)(*[c.d_points for c in clouds]),
                                                                (C.c_void_p * n)(*[c.d_normals for c in clouds]),
                                                                DevicePointCloud._colors_array(clouds), caps, lens),
                    "a3d_range_image_to_point_clouds_rgb",
                )
            else:
                _abi.check(
                    ctx.lib.a3d_range_image_to_point_clouds(_handle_array(images), n,
                                                            (C.c_void_p * n)(*[c.d_points for c in clouds]),
                                                            (C.c_void_p * n)(*[c.d_normals for c in clouds]), caps, lens),
                    "a3d_range_image_to_point_clouds",
                )
        except BaseException:
            for c in clouds:
                c.free()
            raise
        for c, k in zip(clouds, lens):
            c.n = int(k)
        return clouds

    @staticmethod
    def _allocate(ctx, n, with_normals, with_colors=False):
        """An uninitialised resident cloud of n points (at least one point's worth of memory, so that `d_normals is None`
        keeps meaning "no normals", and `d_colors is None` "no colours")."""
        c = DevicePointCloud.__new__(DevicePointCloud)
        c.ctx, c.n = ctx, int(n)
        c.d_points, c.d_normals, c.d_colors = None, None, None
        try:
            c.d_points = ctx.malloc(max(1, c.n) * 12)
            c.d_normals = ctx.malloc(max(1, c.n) * 12) if with_normals else None
            c.d_colors = ctx.malloc(max(1, c.n) * 3) if with_colors else None
        except BaseException:
            c.free()
            raise
        return c

    @staticmethod
    def _resident_batch(clouds, transforms, what):
        """(clouds, their shared context, PoseC array or None) for the a3d_point_clouds_* calls."""
        clouds = list(clouds)
        for c in clouds:
            if not isinstance(c, DevicePointCloud):
                raise TypeError(f"{what} takes DevicePointCloud (got {type(c).__name__}); there is no host fallback")
        ctx = clouds[0].ctx
        if any(c.ctx is not ctx for c in clouds):
            raise _abi.InvalidParameter(f"{what}: the clouds must share a context")
        poses = None
        if transforms is not None:
            transforms = list(transforms)
            if len(transforms) != len(clouds):
                raise _abi.InvalidParameter(f"{what}: {len(clouds)} clouds but {len(transforms)} transforms")
            poses = (_abi.PoseC * len(clouds))(*[t.to_c() for t in transforms])
        return clouds, ctx, poses

    @staticmethod
    def _views(clouds):
        return (_abi.PointCloudViewC * len(clouds))(*[c.view() for c in clouds])

    @staticmethod
    def _colors_array(clouds):
        """The array of colour pointers parallel to _views(clouds): NULL for a cloud without colours."""
        return (C.c_void_p * len(clouds))(*[c.d_colors for c in clouds])

    @staticmethod
    def transform_many(clouds, transforms):
        """[transforms[i] * clouds[i]] (&Transform * &PointCloud, src/pointcloud.rs:40-52) as new resident clouds, in ONE
        call and one launch (a3d_point_clouds_transform_device).  Each result has normals iff its input has them, and a
        copy of its input's colours (the reference clones them, pointcloud.rs:49: one device-to-device copy each)."""
        if transforms is None:
            raise TypeError("transform_many needs one Transform per cloud")
        clouds = list(clouds)
        if not clouds:
            return []
        clouds, ctx, poses = DevicePointCloud._resident_batch(clouds, transforms, "transform_many")
        n, outs = len(clouds), []
        try:
            for c in clouds:
                outs.append(DevicePointCloud._allocate(ctx, c.n, c.d_normals is not None, c.d_colors is not None))
            _abi.check(
                ctx.lib.a3d_point_clouds_transform_device(ctx.handle, DevicePointCloud._views(clouds), poses, n,
                                                          (C.c_void_p * n)(*[o.d_points for o in outs]),
                                                          (C.c_void_p * n)(*[o.d_normals for o in outs])),
                "a3d_point_clouds_transform_device",
            )
            for c, o in zip(clouds, outs):
                if c.d_colors is not None and c.n:
                    _abi.check(ctx.lib.a3d_memcpy_d2d(ctx.handle, o.d_colors, c.d_colors, c.n * 3), "a3d_memcpy_d2d")
        except BaseException:
            for o in outs:
                o.free()
            raise
        return outs

    def transformed(self, transform):
        """transform * self as a new resident cloud (normals iff this cloud has them)."""
        return DevicePointCloud.transform_many([self], [transform])[0]

    def transform_(self, transform):
        """self = transform * self, in place (every point is read before it is written); returns self.  Colours stay
        as they are."""
        pose = transform.to_c()
        v = self.view()
        _abi.check(
            self.ctx.lib.a3d_point_clouds_transform_device(self.ctx.handle, C.byref(v), C.byref(pose), 1,
                                                           (C.c_void_p * 1)(self.d_points),
                                                           (C.c_void_p * 1)(self.d_normals)),
            "a3d_point_clouds_transform_device",
        )
        return self

    @staticmethod
    def merge(clouds, transforms=None, normals=None, colors=None):
        """One resident cloud holding transforms[i] * clouds[i] back to back, cloud order then point order
        (a3d_point_clouds_merge_device): frames brought into one coordinate system, a valid target for Icp / IcpBatch.
        transforms=None concatenates bit for bit.  The result has normals when the non-empty clouds all have them and
        none when none has; a mix raises InvalidParameter unless normals=False asks for points only.  `colors` follows the
        same rule for the clouds' colours (a3d_point_clouds_merge_rgb_device)."""
        clouds = list(clouds)
        if not clouds:
            raise _abi.InvalidParameter("merge needs at least one cloud (an empty list has no context to allocate on)")
        clouds, ctx, poses = DevicePointCloud._resident_batch(clouds, transforms, "merge")
        if normals is None:
            have = {c.d_normals is not None for c in clouds if c.n > 0} or {c.d_normals is not None for c in clouds}
            if len(have) > 1:
                raise _abi.InvalidParameter("merge: some clouds have normals and some do not (normals=False merges the points only)")
            normals = have.pop()
        if colors is None:
            have = {c.d_colors is not None for c in clouds if c.n > 0} or {c.d_colors is not None for c in clouds}
            if len(have) > 1:
                raise _abi.InvalidParameter("merge: some clouds have colours and some do not (colors=False merges without them)")
            colors = have.pop()
        total = sum(c.n for c in clouds)
        out = DevicePointCloud._allocate(ctx, total, bool(normals), bool(colors))
        try:
            n_out = C.c_uint64()
            if colors:
                _abi.check(
                    ctx.lib.a3d_point_clouds_merge_rgb_device(ctx.handle, DevicePointCloud._views(clouds),
                                                              DevicePointCloud._colors_array(clouds), poses, len(clouds),
                                                              out.d_points, out.d_normals, out.d_colors, total,
                                                              C.byref(n_out)),
                    "a3d_point_clouds_merge_rgb_device",
                )
            else:
                _abi.check(
                    ctx.lib.a3d_point_clouds_merge_device(ctx.handle, DevicePointCloud._views(clouds), poses, len(clouds),
                                                          out.d_points, out.d_normals, total, C.byref(n_out)),
                    "a3d_point_clouds_merge_device",
                )
        except BaseException:
            out.free()
            raise
        out.n = int(n_out.value)
        return out

    @staticmethod
    def _voxel_downsample(clouds, voxel_size, origin, return_index, mode="nearest", return_counts=False):
        """([downsampled clouds], [uint32 host index arrays] or None): one a3d_point_clouds_voxel_downsample_device call;
        with mode="mean" ([clouds], [index arrays] or None, [uint32 host count arrays] or None): one
        a3d_point_clouds_voxel_mean_device call."""
        if mode not in ("nearest", "mean"):
            raise _abi.InvalidParameter(f"voxel_downsample: mode is 'nearest' or 'mean', not {mode!r}")
        if return_counts and mode != "mean":
            raise _abi.InvalidParameter("voxel_downsample: return_counts needs mode='mean' (a nearest-point cell has one row)")
        clouds = list(clouds)
        if mode == "mean":
            return DevicePointCloud._voxel_mean(clouds, voxel_size, origin, return_index, return_counts)
        if not clouds:
            return [], ([] if return_index else None)
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "voxel_downsample")
        o = DevicePointCloud._origin3(origin)

        def call(a):  # (the plain entry point forwards to this one with NULL colours)
            _abi.check(
                ctx.lib.a3d_point_clouds_voxel_downsample_rgb_device(
                    ctx.handle, a.views, a.colors, a.n, float(voxel_size), o, a.out_points, a.out_normals, a.out_colors,
                    a.side["index"], a.capacities, a.lens, None),
                "a3d_point_clouds_voxel_downsample_rgb_device",
            )

        outs, host = DevicePointCloud._compact(ctx, clouds, index=return_index, call=call)
        return outs, host["index"]

    @staticmethod
    def _origin3(origin):
        if origin is None:
            return None
        o = np.ascontiguousarray(origin, np.float32).reshape(-1)
        if o.size != 3:
            raise _abi.InvalidParameter("voxel_downsample: the origin has three coordinates")
        return (C.c_float * 3)(*o.tolist())

    @staticmethod
    def _compact(ctx, clouds, call, **side):
        """What the wrappers of the compacting calls share (voxel_downsample in both modes, select_many): allocates one
        output per cloud, shaped like its input, and for each name of `side` given as true one u32 device buffer per
        cloud; runs call(a), where `a` holds the call's ctypes arrays (n, views, colors, out_points, out_normals,
        out_colors, capacities, lens, and side[name]: the array of that side's buffers, or None); sets each output's
        length from lens.  Returns (outputs, {name: [uint32 host arrays of the output's length] or None}).  The outputs are
        freed if anything fails, the side buffers always."""
        n, outs = len(clouds), []
        d_side = {name: [] for name, wanted in side.items() if wanted}
        try:
            for c in clouds:
                outs.append(DevicePointCloud._allocate(ctx, c.n, c.d_normals is not None, c.d_colors is not None))
                for buffers in d_side.values():
                    buffers.append(ctx.malloc(max(1, c.n) * 4))
            colours = any(c.d_colors is not None for c in clouds)
            a = types.SimpleNamespace(
                n=n, views=DevicePointCloud._views(clouds), colors=DevicePointCloud._colors_array(clouds) if colours else None,
                out_points=(C.c_void_p * n)(*[x.d_points for x in outs]),
                out_normals=(C.c_void_p * n)(*[x.d_normals for x in outs]),
                out_colors=DevicePointCloud._colors_array(outs) if colours else None,
                side={name: (C.c_void_p * n)(*d_side[name]) if name in d_side else None for name in side},
                capacities=(C.c_uint64 * n)(*[c.n for c in clouds]), lens=(C.c_uint64 * n)())
            call(a)
            for x, k in zip(outs, a.lens):
                x.n = int(k)
            host = {name: [ctx.to_host(d, np.empty(x.n, np.uint32)) if x.n else np.empty(0, np.uint32)
                           for d, x in zip(d_side[name], outs)] if name in d_side else None for name in side}
        except BaseException:
            for x in outs:
                x.free()
            raise
        finally:
            for buffers in d_side.values():
                for d in buffers:
                    ctx.free(d)
        return outs, host

    @staticmethod
    def _voxel_mean(clouds, voxel_size, origin, return_index, return_counts):
        """The mode="mean" half of _voxel_downsample: one a3d_point_clouds_voxel_mean_device call."""
        if not clouds:
            return [], ([] if return_index else None), ([] if return_counts else None)
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "voxel_downsample")
        o = DevicePointCloud._origin3(origin)

        def call(a):
            _abi.check(
                ctx.lib.a3d_point_clouds_voxel_mean_device(
                    ctx.handle, a.views, a.colors, a.n, float(voxel_size), o, a.out_points, a.out_normals, a.out_colors,
                    a.side["index"], a.side["counts"], a.capacities, a.lens, None),
                "a3d_point_clouds_voxel_mean_device",
            )

        outs, host = DevicePointCloud._compact(ctx, clouds, index=return_index, counts=return_counts, call=call)
        return outs, host["index"], host["counts"]

    @staticmethod
    def voxel_downsample_many(clouds, voxel_size, origin=None, mode="nearest"):
        """[c.voxel_downsample(voxel_size, origin, mode=mode) for c in clouds] as new resident clouds of one context, in
        ONE call whose launch count does not depend on the number of clouds (a3d_point_clouds_voxel_downsample_device;
        mode="mean": a3d_point_clouds_voxel_mean_device).  Each result keeps the buffers sized for its input (len() is
        the kept count) and has normals iff its input has them, and colours iff its input has them."""
        return DevicePointCloud._voxel_downsample(clouds, voxel_size, origin, False, mode)[0]

    def voxel_downsample(self, voxel_size, origin=None, return_index=False, mode="nearest", return_counts=False):
        """One point per occupied cell of the grid of pitch `voxel_size` anchored at `origin` (default (0, 0, 0)), as a
        new resident cloud: the input point nearest to the cell's centre (ties: the lowest index), never an average, so
        the result is a subsequence of this cloud, points, normals and colours bit for bit, and does not depend on the order of
        the points.  Points whose cell is not finite or outside [-2^20, 2^20) per axis (NaN, infinities, far outliers)
        are dropped.  return_index=True returns (cloud, index): `index` is a HOST uint32 array, index[k] = the position
        in this cloud of the result's point k (one 4-byte-per-kept-point download; nothing else leaves the device).

        mode="mean" gives what PCL's VoxelGrid and Open3D's voxel_down_sample give instead: per occupied cell the centroid
        of its points, the mean of their normals (renormalised; zero if they cancel) and the mean of their colours
        (rounded half up), by the integer rule of a3d_point_clouds_voxel_mean_device (include/align3d_hip.h): the same
        cells, the same count of dropped points, rows in first-occurrence order, a cell of one point copied bit for bit,
        and the same bits under any permutation of this cloud's rows.  `index` is then each cell's lowest input index,
        and return_counts=True appends a HOST uint32 array of the cells' point counts: (cloud, counts) or (cloud, index,
        counts).  Any other mode, or return_counts with mode="nearest", raises InvalidParameter."""
        res = DevicePointCloud._voxel_downsample([self], voxel_size, origin, return_index, mode, return_counts)
        extras = [x[0] for x in res[1:] if x is not None]
        return (res[0][0], *extras) if extras else res[0][0]

    @staticmethod
    def estimate_normals_many(clouds, radius, viewpoints=None, min_neighbors=3, orient="viewpoint", curvature=False,
                              counts=False, dropped=False):
        """estimate_normals for resident clouds of one context in ONE call and one wait, whatever their number
        (a3d_point_clouds_estimate_normals_device).  viewpoints: None (the origin for every cloud) or one entry per cloud,
        each None, three coordinates, or a Transform (a camera-to-world pose, whose translation is taken).  Returns the
        valid-row count of each cloud; with curvature / counts, a tuple (valid, [curvature arrays], [count arrays]) of
        what was asked for, downloaded to the host; dropped=True appends the per-cloud number of dropped rows (coordinates
        that are not finite or beyond 2^20 cells) to that tuple."""
        clouds = list(clouds)
        extras = bool(curvature) + bool(counts) + bool(dropped)
        if orient not in ("viewpoint", "normals"):
            raise _abi.InvalidParameter(f'estimate_normals: orient is "viewpoint" or "normals" (got {orient!r})')
        if not clouds:
            return ([],) * (1 + extras) if extras else []
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "estimate_normals")
        n = len(clouds)
        eyes = None
        if viewpoints is not None:
            viewpoints = list(viewpoints)
            if len(viewpoints) != n:
                raise _abi.InvalidParameter(f"estimate_normals: {n} clouds but {len(viewpoints)} viewpoints")
            e = np.zeros((n, 3), np.float32)
            for i, v in enumerate(viewpoints):
                if isinstance(v, Transform):
                    v = v.t
                if v is not None:
                    v = np.ascontiguousarray(v, np.float32).reshape(-1)
                    if v.size != 3:
                        raise _abi.InvalidParameter("estimate_normals: a viewpoint has three coordinates")
                    e[i] = v
            eyes = (C.c_float * (3 * n))(*e.reshape(-1).tolist())
        by_normals = orient == "normals"
        if by_normals and any(c.d_normals is None and c.n for c in clouds):
            raise _abi.A3dError(_abi.A3D_MISSING_FIELD, 'estimate_normals: orient="normals" on a cloud without normals')
        fresh, d_curv, d_counts = [], [], []
        try:
            for c in clouds:
                if c.d_normals is None:
                    c.d_normals = ctx.malloc(max(1, c.n) * 12)
                    fresh.append(c)
                if curvature:
                    d_curv.append(ctx.malloc(max(1, c.n) * 4))
                if counts:
                    d_counts.append(ctx.malloc(max(1, c.n) * 4))
            valid, n_dropped = (C.c_uint64 * n)(), (C.c_uint64 * n)()
            _abi.check(
                ctx.lib.a3d_point_clouds_estimate_normals_device(
                    ctx.handle, DevicePointCloud._views(clouds), n, float(radius), int(min_neighbors), eyes,
                    1 if by_normals else 0, (C.c_void_p * n)(*[c.d_normals for c in clouds]),
                    (C.c_void_p * n)(*d_curv) if curvature else None, (C.c_void_p * n)(*d_counts) if counts else None,
                    valid, n_dropped),
                "a3d_point_clouds_estimate_normals_device",
            )
            out = ([int(v) for v in valid],)
            if curvature:
                out += ([ctx.to_host(d, np.empty(c.n, np.float32)) if c.n else np.empty(0, np.float32)
                         for d, c in zip(d_curv, clouds)],)
            if counts:
                out += ([ctx.to_host(d, np.empty(c.n, np.uint32)) if c.n else np.empty(0, np.uint32)
                         for d, c in zip(d_counts, clouds)],)
            if dropped:
                out += ([int(v) for v in n_dropped],)
        except BaseException:
            for c in fresh:  # a cloud that had no normals has none after a failed call
                ctx.free(c.d_normals)
                c.d_normals = None
            raise
        finally:
            for d in d_curv + d_counts:
                ctx.free(d)
        return out if extras else out[0]

    def estimate_normals(self, radius, viewpoint=None, min_neighbors=3, orient="viewpoint", curvature=False, counts=False,
                         dropped=False):
        """Gives this cloud normals estimated from its own points (a3d_point_clouds_estimate_normals_device): per point,
        the direction of least spread of the points within `radius` (the cells of a grid of pitch `radius` around the
        point's own, then the ball), turned towards `viewpoint` (three coordinates or a camera-to-world Transform; None:
        the origin).  orient="normals" turns it along the normal the row already has instead, which refreshes the normals
        of a voxel map's extract without knowing which camera saw each cell.  Allocates d_normals if the cloud has none
        and overwrites them otherwise.  A row with fewer than min_neighbors (>= 3) neighbours, itself included, with all
        its neighbours on one spot, or with a coordinate that is not finite or beyond 2^20 cells gets the normal
        (0, 0, 0).  Such rows stay in the cloud: a zero normal is at pi / 2 from every normal, so every aligner's
        max_normal_angle gate (below pi / 2) rejects the row, and nothing needs to be compacted.  Returns the number of
        valid rows; with curvature=True and / or counts=True a tuple (valid, curvature [len] f32, counts [len] uint32) of
        what was asked for (host arrays: curvature = smallest eigenvalue / trace, counts = neighbours found); dropped=True
        appends the number of dropped rows."""
        out = DevicePointCloud.estimate_normals_many([self], radius, None if viewpoint is None else [viewpoint],
                                                     min_neighbors, orient, curvature, counts, dropped)
        if not (curvature or counts or dropped):
            return out[0]
        return (out[0][0],) + tuple(x[0] for x in out[1:])

    @staticmethod
    def _per_cloud_u32(value, n, what):
        """A scalar or one entry per cloud as a (c_uint32 * n) array."""
        values = [value] * n if np.isscalar(value) else list(value)
        if len(values) != n:
            raise _abi.InvalidParameter(f"{what}: {n} clouds but {len(values)} bounds")
        for v in values:
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise _abi.InvalidParameter(f"{what}: a bound must fit 32 unsigned bits (got {v})")
        return (C.c_uint32 * n)(*[int(v) for v in values])

    @staticmethod
    def select_many(clouds, values, lo=1, hi=0xFFFFFFFF, return_index=False):
        """[c.select(v, lo, hi) for c, v in zip(clouds, values)] as new resident clouds of one context, in ONE call whose
        launch count does not depend on the number of clouds (a3d_point_clouds_select_device).  values: one entry per
        cloud, a host array of len() booleans or unsigned integers (uploaded as u32) or a device pointer to len() u32
        (ctypes.c_void_p, taken as it is); lo, hi: one number for all clouds or one per cloud.  Returns the clouds, or
        (clouds, [uint32 host index arrays]) with return_index=True."""
        clouds, values = list(clouds), list(values)
        if len(values) != len(clouds):
            raise _abi.InvalidParameter(f"select: {len(clouds)} clouds but {len(values)} value arrays")
        if not clouds:
            return ([], []) if return_index else []
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "select")
        n = len(clouds)
        lo, hi = DevicePointCloud._per_cloud_u32(lo, n, "select"), DevicePointCloud._per_cloud_u32(hi, n, "select")
        uploaded, d_values = [], []

        def call(a):
            _abi.check(
                ctx.lib.a3d_point_clouds_select_device(
                    ctx.handle, a.views, a.colors, n, (C.c_void_p * n)(*d_values), lo, hi, a.out_points, a.out_normals,
                    a.out_colors, a.side["index"], a.capacities, a.lens),
                "a3d_point_clouds_select_device",
            )

        try:
            for c, v in zip(clouds, values):
                if isinstance(v, (C.c_void_p, int)):
                    d_values.append(v if isinstance(v, C.c_void_p) else C.c_void_p(v))
                    continue
                v = np.asarray(v)
                if v.ndim != 1 or len(v) != c.n:
                    raise _abi.InvalidParameter(f"select: a cloud of {c.n} rows but values of shape {v.shape}")
                if v.dtype != np.bool_ and not (np.issubdtype(v.dtype, np.integer) and (v >= 0).all() and (v <= 0xFFFFFFFF).all()):
                    raise _abi.InvalidParameter(f"select: values are booleans or unsigned 32-bit integers (got {v.dtype})")
                uploaded.append(ctx.to_device(np.ascontiguousarray(v, np.uint32)) if c.n else ctx.malloc(4))
                d_values.append(uploaded[-1])
            outs, host = DevicePointCloud._compact(ctx, clouds, index=return_index, call=call)
        finally:
            for d in uploaded:
                ctx.free(d)
        return (outs, host["index"]) if return_index else outs

    def select(self, values_or_mask, lo=1, hi=0xFFFFFFFF, return_index=False):
        """The rows p of this cloud with lo <= values[p] <= hi, in input order, as a new resident cloud
        (a3d_point_clouds_select_device): points, normals and colours copied bit for bit; the coordinates are never looked
        at.  values_or_mask: a host array of len() booleans (True = 1, so the defaults keep the True rows) or unsigned
        integers, uploaded as u32, or a device pointer (ctypes.c_void_p) to len() u32, taken as it is.  The result keeps
        buffers sized for this cloud, like voxel_downsample's.  return_index=True returns (cloud, index): a HOST uint32
        array, index[k] = the row of this cloud that row k of the result was; strictly increasing."""
        out = DevicePointCloud.select_many([self], [values_or_mask], lo, hi, return_index)
        return (out[0][0], out[1][0]) if return_index else out[0]

    @staticmethod
    def neighbor_distances_many(clouds, radius, k):
        """neighbor_distances for resident clouds of one context in ONE call and one wait
        (a3d_point_clouds_knn_distance_device).  Returns ([d_counts], [d_qsum], [stats]): per cloud a device buffer of
        len() u32 neighbour counts, a device buffer of len() u32 distance sums (None when k == 0), and the tuple
        (m, sum Q, sum Q^2) of Python ints.  The buffers are RESIDENT: they go to select() as they are, and the caller
        releases each with the context's free()."""
        clouds = list(clouds)
        if not clouds:
            return [], [], []
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "neighbor_distances")
        n, k = len(clouds), int(k)
        if k < 0:
            raise _abi.InvalidParameter(f"neighbor_distances: k is at least 0 (got {k})")
        d_counts, d_qsum = [], []
        try:
            for c in clouds:
                d_counts.append(ctx.malloc(max(1, c.n) * 4))
                if k:
                    d_qsum.append(ctx.malloc(max(1, c.n) * 4))
            stats = (C.c_uint64 * (4 * n))()
            _abi.check(
                ctx.lib.a3d_point_clouds_knn_distance_device(
                    ctx.handle, DevicePointCloud._views(clouds), n, float(radius), k, (C.c_void_p * n)(*d_counts),
                    (C.c_void_p * n)(*d_qsum) if k else None, stats, None),
                "a3d_point_clouds_knn_distance_device",
            )
        except BaseException:
            for d in d_counts + d_qsum:
                ctx.free(d)
            raise
        tuples = [(int(stats[4 * i]), int(stats[4 * i + 1]), int(stats[4 * i + 2]) + (int(stats[4 * i + 3]) << 32))
                  for i in range(n)]
        return d_counts, d_qsum if k else [None] * n, tuples

    def neighbor_distances(self, radius, k):
        """Per row of this cloud, resident: the number N of rows within `radius` (the row itself included; the cells of
        a grid of pitch `radius` around the row's own, then the ball: estimate_normals' neighbours and its counts, bit for
        bit), and, for k > 0, Q = the sum of the distances to the k nearest OTHER rows within `radius`, each rounded to a
        lattice of radius / 32768 (0xFFFFFFFF for a row with fewer than k others, or with a coordinate that is not finite
        or beyond 2^20 cells).  0 <= k <= 32.  Returns (d_counts, d_qsum, (m, sum Q, sum Q^2)): two device buffers of
        len() u32 (d_qsum is None when k == 0; release them with the context's free()) and the integer sums over the m
        rows that have a Q, the same on every run and for every order of the rows."""
        counts, qsum, stats = DevicePointCloud.neighbor_distances_many([self], radius, k)
        return counts[0], qsum[0], stats[0]

    @staticmethod
    def knn_distance_threshold(stats, std_ratio):
        """The largest Q the statistical filter keeps (a3d_knn_distance_threshold; host only): floor(mean +
        std_ratio * sample standard deviation) of the Q that neighbor_distances summed into stats = (m, sum Q, sum Q^2)."""
        m, total, squares = (int(x) for x in stats)
        if min(m, total, squares) < 0 or max(m, total) >= 1 << 64 or squares >= 1 << 96:
            raise _abi.InvalidParameter("knn_distance_threshold: statistics that no call can have produced")
        words = (C.c_uint64 * 4)(m, total, squares & 0xFFFFFFFF, squares >> 32)
        out = C.c_uint32()
        _abi.check(_abi.load_library().a3d_knn_distance_threshold(words, float(std_ratio), C.byref(out)),
                   "a3d_knn_distance_threshold")
        return int(out.value)

    @staticmethod
    def remove_radius_outliers_many(clouds, radius, min_neighbors, return_index=False):
        """[c.remove_radius_outliers(radius, min_neighbors) for c in clouds] for resident clouds of one context: one knn
        call (k = 0) and one select call, whatever the number of clouds."""
        clouds = list(clouds)
        if not clouds:
            return ([], []) if return_index else []
        ctx = clouds[0].ctx
        counts, _, _ = DevicePointCloud.neighbor_distances_many(clouds, radius, 0)
        try:
            return DevicePointCloud.select_many(clouds, counts, int(min_neighbors), 0xFFFFFFFF, return_index)
        finally:
            for d in counts:
                ctx.free(d)

    def remove_radius_outliers(self, radius, min_neighbors, return_index=False):
        """This cloud without the rows that have fewer than `min_neighbors` rows within `radius`, THE ROW ITSELF COUNTED,
        as a new resident cloud in input order with normals and colours when this cloud has them: the k = 0 call of
        neighbor_distances followed by select(counts, lo=min_neighbors).  That rule is the definition.  PCL's
        RadiusOutlierRemoval(min_neighbors_in_radius = n) keeps a point with at least n neighbours, itself included,
        as here; Open3D's remove_radius_outlier(nb_points, radius) counts the point itself as well and keeps it when the
        count EXCEEDS nb_points, so it corresponds to min_neighbors = nb_points + 1.  Neighbours are estimate_normals'
        (the 27 cells of a grid of pitch `radius`, then the ball); a row with a coordinate that is not finite or beyond
        2^20 cells has no neighbours and goes for every min_neighbors >= 1.  return_index as in select()."""
        out = DevicePointCloud.remove_radius_outliers_many([self], radius, min_neighbors, return_index)
        return (out[0][0], out[1][0]) if return_index else out[0]

    @staticmethod
    def remove_statistical_outliers_many(clouds, radius, k, std_ratio, return_index=False):
        """[c.remove_statistical_outliers(radius, k, std_ratio) for c in clouds] for resident clouds of one context, each
        with its own mean and deviation: one knn call, the thresholds on the host, one select call."""
        clouds = list(clouds)
        if not clouds:
            return ([], []) if return_index else []
        if int(k) < 1:
            raise _abi.InvalidParameter(f"remove_statistical_outliers: k is at least 1 (got {k})")
        ctx = clouds[0].ctx
        counts, qsum, stats = DevicePointCloud.neighbor_distances_many(clouds, radius, k)
        try:
            hi = [DevicePointCloud.knn_distance_threshold(s, std_ratio) for s in stats]
            return DevicePointCloud.select_many(clouds, qsum, 0, hi, return_index)
        finally:
            for d in counts + qsum:
                ctx.free(d)

    def remove_statistical_outliers(self, radius, k, std_ratio, return_index=False):
        """This cloud without the rows whose mean distance to their k nearest other rows is more than `std_ratio` sample
        standard deviations above the cloud's mean of that figure (PCL StatisticalOutlierRemoval(mean_k, stddev_mul),
        Open3D remove_statistical_outlier(nb_neighbors, std_ratio)), as a new resident cloud in input order with normals
        and colours when this cloud has them: neighbor_distances(radius, k), knn_distance_threshold, select(qsum, 0, T).
        The k nearest are searched WITHIN `radius` only: PCL and Open3D search without a bound, here the bound keeps the
        search inside the 27 cells around the row, and a row with fewer than k others within `radius` is an outlier by
        rule and takes no part in the mean and the deviation.  Choose `radius` a few times the spacing the k-th neighbour
        of an inlier has.  1 <= k <= 32.  All decisions are on integers (distances on a lattice of radius / 32768), so
        the result does not depend on the order of the rows.  return_index as in select()."""
        out = DevicePointCloud.remove_statistical_outliers_many([self], radius, k, std_ratio, return_index)
        return (out[0][0], out[1][0]) if return_index else out[0]

    @staticmethod
    def _cluster_call(clouds, radius, min_points, row_sizes):
        """One a3d_point_clouds_cluster_device over resident clouds of one context.  Returns (ctx, [d_labels],
        [d_row_sizes] or None, [sizes], [roots]); the device buffers are the caller's to free."""
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "cluster")
        n, m = len(clouds), int(min_points)
        if not 1 <= m <= 0xFFFFFFFF:
            raise _abi.InvalidParameter(f"cluster: min_points is at least 1 (got {min_points})")
        d_labels, d_rows, d_sizes, d_roots = [], [], [], []
        try:
            for c in clouds:
                for group in (d_labels, d_sizes, d_roots) + ((d_rows,) if row_sizes else ()):
                    group.append(ctx.malloc(max(1, c.n) * 4))
            found = (C.c_uint64 * n)()
            _abi.check(
                ctx.lib.a3d_point_clouds_cluster_device(
                    ctx.handle, DevicePointCloud._views(clouds), n, float(radius), m, (C.c_void_p * n)(*d_labels),
                    (C.c_void_p * n)(*d_rows) if row_sizes else None, (C.c_void_p * n)(*d_sizes),
                    (C.c_void_p * n)(*d_roots), found, None, None),
                "a3d_point_clouds_cluster_device",
            )
            sizes = [ctx.to_host(d, np.empty(int(k), np.uint32)) if k else np.empty(0, np.uint32)
                     for d, k in zip(d_sizes, found)]
            roots = [ctx.to_host(d, np.empty(int(k), np.uint32)) if k else np.empty(0, np.uint32)
                     for d, k in zip(d_roots, found)]
        except BaseException:
            for d in d_labels + d_rows:
                ctx.free(d)
            raise
        finally:
            for d in d_sizes + d_roots:
                ctx.free(d)
        return ctx, d_labels, d_rows if row_sizes else None, sizes, roots

    @staticmethod
    def cluster_many(clouds, radius, min_points=1):
        """cluster for resident clouds of one context in ONE call and one wait (a3d_point_clouds_cluster_device).
        Returns ([d_labels], [sizes], [roots]): per cloud a RESIDENT buffer of len() u32 labels, and host uint32 arrays of
        the C cluster sizes and the C root rows.  The label buffers go to select() as they are; the caller releases each
        with the context's free()."""
        clouds = list(clouds)
        if not clouds:
            return [], [], []
        _, d_labels, _, sizes, roots = DevicePointCloud._cluster_call(clouds, radius, min_points, False)
        return d_labels, sizes, roots

    def cluster(self, radius, min_points=1):
        """Which rows of this cloud belong together: DBSCAN on the device.  Neighbours are estimate_normals' and
        neighbor_distances' (the 27 cells of a grid of pitch `radius`, then the ball, the row itself counted).  A row with
        at least `min_points` neighbours is a core row; core rows within `radius` of each other share a cluster; a row
        that is not core but has a core row within `radius` is a BORDER row and joins the cluster of the NEAREST core row
        (the lower row on a tie); every other row, and every row with a coordinate that is not finite or beyond 2^20
        cells, is noise with label 0xFFFFFFFF.  Clusters are numbered 0 ... C-1 by their lowest core row.  Open3D's
        cluster_dbscan(eps, min_points) takes the same two numbers, counts the point itself too and numbers clusters the
        same way: core rows get the same labels; a border row within reach of several clusters goes to the first that
        reaches it there and to the nearest here.  PCL's EuclideanClusterExtraction(tolerance) is min_points = 1 (every
        row is core, no border rows, no noise but the refused rows); its min / max cluster size is
        remove_small_clusters().  Returns (d_labels, sizes, roots): a RESIDENT buffer of len() u32 (select(d_labels, c, c)
        is cluster c, select(d_labels, 0, 0xFFFFFFFE) drops the noise; release it with the context's free()) and host
        uint32 arrays sizes[C] (border rows included) and roots[C] (strictly increasing).  All decisions are on integers:
        the same result on every run."""
        labels, sizes, roots = DevicePointCloud.cluster_many([self], radius, min_points)
        return labels[0], sizes[0], roots[0]

    @staticmethod
    def remove_small_clusters_many(clouds, radius, min_points, min_size, max_size=0xFFFFFFFF, return_index=False):
        """[c.remove_small_clusters(radius, min_points, min_size, max_size) for c in clouds] for resident clouds of one
        context: one cluster call and one select call, whatever the number of clouds."""
        clouds = list(clouds)
        if not clouds:
            return ([], []) if return_index else []
        if int(min_size) < 1:
            raise _abi.InvalidParameter(f"remove_small_clusters: min_size is at least 1 (got {min_size})")
        ctx, d_labels, d_rows, _, _ = DevicePointCloud._cluster_call(clouds, radius, min_points, True)
        try:
            return DevicePointCloud.select_many(clouds, d_rows, int(min_size), int(max_size), return_index)
        finally:
            for d in d_labels + d_rows:
                ctx.free(d)

    def remove_small_clusters(self, radius, min_points, min_size, max_size=0xFFFFFFFF, return_index=False):
        """This cloud without the noise and without the rows of clusters of fewer than `min_size` or more than `max_size`
        rows (border rows count), as a new resident cloud in input order with normals and colours when this cloud has
        them: cluster(radius, min_points) with the size of each row's cluster, then select(row_sizes, min_size,
        max_size).  min_size >= 1.  With min_points = 1 this is PCL's EuclideanClusterExtraction(tolerance = radius,
        min_cluster_size, max_cluster_size) with the surviving clusters put back together; with Open3D it is
        cluster_dbscan(radius, min_points) and a filter on the label counts.  It removes what the radius filter keeps: a
        floating clump whose points all have neighbours.  return_index as in select()."""
        out = DevicePointCloud.remove_small_clusters_many([self], radius, min_points, min_size, max_size, return_index)
        return (out[0][0], out[1][0]) if return_index else out[0]

    def largest_cluster(self, radius, min_points=1, return_index=False):
        """The cluster of cluster(radius, min_points) with the most rows (border rows count; the lowest label on a tie) as
        a new resident cloud in input order: one cluster call and one select on the labels.  A cloud without a cluster
        gives an empty cloud.  return_index as in select()."""
        d_labels, sizes, _ = self.cluster(radius, min_points)
        try:
            if len(sizes) == 0:
                return self.select(d_labels, 1, 0, return_index)
            c = int(np.argmax(sizes))  # the first of the largest
            return self.select(d_labels, c, c, return_index)
        finally:
            self.ctx.free(d_labels)

    @staticmethod
    def plane_hypotheses(seed, length, num_iterations):
        """The candidate triples segment_plane scores by default (a3d_plane_hypotheses; host only): a uint32
        [num_iterations, 3] array of row numbers below `length`, candidate h a function of (seed, h, length) alone."""
        seed, length, h = int(seed), int(length), int(num_iterations)
        if not (0 <= seed < 1 << 64 and 0 <= length < 1 << 64 and 0 <= h < 1 << 64):
            raise _abi.InvalidParameter("plane_hypotheses: seed, length and num_iterations are unsigned 64-bit integers")
        out = np.zeros((h if h <= 4096 else 0, 3), np.uint32)
        _abi.check(_abi.load_library().a3d_plane_hypotheses(seed, length, h, out.ctypes.data_as(C.POINTER(C.c_uint32))),
                   "a3d_plane_hypotheses")
        return out

    @staticmethod
    def plane_from_moments(moments, point, distance_threshold, fallback_normal):
        """(plane float64 [4], valid) from one record of refit moments (a3d_plane_from_moments; host only): 16 integers
        N, S[3], Lo[6], Hi[6] (signed ones as they are), the f32 point they were taken against, the call's threshold and
        the normal an invalid refit keeps."""
        words = [int(m) for m in moments]
        if len(words) != 16 or any(not -(1 << 63) <= m < 1 << 64 for m in words):
            raise _abi.InvalidParameter("plane_from_moments: 16 integers of 64 bits")
        m = (C.c_uint64 * 16)(*[w & 0xFFFFFFFFFFFFFFFF for w in words])
        a = (C.c_float * 3)(*np.ascontiguousarray(point, np.float32).reshape(3).tolist())
        f = (C.c_float * 3)(*np.ascontiguousarray(fallback_normal, np.float32).reshape(3).tolist())
        plane, valid = (C.c_double * 4)(), C.c_uint32()
        _abi.check(_abi.load_library().a3d_plane_from_moments(m, a, float(distance_threshold), f, plane, C.byref(valid)),
                   "a3d_plane_from_moments")
        return np.array(plane[:], np.float64), bool(valid.value)

    @staticmethod
    def segment_plane_many(clouds, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None):
        """segment_plane for resident clouds of one context in ONE call (a3d_point_clouds_segment_plane_device): the
        number of launches does not depend on the number of clouds.  triples: None (every non-empty cloud gets
        plane_hypotheses(seed, len, num_iterations), an empty one no candidates), or one entry per cloud, each None or an
        integer array [H, 3] of row numbers.  Returns ([plane float64 [4]], [d_flags], [inliers]): the flags buffers are
        RESIDENT, len() u32 each; the caller releases each with the context's free()."""
        clouds = list(clouds)
        if not clouds:
            return [], [], []
        clouds, ctx, _ = DevicePointCloud._resident_batch(clouds, None, "segment_plane")
        n, refine = len(clouds), int(refine)
        if not 0 <= refine <= 8:
            raise _abi.InvalidParameter(f"segment_plane: refine is 0 to 8 rounds (got {refine})")
        if not 0 <= int(num_iterations) <= 4096:
            raise _abi.InvalidParameter(f"segment_plane: num_iterations is at most 4096 (got {num_iterations})")
        if triples is None:
            triples = [None] * n
        triples = list(triples)
        if len(triples) != n:
            raise _abi.InvalidParameter(f"segment_plane: {n} clouds but {len(triples)} arrays of triples")
        host = []
        for c, tr in zip(clouds, triples):
            if tr is None:
                tr = DevicePointCloud.plane_hypotheses(seed, c.n, num_iterations if c.n else 0)
            else:
                tr = np.asarray(tr)
                if tr.ndim != 2 or tr.shape[1] != 3 or not (np.issubdtype(tr.dtype, np.integer) or tr.size == 0):
                    raise _abi.InvalidParameter(f"segment_plane: triples are an integer array [H, 3] (got {tr.shape} {tr.dtype})")
                if tr.size and (tr.min() < 0 or tr.max() >= c.n):
                    raise _abi.InvalidParameter(f"segment_plane: a triple names a row outside a cloud of {c.n} rows")
                if len(tr) > 4096:
                    raise _abi.InvalidParameter(f"segment_plane: at most 4096 candidates per cloud (got {len(tr)})")
            host.append(np.ascontiguousarray(tr, np.uint32).reshape(-1, 3))
        d_flags = []
        try:
            for c in clouds:
                d_flags.append(ctx.malloc(max(1, c.n) * 4))
            planes, inliers = (C.c_double * (4 * n))(), (C.c_uint64 * n)()
            _abi.check(
                ctx.lib.a3d_point_clouds_segment_plane_device(
                    ctx.handle, DevicePointCloud._views(clouds), n, float(distance_threshold), refine,
                    (C.c_void_p * n)(*[t.ctypes.data if len(t) else None for t in host]),
                    (C.c_uint32 * n)(*[len(t) for t in host]), (C.c_void_p * n)(*d_flags), None, planes, None, inliers, None),
                "a3d_point_clouds_segment_plane_device",
            )
        except BaseException:
            for d in d_flags:
                ctx.free(d)
            raise
        return ([np.array(planes[4 * i:4 * i + 4], np.float64) for i in range(n)], d_flags, [int(k) for k in inliers])

    def segment_plane(self, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None):
        """The dominant plane of this cloud, found on the device: RANSAC with EVERY candidate scored.  Each of the
        `num_iterations` candidates (at most 4096) is the plane through three rows; a row is an inlier of a plane iff its
        distance to it is at most `distance_threshold`; the candidate with the most inliers wins (the lowest number on a
        tie), its inliers are flagged and the plane is refitted to them by least squares (the direction of least spread
        of the flagged rows, through their centroid).  refine=R repeats flagging and refit R times against the refitted
        plane (at most 8).  Returns (plane, d_flags, inliers): plane = float64 (a, b, c, d) with a*x + b*y + c*z + d = 0,
        (a, b, c) a unit normal turned so that d >= 0 (the origin on its positive side); d_flags = a RESIDENT buffer of
        len() u32, 1 for the rows of the plane and 0 for the rest, which goes to select() as it is (release it with the
        context's free()); inliers = the number of flagged rows.  A cloud without three rows that span a plane among its
        candidates gives the plane (0, 0, 0, 0), no flagged row and inliers = 0.
        This is PCL's SACSegmentation(SACMODEL_PLANE, SAC_RANSAC) with setDistanceThreshold / setMaxIterations (and
        setOptimizeCoefficients for the refit), and Open3D's segment_plane(distance_threshold, ransac_n=3,
        num_iterations): refine=0 is Open3D's result shape, the inliers of the best candidate and the model refitted to
        them.  What does NOT correspond: there is no early exit by inlier probability, all candidates are always scored,
        so num_iterations is the work done and not an upper bound; and the sampling is a counter-based rule of our own
        (plane_hypotheses: candidate h depends on seed, h and len() only), not the generators of those libraries, so the
        same seed does not give their planes.  triples= takes the caller's own candidates ([H, 3] row numbers) instead.
        A row with a NaN or an infinity is never an inlier.  Every decision is on integers or on bits that no order
        changes: the same result on every run."""
        planes, flags, inliers = DevicePointCloud.segment_plane_many([self], distance_threshold, num_iterations, seed, refine,
                                                                    None if triples is None else [triples])
        return planes[0], flags[0], inliers[0]

    @staticmethod
    def split_plane_many(clouds, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None, return_index=False):
        """split_plane for resident clouds of one context: one segment call and one select call over the clouds taken
        twice, whatever their number.  Returns ([planes], [plane clouds], [rest clouds]), with return_index=True also
        ([plane index arrays], [rest index arrays])."""
        clouds = list(clouds)
        if not clouds:
            return ([], [], [], [], []) if return_index else ([], [], [])
        n, ctx = len(clouds), clouds[0].ctx
        planes, d_flags, _ = DevicePointCloud.segment_plane_many(clouds, distance_threshold, num_iterations, seed, refine, triples)
        try:
            out = DevicePointCloud.select_many(clouds + clouds, d_flags + d_flags, [1] * n + [0] * n, [1] * n + [0] * n,
                                               return_index)
        finally:
            for d in d_flags:
                ctx.free(d)
        if return_index:
            return planes, out[0][:n], out[0][n:], out[1][:n], out[1][n:]
        return planes, out[:n], out[n:]

    def split_plane(self, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None, return_index=False):
        """This cloud cut at its dominant plane: (plane, plane_cloud, rest_cloud), two new resident clouds in input order
        with normals and colours carried bit for bit when this cloud has them: segment_plane, then ONE select over the
        cloud taken twice (flags == 1 and flags == 0).  return_index=True returns (plane, plane_cloud, rest_cloud,
        plane_index, rest_index), the index arrays as in select().  The arguments, and what corresponds to PCL
        (SACSegmentation + ExtractIndices, negative and not) and Open3D (segment_plane + select_by_index, inverted and
        not), are segment_plane's."""
        out = DevicePointCloud.split_plane_many([self], distance_threshold, num_iterations, seed, refine,
                                                None if triples is None else [triples], return_index)
        return tuple(x[0] for x in out)

    @staticmethod
    def remove_plane_many(clouds, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None, return_index=False):
        """[c.remove_plane(...) for c in clouds] for resident clouds of one context: one segment call and one select
        call, whatever the number of clouds."""
        clouds = list(clouds)
        if not clouds:
            return ([], []) if return_index else []
        ctx = clouds[0].ctx
        _, d_flags, _ = DevicePointCloud.segment_plane_many(clouds, distance_threshold, num_iterations, seed, refine, triples)
        try:
            return DevicePointCloud.select_many(clouds, d_flags, 0, 0, return_index)
        finally:
            for d in d_flags:
                ctx.free(d)

    def remove_plane(self, distance_threshold, num_iterations=1000, seed=0, refine=0, triples=None, return_index=False):
        """This cloud without its dominant plane (the floor, the table), as a new resident cloud in input order with
        normals and colours when this cloud has them: segment_plane followed by select(flags, 0, 0).  It is the step before
        cluster() in a tabletop pipeline: objects that stand on one plane are one cluster until it is gone.  Calling it
        again on the result takes the next plane out.  return_index as in select(); everything else as segment_plane."""
        out = DevicePointCloud.remove_plane_many([self], distance_threshold, num_iterations, seed, refine,
                                                 None if triples is None else [triples], return_index)
        return (out[0][0], out[1][0]) if return_index else out[0]

    def render(self, camera, camera_to_world=None, radius=0.0, return_index=False):
        """What a pinhole camera sees of this cloud, as a new DeviceRangeImage (a3d_point_cloud_render_device): the
        inverse of from_range_image, PinholeCamera::project_to_image (src/camera.rs:177-202) over every point.  `camera`
        is a CameraIntrinsics whose width / height are the image's size; `camera_to_world` has the sense of
        PinholeCamera::new (its f32 inverse is applied; None: no pose, no arithmetic).  Per pixel the nearest point wins
        (ties: the lowest index) and the image holds that point in the camera's frame, its normal and its colour when
        the cloud has them; radius > 0 (metres) lets a point cover the pixels its disc would, at most 17 x 17.  The image
        goes to pyramid() and MultiscaleAlign like any other.  return_index=True returns (image, index): a HOST uint32
        [h][w] array of the winning point per pixel, 0xFFFFFFFF where there is none."""
        v = self.view()
        return _render(self.ctx, "DevicePointCloud.render", camera, camera_to_world, radius, return_index,
                       lambda pose, k, r, d_index, out: self.ctx.lib.a3d_point_cloud_render_device(
                           self.ctx.handle, C.byref(v), self.d_colors, pose, k.fx, k.fy, k.cx, k.cy, k.width, k.height, r,
                           d_index, out), "a3d_point_cloud_render_device")

    def len(self):
        return self.n

    def download(self):
        """(points [len,3], normals [len,3] or None) read back to the host."""
        pts = self.ctx.to_host(self.d_points, np.empty((self.n, 3), np.float32)) if self.n else np.empty((0, 3), np.float32)
        if self.d_normals is None:
            return pts, None
        nrm = self.ctx.to_host(self.d_normals, np.empty((self.n, 3), np.float32)) if self.n else np.empty((0, 3), np.float32)
        return pts, nrm

    def has_colors(self):
        return self.d_colors is not None

    def download_colors(self):
        """The colours [len, 3] uint8 (RGB) read back to the host, or None for a cloud without colours."""
        if self.d_colors is None:
            return None
        return self.ctx.to_host(self.d_colors, np.empty((self.n, 3), np.uint8)) if self.n else np.empty((0, 3), np.uint8)

    def view(self):
        v = _abi.PointCloudViewC()
        v.points = self.d_points
        v.normals = self.d_normals
        v.len = self.n
        return v

    def free(self):
        for p in (self.d_points, self.d_normals, getattr(self, "d_colors", None)):
            if p is not None and self.ctx.handle:
                self.ctx.free(p)
        self.d_points = self.d_normals = self.d_colors = None


def _resident_cloud(owner, cloud, what):
    """`cloud` if it is a DevicePointCloud of `owner`'s context; `what` names the method that was given it."""
    name = type(owner).__name__
    if not isinstance(cloud, DevicePointCloud):
        raise TypeError(f"{name}.{what} takes a DevicePointCloud (got {type(cloud).__name__}); there is no host fallback")
    if cloud.ctx is not owner.ctx:
        kind = "map" if isinstance(owner, DeviceVoxelMap) else "volume"
        raise _abi.InvalidParameter(f"{name}.{what}: the cloud must live on the {kind}'s context")
    return cloud


def _device_queries(owner, queries, what):
    """(device pointer, m, buffer to free or None) of `queries`: a resident cloud of `owner`'s context, or an [m, 3] array
    uploaded for the call."""
    if isinstance(queries, DevicePointCloud):
        return _resident_cloud(owner, queries, what).d_points, queries.n, None
    q = np.ascontiguousarray(queries, np.float32)
    if q.ndim != 2 or q.shape[1] != 3:
        raise _abi.InvalidParameter(f"{type(owner).__name__}.{what}: queries is a DevicePointCloud or an [m, 3] array")
    own = owner.ctx.to_device(q) if len(q) else None
    return own, len(q), own


class DeviceVoxelMap:
    """A persistent voxel map in HBM (a3d_voxel_map_*): resident clouds go in frame by frame, and after any sequence of
    inserts extract() is DevicePointCloud.merge(all inserted clouds, their transforms).voxel_downsample(voxel_size,
    origin) bit for bit — points, normals, order and indices — however the inserts were grouped.  normals=True: the map
    keeps a normal per cell and every inserted cloud must have normals.  colors=True: the same for colours (the winner's
    colour per cell; extract() then returns a cloud with colours).  reserve_cells: cells the first table holds without
    growing.  mode="mean" (a3d_voxel_map_new_mean): a map of cell means, kept as running integer sums; the contract is the
    same with voxel_downsample(voxel_size, origin, mode="mean") in place of the nearest-point downsample: centroid, mean
    normal, mean colour, representative index and count per cell, bit for bit, however the inserts were grouped.  Every
    method works on either kind of map."""

    def __init__(self, ctx, voxel_size, origin=None, normals=True, reserve_cells=0, colors=False, mode="nearest"):
        if mode not in ("nearest", "mean"):
            raise _abi.InvalidParameter(f'DeviceVoxelMap: mode is "nearest" or "mean" (got {mode!r})')
        self.ctx = ctx
        self.normals = bool(normals)
        self.colors = bool(colors)
        self.mode = mode
        self.handle = C.c_void_p()
        o = None
        if origin is not None:
            o = np.ascontiguousarray(origin, np.float32).reshape(-1)
            if o.size != 3:
                raise _abi.InvalidParameter("DeviceVoxelMap: the origin has three coordinates")
            o = (C.c_float * 3)(*o.tolist())
        if mode == "mean":
            _abi.check(ctx.lib.a3d_voxel_map_new_mean(ctx.handle, float(voxel_size), o, int(self.normals), int(self.colors),
                                                      int(reserve_cells), C.byref(self.handle)), "a3d_voxel_map_new_mean")
        elif self.colors:
            _abi.check(ctx.lib.a3d_voxel_map_new_rgb(ctx.handle, float(voxel_size), o, int(self.normals), 1, int(reserve_cells),
                                                     C.byref(self.handle)), "a3d_voxel_map_new_rgb")
        else:
            _abi.check(ctx.lib.a3d_voxel_map_new(ctx.handle, float(voxel_size), o, int(self.normals), int(reserve_cells),
                                                 C.byref(self.handle)), "a3d_voxel_map_new")

    def insert_many(self, clouds, transforms=None):
        """Inserts resident clouds of the map's context, cloud i under transforms[i] (None: as they are), in ONE call;
        returns the dropped count of each cloud (points whose cell is not finite or out of range: they still consume a
        sequence number)."""
        clouds = list(clouds)
        if not clouds:
            return []
        clouds, ctx, poses = DevicePointCloud._resident_batch(clouds, transforms, "DeviceVoxelMap.insert_many")
        if ctx is not self.ctx:
            raise _abi.InvalidParameter("DeviceVoxelMap.insert_many: the clouds must live on the map's context")
        n = len(clouds)
        dropped = (C.c_uint64 * n)()
        if self.colors:
            _abi.check(self.ctx.lib.a3d_voxel_map_insert_rgb(self.handle, DevicePointCloud._views(clouds),
                                                             DevicePointCloud._colors_array(clouds), poses, n, dropped, None),
                       "a3d_voxel_map_insert_rgb")
        else:
            _abi.check(self.ctx.lib.a3d_voxel_map_insert(self.handle, DevicePointCloud._views(clouds), poses, n, dropped, None),
                       "a3d_voxel_map_insert")
        return [int(d) for d in dropped]

    def insert(self, cloud, transform=None):
        """Inserts one resident cloud (under `transform`); returns its dropped count."""
        return self.insert_many([cloud], None if transform is None else [transform])[0]

    def extract(self, return_index=False, return_counts=False):
        """The map as a new DevicePointCloud of exactly cells() rows, in ascending sequence number (the order of the
        downsampled merged cloud; the same bits on every run).  return_index=True returns (cloud, index): `index` is a
        HOST uint32 array, index[k] = the position of row k in the merged cloud of everything inserted (on a map of
        means: of the cell's representative, its first point).  return_counts=True (a map of means only, else
        InvalidParameter) appends `counts`, a HOST uint32 array of the points offered to each row's cell, saturating:
        the order is (cloud, index, counts), as voxel_downsample returns them."""
        if return_counts and self.mode != "mean":
            raise _abi.InvalidParameter('DeviceVoxelMap.extract: return_counts needs a map of means (mode="mean")')
        ctx, cells = self.ctx, self.cells()
        out = DevicePointCloud._allocate(ctx, cells, self.normals, self.colors)
        d_index = d_counts = None
        try:
            if return_index:
                d_index = ctx.malloc(max(1, cells) * 4)
            if return_counts:
                d_counts = ctx.malloc(max(1, cells) * 4)
            n_out = C.c_uint64()
            if return_counts:
                _abi.check(ctx.lib.a3d_voxel_map_extract_mean(self.handle, out.d_points, out.d_normals, out.d_colors, d_index,
                                                              d_counts, cells, C.byref(n_out)), "a3d_voxel_map_extract_mean")
            elif self.colors:
                _abi.check(ctx.lib.a3d_voxel_map_extract_rgb(self.handle, out.d_points, out.d_normals, out.d_colors, d_index,
                                                             cells, C.byref(n_out)), "a3d_voxel_map_extract_rgb")
            else:
                _abi.check(ctx.lib.a3d_voxel_map_extract(self.handle, out.d_points, out.d_normals, d_index, cells,
                                                         C.byref(n_out)), "a3d_voxel_map_extract")
            out.n = int(n_out.value)
            result = [out]
            for wanted, d_words in ((return_index, d_index), (return_counts, d_counts)):
                if wanted:
                    result.append(ctx.to_host(d_words, np.empty(out.n, np.uint32)) if out.n else np.empty(0, np.uint32))
        except BaseException:
            out.free()
            raise
        finally:
            for d_words in (d_index, d_counts):
                if d_words is not None:
                    ctx.free(d_words)
        return tuple(result) if len(result) > 1 else out

    def bytes_per_slot(self):
        """Device memory per slot of the table (include/align3d_hip.h): 16 + 12 (+ 12 with normals) (+ 4 with colours),
        and in a map of means 8 + 24 (+ 24 with normals) (+ 24 with colours) + 4 more."""
        nearest = 16 + 12 + (12 if self.normals else 0) + (4 if self.colors else 0)
        if self.mode != "mean":
            return nearest
        return nearest + 8 + 24 + (24 if self.normals else 0) + (24 if self.colors else 0) + 4

    def stats(self):
        """{cells, slots, total, dropped_total, growths} (a3d_voxel_map_stats); a map of means adds mode = "mean" and its
        bytes_per_slot (a nearest-point map's dict is what it always was; its mode is the attribute `mode`)."""
        s = _abi.VoxelMapStatsC()
        _abi.check(self.ctx.lib.a3d_voxel_map_get_stats(self.handle, C.byref(s)), "a3d_voxel_map_get_stats")
        d = s.as_dict()
        if self.mode == "mean":
            d["mode"], d["bytes_per_slot"] = self.mode, self.bytes_per_slot()
        return d

    def cells(self):
        return self.stats()["cells"]

    def total(self):
        return self.stats()["total"]

    def retain(self, box=None, min_seq=0, marks=None):
        """Keeps the cells whose winner has sequence number >= min_seq and, with box = (min3, max3), whose stored point
        lies inside the closed box, and numbers them 0 ... k-1 in their old order: the map is then a new map into which
        the surviving rows went as one cloud (a3d_voxel_map_retain), total() is k and the table has shrunk to fit.
        Returns the number of removed cells, or (removed, new_marks) when `marks` (sequence numbers, e.g. total() at frame
        boundaries) is given: new_marks[i], a numpy uint64 array, is the survivors below marks[i], the same boundary in
        the new numbering.  On a map of means the box is tested on the cell's mean row and min_seq on the seq of its
        representative, its FIRST point (age by last observation is not kept); the survivors keep their sums and counts,
        and later inserts go on summing into them: the map is then the mean downsample of everything ever offered to the
        surviving cells followed by whatever comes later, not a new map of the surviving rows."""
        lo = hi = None
        if box is not None:
            try:
                lo, hi = box
            except (TypeError, ValueError):
                raise _abi.InvalidParameter("DeviceVoxelMap.retain: the box is (min3, max3)") from None
            bounds = []
            for b in (lo, hi):
                b = np.ascontiguousarray(b, np.float32).reshape(-1)
                if b.size != 3:
                    raise _abi.InvalidParameter("DeviceVoxelMap.retain: a corner of the box has three coordinates")
                bounds.append((C.c_float * 3)(*b.tolist()))
            lo, hi = bounds
        min_seq = int(min_seq)
        if not 0 <= min_seq < 1 << 64:
            raise _abi.InvalidParameter("DeviceVoxelMap.retain: min_seq is a sequence number (0 <= min_seq < 2^64)")
        old = new = None
        n = 0
        if marks is not None:
            m = np.asarray(marks)
            if m.ndim != 1 or (m.size and (m.dtype.kind not in "iu" or (m.dtype.kind == "i" and (m < 0).any()))):
                raise _abi.InvalidParameter("DeviceVoxelMap.retain: marks is a 1-d array of sequence numbers")
            m = np.ascontiguousarray(m, np.uint64)
            n = m.size
            out = np.zeros(n, np.uint64)
            if n:
                old, new = m.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64))
        removed = C.c_uint64()
        _abi.check(self.ctx.lib.a3d_voxel_map_retain(self.handle, lo, hi, min_seq, old, n, new, C.byref(removed)),
                   "a3d_voxel_map_retain")
        return int(removed.value) if marks is None else (int(removed.value), out)

    def compact(self):
        """retain() with nothing to remove: renumbers the cells 0 ... cells-1 and shrinks the table to fit."""
        return self.retain()

    def nearest(self, queries, transform=None):
        """The map's association (a3d_voxel_map_nearest_device) for every point of `queries`, a DevicePointCloud of the
        map's context or an [m, 3] float32 array (uploaded for the call), moved by `transform` first (None: as they
        are).  Returns host arrays (seq uint32, dist2 float32): the sequence number of the nearest stored row among the
        27 cells around the query and the squared distance to it; 0xFFFFFFFF and +inf where there is none.  It is the
        exact nearest row wherever that row lies within about one cell of the query, and not R3dTree.nearest."""
        ctx = self.ctx
        d_q, m, own = _device_queries(self, queries, "nearest")
        seq, dist2 = np.empty(m, np.uint32), np.empty(m, np.float32)
        if m == 0:
            return seq, dist2
        pose = None if transform is None else C.byref(transform.to_c())
        d_seq = d_dist = None
        try:
            d_seq, d_dist = ctx.malloc(m * 4), ctx.malloc(m * 4)
            _abi.check(ctx.lib.a3d_voxel_map_nearest_device(self.handle, d_q, m, pose, d_seq, d_dist),
                       "a3d_voxel_map_nearest_device")
            ctx.to_host(d_seq, seq), ctx.to_host(d_dist, dist2)
        finally:
            for p in (own, d_seq, d_dist):
                if p is not None:
                    ctx.free(p)
        return seq, dist2

    def align(self, source, params, initial=None):
        """Frame-to-map point-to-plane ICP (a3d_voxel_map_icp_align_device): Icp.align's loop with the map's association
        in place of the kd-tree, started from `initial` (None: Transform.eye()).  Returns the Transform that maps
        `source` as given into the map's frame; no extract, no tree build, and the map is not changed.  Map and source
        need normals."""
        v = _resident_cloud(self, source, "align").view()
        p = params.to_c()
        init = None if initial is None else C.byref(initial.to_c())
        out = _abi.PoseC()
        _abi.check(self.ctx.lib.a3d_voxel_map_icp_align_device(self.handle, C.byref(p), C.byref(v), init, C.byref(out)),
                   "a3d_voxel_map_icp_align_device")
        return Transform.from_c(out)

    def accumulate(self, source, params, transform):
        """One pass of align's per-point loop under `transform` (test hook, as Icp.accumulate): {H, g, ssq, count}."""
        v = _resident_cloud(self, source, "accumulate").view()
        p = params.to_c()
        t = transform.to_c()
        g = _abi.GnStateC()
        _abi.check(self.ctx.lib.a3d_voxel_map_icp_accumulate_device(self.handle, C.byref(p), C.byref(v), C.byref(t),
                                                                    C.byref(g)), "a3d_voxel_map_icp_accumulate_device")
        return g.as_dict()

    def last_device_ms(self):
        """Device time (ms) of the iteration launches of the most recent align."""
        ms = C.c_float()
        _abi.check(self.ctx.lib.a3d_voxel_map_icp_last_device_ms(self.handle, C.byref(ms)))
        return ms.value

    def render(self, camera, camera_to_world=None, radius=0.0, return_index=False):
        """DevicePointCloud.render over the live map (a3d_voxel_map_render): bit for bit what extract().render(...) gives,
        the index plane (extract rows) included, without a cloud of its own: the model image of frame-to-model tracking,
        with the map's normals and colours when it keeps them.  The map is not changed."""
        return _render(self.ctx, "DeviceVoxelMap.render", camera, camera_to_world, radius, return_index,
                       lambda pose, k, r, d_index, out: self.ctx.lib.a3d_voxel_map_render(
                           self.handle, pose, k.fx, k.fy, k.cx, k.cy, k.width, k.height, r, d_index, out),
                       "a3d_voxel_map_render")

    def clear(self):
        """Empties the map and keeps its allocation; sequence numbers restart at 0."""
        _abi.check(self.ctx.lib.a3d_voxel_map_clear(self.handle), "a3d_voxel_map_clear")

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.a3d_voxel_map_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceTriangleMesh:
    """A triangle mesh resident in HBM, the reference's Geometry (src/io/geometry.rs) with faces: `vertices` is a
    DevicePointCloud with normals (and colours iff the source had them), `d_faces` [len_faces][3] u32 vertex indices in
    device memory.  Made by DeviceTsdfVolume.extract_triangle_mesh; it owns its buffers (`free()`)."""

    def __init__(self, vertices, d_faces, len_faces):
        self.ctx = vertices.ctx
        self.vertices = vertices
        self.d_faces = d_faces
        self.len_faces = int(len_faces)

    @property
    def len_vertices(self):
        return self.vertices.len()

    def download(self):
        """{points [V, 3] f32, normals [V, 3] f32, colors [V, 3] u8 or None, faces [F, 3] u32} on the host: Geometry's
        field names."""
        points, normals = self.vertices.download()
        faces = (self.ctx.to_host(self.d_faces, np.empty((self.len_faces, 3), np.uint32)) if self.len_faces
                 else np.empty((0, 3), np.uint32))
        return {"points": points, "normals": normals, "colors": self.vertices.download_colors(), "faces": faces}

    def free(self):
        if self.vertices is not None:
            self.vertices.free()
        if self.d_faces is not None and self.ctx.handle:
            self.ctx.free(self.d_faces)
        self.d_faces = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceTsdfVolume:
    """A dense truncated signed distance volume in HBM (a3d_tsdf_volume_*): dims = (nx, ny, nz) voxels of pitch voxel_size,
    the centre of voxel (0, 0, 0) at `origin` in the world.  Resident range images are fused into it along their viewing
    rays (integrate: a running mean of the truncated projective distance, capped at max_weight observations; colors=True
    keeps a running mean colour and every image must have colours), and raycast() gives the dense model image a camera
    sees: points, normals from the distance field's gradient, colours, an ordinary DeviceRangeImage for pyramid(),
    MultiscaleAlign and DevicePointCloud.from_range_image.  sample() answers how far a point is from the fused surface
    and in which direction, and align() aligns a resident cloud against that field directly (point-to-SDF ICP: no
    raycast, no camera).  truncation defaults to 4 voxel sizes.  The rules are stated in include/align3d_hip.h; every
    result is the same bits on every run."""

    def __init__(self, ctx, dims, voxel_size, origin, truncation=None, max_weight=64, colors=False):
        try:
            nx, ny, nz = (int(d) for d in dims)
        except (TypeError, ValueError):
            raise TypeError("DeviceTsdfVolume: dims is (nx, ny, nz)") from None
        o = np.ascontiguousarray(origin, np.float32).reshape(-1)
        if o.size != 3:
            raise _abi.InvalidParameter("DeviceTsdfVolume: the origin has three coordinates")
        if min(nx, ny, nz) < 0 or int(max_weight) < 0:
            raise _abi.InvalidParameter("DeviceTsdfVolume: dimensions and max_weight are positive")
        self.ctx = ctx
        self.dims = (nx, ny, nz)
        self.voxel_size = float(voxel_size)
        self.truncation = float(np.float32(4.0) * np.float32(voxel_size)) if truncation is None else float(truncation)
        self.origin = o.copy()
        self.max_weight = int(max_weight)
        self.colors = bool(colors)
        self.handle = C.c_void_p()
        _abi.check(ctx.lib.a3d_tsdf_volume_new(ctx.handle, nx, ny, nz, self.voxel_size, (C.c_float * 3)(*o.tolist()),
                                               self.truncation, self.max_weight, int(self.colors), C.byref(self.handle)),
                   "a3d_tsdf_volume_new")

    def integrate_many(self, images, poses):
        """Fuses resident images of the volume's context, image f seen from the camera pose poses[f] (camera_to_world, a
        Transform), in order and in ONE call: one read and at most one write of the volume per 64 frames."""
        images, poses = list(images), list(poses)
        for im in images:
            if not isinstance(im, DeviceRangeImage):
                raise TypeError(f"DeviceTsdfVolume.integrate takes DeviceRangeImages (got {type(im).__name__}); there is no host fallback")
        for p in poses:
            if not isinstance(p, Transform):
                raise TypeError(f"DeviceTsdfVolume.integrate: camera_to_world is a Transform (got {type(p).__name__})")
        if len(images) != len(poses):
            raise _abi.InvalidParameter(f"DeviceTsdfVolume.integrate_many: {len(images)} images but {len(poses)} poses")
        if not images:
            return
        w2c = (_abi.PoseC * len(poses))(*[p.inverse().to_c() for p in poses])
        _abi.check(self.ctx.lib.a3d_tsdf_volume_integrate(self.handle, _handle_array(images), w2c, len(images)),
                   "a3d_tsdf_volume_integrate")

    def integrate(self, image, camera_to_world):
        """Fuses one resident image seen from camera_to_world."""
        self.integrate_many([image], [camera_to_world])

    def raycast(self, intrinsics, camera_to_world, z_near, z_far, step=None):
        """The model image the camera `intrinsics` (a CameraIntrinsics: its width and height are the image's size) at
        camera_to_world sees: every ray is sampled from z_near to z_far every `step` (default: half the truncation) and
        stops at the first crossing from in front of a surface to behind it.  A new DeviceRangeImage with normals, with
        colours iff the volume keeps them; the volume is not changed."""
        if not isinstance(intrinsics, CameraIntrinsics):
            raise TypeError(f"DeviceTsdfVolume.raycast takes a CameraIntrinsics (got {type(intrinsics).__name__})")
        if not isinstance(camera_to_world, Transform):
            raise TypeError(f"DeviceTsdfVolume.raycast: camera_to_world is a Transform (got {type(camera_to_world).__name__})")
        k = intrinsics
        if k.width < 0 or k.height < 0:
            raise _abi.InvalidParameter(f"DeviceTsdfVolume.raycast: the camera's width and height are the image's size (got {k.width} x {k.height})")
        if step is None:
            step = float(np.float32(0.5) * np.float32(self.truncation))
        pose = camera_to_world.to_c()
        handle = C.c_void_p()
        _abi.check(self.ctx.lib.a3d_tsdf_volume_raycast(self.handle, C.byref(pose), k.fx, k.fy, k.cx, k.cy, k.width, k.height,
                                                        float(z_near), float(z_far), float(step), C.byref(handle)),
                   "a3d_tsdf_volume_raycast")
        return DeviceRangeImage(self.ctx, handle=handle)

    def download(self):
        """(D, W, colours): host arrays [nz, ny, nx] float32 of the fused distance in units of the truncation and of the
        observation count, and [nz, ny, nx, 3] uint8 of the colours (None for a volume without)."""
        nx, ny, nz = self.dims
        rec = np.empty((nz, ny, nx, 2), np.float32)
        col = np.empty((nz, ny, nx), np.uint32) if self.colors else None
        _abi.check(self.ctx.lib.a3d_tsdf_volume_download(self.handle, _abi.ptr(rec), _abi.ptr(col)), "a3d_tsdf_volume_download")
        rgb = None
        if col is not None:
            rgb = np.stack([col & 0xFF, (col >> 8) & 0xFF, (col >> 16) & 0xFF], -1).astype(np.uint8)
        return np.ascontiguousarray(rec[..., 0]), np.ascontiguousarray(rec[..., 1]), rgb

    def upload(self, D, W, colors=None):
        """The inverse of download(): every voxel's D and W ([nz, ny, nx] float32, any bit pattern) and, with `colors`
        ([nz, ny, nx, 3] uint8), every colour; colors=None leaves the colours as they are.  Restores a saved volume."""
        nx, ny, nz = self.dims
        D, W = np.asarray(D, np.float32), np.asarray(W, np.float32)
        if D.shape != (nz, ny, nx) or W.shape != (nz, ny, nx):
            raise _abi.InvalidParameter(f"DeviceTsdfVolume.upload: D and W are [nz, ny, nx] = {(nz, ny, nx)} arrays")
        rec = np.empty((nz, ny, nx, 2), np.float32)
        rec.view(np.uint32)[..., 0], rec.view(np.uint32)[..., 1] = D.view(np.uint32), W.view(np.uint32)  # (NaN payloads too)
        col = None
        if colors is not None:
            c = np.asarray(colors, np.uint8)
            if c.shape != (nz, ny, nx, 3):
                raise _abi.InvalidParameter("DeviceTsdfVolume.upload: colors is a [nz, ny, nx, 3] uint8 array")
            c = c.astype(np.uint32)
            col = np.ascontiguousarray(c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16)
        _abi.check(self.ctx.lib.a3d_tsdf_volume_upload(self.handle, _abi.ptr(rec), _abi.ptr(col)), "a3d_tsdf_volume_upload")

    def _extract(self, min_weight, want_faces, normals, colors):
        """Count-only first, then exactly sized buffers: (vertices: DevicePointCloud, d_faces or None, faces)."""
        ctx, lib = self.ctx, self.ctx.lib
        nv, nf = C.c_uint64(), C.c_uint64()
        _abi.check(lib.a3d_tsdf_volume_extract_surface(self.handle, int(min_weight), int(want_faces), None, None, None, 0, None, 0,
                                                       C.byref(nv), C.byref(nf)), "a3d_tsdf_volume_extract_surface")
        cloud = DevicePointCloud._allocate(ctx, nv.value, normals, colors)
        d_faces = None
        try:
            if want_faces:
                d_faces = ctx.malloc(max(1, nf.value) * 12)
            _abi.check(lib.a3d_tsdf_volume_extract_surface(self.handle, int(min_weight), int(want_faces), cloud.d_points,
                                                           cloud.d_normals, cloud.d_colors, nv.value, d_faces, nf.value,
                                                           C.byref(nv), C.byref(nf)), "a3d_tsdf_volume_extract_surface")
        except BaseException:
            cloud.free()
            if d_faces is not None:
                ctx.free(d_faces)
            raise
        return cloud, d_faces, int(nf.value)

    def extract_point_cloud(self, min_weight=1, normals=True, colors=None):
        """The surface as a new DevicePointCloud that depends on no viewpoint: one point on every axis edge of the voxel
        grid whose ends are both observed at least min_weight times and lie on different sides of the surface (Open3D's
        extract_point_cloud), in voxel order, in the world frame, with the field's gradient as the normal (pointing out of
        the surface; zero beside unobserved voxels) and the nearest voxel's colour.  colors=None: iff the volume keeps
        colours; colors=True on a volume without raises A3D_MISSING_FIELD.  The same bits on every run."""
        colors = self.colors if colors is None else bool(colors)
        return self._extract(min_weight, False, bool(normals), colors)[0]

    def extract_triangle_mesh(self, min_weight=1):
        """The surface as a new DeviceTriangleMesh: marching tetrahedra on the Kuhn split of every cell whose eight
        corners are observed at least min_weight times (about twice the triangles of marching cubes, no ambiguous case),
        wound counter-clockwise seen from outside; the vertices carry normals, and colours iff the volume keeps them."""
        cloud, d_faces, faces = self._extract(min_weight, True, True, self.colors)
        return DeviceTriangleMesh(cloud, d_faces, faces)

    def sample(self, queries, pose=None):
        """The field at every point of `queries` (a3d_tsdf_volume_sample_device), a DevicePointCloud of the volume's
        context or an [m, 3] float32 array (uploaded for the call), moved by `pose` first (None: as they are).  Returns
        host arrays (distance [m] float32, normals [m, 3] float32): the signed metric distance to the fused surface,
        positive in free space, and the unit direction of growing distance in the world frame.  NaN and a zero normal
        where the field has no value (outside the volume, or beside a voxel never observed); the distance with a zero
        normal where it has no direction (at the truncation, or beside a hole).  The volume is not changed."""
        ctx = self.ctx
        d_q, m, own = _device_queries(self, queries, "sample")
        distance, normals = np.empty(m, np.float32), np.empty((m, 3), np.float32)
        if m == 0:
            return distance, normals
        pose = None if pose is None else C.byref(pose.to_c())
        d_dist = d_nrm = None
        try:
            d_dist, d_nrm = ctx.malloc(m * 4), ctx.malloc(m * 12)
            _abi.check(ctx.lib.a3d_tsdf_volume_sample_device(self.handle, d_q, m, pose, d_dist, d_nrm),
                       "a3d_tsdf_volume_sample_device")
            ctx.to_host(d_dist, distance), ctx.to_host(d_nrm, normals)
        finally:
            for p in (own, d_dist, d_nrm):
                if p is not None:
                    ctx.free(p)
        return distance, normals

    def align(self, cloud, params, initial=None):
        """Frame-to-model point-to-plane ICP against the field itself (a3d_tsdf_volume_icp_align_device): Icp.align's loop
        with the field's distance and gradient in place of the kd-tree, started from `initial` (None: Transform.eye()).
        Returns the Transform that maps `cloud` as given into the volume's world frame; no raycast, no pyramid, no
        tree, and the volume is not changed.  The cloud needs normals."""
        v = _resident_cloud(self, cloud, "align").view()
        p = params.to_c()
        init = None if initial is None else C.byref(initial.to_c())
        out = _abi.PoseC()
        _abi.check(self.ctx.lib.a3d_tsdf_volume_icp_align_device(self.handle, C.byref(p), C.byref(v), init, C.byref(out)),
                   "a3d_tsdf_volume_icp_align_device")
        return Transform.from_c(out)

    def accumulate(self, cloud, params, pose=None):
        """One pass of align's per-point loop under `pose` (None: the identity); test hook, as Icp.accumulate:
        {H, g, ssq, count}."""
        v = _resident_cloud(self, cloud, "accumulate").view()
        p = params.to_c()
        t = None if pose is None else C.byref(pose.to_c())
        g = _abi.GnStateC()
        _abi.check(self.ctx.lib.a3d_tsdf_volume_icp_accumulate_device(self.handle, C.byref(p), C.byref(v), t, C.byref(g)),
                   "a3d_tsdf_volume_icp_accumulate_device")
        return g.as_dict()

    def last_device_ms(self):
        """Device time (ms) of the iteration launches of the most recent align."""
        ms = C.c_float()
        _abi.check(self.ctx.lib.a3d_tsdf_volume_icp_last_device_ms(self.handle, C.byref(ms)))
        return ms.value

    def info(self):
        """{dims, voxel_size, truncation, origin, max_weight, colors} as the library holds them (a3d_tsdf_volume_info)."""
        dims, v, tau, o = (C.c_uint64 * 3)(), C.c_float(), C.c_float(), (C.c_float * 3)()
        mw, col = C.c_uint64(), C.c_int32()
        _abi.check(self.ctx.lib.a3d_tsdf_volume_info(self.handle, dims, C.byref(v), C.byref(tau), o, C.byref(mw), C.byref(col)),
                   "a3d_tsdf_volume_info")
        return {"dims": tuple(int(d) for d in dims), "voxel_size": v.value, "truncation": tau.value,
                "origin": tuple(float(x) for x in o), "max_weight": int(mw.value), "colors": bool(col.value)}

    def clear(self):
        """Back to "never observed" everywhere; the allocation stays."""
        _abi.check(self.ctx.lib.a3d_tsdf_volume_clear(self.handle), "a3d_tsdf_volume_clear")

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.a3d_tsdf_volume_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Icp:
    """Icp (src/icp/pcl_icp.rs:15-108): point-to-plane ICP with kd-tree correspondences.  `target` / `source` may be
    PointCloud (host arrays, as in the reference) or DevicePointCloud (already resident)."""

    def __init__(self, ctx, params, target):
        self.ctx = ctx
        self.params = params
        self.target = target
        self.initial_transform = Transform.eye()  # public field the reference ignores (pcl_icp.rs:59)
        self.handle = C.c_void_p()
        p = params.to_c()
        v = target.view()
        fn = ctx.lib.a3d_pcl_icp_new_device if isinstance(target, DevicePointCloud) else ctx.lib.a3d_pcl_icp_new
        _abi.check(fn(ctx.handle, C.byref(p), C.byref(v), C.byref(self.handle)), "Icp::new")

    @staticmethod
    def new(ctx, params, target):
        return Icp(ctx, params, target)

    def align(self, source):
        v = source.view()
        out = _abi.PoseC()
        fn = self.ctx.lib.a3d_pcl_icp_align_device if isinstance(source, DevicePointCloud) else self.ctx.lib.a3d_pcl_icp_align
        _abi.check(fn(self.handle, C.byref(v), C.byref(out)), "Icp::align")
        return Transform.from_c(out)

    def last_device_ms(self):
        ms = C.c_float()
        _abi.check(self.ctx.lib.a3d_pcl_icp_last_device_ms(self.handle, C.byref(ms)))
        return ms.value

    def accumulate(self, source, transform):
        v = source.view()
        t = transform.to_c()
        g = _abi.GnStateC()
        _abi.check(self.ctx.lib.a3d_pcl_icp_accumulate(self.handle, C.byref(v), C.byref(t), C.byref(g)))
        return g.as_dict()

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.a3d_pcl_icp_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class IcpBatch:
    """P independent Icp::new(params, target_p).align(source_p) (src/icp/pcl_icp.rs:31-107) over resident clouds in one
    launch sequence (a3d_pcl_icp_batch_*).  DevicePointCloud only: clouds in host memory go through Icp."""

    def __init__(self, ctx, params, targets):
        self.ctx = ctx
        self.params = params
        self.handle = C.c_void_p()
        self.targets = self._resident(targets, "target")  # kept: the clouds outlive the handle
        self.sources = []
        self.n_pairs = len(self.targets)
        p = params.to_c()
        _abi.check(ctx.lib.a3d_pcl_icp_batch_new_device(ctx.handle, C.byref(p), self.n_pairs, self._views(self.targets),
                                                        C.byref(self.handle)), "IcpBatch::new")

    @staticmethod
    def new(ctx, params, targets):
        return IcpBatch(ctx, params, targets)

    @staticmethod
    def _resident(clouds, what):
        clouds = list(clouds)
        for c in clouds:
            if not isinstance(c, DevicePointCloud):
                raise TypeError(f"IcpBatch takes DevicePointCloud {what}s (got {type(c).__name__}); host clouds go through Icp")
        return clouds

    @staticmethod
    def _views(clouds):
        return (_abi.PointCloudViewC * max(1, len(clouds)))(*[c.view() for c in clouds])

    def _sources(self, sources):
        sources = self._resident(sources, "source")
        if len(sources) != self.n_pairs:
            raise _abi.InvalidParameter(f"IcpBatch of {self.n_pairs} pairs got {len(sources)} sources")
        return sources

    def align(self, sources):
        """Runs all pairs; returns (list of Transform, int32 status array: A3D_OK or A3D_SOLVE_FAILED per pair)."""
        sources = self._sources(sources)
        poses = (_abi.PoseC * max(1, self.n_pairs))()
        status = np.zeros(self.n_pairs, np.int32)
        _abi.check(self.ctx.lib.a3d_pcl_icp_batch_align_device(self.handle, self._views(sources), poses,
                                                               status.ctypes.data_as(C.POINTER(C.c_int32))),
                   "IcpBatch::align")
        self.sources = sources
        return [Transform.from_c(poses[i]) for i in range(self.n_pairs)], status

    def enqueue(self, sources):
        """Enqueues one pass without synchronising the host; results() reads it."""
        sources = self._sources(sources)
        _abi.check(self.ctx.lib.a3d_pcl_icp_batch_align_device(self.handle, self._views(sources), None, None),
                   "IcpBatch::enqueue")
        self.sources = sources  # read by the device until the pass is complete

    def results(self):
        """(list of Transform, int32 status array) of the most recent pass; waits for that pass only."""
        poses = (_abi.PoseC * max(1, self.n_pairs))()
        status = np.zeros(self.n_pairs, np.int32)
        _abi.check(self.ctx.lib.a3d_pcl_icp_batch_results(self.handle, poses, status.ctypes.data_as(C.POINTER(C.c_int32))),
                   "IcpBatch::results")
        return [Transform.from_c(poses[i]) for i in range(self.n_pairs)], status

    def last_device_ms(self):
        ms = C.c_float()
        _abi.check(self.ctx.lib.a3d_pcl_icp_batch_last_device_ms(self.handle, C.byref(ms)))
        return ms.value

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.a3d_pcl_icp_batch_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
