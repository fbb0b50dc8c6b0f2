"""Colours on resident point clouds on the GPU: from range images (a3d_range_image_to_point_clouds_rgb), through the
merge (a3d_point_clouds_merge_rgb_device), a transform (a copy) and the voxel-grid downsample
(a3d_point_clouds_voxel_downsample_rgb_device).

A colour is a payload that follows its point, so the expected colour of an output row is colors_in[index], `index` from
the mask or from the numpy restatement (voxel_restatement.py), never from the code under test.  Input colours identify
their row (colors_util.row_colors).  Every output goes into a buffer filled with a canary byte from end to end with guard
bytes on both sides (colors_util.Guarded): colour buffers start 4-byte aligned and end wherever 3 * capacity ends, and
every byte past 3 * out_len must still hold the canary.  Points, normals, indices and counts must be the bits the entry
without colours writes in the same test."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import voxel_restatement as V
from align3d_amd import (A3dError, CameraIntrinsics, DevicePointCloud, PointCloud, RangeImage, RangeImageBuilder,
                         Transform, _abi)
from align3d_amd.range_image import DeviceRangeImage
from colors_util import Guarded, check_rows, row_colors, untouched
from data_util import SlamTbSample
from gpu_util import oracle_frame, to_range_image

pytestmark = pytest.mark.gpu

MERGE_LENS = (1, 0, 63, 64, 65, 2, 2047, 2049)
SIZES = (0, 1, 63, 64, 65, 2047, 2049)
VOXELS = (0.02, 0.5, 1e3)
SPARE_ROWS = 3
OK, INVALID, MISSING = _abi.A3D_OK, _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the recipe of test_gpu_voxel_map.py): NaNs, infinities, -0.0 and far outliers occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _uniform(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.25, 3.25, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def _device_cloud(ctx, points, normals, colors):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[None if b is None else b.ptr for b in bufs])


# ---- from images ----------------------------------------------------------------------------------------------------

def _from_images(ctx, images, normals, colors, caps, rgb=True):
    """The raw batch call into guarded buffers.  normals / colors: per image, whether an output is passed.  Returns
    (status, lens, points bufs, normals bufs, colours bufs)."""
    n = len(images)
    gp = [Guarded(ctx, 12 * c) for c in caps]
    gn = [Guarded(ctx, 12 * c) if want else None for c, want in zip(caps, normals)]
    gc = [Guarded(ctx, 3 * c) if want else None for c, want in zip(caps, colors)]
    handles = (C.c_void_p * n)(*[im.handle for im in images])
    lens = (C.c_uint64 * n)(*[12345] * n)
    c_caps = (C.c_uint64 * n)(*caps)
    if rgb:
        st = ctx.lib.a3d_range_image_to_point_clouds_rgb(handles, n, _ptrs(gp), _ptrs(gn), _ptrs(gc), c_caps, lens)
    else:
        st = ctx.lib.a3d_range_image_to_point_clouds(handles, n, _ptrs(gp), _ptrs(gn), c_caps, lens)
    return st, [int(x) for x in lens], gp, gn, gc


def _check_image_batch(ctx, images, hosts, rgbs, label):
    """Every image of the batch against its host arrays: colours rgb[mask != 0], points and normals the bits of the
    entry without colours.  rgbs[i] None: the image has no colours and gets a NULL entry."""
    caps = [h.mask.size for h in hosts]
    normals = [h.normals is not None for h in hosts]
    colors = [r is not None for r in rgbs]
    st, lens, gp, gn, gc = _from_images(ctx, images, normals, colors, caps)
    st0, lens0, gp0, gn0, _ = _from_images(ctx, images, normals, [False] * len(images), caps, rgb=False)
    assert st == OK and st0 == OK and lens == lens0, label
    for i, (host, rgb) in enumerate(zip(hosts, rgbs)):
        keep = host.mask.reshape(-1) != 0
        assert lens[i] == int(keep.sum()), (label, i)
        old_points, _ = gp0[i].read()
        check_rows(gp0[i], lens[i], host.points.reshape(-1, 3)[keep], 12, f"{label} old points {i}")
        check_rows(gp[i], lens[i], old_points[:12 * lens[i]], 12, f"{label} points {i}")
        if normals[i]:
            old_normals, _ = gn0[i].read()
            check_rows(gn0[i], lens[i], host.normals.reshape(-1, 3)[keep], 12, f"{label} old normals {i}")
            check_rows(gn[i], lens[i], old_normals[:12 * lens[i]], 12, f"{label} normals {i}")
        if rgb is not None:
            check_rows(gc[i], lens[i], rgb.reshape(-1, 3)[keep], 3, f"{label} colours {i}")


def _synthetic(seed, h, w, mask, normals=True):
    pts = _raw_bits(seed, h * w).reshape(h, w, 3)
    nrm = _raw_bits(seed + 1000, h * w).reshape(h, w, 3) if normals else None
    return RangeImage(pts, np.ascontiguousarray(mask, np.uint8).reshape(h, w), CameraIntrinsics(500.0, 500.0, w / 2, h / 2, w, h),
                      normals=nrm)


def _masks(h, w):
    checker = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    last = np.zeros((h, w), np.uint8)
    last[-1, -1] = 2
    return {"all set": np.full((h, w), 1, np.uint8), "none set": np.zeros((h, w), np.uint8), "checkerboard": checker,
            "only the last pixel": last}


def test_from_images_fixture_frame_through_the_builder_and_uploaded(ctx):
    s = SlamTbSample("sample1")
    depth, rgb = s.load(0)
    fr = oracle_frame("sample1", 0)
    host = to_range_image(fr)
    built = RangeImageBuilder(ctx).pyramid_levels(1).build(CameraIntrinsics(*s.intrinsics(0), 640, 480), depth, rgb,
                                                           s.depth_scale(0))[0]
    uploaded = DeviceRangeImage(ctx, host)
    assert built.has_colors() and not uploaded.has_colors()
    uploaded.set_colors(rgb)
    assert uploaded.has_colors()
    built_host = built.download()  # (its mask is the kernels' input, and the oracle's)
    assert np.array_equal(built_host.mask, fr.mask)
    _check_image_batch(ctx, [built, uploaded], [built_host, host], [rgb, rgb], "sample1 frame 0")
    # the Python wrapper: opt-in, the host path's colours
    want = PointCloud.from_range_image(host)
    assert want.len() == 270213 and np.array_equal(want.colors, rgb.reshape(-1, 3)[fr.mask.reshape(-1) != 0])
    plain, coloured = DevicePointCloud.from_range_image(built), DevicePointCloud.from_range_image(built, colors=True)
    assert not plain.has_colors() and plain.download_colors() is None and len(plain.download()) == 2
    assert coloured.has_colors() and np.array_equal(coloured.download_colors(), want.colors)
    for x in (plain, coloured, built, uploaded):
        x.free()


@pytest.mark.parametrize("shape", [(8, 8), (64, 1), (65, 33)])
def test_from_images_synthetic_masks(ctx, shape):
    h, w = shape
    hosts, rgbs, images = [], [], []
    for k, (name, mask) in enumerate(_masks(h, w).items()):
        hosts.append(_synthetic(10 * k + h, h, w, mask, normals=bool(k % 2)))
        rgbs.append(row_colors(k, h * w).reshape(h, w, 3))
        images.append(DeviceRangeImage(ctx, hosts[-1]).set_colors(rgbs[-1]))
    _check_image_batch(ctx, images, hosts, rgbs, f"{h}x{w}")  # one batch ...
    for im, host, rgb in zip(images, hosts, rgbs):            # ... and each alone
        _check_image_batch(ctx, [im], [host], [rgb], f"{h}x{w} alone")
    for im in images:
        im.free()


def test_from_images_mixed_batch_and_missing_field(ctx):
    h, w = 65, 33
    mask = _masks(h, w)["checkerboard"]
    hosts = [_synthetic(1, h, w, mask), _synthetic(2, h, w, mask)]
    rgb = row_colors(0, h * w).reshape(h, w, 3)
    images = [DeviceRangeImage(ctx, hosts[0]).set_colors(rgb), DeviceRangeImage(ctx, hosts[1])]
    assert images[0].has_colors() and not images[1].has_colors()
    _check_image_batch(ctx, images, hosts, [rgb, None], "mixed batch")
    # colours asked of the image without them: decided before any launch, nothing written for either image
    st, lens, gp, gn, gc = _from_images(ctx, images, [True, True], [True, True], [h * w] * 2)
    assert st == MISSING and lens == [12345, 12345]
    for buf in (*gp, *gn, *gc):
        untouched(buf, "missing field")
    with pytest.raises(A3dError) as e:
        DevicePointCloud.from_range_images(images, colors=True)
    assert e.value.status == MISSING
    # a capacity one short for one image: nothing written for any, colours included; every count reported
    kept = int((mask != 0).sum())
    st, lens, gp, gn, gc = _from_images(ctx, images, [True, True], [True, False], [kept - 1, kept])
    assert st == INVALID and lens == [kept, kept]
    for buf in (*gp, *gn, gc[0]):
        untouched(buf, "capacity one short")
    for im in images:
        im.free()


# ---- merge ----------------------------------------------------------------------------------------------------------

def _merge(ctx, clouds, poses, capacity, rgb=True, colors="own"):
    n = len(clouds)
    gp, gn, gc = Guarded(ctx, 12 * capacity), Guarded(ctx, 12 * capacity), Guarded(ctx, 3 * capacity) if rgb else None
    views = DevicePointCloud._views(clouds)
    c_poses = None if poses is None else (_abi.PoseC * n)(*poses)
    out_len = C.c_uint64(12345)
    if rgb:
        d_colors = DevicePointCloud._colors_array(clouds) if colors == "own" else colors
        st = ctx.lib.a3d_point_clouds_merge_rgb_device(ctx.handle, views, d_colors, c_poses, n, gp.ptr, gn.ptr, gc.ptr,
                                                       capacity, C.byref(out_len))
    else:
        st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, views, c_poses, n, gp.ptr, gn.ptr, capacity, C.byref(out_len))
    return st, int(out_len.value), gp, gn, gc


@pytest.mark.parametrize("with_poses", [False, True])
def test_merge_every_start_offset_mod_4(ctx, with_poses):
    starts = np.concatenate([[0], np.cumsum(MERGE_LENS)[:-1]]) * 3
    total = sum(MERGE_LENS)
    assert {int(s) % 4 for s, n in zip(starts, MERGE_LENS) if n} == {0, 1, 2, 3} and (3 * total) % 4 != 0
    hosts = [_uniform(300 + j, n) + (row_colors(j, n),) for j, n in enumerate(MERGE_LENS)]
    clouds = [_device_cloud(ctx, *h) for h in hosts]
    rng = np.random.default_rng(5)
    poses = [O.exp_se3(rng.uniform(-0.6, 0.6, size=6).astype(np.float32)) for _ in MERGE_LENS] if with_poses else None
    want_colors = np.concatenate([c for _, _, c in hosts])
    st0, len0, gp0, gn0, _ = _merge(ctx, clouds, poses, total + SPARE_ROWS, rgb=False)
    st, out_len, gp, gn, gc = _merge(ctx, clouds, poses, total + SPARE_ROWS)
    assert st == OK and st0 == OK and out_len == len0 == total
    old_points, old_normals = gp0.read()[0], gn0.read()[0]
    if not with_poses:  # (under poses the old entry is checked against the oracle by test_gpu_cloud_transform.py)
        assert np.array_equal(old_points[:12 * total], np.concatenate([p for p, _, _ in hosts]).view(np.uint8).reshape(-1))
    check_rows(gp, total, old_points[:12 * total], 12, "merged points")
    check_rows(gn, total, old_normals[:12 * total], 12, "merged normals")
    check_rows(gc, total, want_colors, 3, "merged colours")
    gp0.free(), gn0.free()
    # a capacity of total - 1 writes nothing and reports the total
    st, out_len, gp, gn, gc = _merge(ctx, clouds, poses, total - 1)
    assert st == INVALID and out_len == total
    for buf in (gp, gn, gc):
        untouched(buf, "capacity total - 1")
    # the wrapper: colours follow the rule of normals
    t = None if poses is None else [Transform.from_c(p) for p in poses]
    merged = DevicePointCloud.merge(clouds, t)
    assert merged.has_colors() and np.array_equal(merged.download_colors(), want_colors)
    plain = DevicePointCloud.merge(clouds, t, colors=False)
    assert not plain.has_colors()
    assert np.array_equal(plain.download()[0].view(np.uint32), merged.download()[0].view(np.uint32))
    bare = _device_cloud(ctx, hosts[2][0], hosts[2][1], None)
    with pytest.raises(_abi.InvalidParameter):
        DevicePointCloud.merge([clouds[0], bare], None)
    mixed = DevicePointCloud.merge([clouds[0], bare], None, colors=False)
    assert not mixed.has_colors() and mixed.len() == 1 + 63
    # the C entry: a colour output with a cloud that has none is A3D_MISSING_FIELD and writes nothing
    st, out_len, gp, gn, gc = _merge(ctx, [clouds[0], bare], None, 64 + SPARE_ROWS)
    assert st == MISSING and out_len == 12345
    for buf in (gp, gn, gc):
        untouched(buf, "missing field")
    for x in (merged, plain, bare, mixed, *clouds):
        x.free()


def test_transformed_copies_the_colours_and_in_place_leaves_them(ctx):
    n = 2049
    points, normals = _uniform(7, n)
    colors = row_colors(4, n)
    cloud = _device_cloud(ctx, points, normals, colors)
    pose = Transform.from_c(O.exp_se3(np.asarray([0.3, -0.2, 0.1, 0.4, 0.5, 0.3], np.float32)))
    moved = cloud.transformed(pose)
    assert moved.has_colors() and moved.d_colors.value != cloud.d_colors.value
    assert np.array_equal(moved.download_colors(), colors)
    assert np.array_equal(moved.download()[0].view(np.uint32), O.transform_points(pose.to_c(), points).view(np.uint32))
    address = cloud.d_colors.value
    assert cloud.transform_(pose) is cloud and cloud.d_colors.value == address
    assert np.array_equal(cloud.download_colors(), colors)
    assert np.array_equal(cloud.download()[0].view(np.uint32), moved.download()[0].view(np.uint32))
    bare = _device_cloud(ctx, points, normals, None)
    bare_moved = bare.transformed(pose)
    assert not bare_moved.has_colors()
    for x in (cloud, moved, bare, bare_moved):
        x.free()


# ---- downsample -----------------------------------------------------------------------------------------------------

def _downsample(ctx, clouds, voxel, caps, rgb=True, want_colors=None):
    """The raw batch call into guarded buffers; want_colors[i] False: NULL entries for cloud i's colours, in and out."""
    n = len(clouds)
    want_colors = [rgb] * n if want_colors is None else want_colors
    gp = [Guarded(ctx, 12 * c) for c in caps]
    gn = [Guarded(ctx, 12 * c) for c in caps]
    gi = [Guarded(ctx, 4 * c) for c in caps]
    gc = [Guarded(ctx, 3 * c) if want else None for c, want in zip(caps, want_colors)]
    lens, dropped = (C.c_uint64 * n)(*[12345] * n), (C.c_uint64 * n)(*[12345] * n)
    views, c_caps = DevicePointCloud._views(clouds), (C.c_uint64 * n)(*caps)
    if rgb:
        d_colors = (C.c_void_p * n)(*[c.d_colors if want else None for c, want in zip(clouds, want_colors)])
        st = ctx.lib.a3d_point_clouds_voxel_downsample_rgb_device(ctx.handle, views, d_colors, n, voxel, None, _ptrs(gp),
                                                                  _ptrs(gn), _ptrs(gc), _ptrs(gi), c_caps, lens, dropped)
    else:
        st = ctx.lib.a3d_point_clouds_voxel_downsample_device(ctx.handle, views, n, voxel, None, _ptrs(gp), _ptrs(gn),
                                                              _ptrs(gi), c_caps, lens, dropped)
    return st, [int(x) for x in lens], [int(x) for x in dropped], gp, gn, gi, gc


def _check_downsample(ctx, clouds, hosts, voxel, want_colors, label):
    caps = [len(h[0]) + SPARE_ROWS for h in hosts]
    st, lens, dropped, gp, gn, gi, gc = _downsample(ctx, clouds, voxel, caps, want_colors=want_colors)
    st0, lens0, dropped0, gp0, gn0, gi0, _ = _downsample(ctx, clouds, voxel, caps, rgb=False)
    assert st == OK and st0 == OK and lens == lens0 and dropped == dropped0, label
    for i, (points, normals, colors) in enumerate(hosts):
        exp_p, exp_n, exp_i, exp_dropped = V.voxel_downsample_cloud(points, normals, voxel)
        k = len(exp_i)
        assert lens[i] == k and dropped[i] == exp_dropped, (label, i)
        old = [b.read()[0] for b in (gp0[i], gn0[i], gi0[i])]
        check_rows(gp0[i], k, exp_p, 12, f"{label} old points {i}")
        check_rows(gn0[i], k, exp_n, 12, f"{label} old normals {i}")
        check_rows(gi0[i], k, exp_i, 4, f"{label} old index {i}")
        check_rows(gp[i], k, old[0][:12 * k], 12, f"{label} points {i}")
        check_rows(gn[i], k, old[1][:12 * k], 12, f"{label} normals {i}")
        check_rows(gi[i], k, old[2][:4 * k], 4, f"{label} index {i}")
        if want_colors[i]:
            check_rows(gc[i], k, colors[exp_i], 3, f"{label} colours {i}")
    return lens


@pytest.fixture(scope="module")
def sized_clouds(ctx):
    hosts = [_uniform(400 + j, n) + (row_colors(j, n),) for j, n in enumerate(SIZES)]
    clouds = [_device_cloud(ctx, *h) for h in hosts]
    yield hosts, clouds
    for c in clouds:
        c.free()


@pytest.mark.parametrize("voxel", VOXELS)
def test_downsample_sizes_one_cloud_per_call(ctx, sized_clouds, voxel):
    hosts, clouds = sized_clouds
    kept = []
    for host, cloud in zip(hosts, clouds):
        kept += _check_downsample(ctx, [cloud], [host], voxel, [True], f"v = {voxel}, n = {len(host[0])}")
    if voxel == 1e3:
        assert kept == [min(n, 1) for n in SIZES]  # everything in one cell: the winner is rarely row 0
    if voxel == 0.5:
        assert kept[-1] < SIZES[-1] // 4  # cells are shared: most rows lose


def test_downsample_all_sizes_in_one_call_with_one_cloud_lacking_colours(ctx, sized_clouds):
    hosts, clouds = sized_clouds
    bare_at = 4
    bare = _device_cloud(ctx, hosts[bare_at][0], hosts[bare_at][1], None)
    batch = [bare if i == bare_at else c for i, c in enumerate(clouds)]
    want = [i != bare_at for i in range(len(SIZES))]
    for voxel in VOXELS:
        _check_downsample(ctx, batch, hosts, voxel, want, f"one call, v = {voxel}")
    # a colour output for the cloud without colours: A3D_MISSING_FIELD, nothing written for any cloud
    caps = [n + SPARE_ROWS for n in SIZES]
    gp = [Guarded(ctx, 12 * c) for c in caps]
    gc = [Guarded(ctx, 3 * c) for c in caps]
    n = len(batch)
    lens = (C.c_uint64 * n)(*[12345] * n)
    st = ctx.lib.a3d_point_clouds_voxel_downsample_rgb_device(
        ctx.handle, DevicePointCloud._views(batch), DevicePointCloud._colors_array(batch), n, 0.5, None, _ptrs(gp), None,
        _ptrs(gc), None, (C.c_uint64 * n)(*caps), lens, None)
    assert st == MISSING and list(lens) == [12345] * n
    for buf in (*gp, *gc):
        untouched(buf, "missing field")
    # the wrappers: a result has colours iff its input has them
    outs = DevicePointCloud.voxel_downsample_many(batch, 0.5)
    for i, (out, host) in enumerate(zip(outs, hosts)):
        index, _ = V.voxel_downsample(host[0], 0.5)
        assert out.has_colors() == want[i] and out.len() == len(index)
        if want[i]:
            assert np.array_equal(out.download_colors(), host[2][index])
        out.free()
    thin, index = clouds[-1].voxel_downsample(0.5, return_index=True)
    assert np.array_equal(thin.download_colors(), hosts[-1][2][index])
    thin.free(), bare.free()


def test_downsample_hostile_bit_patterns_and_a_capacity_one_short(ctx):
    n = 2049
    points, normals, colors = _raw_bits(77, n), _raw_bits(78, n), row_colors(9, n)
    tame = np.random.default_rng(79).uniform(-3.0, 3.0, size=(n // 2, 3)).astype(np.float32)
    points[1::2][:len(tame)] = tame  # half the rows are kept, among NaN, infinite and far rows that are dropped
    cloud = _device_cloud(ctx, points, normals, colors)
    index, dropped = V.voxel_downsample(points, 0.5)
    assert dropped > n // 4 and n // 4 < len(index) < n - dropped
    _check_downsample(ctx, [cloud], [(points, normals, colors)], 0.5, [True], "raw bits")
    st, lens, drop, gp, gn, gi, gc = _downsample(ctx, [cloud], 0.5, [len(index) - 1])
    assert st == INVALID and lens == [len(index)] and drop == [dropped]
    for buf in (*gp, *gn, *gi, *gc):
        untouched(buf, "capacity one short")
    cloud.free()
