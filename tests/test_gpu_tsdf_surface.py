"""The surface of a TSDF volume on the GPU (a3d_tsdf_volume_extract_surface / a3d_tsdf_volume_upload;
DeviceTsdfVolume.extract_triangle_mesh / extract_point_cloud / upload).

Every comparison is on bits: points, normals, colours, faces and both counts against the numpy restatement
(tsdf_surface_restatement.py, written from the rule in align3d_hip.h) applied to the field the device holds."""
import ctypes as C

import numpy as np
import pytest

import tsdf_surface_restatement as S
from align3d_amd import (A3dError, CameraIntrinsics, Context, DevicePointCloud, DeviceTriangleMesh, DeviceTsdfVolume,
                         DeviceVoxelMap, Icp, IcpParams, RangeImage, RangeImageBuilder, Transform, _abi)
from align3d_amd.range_image import DeviceRangeImage
from data_util import SlamTbSample

pytestmark = pytest.mark.gpu

F = np.float32
OK, INVALID, MISSING = _abi.A3D_OK, _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD

# (dims, voxel size, origin): 16 x 12 x 10, and 67 x 5 x 3 because nx is not a multiple of 64
VOLUMES = {"16x12x10": ((16, 12, 10), 0.1, (-0.8, -0.6, 0.5)), "67x5x3": ((67, 5, 3), 0.03, (-1.0, -0.07, 0.96))}
CAMERA = CameraIntrinsics(21.3, 20.7, 11.5, 9.75, 24, 20)
FUSED_FROM = (Transform.eye(), Transform((0.1, -0.05, 0.0), (0.0, 0.08715574, 0.0, 0.9961947)),
              Transform((-0.12, 0.04, 0.02), (0.0610485, 0.0, 0.0, 0.99813479)), Transform((0.0, 0.1, -0.03), (0.0, 0.0, 0.0, 1.0)),
              Transform((0.05, 0.0, 0.01), (0.0, -0.04361939, 0.0, 0.99904822)))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _frame(seed, cam, depth=(0.15, 1.2)):
    """As test_gpu_tsdf._frame: a seeded range image in the camera's own frame: a smooth surface with a step in it, mask
    holes, and kept pixels whose z is NaN, +-inf, 0 or negative."""
    rng = np.random.default_rng(seed)
    w, h = cam.width, cam.height
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lo, hi = depth
    z = lo + (hi - lo) * (0.5 + 0.5 * np.sin(cols * rng.uniform(0.1, 0.5) + rng.uniform(0, 6)) * np.cos(rows * rng.uniform(0.1, 0.7)))
    z = np.where(cols > w * rng.uniform(0.3, 0.7), z, z * 0.6 + 0.05).astype(F)
    mask = (rng.random((h, w)) < 0.85).astype(np.uint8)
    bad = rng.permutation(w * h)[:6]
    z.reshape(-1)[bad[:min(6, len(bad))]] = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], F)[:len(bad)]
    mask.reshape(-1)[bad] = 1
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        pts = np.stack([(cols - cam.cx) * z64 / cam.fx, (rows - cam.cy) * z64 / cam.fy, z64], -1).astype(F)
    return RangeImage(pts, mask, cam, colors=rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


def _fused(ctx, name, colors):
    """A bumpy wall with holes about a metre in front of five nearby cameras, fused on the device: W runs from 0 to 5."""
    dims, v, origin = VOLUMES[name]
    dev = DeviceTsdfVolume(ctx, dims, v, origin, truncation=0.3 if name == "16x12x10" else 0.09, max_weight=64, colors=colors)
    images = []
    for f in range(len(FUSED_FROM)):
        host = _frame(50 + f, CAMERA, depth=(0.9, 1.15))
        image = DeviceRangeImage(ctx, host)
        if colors:
            image.set_colors(host.colors)
        images.append(image)
    dev.integrate_many(images, FUSED_FROM)
    for image in images:
        image.free()
    return dev


def _restated(dev):
    """The field the device holds, as the restatement's volume."""
    D, W, rgb = dev.download()
    return S.volume_of(D, W, rgb, dev.voxel_size, dev.origin)


def _counts(dev, min_weight, want_faces):
    nv, nf = C.c_uint64(77), C.c_uint64(77)
    st = dev.ctx.lib.a3d_tsdf_volume_extract_surface(dev.handle, min_weight, want_faces, None, None, None, 0, None, 0,
                                                     C.byref(nv), C.byref(nf))
    assert st == OK
    return int(nv.value), int(nf.value)


def _mesh(dev, min_weight=1):
    mesh = dev.extract_triangle_mesh(min_weight)
    try:
        assert isinstance(mesh, DeviceTriangleMesh) and isinstance(mesh.vertices, DevicePointCloud)
        got = mesh.download()
        assert got["points"].shape == (mesh.len_vertices, 3) and got["faces"].shape == (mesh.len_faces, 3)
        assert got["faces"].dtype == np.uint32 and got["normals"].shape == got["points"].shape
        assert (got["colors"] is not None) == dev.colors == mesh.vertices.has_colors()
        return got
    finally:
        mesh.free()


def _cloud(dev, min_weight=1, normals=True, colors=None):
    cloud = dev.extract_point_cloud(min_weight, normals=normals, colors=colors)
    try:
        points, nrm = cloud.download()
        return {"points": points, "normals": nrm, "colors": cloud.download_colors()}
    finally:
        cloud.free()


def _same(got, want, label):
    assert got["points"].shape == want["points"].shape, label
    assert np.array_equal(_bits(got["points"]), _bits(want["points"])), label
    assert np.array_equal(_bits(got["normals"]), _bits(want["normals"])), label
    assert (got["colors"] is None) == (want["colors"] is None), label
    if want["colors"] is not None:
        assert np.array_equal(got["colors"], want["colors"]), label
    if want.get("faces") is not None:
        assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"]), label


def _assert_surface(dev, min_weight, label):
    """Mesh and cloud forms and the count-only calls against the restatement; returns the restated mesh."""
    vol = _restated(dev)
    want_mesh, want_cloud = S.extract(vol, min_weight, True), S.extract(vol, min_weight, False)
    got_mesh, got_cloud = _mesh(dev, min_weight), _cloud(dev, min_weight)
    _same(got_mesh, want_mesh, (label, "mesh"))
    _same(got_cloud, want_cloud, (label, "cloud"))
    assert _counts(dev, min_weight, 1) == (len(want_mesh["points"]), len(want_mesh["faces"])), label
    assert _counts(dev, min_weight, 0) == (len(want_cloud["points"]), 0), label
    keep = np.isin(want_mesh["cls"], S.CLOUD_CLASSES)  # the cloud is the mesh's axis-edge vertices, in order
    assert np.array_equal(_bits(got_cloud["points"]), _bits(got_mesh["points"][keep])), label
    assert np.array_equal(_bits(got_cloud["normals"]), _bits(got_mesh["normals"][keep])), label
    if dev.colors:
        assert np.array_equal(got_cloud["colors"], got_mesh["colors"][keep]), label
    return want_mesh


def _uploaded(ctx, D, W, rgb=None, v=0.1, origin=(0.25, -0.5, 1.0)):
    D = np.asarray(D, F)
    nz, ny, nx = D.shape
    dev = DeviceTsdfVolume(ctx, (nx, ny, nz), v, origin, colors=rgb is not None)
    dev.upload(D, np.asarray(W, F), rgb)
    return dev


# ---- 1. fused volumes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_weight", (1, 2))
@pytest.mark.parametrize("colors", (True, False), ids=("rgb", "plain"))
@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_fused_volumes(ctx, name, colors, min_weight):
    dev = _fused(ctx, name, colors)
    before = dev.download()
    want = _assert_surface(dev, min_weight, (name, colors, min_weight))
    # the case is meaningful: vertices of every class, triangles, normals both present and zeroed beside holes, and
    # min_weight = 2 drops some of what min_weight = 1 keeps
    assert len(want["points"]) > 100 and len(want["faces"]) > 100 and set(want["cls"].tolist()) == set(S.MESH_CLASSES)
    bare = ~_bits(want["normals"]).any(axis=1)
    assert bare.any() and (~bare).any() == (VOLUMES[name][0][2] > 3)  # (three layers leave no room for g* +- ez)
    if min_weight == 2:
        assert len(want["points"]) < len(S.extract(_restated(dev), 1, True)["points"])
    after = dev.download()
    for a, b in zip(before, after):  # the volume is never changed
        assert (a is None and b is None) or np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # without normals, and colours refused or left out on request
    plain = _cloud(dev, min_weight, normals=False, colors=False)
    assert plain["normals"] is None and plain["colors"] is None
    assert np.array_equal(_bits(plain["points"]), _bits(S.extract(_restated(dev), min_weight, False)["points"]))
    dev.free()


# ---- 2. uploaded fields ----------------------------------------------------------------------------------------------

def test_a_sphere_is_closed_and_wound_outwards(ctx):
    """Radius 4.3 voxels in 12^3, every voxel observed: the DEVICE's faces are a closed surface with every edge used once
    in each direction, V - E + F = 2, a positive signed volume near the sphere's, and normals that point outwards."""
    n, r, v = 12, 4.3, 0.1
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    centre = 5.4
    D = ((np.sqrt((i - centre) ** 2 + (j - centre) ** 2 + (k - centre) ** 2) - r) / 4.0).astype(F)
    rgb = np.stack([i * 20, j * 20, k * 20], -1).astype(np.uint8)
    dev = _uploaded(ctx, D, np.ones_like(D), rgb, v=v, origin=(0.0, 0.0, 0.0))
    _assert_surface(dev, 1, "sphere")
    got = _mesh(dev)
    faces, nv = got["faces"], len(got["points"])
    assert S.closed_and_oriented(faces) and len(np.unique(faces)) == nv
    assert S.euler_by_component(faces, nv) == [2]
    volume = S.signed_volume(got["points"], faces)
    assert 0.9 < volume / (4.0 / 3.0 * np.pi * (r * v) ** 3) < 1.0  # (a polyhedron inscribed in the sphere)
    radial = got["points"].astype(np.float64) - centre * v
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(got["normals"], axis=1) - 1.0).max() < 1e-6
    assert np.einsum("ij,ij->i", radial, got["normals"].astype(np.float64)).min() > 0.9
    dev.free()


SPECIAL = F([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-39, -1e-39, 0.5, -0.5, 0.5, -0.5, 3e38, -3e38])


def _special_field(seed, shape=(6, 7, 9)):
    rng = np.random.default_rng(seed)
    D = SPECIAL[rng.integers(0, len(SPECIAL), shape)]  # equal neighbours are common: 14 values
    W = rng.integers(1, 4, shape).astype(F)
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    return D, W, rgb


def test_exact_zeros_signed_zeros_ties_units_and_denormals(ctx):
    D, W, rgb = _special_field(1)
    dev = _uploaded(ctx, D, W, rgb)
    for min_weight in (1, 2, 3, 4):
        want = _assert_surface(dev, min_weight, ("special", min_weight))
        if min_weight == 1:
            f, p = want["faces"], _bits(want["points"])
            degenerate = (p[f[:, 0]] == p[f[:, 1]]).all(axis=1) | (p[f[:, 1]] == p[f[:, 2]]).all(axis=1)
            assert degenerate.any() and (~degenerate).any()  # kept, as the rule says
            assert len(want["points"]) > 500
        if min_weight == 4:
            assert len(want["points"]) == 0 and len(want["faces"]) == 0
    dev.free()


def test_weight_holes_infinite_and_nan_distances(ctx):
    """W = 0 holes cut cells, vertices and (through tri's own W > 0 test) normals; D = +-inf and NaN with W > 0 are not
    valid although tri() still reads them."""
    rng = np.random.default_rng(2)
    D, W, rgb = _special_field(3, (8, 9, 12))
    D = np.where(rng.random(D.shape) < 0.5, rng.normal(size=D.shape).astype(F), D).astype(F)
    W[rng.random(W.shape) < 0.03] = 0
    odd = rng.random(D.shape)
    D[odd < 0.005] = np.inf
    D[(odd >= 0.005) & (odd < 0.01)] = -np.inf
    D[(odd >= 0.01) & (odd < 0.015)] = np.nan
    assert (np.isinf(D) & (W > 0)).any() and (np.isnan(D) & (W > 0)).any() and (W == 0).any()
    dev = _uploaded(ctx, D, W, rgb)
    want = _assert_surface(dev, 1, "holes")
    bare = ~_bits(want["normals"]).any(axis=1)
    assert bare.sum() > 100 and (~bare).sum() > 100 and len(want["faces"]) > 100
    _assert_surface(dev, 2, "holes, min_weight 2")
    dev.free()


def _rippled_ball(shape=(96, 96, 136)):
    """A rippled ball of radius 40 voxels in 136 x 96 x 96 with a sprinkle of unobserved voxels: 4896 blocks of 256 voxels,
    so the block sums are scanned in two tiles (4096 and 800 blocks), and the surface crosses the tiles' border."""
    nz, ny, nx = shape
    k, j, i = np.meshgrid(np.arange(nz, dtype=F), np.arange(ny, dtype=F), np.arange(nx, dtype=F), indexing="ij")
    r = np.sqrt((i - F(68.0)) ** 2 + (j - F(48.0)) ** 2 + (k - F(50.0)) ** 2)
    D = ((r - F(40.3) + F(1.5) * np.sin(i * F(0.7)) * np.cos(j * F(0.5) + k * F(0.3))) / F(4.0)).astype(F)
    W = (np.random.default_rng(8).random(shape) >= 0.003).astype(F)
    return D, W


def test_block_sums_scanned_in_more_than_one_tile(ctx):
    D, W = _rippled_ball()
    dev = _uploaded(ctx, D, W, None, v=0.02, origin=(-1.0, -1.0, 0.5))
    vol = S.volume_of(D, W, None, 0.02, (-1.0, -1.0, 0.5))
    want = S.extract(vol, 1, True)
    assert D.size > 256 * 4096 and len(want["faces"]) > 100000
    first_of_second_tile = 256 * 4096  # vertices and cells on both sides of the tiles' border
    assert (want["voxel"] < first_of_second_tile).sum() > 10000 and (want["voxel"] >= first_of_second_tile).sum() > 10000
    _same(_mesh(dev), want, "two tiles")
    assert _counts(dev, 1, 1) == (len(want["points"]), len(want["faces"]))
    cloud = _cloud(dev)
    keep = np.isin(want["cls"], S.CLOUD_CLASSES)
    assert np.array_equal(_bits(cloud["points"]), _bits(want["points"][keep]))
    assert np.array_equal(_bits(cloud["normals"]), _bits(want["normals"][keep]))
    dev.free()


def test_all_256_sign_patterns_of_one_cell(ctx):
    rng = np.random.default_rng(4)
    dev = DeviceTsdfVolume(ctx, (2, 2, 2), 0.5, (0.0, 1.0, 2.0))
    W = np.ones((2, 2, 2), F)
    triangles = 0
    for pattern in range(256):
        magnitude = rng.uniform(0.05, 1.0, 8).astype(F)
        sign = np.asarray([-1.0 if pattern >> c & 1 else 1.0 for c in range(8)], F)
        dev.upload((magnitude * sign).reshape(2, 2, 2), W)
        vol = _restated(dev)
        want = S.extract(vol, 1, True)
        _same(_mesh(dev), want, pattern)
        assert _counts(dev, 1, 1) == (len(want["points"]), len(want["faces"]))
        triangles += len(want["faces"])
        assert (len(want["faces"]) == 0) == (pattern in (0, 255))
    assert triangles > 256 * 6
    dev.free()


def test_empty_and_uncrossed_volumes_give_nothing(ctx):
    dev = DeviceTsdfVolume(ctx, (16, 12, 10), 0.1, (0.0, 0.0, 0.0), colors=True)
    for want_faces in (0, 1):
        assert _counts(dev, 1, want_faces) == (0, 0)
    got = _mesh(dev)
    assert got["points"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["colors"].shape == (0, 3)
    assert _cloud(dev)["points"].shape == (0, 3)
    for value in (0.75, -0.75):  # observed everywhere, all on one side
        dev.upload(np.full((10, 12, 16), value, F), np.ones((10, 12, 16), F))
        assert _counts(dev, 1, 1) == (0, 0) and _counts(dev, 1, 0) == (0, 0)
        assert _mesh(dev)["points"].shape == (0, 3)
    dev.free()


# ---- 3. capacities, refusals -----------------------------------------------------------------------------------------

def _raw(dev, want_faces, vcap, fcap, normals=True, colors=True, poison=0xA5):
    """One call into poisoned buffers of exactly the capacities: (status, counts, buffers read back)."""
    ctx = dev.ctx
    sizes = {"points": vcap * 12, "normals": vcap * 12 if normals else 0, "colors": vcap * 3 if colors else 0,
             "faces": fcap * 12 if want_faces else 0}
    host = {k: np.full(max(1, n), poison, np.uint8) for k, n in sizes.items()}
    device = {k: (ctx.to_device(host[k]) if sizes[k] or k in ("points", "faces") else None) for k in sizes}
    if not want_faces:
        device["faces"] = None
    nv, nf = C.c_uint64(77), C.c_uint64(77)
    try:
        st = ctx.lib.a3d_tsdf_volume_extract_surface(dev.handle, 1, want_faces, device["points"], device["normals"],
                                                     device["colors"], vcap, device["faces"], fcap, C.byref(nv), C.byref(nf))
        back = {k: ctx.to_host(p, np.empty_like(host[k])) for k, p in device.items() if p is not None}
    finally:
        for p in device.values():
            if p is not None:
                ctx.free(p)
    return st, (int(nv.value), int(nf.value)), back


def test_a_capacity_one_short_writes_nothing(ctx):
    dev = _fused(ctx, "16x12x10", True)
    nv, nf = _counts(dev, 1, 1)
    cv, _ = _counts(dev, 1, 0)
    assert nv > 100 and nf > 100 and 0 < cv < nv
    for want_faces, vcap, fcap in ((1, nv - 1, nf), (1, nv, nf - 1), (1, nv - 1, nf - 1), (0, cv - 1, 0), (1, 0, 0)):
        st, counts, back = _raw(dev, want_faces, vcap, fcap)
        assert st == INVALID and counts == ((nv, nf) if want_faces else (cv, 0)), (want_faces, vcap, fcap)
        for name, buffer in back.items():
            assert (buffer == 0xA5).all(), (want_faces, vcap, fcap, name)  # every byte unchanged
    # exactly enough, and more than enough: the same rows, and nothing behind them is touched
    want = S.extract(_restated(dev), 1, True)
    for extra in (0, 3):
        st, counts, back = _raw(dev, 1, nv + extra, nf + extra)
        assert st == OK and counts == (nv, nf)
        assert np.array_equal(back["points"][:nv * 12].view(np.uint32).reshape(-1, 3), _bits(want["points"]))
        assert np.array_equal(back["normals"][:nv * 12].view(np.uint32).reshape(-1, 3), _bits(want["normals"]))
        assert np.array_equal(back["colors"][:nv * 3].reshape(-1, 3), want["colors"])
        assert np.array_equal(back["faces"][:nf * 12].view(np.uint32).reshape(-1, 3), want["faces"])
        if extra:
            for name, used in (("points", nv * 12), ("normals", nv * 12), ("colors", nv * 3), ("faces", nf * 12)):
                assert (back[name][used:] == 0xA5).all(), name
    # the face arguments are ignored in the point-cloud form
    st, counts, back = _raw(dev, 0, cv, 0, normals=False, colors=False)
    assert st == OK and counts == (cv, 0)
    assert np.array_equal(back["points"].view(np.uint32).reshape(-1, 3), _bits(S.extract(_restated(dev), 1, False)["points"]))
    dev.free()


def _block_address(dev):
    """The device address of the volume's records, read from the handle: a3d_tsdf_volume begins {ctx, nx, ny, nz, max_weight,
    v, tau, ox, oy, oz, with_colors, block} (tsdf.hpp).  The fields in front are checked, so that a changed layout fails
    here and not on the device."""
    words = C.cast(dev.handle, C.POINTER(C.c_uint64))
    dims = C.cast(dev.handle, C.POINTER(C.c_uint32))
    floats = C.cast(dev.handle, C.POINTER(C.c_float))
    assert words[0] == dev.ctx.handle.value and (dims[2], dims[3], dims[4]) == tuple(dev.dims)
    assert floats[6] == F(dev.voxel_size) and floats[8] == F(dev.origin[0])
    return int(words[6])


def test_refusals_on_the_device(ctx):
    plain = _fused(ctx, "16x12x10", False)
    lib = ctx.lib
    nv, nf = _counts(plain, 1, 1)
    block, block_bytes = _block_address(plain), 16 * 12 * 10 * 8
    assert nv > 0 and nf > 0 and nv * 12 + 16 <= block_bytes and nf * 12 <= block_bytes  # (the outputs below lie inside it)
    d_points, d_colors, d_faces = ctx.malloc(nv * 12 + 64), ctx.malloc(nv * 3), ctx.malloc(nf * 12)
    a, b = C.c_uint64(77), C.c_uint64(77)

    def call(points, normals, colors, faces, min_weight=1):
        as_pointer = lambda p: C.c_void_p(p) if isinstance(p, int) else p  # noqa: E731
        return lib.a3d_tsdf_volume_extract_surface(plain.handle, min_weight, 1, as_pointer(points), as_pointer(normals), colors,
                                                   nv, as_pointer(faces), nf, C.byref(a), C.byref(b))

    before = plain.download()
    # a colour output on a volume without colours
    assert call(d_points, None, d_colors, d_faces) == MISSING
    with pytest.raises(A3dError):
        plain.extract_point_cloud(colors=True)
    # outputs that overlap each other
    assert call(d_points, d_points.value + 48, None, d_faces) == INVALID
    assert call(d_points, None, None, d_points) == INVALID
    # outputs that overlap the volume
    assert call(block + 16, None, None, d_faces) == INVALID
    assert call(d_points, block, None, d_faces) == INVALID
    assert call(d_points, None, None, block + block_bytes - nf * 12) == INVALID
    # min_weight out of range
    for bad in (0, (1 << 24) + 1):
        assert call(d_points, None, None, d_faces, min_weight=bad) == INVALID
    assert (a.value, b.value) == (77, 77)  # decided before any launch: the counts are untouched
    assert lib.a3d_tsdf_volume_extract_surface(plain.handle, 1 << 24, 1, None, None, None, 0, None, 0, C.byref(a), C.byref(b)) == OK
    assert (a.value, b.value) == (0, 0)
    assert call(d_points, None, None, d_faces) == OK and (a.value, b.value) == (nv, nf)
    after = plain.download()
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(_bits(before[1]), _bits(after[1]))
    # upload: shapes and colours are checked
    with pytest.raises(A3dError):
        plain.upload(np.zeros((10, 12, 15), F), np.zeros((10, 12, 15), F))
    with pytest.raises(A3dError):
        plain.upload(np.zeros((10, 12, 16), F), np.zeros((10, 12, 16), F), np.zeros((10, 12, 16, 3), np.uint8))
    assert lib.a3d_tsdf_volume_upload(plain.handle, _abi.ptr(np.zeros((10, 12, 16, 2), F)),
                                      _abi.ptr(np.zeros((10, 12, 16), np.uint32))) == MISSING
    for p in (d_points, d_colors, d_faces):
        ctx.free(p)
    plain.free()


def test_upload_then_download_round_trips_every_bit(ctx):
    rng = np.random.default_rng(6)
    shape = (3, 5, 67)
    Dbits = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    Wbits = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    Dbits[0, 0, :4] = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000)  # quiet and signalling NaNs with payloads, -0
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    dev = DeviceTsdfVolume(ctx, (67, 5, 3), 0.03, (0.0, 0.0, 0.0), colors=True)
    dev.upload(Dbits.view(F), Wbits.view(F), rgb)
    D, W, back = dev.download()
    assert np.array_equal(D.view(np.uint32), Dbits) and np.array_equal(W.view(np.uint32), Wbits) and np.array_equal(back, rgb)
    dev.upload(np.zeros(shape, F), np.ones(shape, F))  # colors=None: the colours stay
    D, W, back = dev.download()
    assert not D.view(np.uint32).any() and (W == 1).all() and np.array_equal(back, rgb)
    dev.free()


# ---- 4. the same bits ------------------------------------------------------------------------------------------------

def _both(dev):
    return _mesh(dev), _cloud(dev)


def test_same_bits_on_a_second_run_and_from_the_diagnostics_library(ctx, diag_ctx):
    results = []
    for context in (ctx, ctx, diag_ctx):
        dev = _fused(context, "67x5x3", True)
        results.append((_both(dev), _both(dev)))
        vol = _restated(dev)
        dev.free()
    want_mesh, want_cloud = S.extract(vol, 1, True), S.extract(vol, 1, False)
    assert len(want_mesh["faces"]) > 50
    for runs in results:
        for mesh, cloud in runs:
            _same(mesh, want_mesh, "mesh")
            _same(cloud, want_cloud, "cloud")


def test_same_bits_whatever_scratch_arenas_and_spare_blocks_hold():
    """The masks, offsets and block sums live in scratch region 3 and the volume in a block the context may hand back from
    a freed one: each filled with 0x00, 0xFF and 0x5A before the same calls; a larger volume's extract leaves its own
    leftovers under the smaller one's."""
    own = Context(0)
    dev = _fused(own, "16x12x10", True)
    vol = _restated(dev)
    want_mesh, want_cloud = S.extract(vol, 1, True), S.extract(vol, 1, False)
    mesh, cloud = _both(dev)
    _same(mesh, want_mesh, "before"), _same(cloud, want_cloud, "before")
    dev.free()
    big = _uploaded(own, *_special_field(9, (20, 21, 40)))  # leftovers of another layout in region 3
    _mesh(big)
    big.free()
    for byte in (0x00, 0xFF, 0x5A):
        filled = own.selftest_fill_scratch(byte)
        assert filled[3] > 0 and filled[7] > 0, filled
        dev = _fused(own, "16x12x10", True)
        mesh, cloud = _both(dev)
        _same(mesh, want_mesh, byte), _same(cloud, want_cloud, byte)
        own.selftest_fill_scratch(byte)  # between two calls on the same volume too
        _same(_mesh(dev), want_mesh, byte)
        dev.free()
    own.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------

def test_a_cloud_from_a_fused_sample1_volume_enters_icp_and_the_voxel_map(ctx):
    s = SlamTbSample("sample1")
    ids = s.ids[:3]
    cam0 = CameraIntrinsics(*s.intrinsics(ids[0]), 640, 480)
    built = RangeImageBuilder(ctx).pyramid_levels(3).build_many(cam0, [s.load(i) for i in ids], s.depth_scale(ids[0]))
    levels = [pyramid[2] for pyramid in built]
    world = Transform.from_matrix4(s.rt_cam(ids[0])).inverse()
    poses = [world * Transform.from_matrix4(s.rt_cam(i)) for i in ids]
    dev = DeviceTsdfVolume(ctx, (64, 64, 64), 0.04, (-1.28, -1.28, 0.2), colors=True)
    dev.integrate_many(levels, poses)
    vol = _restated(dev)
    cloud = dev.extract_point_cloud()
    want = S.extract(vol, 1, False)
    points, normals = cloud.download()
    assert cloud.len() == len(want["points"]) > 3000 and cloud.has_colors()
    assert np.array_equal(_bits(points), _bits(want["points"])) and np.array_equal(_bits(normals), _bits(want["normals"]))
    assert np.array_equal(cloud.download_colors(), want["colors"])
    assert _bits(normals).any(axis=1).sum() > 2000
    icp = Icp(ctx, IcpParams.default(), cloud)
    source = DevicePointCloud.from_range_image(levels[1])
    pose = icp.align(source)
    assert np.isfinite(pose.t).all() and np.isfinite(pose.q).all()
    voxel_map = DeviceVoxelMap(ctx, 0.05, colors=True)
    voxel_map.insert(cloud)
    assert 0 < voxel_map.cells() <= cloud.len()
    mesh = dev.extract_triangle_mesh(2)
    assert mesh.len_faces > 1000 and mesh.len_vertices > 1000
    for thing in (mesh, voxel_map, icp, source, cloud, dev):
        thing.free()
    for pyramid in built:
        for lv in pyramid:
            lv.free()
