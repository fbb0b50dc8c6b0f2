"""Voxel-grid downsampling by cell mean (a3d_point_clouds_voxel_mean_device, DevicePointCloud.voxel_downsample(mode="mean")
/ voxel_downsample_many) on the GPU.

Every comparison is on uint32 / uint8 views, bit for bit, and the expected value is always the numpy restatement of the
rule (voxel_mean_restatement.py), never the code under test.  The raw call writes into buffers that are filled with a
canary from end to end, with CANARY_WORDS more of it on both sides (the _Guarded recipe of test_gpu_voxel_downsample.py;
colour buffers are bytes, so theirs is a byte canary): whatever the call did not have to write must still hold it."""
import ctypes as C

import numpy as np
import pytest

import voxel_mean_restatement as M
import voxel_restatement as V
from align3d_amd import DevicePointCloud, InvalidParameter, PointCloud, _abi

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 2047, 2049, 270213)
VOXELS = (0.005, 0.02, 0.1, 1e3, 1e-5)  # 1e3: everything in one cell (N = len); 1e-5: every point alone
ORIGINS = (None, (0.013, -0.4, 7.5))
CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)
CANARY_BYTE = np.uint8(0xA5)
FIELDS = ("points", "normals", "colors", "index", "counts")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uniform(seed, n, with_normals=True, with_colors=True):
    """([n, 3] seeded points in the cube [0.25, 3.25)^3, normals or None, colours or None): the cube lies inside one cell
    of a 1e3 grid under both ORIGINS."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(0.25, 3.25, size=(n, 3)).astype(np.float32)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    normals /= np.maximum(np.linalg.norm(normals, axis=1), np.float32(1e-6))[:, None]
    colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    return points, (normals if with_normals else None), (colors if with_colors else None)


def _raw_bits(seed, n):
    """[n, 3] raw random bits: NaNs with payloads, infinities, -0.0, denormals and magnitudes far beyond the cell range."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _device_cloud(ctx, points, normals=None, colors=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


class _Guarded:
    """A device buffer of `count` rows of `width` elements (uint32 words, or bytes for colours), canary-filled from end to
    end, CANARY_WORDS more elements on both sides."""

    def __init__(self, ctx, count, width, dtype=np.uint32):
        self.ctx, self.count, self.width, self.dtype = ctx, count, width, dtype
        self.canary = CANARY if dtype == np.uint32 else CANARY_BYTE
        self.items = 2 * CANARY_WORDS + width * count
        self.base = ctx.to_device(np.full(self.items, self.canary, dtype))
        self.ptr = C.c_void_p(self.base.value + np.dtype(dtype).itemsize * CANARY_WORDS)

    def read(self):
        """(the body as [count, width], True iff both guards are intact)."""
        w = self.ctx.to_host(self.base, np.empty(self.items, self.dtype))
        body = w[CANARY_WORDS:self.items - CANARY_WORDS].reshape(self.count, self.width)
        return body, bool((w[:CANARY_WORDS] == self.canary).all() and (w[self.items - CANARY_WORDS:] == self.canary).all())

    def free(self):
        self.ctx.free(self.base)


def _call(ctx, clouds, voxel, origin, normals=True, colors=True, index=True, counts=True, capacities=None):
    """The raw call on resident clouds into guarded buffers.  Returns (status, lens, dropped, per cloud {field: body or
    None, field + "_canary": its canary}); asserts the guards."""
    n = len(clouds)
    caps = [c.len() for c in clouds] if capacities is None else list(capacities)
    g = {"points": [_Guarded(ctx, k, 3) for k in caps],
         "normals": [_Guarded(ctx, k, 3) if normals and c.d_normals is not None else None for c, k in zip(clouds, caps)],
         "colors": [_Guarded(ctx, k, 3, np.uint8) if colors and c.d_colors is not None else None for c, k in zip(clouds, caps)],
         "index": [_Guarded(ctx, k, 1) if index else None for k in caps],
         "counts": [_Guarded(ctx, k, 1) if counts else None for k in caps]}
    lens, dropped = (C.c_uint64 * n)(*[12345] * n), (C.c_uint64 * n)(*[12345] * n)
    o = None if origin is None else (C.c_float * 3)(*origin)
    views = (_abi.PointCloudViewC * n)(*[c.view() for c in clouds])

    def ptrs(name, wanted=True):
        return (C.c_void_p * n)(*[x.ptr if x else None for x in g[name]]) if wanted else None

    st = ctx.lib.a3d_point_clouds_voxel_mean_device(
        ctx.handle, views, (C.c_void_p * n)(*[c.d_colors for c in clouds]), n, voxel, o, ptrs("points"),
        ptrs("normals", normals), ptrs("colors", colors), ptrs("index", index), ptrs("counts", counts), (C.c_uint64 * n)(*caps),
        lens, dropped)
    outs = []
    for i in range(n):
        out = {}
        for name in FIELDS:
            buf = g[name][i]
            out[name] = None
            if buf is not None:
                out[name], intact = buf.read()
                out[name + "_canary"] = buf.canary
                assert intact, f"the call wrote outside its {name} buffer"
                buf.free()
        outs.append(out)
    return st, list(lens), list(dropped), outs


def _assert_matches(out, got_len, got_dropped, expected):
    """One cloud's buffers against the restatement; everything behind the rows still holds the canary."""
    exp_p, exp_n, exp_c, exp_i, exp_k, exp_dropped = expected
    m = len(exp_i)
    assert (got_len, got_dropped) == (m, exp_dropped)
    want = {"points": _bits(exp_p).reshape(-1, 3), "normals": None if exp_n is None else _bits(exp_n).reshape(-1, 3),
            "colors": exp_c, "index": exp_i[:, None], "counts": exp_k[:, None]}
    for name in FIELDS:
        if out[name] is not None:
            bad = np.flatnonzero((out[name][:m] != want[name]).any(axis=1))
            assert bad.size == 0, (name, bad[:5], out[name][bad[:5]], want[name][bad[:5]], exp_k[bad[:5]])
            assert (out[name][m:] == out[name + "_canary"]).all(), name


def _rows(p, n, c, k):
    cols = [_bits(p)] + ([] if n is None else [_bits(n)]) + ([] if c is None else [c.astype(np.uint32)])
    r = np.concatenate(cols + [k.astype(np.uint32)[:, None]], axis=1)
    return r[np.lexsort(r.T[::-1])]


@pytest.mark.parametrize("n", SIZES)
def test_size_and_parameter_grid(ctx, n):
    points, normals, colors = _uniform(100 + n % 97, n)
    full, bare = _device_cloud(ctx, points, normals, colors), _device_cloud(ctx, points)
    for voxel in VOXELS:
        for origin in ORIGINS:
            expected = M.voxel_mean(points, normals, colors, voxel, origin)
            if n <= 2049 or voxel == 0.02:  # len and dropped are the nearest-point downsample's
                near_index, near_dropped = V.voxel_downsample(points, voxel, origin)
                assert len(expected[3]) == len(near_index) and expected[5] == near_dropped
            if voxel == 1e3 and n:
                assert expected[4].tolist() == [n]
            if voxel == 1e-5 and n == 2047:
                assert (expected[4] == 1).all()
            if voxel == 0.1 and n == 270213:
                assert 20000 < len(expected[3]) <= 31 ** 3
                err = np.abs(expected[0].astype(np.float64) - M.exact_mean(points, voxel, origin)).max()
                assert err <= M.error_bound(points, voxel, origin)
            st, lens, dropped, outs = _call(ctx, [full], voxel, origin)
            assert st == _abi.A3D_OK, (n, voxel, origin)
            assert all(outs[0][f] is not None for f in FIELDS)
            _assert_matches(outs[0], lens[0], dropped[0], expected)
            # the same points without normals, colours, index or counts: the same points
            st, lens, dropped, outs = _call(ctx, [bare], voxel, origin, index=False, counts=False)
            assert st == _abi.A3D_OK and all(outs[0][f] is None for f in FIELDS[1:])
            _assert_matches(outs[0], lens[0], dropped[0], expected)
    # every combination of the optional outputs, once
    expected = M.voxel_mean(points, normals, colors, 0.1, ORIGINS[1])
    for with_n, with_c, with_i, with_k in ((True, False, False, True), (False, True, True, False), (False, False, True, True),
                                           (True, True, False, False)):
        st, lens, dropped, outs = _call(ctx, [full], 0.1, ORIGINS[1], normals=with_n, colors=with_c, index=with_i, counts=with_k)
        assert st == _abi.A3D_OK
        assert [outs[0][f] is not None for f in FIELDS[1:]] == [with_n, with_c, with_i, with_k]
        _assert_matches(outs[0], lens[0], dropped[0], expected)
    full.free(), bare.free()


def test_hostile_bit_patterns_as_points_and_as_normals(ctx):
    for k, n in enumerate((65, 2049, 100003)):
        points, normals = _raw_bits(4000 + k, n), _raw_bits(5000 + k, n)
        colors = np.random.default_rng(k).integers(0, 256, size=(n, 3), dtype=np.uint8)
        assert np.isnan(points).any() and np.isinf(points).any() and np.isnan(normals).any()
        cloud = _device_cloud(ctx, points, normals, colors)
        for voxel, origin in ((0.02, None), (1e3, (0.5, -2.0, 1e-3)), (64.0, None)):
            expected = M.voxel_mean(points, normals, colors, voxel, origin)
            if n == 100003:
                assert expected[5] > 0 and len(expected[3]) > 0
            st, lens, dropped, outs = _call(ctx, [cloud], voxel, origin)
            assert st == _abi.A3D_OK
            _assert_matches(outs[0], lens[0], dropped[0], expected)
        cloud.free()
    # hostile normals on points that do share cells: rows that count and rows that do not, in one cell
    points, _, colors = _uniform(7, 20000)
    normals = _raw_bits(6000, 20000)
    normals[::3] = _uniform(8, 20000)[1][::3]
    normals[5::7] = np.float32([3.0, 0.0, 0.0])
    normals[6::11] = np.float32([0.0, -2.0, 2.0])  # |n_k| == 2 still counts
    expected = M.voxel_mean(points, normals, colors, 1.0)
    assert len(expected[4]) == 64 and (expected[4] > 1).all()  # 4 cells per axis: every cell mixes rows that count and rows that do not
    cloud = _device_cloud(ctx, points, normals, colors)
    st, lens, dropped, outs = _call(ctx, [cloud], 1.0, None)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    cloud.free()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_accumulator_edge_offsets_pass_2_to_the_32(ctx, sign):
    """270 213 points at ctr + sign * 0.4999 v of one cell: |S_k| = 270213 * 16381 > 2^32."""
    v = np.float32(0.25)
    centre = (np.float32([2, -3, 4]) + np.float32(0.5)) * v
    points = np.tile(centre + np.float32(sign * 0.4999) * v, (270213, 1)).astype(np.float32)
    expected = M.voxel_mean(points, None, None, float(v))
    assert expected[4].tolist() == [270213] and 270213 * 16381 > 2**32
    assert np.abs(expected[0][0].astype(np.float64) - points[0]).max() <= M.error_bound(points, float(v))
    cloud = _device_cloud(ctx, points)
    st, lens, dropped, outs = _call(ctx, [cloud], float(v), None)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    cloud.free()


def test_accumulator_edge_normals_pass_2_to_the_32(ctx):
    """4 097 unit normals along one axis in one cell: T_k = 4097 * 2^20 > 2^32, on each axis and sign in turn."""
    rng = np.random.default_rng(3)
    points = (np.float32([0.3, 0.3, 0.3]) + rng.uniform(0, 0.1, size=(4097, 3))).astype(np.float32)
    cloud_points = _device_cloud(ctx, points)
    for axis in range(3):
        for sign in (1.0, -1.0):
            normals = np.zeros((4097, 3), np.float32)
            normals[:, axis] = sign
            expected = M.voxel_mean(points, normals, None, 0.5)
            assert expected[4].tolist() == [4097] and 4097 * 2**20 > 2**32
            assert np.array_equal(expected[1][0], normals[0])
            cloud = _device_cloud(ctx, points, normals)
            st, lens, dropped, outs = _call(ctx, [cloud], 0.5, None)
            assert st == _abi.A3D_OK
            _assert_matches(outs[0], lens[0], dropped[0], expected)
            cloud.free()
    cloud_points.free()


def test_batch_of_mixed_clouds_equals_single_calls_and_runs_are_identical(ctx):
    sizes = (70001, 0, 2049, 65, 30001, 1, 0, 4096)
    hosts = [_uniform(900 + i, n, with_normals=i not in (2, 4), with_colors=i not in (3, 4)) for i, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, *h) for h in hosts]
    voxel, origin = 0.05, (0.5, 0.25, -0.125)
    runs = [_call(ctx, clouds, voxel, origin) for _ in range(2)]
    for st, lens, dropped, outs in runs:
        assert st == _abi.A3D_OK
        for out, got_len, got_dropped, h in zip(outs, lens, dropped, hosts):
            assert (out["normals"] is None) == (h[1] is None) and (out["colors"] is None) == (h[2] is None)
            _assert_matches(out, got_len, got_dropped, M.voxel_mean(*h, voxel, origin))
    for a, b in zip(runs[0][3], runs[1][3]):  # determinism: two calls, the same bits
        for name in FIELDS:
            assert (a[name] is None and b[name] is None) or np.array_equal(a[name], b[name])
    for i, cloud in enumerate(clouds):  # each cloud alone gives what it gave in the batch
        st, lens, dropped, outs = _call(ctx, [cloud], voxel, origin)
        assert st == _abi.A3D_OK and lens[0] == runs[0][1][i] and dropped[0] == runs[0][2][i]
        for name in FIELDS:
            assert (outs[0][name] is None and runs[0][3][i][name] is None) or np.array_equal(outs[0][name], runs[0][3][i][name])
    # the Python batch form
    many = DevicePointCloud.voxel_downsample_many(clouds, voxel, origin, mode="mean")
    assert len(many) == len(clouds)
    for dc, h in zip(many, hosts):
        exp = M.voxel_mean(*h, voxel, origin)
        got_p, got_n = dc.download()
        got_c = dc.download_colors()
        assert dc.len() == len(exp[3]) and np.array_equal(_bits(got_p), _bits(exp[0]))
        assert (got_n is None) == (h[1] is None) and (got_c is None) == (h[2] is None)
        assert got_n is None or np.array_equal(_bits(got_n), _bits(exp[1]))
        assert got_c is None or np.array_equal(got_c, exp[2])
    for x in (*clouds, *many):
        x.free()


def test_permuted_cloud_gives_the_same_rows_and_singletons_come_back_in_place(ctx):
    points, normals, colors = _uniform(70, 50000)
    perm = np.random.default_rng(71).permutation(len(points))
    a = _device_cloud(ctx, points, normals, colors)
    b = _device_cloud(ctx, points[perm], normals[perm], colors[perm])
    for voxel in (0.1, 1e3):
        ra, ia, ka = a.voxel_downsample(voxel, mode="mean", return_index=True, return_counts=True)
        rb, ib, kb = b.voxel_downsample(voxel, mode="mean", return_index=True, return_counts=True)
        exp = M.voxel_mean(points, normals, colors, voxel)
        assert ra.len() == rb.len() == len(exp[3]) and np.array_equal(ia, exp[3]) and np.array_equal(ka, exp[4])
        assert ia.dtype == ka.dtype == np.uint32 and (ka > 1).any()
        rows_a = _rows(*ra.download(), ra.download_colors(), ka)
        assert np.array_equal(rows_a, _rows(exp[0], exp[1], exp[2], exp[4]))
        assert np.array_equal(rows_a, _rows(*rb.download(), rb.download_colors(), kb))
        # the same cells as the nearest-point downsample
        near, near_index = a.voxel_downsample(voxel, return_index=True)
        _, key, _ = V.voxel_keys(points, voxel)
        assert near.len() == ra.len() and np.array_equal(np.sort(key[near_index]), np.sort(key[ia]))
        for x in (ra, rb, near):
            x.free()
    alone, index, counts = a.voxel_downsample(1e-5, mode="mean", return_index=True, return_counts=True)
    got_p, got_n = alone.download()
    assert np.array_equal(index, np.arange(len(points), dtype=np.uint32)) and (counts == 1).all()
    assert np.array_equal(_bits(got_p), _bits(points)) and np.array_equal(_bits(got_n), _bits(normals))
    assert np.array_equal(alone.download_colors(), colors)
    for x in (a, b, alone):
        x.free()


def test_capacity_one_short_writes_nothing_and_reports_every_count(ctx):
    sizes = (70001, 2049, 0, 30000)
    hosts = [_uniform(950 + i, n) for i, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, *h) for h in hosts]
    voxel = 0.1
    rows = [len(V.voxel_downsample(h[0], voxel)[0]) for h in hosts]
    assert rows[1] > 1 and rows[2] == 0
    for short in (0, 1, 3):
        caps = list(rows)
        caps[short] -= 1
        st, lens, dropped, outs = _call(ctx, clouds, voxel, None, capacities=caps)
        assert st == _abi.A3D_INVALID_PARAMETER
        assert lens == rows and dropped == [0] * len(sizes)
        for out in outs:
            for name in FIELDS:
                assert (out[name] == out[name + "_canary"]).all(), name
    st, lens, dropped, outs = _call(ctx, clouds, voxel, None, capacities=rows)  # exactly enough is enough
    assert st == _abi.A3D_OK and lens == rows
    for out, got_len, got_dropped, h in zip(outs, lens, dropped, hosts):
        _assert_matches(out, got_len, got_dropped, M.voxel_mean(*h, voxel))
    for x in clouds:
        x.free()


def test_wrapper_modes(ctx):
    points, normals, colors = _uniform(80, 2049)
    cloud = _device_cloud(ctx, points, normals, colors)
    # mode="nearest" is the existing call, bit for bit
    old, old_index = cloud.voxel_downsample(0.1, ORIGINS[1], return_index=True)
    new, new_index = cloud.voxel_downsample(0.1, ORIGINS[1], return_index=True, mode="nearest")
    exp_p, exp_n, exp_i, _ = V.voxel_downsample_cloud(points, normals, 0.1, ORIGINS[1])
    assert np.array_equal(old_index, new_index) and np.array_equal(new_index, exp_i)
    for dc in (old, new):
        p, nrm = dc.download()
        assert np.array_equal(_bits(p), _bits(exp_p)) and np.array_equal(_bits(nrm), _bits(exp_n))
        assert np.array_equal(dc.download_colors(), colors[exp_i])
    many = DevicePointCloud.voxel_downsample_many([cloud], 0.1, ORIGINS[1], mode="nearest")
    assert np.array_equal(_bits(many[0].download()[0]), _bits(exp_p))
    # mode="mean": every shape of the return value
    exp = M.voxel_mean(points, normals, colors, 0.1, ORIGINS[1])
    mean = cloud.voxel_downsample(0.1, ORIGINS[1], mode="mean")
    assert isinstance(mean, DevicePointCloud) and mean.len() == len(exp[3])
    assert mean.d_normals is not None and mean.d_colors is not None
    assert np.array_equal(_bits(mean.download()[0]), _bits(exp[0])) and np.array_equal(mean.download_colors(), exp[2])
    m2, counts = cloud.voxel_downsample(0.1, ORIGINS[1], mode="mean", return_counts=True)
    m3, index = cloud.voxel_downsample(0.1, ORIGINS[1], mode="mean", return_index=True)
    assert np.array_equal(counts, exp[4]) and counts.dtype == np.uint32 and np.array_equal(index, exp[3])
    bare = _device_cloud(ctx, points)
    m4 = bare.voxel_downsample(0.1, ORIGINS[1], mode="mean")
    assert m4.d_normals is None and m4.d_colors is None and np.array_equal(_bits(m4.download()[0]), _bits(exp[0]))
    with pytest.raises(InvalidParameter):
        cloud.voxel_downsample(0.1, mode="median")
    with pytest.raises(InvalidParameter):
        cloud.voxel_downsample(0.1, return_counts=True)
    with pytest.raises(InvalidParameter):
        DevicePointCloud.voxel_downsample_many([cloud], 0.1, mode="centroid")
    for x in (cloud, bare, old, new, many[0], mean, m2, m3, m4):
        x.free()
