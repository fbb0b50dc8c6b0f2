"""Outlier removal for resident clouds on the GPU (a3d_point_clouds_knn_distance_device, a3d_point_clouds_select_device,
DevicePointCloud.select / neighbor_distances / remove_radius_outliers / remove_statistical_outliers).

Every comparison is on integer arrays or uint32 views, bit for bit, and the expected value is always the numpy
restatement of the rule (outlier_restatement.py), never the code under test.  The raw calls write into buffers that are
filled with a canary from end to end, with more of it on both sides; colour outputs are guarded byte by byte and start at
every residue of the address mod 4.

The restatement is brute force over pairs, so the sizes are what it can afford in a few seconds: the size grid runs every
radius up to 2049 points; 20 000 points in one cell are checked on 512 seeded rows against all candidates; the cloud of
more than 4096 chunks (two chunks per tile) on the rows of one thin slab of cells."""
import ctypes as C
import os

import numpy as np
import pytest

import outlier_restatement as R
from align3d_amd import A3dError, DevicePointCloud, PointCloud, _abi
from outlier_cases import RADIUS, effectiveness_cloud, sentinel_edge_cloud
from test_gpu_cloud_normals import (BATCH_LENGTHS, CANARY, RADII, SIZES, _bits, _cube, _cube_and_sheet, _Guarded, _raw_bits,
                                    _sample1_frames)

pytestmark = pytest.mark.gpu

KS = (0, 1, 8, 9, 16, 17, 32)  # every width of the register array (none, 8, 16, 32) at its lower and upper edge
GUARD_BYTES = 256


def _device_cloud(ctx, points, normals=None, colors=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


def _dev_u32(ctx, values):
    values = np.ascontiguousarray(values, np.uint32)
    return ctx.to_device(values) if len(values) else ctx.malloc(4)


class _GuardedBytes:
    """A device buffer of `nbytes` bytes that starts `offset` bytes past a 4-byte boundary, 0xA5 from end to end and on
    GUARD_BYTES bytes on both sides."""

    def __init__(self, ctx, nbytes, offset=0):
        self.ctx, self.nbytes, self.offset = ctx, nbytes, offset
        self.total = 2 * GUARD_BYTES + nbytes + offset
        self.base = ctx.to_device(np.full(self.total, 0xA5, np.uint8))
        self.ptr = C.c_void_p(self.base.value + GUARD_BYTES + offset)

    def read(self):
        """(the body as uint8, True iff every byte around it is intact)."""
        b = self.ctx.to_host(self.base, np.empty(self.total, np.uint8))
        lo, hi = GUARD_BYTES + self.offset, GUARD_BYTES + self.offset + self.nbytes
        return b[lo:hi], bool((b[:lo] == 0xA5).all() and (b[hi:] == 0xA5).all())

    def free(self):
        self.ctx.free(self.base)


def _knn(ctx, clouds, radius, k, counts=True):
    """The raw call into guarded buffers: (status, [stats 4-tuples], [dropped], per cloud {counts, qsum: uint32 or None})."""
    n = len(clouds)
    g_counts = [_Guarded(ctx, c.len(), 1) if counts else None for c in clouds]
    g_qsum = [_Guarded(ctx, c.len(), 1) for c in clouds]  # handed over for k == 0 as well: it must stay untouched
    stats, dropped = (C.c_uint64 * (4 * n))(*[12345] * (4 * n)), (C.c_uint64 * n)(*[12345] * n)
    st = ctx.lib.a3d_point_clouds_knn_distance_device(
        ctx.handle, (_abi.PointCloudViewC * n)(*[c.view() for c in clouds]), n, radius, k,
        (C.c_void_p * n)(*[g.ptr for g in g_counts]) if counts else None, (C.c_void_p * n)(*[g.ptr for g in g_qsum]), stats,
        dropped)
    outs = []
    for gc, gq in zip(g_counts, g_qsum):
        out = {"counts": None, "qsum": None}
        for name, g in (("counts", gc), ("qsum", gq)):
            if g is not None:
                body, intact = g.read()
                assert intact, f"the call wrote outside its {name} buffer"
                out[name] = body[:, 0]
                g.free()
        if k == 0:
            assert (out["qsum"] == CANARY).all(), "the count-only form wrote a distance sum"
            out["qsum"] = None
        outs.append(out)
    return st, [tuple(int(v) for v in stats[4 * i:4 * i + 4]) for i in range(n)], list(dropped), outs


def _assert_knn(out, got_stats, got_dropped, points, radius, k, expected=None):
    counts, qsum, stats = expected or R.knn_distance(points, radius, k)
    assert np.array_equal(out["counts"], counts)
    if k:
        assert np.array_equal(out["qsum"], qsum)
    assert got_stats == stats and got_dropped == int((counts == 0).sum())


@pytest.mark.parametrize("k", KS)
def test_knn_size_and_radius_grid(ctx, k):
    for i, n in enumerate(SIZES):
        points = _cube(100 + i, n)
        cloud = _device_cloud(ctx, points)
        for radius in RADII:
            expected = R.knn_distance(points, radius, k)
            if radius == 1e3 and n:
                assert (expected[0] == n).all() and (k == 0 or (expected[1] != R.NONE).all() == (n - 1 >= k))
            if radius == 1e-5 and n and k:
                assert (expected[1] == R.NONE).all()  # every point alone
            st, stats, dropped, outs = _knn(ctx, [cloud], radius, k)
            assert st == _abi.A3D_OK, (n, radius)
            _assert_knn(outs[0], stats[0], dropped[0], points, radius, k, expected)
        cloud.free()


def test_knn_hostile_identical_and_sentinel_edge_clouds(ctx):
    rng = np.random.default_rng(5)
    r = np.float32(0.0625)
    lattice = (rng.integers(-3, 3, size=(600, 3)).astype(np.float32) * r).astype(np.float32)  # on k * r, many twice
    duplicated = np.repeat(_cube(7, 100, lo=-0.2, side=0.3), 3, axis=0)
    mixed = np.r_[lattice, _cube(6, 700, lo=-1.0, side=0.3), duplicated, _raw_bits(8, 300)][rng.permutation(1900)]
    for points, radius in ((mixed, float(r)), (_raw_bits(9, 300), 0.05)):
        cloud = _device_cloud(ctx, points)
        for k in (0, 3, 8, 20):
            expected = R.knn_distance(points, radius, k)
            assert (expected[0] == 0).sum() > 100
            st, stats, dropped, outs = _knn(ctx, [cloud], radius, k)
            assert st == _abi.A3D_OK
            _assert_knn(outs[0], stats[0], dropped[0], points, radius, k, expected)
        cloud.free()
    same = np.tile(np.float32([0.3, -0.2, 1.5]), (200, 1))  # every t = 0: ties throughout
    cloud = _device_cloud(ctx, same)
    for k in (8, 32):
        st, stats, dropped, outs = _knn(ctx, [cloud], 0.05, k)
        assert st == _abi.A3D_OK and (outs[0]["qsum"] == 0).all() and (outs[0]["counts"] == 200).all()
        assert stats[0] == (200, 0, 0, 0)
    cloud.free()
    for k in (1, 8, 9, 16, 17, 32):  # rows with exactly k - 1, k and k + 1 others
        points = sentinel_edge_cloud(k)
        cloud = _device_cloud(ctx, points)
        st, stats, dropped, outs = _knn(ctx, [cloud], 0.05, k)
        assert st == _abi.A3D_OK and (outs[0]["qsum"][:k] == R.NONE).all() and (outs[0]["qsum"][k:] != R.NONE).all()
        _assert_knn(outs[0], stats[0], dropped[0], points, 0.05, k)
        cloud.free()


def _batch_clouds():
    """Two rounds of BATCH_LENGTHS (empty clouds, a cloud of two tiles); one cloud carries raw-bit rows."""
    clouds = []
    for i in range(2 * len(BATCH_LENGTHS)):
        rng = np.random.default_rng([777, i])
        n = BATCH_LENGTHS[i % len(BATCH_LENGTHS)]
        side = 0.05 * max(1.0, n / 4.0) ** (1.0 / 3.0)
        points = (rng.uniform(-2.0, 2.0, size=3) + rng.uniform(0.0, side, size=(n, 3))).astype(np.float32)
        if i == 5:
            points[::7] = _raw_bits(i, len(points[::7]))
        clouds.append(points)
    return clouds


def test_knn_batch_of_unequal_clouds(ctx):
    host = _batch_clouds()
    clouds = [_device_cloud(ctx, p) for p in host]
    for k in (0, 8, 17):
        st, stats, dropped, outs = _knn(ctx, clouds, 0.05, k)
        assert st == _abi.A3D_OK and sum(dropped) > 5 and sum(1 for c in clouds if c.len() == 0) >= 4
        for i, p in enumerate(host):
            _assert_knn(outs[i], stats[i], dropped[i], p, 0.05, k)
    for c in clouds:
        c.free()


def test_knn_twenty_thousand_points_in_one_cell(ctx):
    points = _cube_and_sheet()
    rows = np.sort(np.random.default_rng(78).choice(20000, size=512, replace=False))
    counts, qsum, _ = R.knn_distance(points, 1e3, 8, rows=rows, slab=False)
    assert (counts[rows] == 20000).all() and (qsum[rows] != R.NONE).all()
    cloud = _device_cloud(ctx, points)
    st, stats, dropped, outs = _knn(ctx, [cloud], 1e3, 8)
    assert st == _abi.A3D_OK and dropped[0] == 0
    assert (outs[0]["counts"] == 20000).all()
    assert np.array_equal(outs[0]["qsum"][rows], qsum[rows])
    assert stats[0] == R.stats_of(outs[0]["qsum"]) and stats[0][0] == 20000  # the sums are those of the rows written
    cloud.free()


def test_knn_two_runs_and_a_row_permutation(ctx):
    points = np.r_[_cube(41, 5000, side=0.6), _raw_bits(42, 50)]
    perm = np.random.default_rng(43).permutation(len(points))
    cloud, shuffled = _device_cloud(ctx, points), _device_cloud(ctx, points[perm])
    first, second, moved = _knn(ctx, [cloud], 0.05, 9), _knn(ctx, [cloud], 0.05, 9), _knn(ctx, [shuffled], 0.05, 9)
    assert first[0] == second[0] == moved[0] == _abi.A3D_OK
    assert first[1] == second[1] == moved[1] and first[1][0][0] > 3000  # the statistics: identical words
    assert first[2] == second[2] == moved[2]
    for name in ("counts", "qsum"):
        assert np.array_equal(first[3][0][name], second[3][0][name]), name
        assert np.array_equal(moved[3][0][name], first[3][0][name][perm]), name  # qsum follows its row
    _assert_knn(first[3][0], first[1][0], first[2][0], points, 0.05, 9)
    cloud.free(), shuffled.free()


@pytest.mark.parametrize("knob,value", [("A3D_OUTLIERS_K", "32"), ("A3D_OUTLIERS_SELECT", "t")])
def test_the_forms_the_diagnostics_build_keeps_give_the_same_bits(ctx, diag_ctx, monkeypatch, knob, value):
    points = np.r_[_cube(51, 3000, side=0.5), _raw_bits(52, 30)]
    small = _cube(53, 65, side=0.2)
    clouds, diag_clouds = [_device_cloud(ctx, p) for p in (points, small)], [_device_cloud(diag_ctx, p) for p in (points, small)]
    for radius, k in ((0.05, 5), (0.05, 12), (1e3, 32)):
        monkeypatch.delenv(knob, raising=False)
        st, stats, dropped, outs = _knn(ctx, clouds, radius, k)
        monkeypatch.setenv(knob, value)
        st2, stats2, dropped2, diag = _knn(diag_ctx, diag_clouds, radius, k)
        assert st == st2 == _abi.A3D_OK and stats == stats2 and dropped == dropped2 and stats[0][0] > 1000
        for i in range(2):
            for name in ("counts", "qsum"):
                assert np.array_equal(outs[i][name], diag[i][name]), (radius, k, i, name)
    for c in clouds + diag_clouds:
        c.free()


def test_knn_counts_are_the_normals_entrys_counts(ctx):
    cube = _device_cloud(ctx, np.r_[_cube(61, 4000, side=0.5), _raw_bits(62, 40)])
    frame = _sample1_frames(ctx)[0]
    assert frame.len() > 100000
    for cloud, radius in ((cube, 0.05), (frame, 0.01)):
        points = cloud.download()[0]
        probe = _device_cloud(ctx, points)  # (estimate_normals gives a cloud normals: not on the shared frame)
        _, want = probe.estimate_normals(radius, counts=True)
        st, stats, dropped, outs = _knn(ctx, [cloud], radius, 0)
        assert st == _abi.A3D_OK and stats[0] == (0, 0, 0, 0)
        assert np.array_equal(outs[0]["counts"], want) and want.max() > 5
        st, stats, dropped, outs = _knn(ctx, [cloud], radius, 8, counts=False)
        assert st == _abi.A3D_OK and outs[0]["counts"] is None
        assert np.array_equal(outs[0]["qsum"] != R.NONE, want.astype(np.int64) - 1 >= 8)
        assert stats[0] == R.stats_of(outs[0]["qsum"])
        probe.free()
    cube.free()


def test_knn_two_chunks_per_tile(ctx):
    """More than 4096 chunks of 1024 points: every tile takes two chunks.  The rows of one thin slab of cells are compared
    with the restatement; every count is compared with the normals entry's."""
    n = 4096 * 1024 + 1500
    rng = np.random.default_rng(91)
    points = rng.uniform(0.0, 2.4, size=(n, 3)).astype(np.float32)
    radius = 0.02
    _, cell = R.NR.cells(points, radius)
    rows = np.flatnonzero(cell[:, 0] == 60)[:256]
    rows = np.sort(np.r_[rows, n - 1]) if cell[n - 1, 0] != 60 else rows
    slab = np.flatnonzero(np.abs(cell[:, 0] - 60) <= 1)
    last = np.flatnonzero(np.abs(cell[:, 0] - cell[n - 1, 0]) <= 1)
    cols = np.union1d(slab, last)  # every candidate the rule admits for those rows
    where = np.searchsorted(cols, rows)
    counts, qsum, _ = R.knn_distance(points[cols], radius, 8, rows=where, chunk=64)
    cloud = _device_cloud(ctx, points)
    st, stats, dropped, outs = _knn(ctx, [cloud], radius, 8)
    assert st == _abi.A3D_OK and dropped[0] == 0
    assert np.array_equal(outs[0]["counts"][rows], counts[where]) and np.array_equal(outs[0]["qsum"][rows], qsum[where])
    assert (qsum[where] != R.NONE).sum() > 100 and (qsum[where] == R.NONE).sum() > 0
    assert stats[0] == R.stats_of(outs[0]["qsum"])
    _, want = cloud.estimate_normals(radius, counts=True)
    assert np.array_equal(outs[0]["counts"], want)
    # the select over the same two-chunk tiles, on the counts
    values = outs[0]["counts"]
    d_values = _dev_u32(ctx, values)
    st, lens, sel = _select(ctx, [cloud], [d_values], [10], [0xFFFFFFFF])
    keep = R.select(values, 10, 0xFFFFFFFF)
    assert st == _abi.A3D_OK and lens[0] == len(keep) and 0 < len(keep) < n
    assert np.array_equal(sel[0]["index"], keep) and np.array_equal(sel[0]["points"], _bits(points[keep]))
    ctx.free(d_values)
    cloud.free()


# ---- select ------------------------------------------------------------------------------------------------------------


def _select(ctx, clouds, d_values, lo, hi, normals=False, colors=False, color_offset=0, capacities=None, index=True):
    """The raw call into guarded buffers of exactly `capacities` rows (default: each cloud's length): (status, [lens], per
    cloud {points [cap, 3] u32, normals, colors [cap, 3] u8, index [cap]: what the buffers hold}); asserts the guards."""
    n = len(clouds)
    caps = [c.len() for c in clouds] if capacities is None else list(capacities)
    g_points = [_Guarded(ctx, cap, 3) for cap in caps]
    g_normals = [_Guarded(ctx, cap, 3) if normals and c.d_normals is not None else None for c, cap in zip(clouds, caps)]
    g_colors = [_GuardedBytes(ctx, 3 * cap, color_offset) if colors and c.d_colors is not None else None
                for c, cap in zip(clouds, caps)]
    g_index = [_Guarded(ctx, cap, 1) if index else None for cap in caps]
    lens = (C.c_uint64 * n)(*[12345] * n)

    def table(guards):
        return (C.c_void_p * n)(*[g.ptr if g is not None else None for g in guards])

    st = ctx.lib.a3d_point_clouds_select_device(
        ctx.handle, (_abi.PointCloudViewC * n)(*[c.view() for c in clouds]),
        (C.c_void_p * n)(*[c.d_colors for c in clouds]) if colors else None, n, (C.c_void_p * n)(*d_values),
        (C.c_uint32 * n)(*lo), (C.c_uint32 * n)(*hi), table(g_points), table(g_normals) if normals else None,
        table(g_colors) if colors else None, table(g_index) if index else None, (C.c_uint64 * n)(*caps), lens)
    outs = []
    for i in range(n):
        out = {}
        for name, g in (("points", g_points[i]), ("normals", g_normals[i]), ("colors", g_colors[i]), ("index", g_index[i])):
            out[name] = None
            if g is not None:
                body, intact = g.read()
                assert intact, f"the call wrote outside its {name} buffer"
                out[name] = body.reshape(-1, 3) if name == "colors" else body[:, 0] if name == "index" else body
                g.free()
        kept = min(int(lens[i]), caps[i]) if st == _abi.A3D_OK else 0
        for name in out:  # what lies past the kept rows is untouched; the caller sees the kept rows only
            if out[name] is not None:
                rest = out[name][kept:]
                assert (rest == (0xA5 if name == "colors" else CANARY)).all(), f"rows past the kept ones were written ({name})"
                out[name] = out[name][:kept]
        outs.append(out)
    return st, [int(v) for v in lens], outs


def _assert_selected(out, got_len, keep, points, normals=None, colors=None):
    assert got_len == len(keep)
    assert np.array_equal(out["index"], keep) and (np.diff(out["index"].astype(np.int64)) > 0).all()
    assert np.array_equal(out["points"], _bits(points[keep]).reshape(-1, 3))
    if normals is not None:
        assert np.array_equal(out["normals"], _bits(normals[keep]).reshape(-1, 3))
    if colors is not None:
        assert np.array_equal(out["colors"], colors[keep])


def test_select_masks(ctx):
    n = 2500  # three tiles
    points = _cube(71, n)
    points[::9] = _raw_bits(72, len(points[::9]))  # the coordinates are never looked at
    cloud = _device_cloud(ctx, points)
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternate": np.arange(n) % 2 == 0,
             "first": np.arange(n) == 0, "last": np.arange(n) == n - 1}
    for row in (63, 64, 65, 1023, 1024, 1025):
        masks[f"only {row}"] = np.arange(n) == row
    masks["random"] = np.random.default_rng(73).random(n) < 0.3
    for name, mask in masks.items():
        d_values = _dev_u32(ctx, mask)
        st, lens, outs = _select(ctx, [cloud], [d_values], [1], [0xFFFFFFFF])
        assert st == _abi.A3D_OK, name
        _assert_selected(outs[0], lens[0], np.flatnonzero(mask).astype(np.uint32), points)
        ctx.free(d_values)
    values = np.random.default_rng(74).integers(0, 12, n).astype(np.uint32)
    values[:4] = (0, 0xFFFFFFFF, 5, 8)
    d_values = _dev_u32(ctx, values)
    for lo, hi in ((5, 8), (8, 5), (5, 5), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (9, 0xFFFFFFFE)):
        st, lens, outs = _select(ctx, [cloud], [d_values], [lo], [hi])  # values at exactly lo and hi; lo > hi
        assert st == _abi.A3D_OK
        keep = R.select(values, lo, hi)
        assert (lo > hi) == (len(keep) == 0) or lo <= hi
        _assert_selected(outs[0], lens[0], keep, points)
    ctx.free(d_values)
    cloud.free()


def test_select_fields_batches_and_overflow(ctx):
    host = _batch_clouds()
    rng = np.random.default_rng(81)
    normals = [rng.normal(size=p.shape).astype(np.float32) if i % 3 else None for i, p in enumerate(host)]
    colors = [rng.integers(0, 256, size=p.shape).astype(np.uint8) if i % 2 else None for i, p in enumerate(host)]
    values = [rng.integers(0, 4, len(p)).astype(np.uint32) for p in host]
    clouds = [_device_cloud(ctx, p, nrm, col) for p, nrm, col in zip(host, normals, colors)]
    d_values = [_dev_u32(ctx, v) for v in values]
    n = len(host)
    lo, hi = [1 + i % 2 for i in range(n)], [2 + i % 2 for i in range(n)]
    keeps = [R.select(v, a, b) for v, a, b in zip(values, lo, hi)]
    assert sum(len(k) for k in keeps) > 1000
    for with_normals, with_colors, offset in ((False, False, 0), (True, False, 0), (True, True, 0), (False, True, 1),
                                              (True, True, 2), (True, True, 3)):
        st, lens, outs = _select(ctx, clouds, d_values, lo, hi, with_normals, with_colors, offset)
        assert st == _abi.A3D_OK
        for i in range(n):
            _assert_selected(outs[i], lens[i], keeps[i], host[i], normals[i] if with_normals else None,
                             colors[i] if with_colors else None)
            assert (outs[i]["normals"] is None) == (not with_normals or normals[i] is None)
    # capacities that fit exactly: the last colour store ends on the buffer's last byte
    st, lens, outs = _select(ctx, clouds, d_values, lo, hi, True, True, 1, capacities=[len(k) for k in keeps])
    assert st == _abi.A3D_OK
    for i in range(n):
        _assert_selected(outs[i], lens[i], keeps[i], host[i], normals[i], colors[i])
    # one capacity one short: A3D_INVALID_PARAMETER, every count reported, nothing written anywhere
    caps = [len(k) for k in keeps]
    big = int(np.argmax(caps))
    caps[big] -= 1
    st, lens, outs = _select(ctx, clouds, d_values, lo, hi, True, True, 3, capacities=caps)
    assert st == _abi.A3D_INVALID_PARAMETER and lens == [len(k) for k in keeps]  # (_select asserted the canaries)
    for d in d_values:
        ctx.free(d)
    for c in clouds:
        c.free()


def test_select_refusals_on_the_device(ctx):
    points = _cube(85, 300)
    nrm = _cube(86, 300)
    cloud, bare = _device_cloud(ctx, points, nrm), _device_cloud(ctx, points)
    d_values = _dev_u32(ctx, np.ones(300, np.uint32))
    out = ctx.malloc(300 * 12)
    lens = (C.c_uint64 * 1)(777)

    def call(c, out_points, out_normals=None, out_colors=None, out_index=None):
        def one(p):
            return None if p is None else (C.c_void_p * 1)(p)
        return ctx.lib.a3d_point_clouds_select_device(
            ctx.handle, (_abi.PointCloudViewC * 1)(c.view()), None, 1, (C.c_void_p * 1)(d_values), (C.c_uint32 * 1)(1),
            (C.c_uint32 * 1)(1), one(out_points), one(out_normals), one(out_colors), one(out_index), (C.c_uint64 * 1)(300), lens)

    assert call(cloud, cloud.d_points) == _abi.A3D_INVALID_PARAMETER  # in place
    # (the normals are an input only when normals are written, as in the downsample)
    assert call(cloud, C.c_void_p(cloud.d_normals.value + 12), out_normals=out) == _abi.A3D_INVALID_PARAMETER
    assert call(cloud, d_values) == _abi.A3D_INVALID_PARAMETER  # on the values
    assert call(cloud, out, out_normals=out) == _abi.A3D_INVALID_PARAMETER  # two outputs on one buffer
    assert call(cloud, out, out_index=C.c_void_p(out.value + 3596)) == _abi.A3D_INVALID_PARAMETER
    assert call(bare, out, out_normals=cloud.d_normals) == _abi.A3D_MISSING_FIELD
    assert call(bare, out, out_colors=cloud.d_normals) == _abi.A3D_MISSING_FIELD
    assert lens[0] == 777
    assert np.array_equal(_bits(cloud.download()[0]), _bits(points)) and np.array_equal(_bits(cloud.download()[1]), _bits(nrm))
    assert call(cloud, out) == _abi.A3D_OK and lens[0] == 300
    ctx.free(out), ctx.free(d_values)
    cloud.free(), bare.free()


# ---- the wrappers ------------------------------------------------------------------------------------------------------


def test_wrappers_equal_the_restatement_end_to_end(ctx):
    points, outlier = effectiveness_cloud()
    rng = np.random.default_rng(95)
    normals = rng.normal(size=points.shape).astype(np.float32)
    colors = rng.integers(0, 256, size=points.shape).astype(np.uint8)
    hostile = np.r_[_cube(96, 900, side=0.4), _raw_bits(97, 60)][rng.permutation(960)]
    full, bare = _device_cloud(ctx, points, normals, colors), _device_cloud(ctx, hostile)
    # the radius filter
    keep = R.remove_radius_outliers(points, RADIUS, 2)
    assert np.array_equal(keep, np.flatnonzero(~outlier))
    out, index = full.remove_radius_outliers(RADIUS, 2, return_index=True)
    assert np.array_equal(index, keep) and out.len() == 1500
    got_p, got_n = out.download()
    assert np.array_equal(_bits(got_p), _bits(points[keep])) and np.array_equal(_bits(got_n), _bits(normals[keep]))
    assert np.array_equal(out.download_colors(), colors[keep])
    out.free()
    # the statistical filter
    keep_s, t = R.remove_statistical_outliers(points, RADIUS, 8, 2.0)
    out, index = full.remove_statistical_outliers(RADIUS, 8, 2.0, return_index=True)
    assert np.array_equal(index, keep_s) and not outlier[index].any() and len(index) >= 0.95 * 1500
    got_p, got_n = out.download()
    assert np.array_equal(_bits(got_p), _bits(points[keep_s])) and np.array_equal(_bits(got_n), _bits(normals[keep_s]))
    assert np.array_equal(out.download_colors(), colors[keep_s])
    out.free()
    # neighbor_distances: resident arrays that go to select as they are, and the sums as Python ints
    d_counts, d_qsum, stats = full.neighbor_distances(RADIUS, 8)
    want = R.knn_distance(points, RADIUS, 8)
    assert np.array_equal(ctx.to_host(d_counts, np.empty(1530, np.uint32)), want[0])
    assert np.array_equal(ctx.to_host(d_qsum, np.empty(1530, np.uint32)), want[1])
    assert stats == (want[2][0], want[2][1], want[2][2] + (want[2][3] << 32))
    assert DevicePointCloud.knn_distance_threshold(stats, 2.0) == t
    again = full.select(d_qsum, 0, t)
    assert again.len() == len(keep_s) and np.array_equal(_bits(again.download()[0]), _bits(points[keep_s]))
    again.free(), ctx.free(d_counts), ctx.free(d_qsum)
    assert full.neighbor_distances(RADIUS, 0)[1] is None
    # a host mask; the many forms, a hostile cloud and an empty one beside the first
    mask = rng.random(1530) < 0.5
    picked, index = full.select(mask, return_index=True)
    assert np.array_equal(index, np.flatnonzero(mask)) and np.array_equal(picked.download_colors(), colors[mask])
    picked.free()
    empty = _device_cloud(ctx, np.empty((0, 3), np.float32))
    outs, indexes = DevicePointCloud.remove_radius_outliers_many([full, bare, empty], 0.05, 3, return_index=True)
    for got, host in zip(indexes, (points, hostile, np.empty((0, 3), np.float32))):
        assert np.array_equal(got, R.remove_radius_outliers(host, 0.05, 3))
    assert 0 < outs[1].len() < 900 and outs[1].d_normals is None and outs[0].has_colors() and outs[2].len() == 0
    for o in outs:
        o.free()
    outs, indexes = DevicePointCloud.remove_statistical_outliers_many([full, bare, empty], 0.06, 4, 1.0, return_index=True)
    for got, host in zip(indexes, (points, hostile, np.empty((0, 3), np.float32))):
        assert np.array_equal(got, R.remove_statistical_outliers(host, 0.06, 4, 1.0)[0])
    assert 0 < outs[1].len() < 900
    assert np.array_equal(_bits(outs[1].download()[0]), _bits(hostile[indexes[1]]))
    for o in outs:
        o.free()
    with pytest.raises(A3dError):
        full.remove_statistical_outliers(RADIUS, 33, 2.0)
    with pytest.raises(A3dError):
        full.remove_radius_outliers(-1.0, 2)
    with pytest.raises(A3dError):
        full.select(np.ones(7, bool))
    for x in (full, bare, empty):
        x.free()
