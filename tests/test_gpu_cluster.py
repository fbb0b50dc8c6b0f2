"""Clustering of resident clouds on the GPU (a3d_point_clouds_cluster_device, DevicePointCloud.cluster /
remove_small_clusters / largest_cluster).

Every comparison is np.array_equal on uint32, and the expected value is always the numpy restatement of the rule
(cluster_restatement.py) or a construction, never the code under test.  The raw call writes every output into buffers that
are filled with a canary from end to end, with more of it on both sides; the words of sizes and roots past the C clusters
must still hold it.

The restatement enumerates pairs, so the sizes are what it can afford in a few seconds; the clouds beyond that (20 000
rows in one cell, four million rows in pairs) have clusters that are known by construction."""
import ctypes as C

import numpy as np
import pytest

import cluster_restatement as R
from align3d_amd import A3dError, DevicePointCloud, PointCloud, _abi
from cluster_cases import (border_ties, bridge, chain, exact_chain, floaters_cloud, pairs_far_apart, pairs_far_apart_expected,
                           raw_bits)
from outlier_cases import RADIUS, sentinel_edge_cloud
from test_gpu_cloud_normals import (BATCH_LENGTHS, CANARY, RADII, SIZES, _bits, _cube, _cube_and_sheet, _Guarded,
                                    _sample1_frames)

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
OUTPUTS = ("labels", "row_sizes", "sizes", "roots")


def _device_cloud(ctx, points, normals=None, colors=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


def _cluster(ctx, clouds, radius, m, fields=OUTPUTS):
    """The raw call into guarded buffers: (status, per cloud {labels, row_sizes: [len]; sizes, roots: the first C words;
    clusters, noise, dropped: the host counts}).  Asserts the guards and that sizes and roots are untouched past C."""
    n = len(clouds)
    guards = {f: [_Guarded(ctx, c.len(), 1) for c in clouds] if f in fields else None for f in OUTPUTS}
    counts = [(C.c_uint64 * n)(*[12345] * n) for _ in range(3)]

    def table(f):
        return (C.c_void_p * n)(*[g.ptr for g in guards[f]]) if guards[f] else None

    st = ctx.lib.a3d_point_clouds_cluster_device(
        ctx.handle, (_abi.PointCloudViewC * n)(*[c.view() for c in clouds]), n, radius, m, table("labels"), table("row_sizes"),
        table("sizes"), table("roots"), *counts)
    outs = []
    for i in range(n):
        out = {"clusters": int(counts[0][i]), "noise": int(counts[1][i]), "dropped": int(counts[2][i])}
        for f in OUTPUTS:
            out[f] = None
            if guards[f]:
                body, intact = guards[f][i].read()
                assert intact, f"the call wrote outside its {f} buffer"
                out[f] = body[:, 0]
                guards[f][i].free()
                if f in ("sizes", "roots") and st == _abi.A3D_OK:
                    assert (out[f][out["clusters"]:] == CANARY).all(), f"{f}: words past the clusters were written"
                    out[f] = out[f][:out["clusters"]]
        outs.append(out)
    return st, outs


def _assert_equal(out, want):
    """One cloud's outputs against the restatement's Clusters."""
    assert np.array_equal(out["labels"], want.labels)
    assert out["clusters"] == len(want.sizes) and out["noise"] == int(want.noise.sum()) and out["dropped"] == want.dropped
    for f in ("row_sizes", "sizes", "roots"):
        if out[f] is not None:
            assert np.array_equal(out[f], getattr(want, f)), f


def _assert_construction(out, labels, sizes, roots):
    assert np.array_equal(out["labels"], labels) and np.array_equal(out["sizes"], sizes) and np.array_equal(out["roots"], roots)
    member = labels != NONE
    row_sizes = np.zeros(len(labels), np.uint32)
    row_sizes[member] = np.asarray(sizes, np.uint32)[labels[member]]
    assert np.array_equal(out["row_sizes"], row_sizes)
    assert out["clusters"] == len(sizes) and out["noise"] == int((~member).sum())


_pairs = {}


def _grid_pairs(i, n, radius):
    """The neighbour pairs of the grid's cloud i at a radius: computed once, shared by the min_points cases."""
    if (i, radius) not in _pairs:
        _pairs[(i, radius)] = R.pairs_brute(_cube(100 + i, n), radius)
    return _pairs[(i, radius)]


@pytest.mark.parametrize("m", (1, 2, 5))
def test_size_and_radius_grid(ctx, m):
    for i, n in enumerate(SIZES):
        points = _cube(100 + i, n)
        cloud = _device_cloud(ctx, points)
        for radius in RADII:
            want = R.cluster_pairs(_grid_pairs(i, n, radius), m)
            if radius == 1e3 and n >= m:
                assert want.sizes.tolist() == [n] * (n > 0) and want.roots.tolist() == [0] * (n > 0)  # one cluster, root 0
            if radius == 1e-5 and m == 1:
                assert np.array_equal(want.labels, np.arange(n))  # n clusters, label = row
            st, outs = _cluster(ctx, [cloud], radius, m)
            assert st == _abi.A3D_OK, (n, radius)
            _assert_equal(outs[0], want)
        cloud.free()


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_chains(ctx, order):
    for n in (2, 64, 65, 1025, 4097):
        cloud = _device_cloud(ctx, chain(n, order))
        st, outs = _cluster(ctx, [cloud], 0.05, 1)
        assert st == _abi.A3D_OK
        _assert_construction(outs[0], np.zeros(n, np.uint32), [n], [0])  # one cluster whatever the order of the rows
        cloud.free()
        if n == 2:  # the one link stretched: two clusters of one row; min_points = 3: nobody is core, all noise
            cloud = _device_cloud(ctx, chain(2, order, stretch=(0, 1.001)))
            st, outs = _cluster(ctx, [cloud], 0.05, 1)
            assert st == _abi.A3D_OK
            _assert_construction(outs[0], np.uint32([0, 1]), [1, 1], [0, 1])
            cloud.free()
            cloud = _device_cloud(ctx, chain(2, order))
            st, outs = _cluster(ctx, [cloud], 0.05, 3)
            assert st == _abi.A3D_OK
            _assert_construction(outs[0], np.full(2, NONE, np.uint32), [], [])
            cloud.free()
        if n >= 64:  # one link stretched to just above r: two clusters; min_points = 3: the two ends are border rows
            k = n // 3
            for points, m in ((chain(n, order, stretch=(k, 1.001)), 1), (chain(n, order), 3)):
                want = R.cluster(points, 0.05, m, by_cell=True)
                assert sorted(want.sizes.tolist()) == ([k + 1, n - k - 1] if m == 1 else [n])
                assert want.border.sum() == (0 if m == 1 else 2)
                cloud = _device_cloud(ctx, points)
                st, outs = _cluster(ctx, [cloud], 0.05, m)
                assert st == _abi.A3D_OK
                _assert_equal(outs[0], want)
                cloud.free()


def test_a_link_of_exactly_the_radius_on_exact_coordinates(ctx):
    for n, k in ((10, 4), (130, 70)):
        cloud = _device_cloud(ctx, exact_chain(n, k))
        st, outs = _cluster(ctx, [cloud], 0.25, 1)
        assert st == _abi.A3D_OK
        labels = np.r_[np.zeros(k + 1), np.ones(n - k - 1)].astype(np.uint32)  # d2 == r2 links; r + 2^-10 does not
        _assert_construction(outs[0], labels, [k + 1, n - k - 1], [0, k + 1])
        cloud.free()


def test_twenty_thousand_rows_in_one_cell_every_union_on_one_root(ctx):
    cloud = _device_cloud(ctx, _cube_and_sheet())
    for m in (1, 20000):
        st, outs = _cluster(ctx, [cloud], 1e3, m)
        assert st == _abi.A3D_OK
        _assert_construction(outs[0], np.zeros(20000, np.uint32), [20000], [0])
    st, outs = _cluster(ctx, [cloud], 1e3, 20001)  # nobody is core
    assert st == _abi.A3D_OK
    _assert_construction(outs[0], np.full(20000, NONE, np.uint32), [], [])
    cloud.free()


def test_hostile_rows_duplicates_and_the_core_edge(ctx):
    rng = np.random.default_rng(5)
    r = np.float32(0.0625)
    lattice = (rng.integers(-3, 3, size=(600, 3)).astype(np.float32) * r).astype(np.float32)  # on k * r, many twice
    duplicated = np.repeat(_cube(7, 100, lo=-0.2, side=0.3), 3, axis=0)
    mixed = np.r_[lattice, _cube(6, 700, lo=-1.0, side=0.3), duplicated, raw_bits(8, 300)][rng.permutation(1900)]
    cloud = _device_cloud(ctx, mixed)
    pairs = R.pairs_brute(mixed, float(r))
    for m in (1, 3, 8):
        want = R.cluster_pairs(pairs, m)
        assert want.dropped > 100 and (want.labels[~pairs.kept] == NONE).all()
        st, outs = _cluster(ctx, [cloud], float(r), m)
        assert st == _abi.A3D_OK
        _assert_equal(outs[0], want)
    cloud.free()
    same = np.tile(np.float32([0.3, -0.2, 1.5]), (200, 1))
    cloud = _device_cloud(ctx, same)
    for m in (1, 200):
        st, outs = _cluster(ctx, [cloud], 0.05, m)
        assert st == _abi.A3D_OK
        _assert_construction(outs[0], np.zeros(200, np.uint32), [200], [0])
    st, outs = _cluster(ctx, [cloud], 0.05, 201)
    assert st == _abi.A3D_OK
    _assert_construction(outs[0], np.full(200, NONE, np.uint32), [], [])
    cloud.free()
    for k in (1, 8, 17):  # clusters of k, k + 1 and k + 2 rows at min_points = k + 1: the first is noise
        cloud = _device_cloud(ctx, sentinel_edge_cloud(k))
        st, outs = _cluster(ctx, [cloud], 0.05, k + 1)
        assert st == _abi.A3D_OK
        labels = np.repeat(np.uint32([NONE, 0, 1]), [k, k + 1, k + 2])
        _assert_construction(outs[0], labels, [k + 1, k + 2], [k, 2 * k + 1])
        cloud.free()


def test_bridge_and_border_ties(ctx):
    points, row, m = bridge()
    want = R.cluster(points, 0.05, m)
    assert len(want.sizes) == 2 and want.border[row]
    cloud = _device_cloud(ctx, points)
    st, outs = _cluster(ctx, [cloud], 0.05, m)
    assert st == _abi.A3D_OK and outs[0]["clusters"] == 2
    _assert_equal(outs[0], want)
    cloud.free()
    points, radius, m, labels = border_ties()
    cloud = _device_cloud(ctx, points)
    st, outs = _cluster(ctx, [cloud], radius, m)
    assert st == _abi.A3D_OK
    _assert_construction(outs[0], labels, [6, 6], [0, 5])
    # the same with the two clusters' rows swapped: the tie goes to the lower ROW, which is now the other cluster's
    swapped = np.r_[points[5:10], points[0:5], points[10:]]
    cloud2 = _device_cloud(ctx, swapped)
    st, outs = _cluster(ctx, [cloud2], radius, m)
    assert st == _abi.A3D_OK
    _assert_construction(outs[0], np.uint32([0] * 5 + [1] * 5 + [0, 0]), [7, 5], [0, 5])
    cloud.free(), cloud2.free()


def _batch_clouds():
    """The recipe of test_gpu_cloud_outliers.py: two rounds of BATCH_LENGTHS (empty clouds, a cloud of two tiles); one cloud
    carries raw-bit rows."""
    clouds = []
    for i in range(2 * len(BATCH_LENGTHS)):
        rng = np.random.default_rng([777, i])
        n = BATCH_LENGTHS[i % len(BATCH_LENGTHS)]
        side = 0.05 * max(1.0, n / 4.0) ** (1.0 / 3.0)
        points = (rng.uniform(-2.0, 2.0, size=3) + rng.uniform(0.0, side, size=(n, 3))).astype(np.float32)
        if i == 5:
            points[::7] = raw_bits(i, len(points[::7]))
        clouds.append(points)
    return clouds


def test_batch_of_unequal_clouds_each_as_if_alone(ctx):
    host = _batch_clouds()
    clouds = [_device_cloud(ctx, p) for p in host]
    for m, fields in ((1, OUTPUTS), (4, OUTPUTS), (4, ("labels",)), (9, ("labels", "roots"))):
        st, outs = _cluster(ctx, clouds, 0.05, m, fields)
        assert st == _abi.A3D_OK and sum(o["dropped"] for o in outs) > 5 and sum(1 for c in clouds if c.len() == 0) >= 4
        for i, p in enumerate(host):
            _assert_equal(outs[i], R.cluster(p, 0.05, m))
    for c in clouds:
        c.free()


def test_batch_of_three_hundred_tiny_clouds(ctx):
    rng = np.random.default_rng(300)
    host = [rng.uniform(0.0, 0.12, size=(int(n), 3)).astype(np.float32) for n in rng.integers(0, 9, size=300)]
    clouds = [_device_cloud(ctx, p) for p in host]
    st, outs = _cluster(ctx, clouds, 0.05, 2)
    assert st == _abi.A3D_OK
    for i, p in enumerate(host):
        _assert_equal(outs[i], R.cluster(p, 0.05, 2))
    assert sum(o["clusters"] for o in outs) > 100 and sum(o["noise"] for o in outs) > 100
    for c in clouds:
        c.free()


def test_two_runs_and_a_row_permutation(ctx):
    points = np.r_[_cube(41, 5000, side=0.6), raw_bits(42, 50)]
    perm = np.random.default_rng(43).permutation(len(points))
    cloud, shuffled = _device_cloud(ctx, points), _device_cloud(ctx, points[perm])
    m = 12  # (on the restatement: 10 clusters, 2025 border rows, 367 noise rows)
    (st1, first), (st2, second), (st3, moved) = (_cluster(ctx, [c], 0.05, m) for c in (cloud, cloud, shuffled))
    assert st1 == st2 == st3 == _abi.A3D_OK
    for f in OUTPUTS + ("clusters", "noise", "dropped"):
        assert np.array_equal(first[0][f], second[0][f]), f  # identical words
    want = R.cluster(points, 0.05, m, by_cell=True)
    _assert_equal(first[0], want)
    _assert_equal(moved[0], R.cluster(points[perm], 0.05, m, by_cell=True))
    assert want.border.sum() > 100 and want.noise.sum() > 100 and len(want.sizes) >= 5
    a, b = first[0]["labels"][perm], moved[0]["labels"]  # row k of the shuffled cloud is row perm[k]
    assert np.array_equal(a == NONE, b == NONE)  # the noise set
    core = want.core[perm]
    pairs = np.unique(np.stack([a[core], b[core]], axis=1), axis=0)  # the core partition: a bijection between the numberings
    assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
    assert sorted(first[0]["sizes"].tolist()) == sorted(moved[0]["sizes"].tolist())
    cloud.free(), shuffled.free()


def _assert_consistent_with_counts(out, counts, m):
    """What the outputs must satisfy given the knn entry's counts (core = counts >= m), without a restatement."""
    labels, core = out["labels"], counts >= m
    member = labels != NONE
    assert member[core].all()  # every core row is in a cluster; the rest of the members are border rows
    c = out["clusters"]
    assert np.array_equal(out["sizes"], np.bincount(labels[member], minlength=c))
    assert core[out["roots"]].all() and np.array_equal(labels[out["roots"]], np.arange(c))
    first_core = np.full(c, len(labels), np.int64)
    np.minimum.at(first_core, labels[core], np.flatnonzero(core))
    assert np.array_equal(out["roots"], first_core)  # the root is the lowest core row
    row_sizes = np.zeros(len(labels), np.uint32)
    row_sizes[member] = out["sizes"][labels[member]]
    assert np.array_equal(out["row_sizes"], row_sizes) and out["noise"] == int((~member).sum())
    if m == 1:
        assert np.array_equal(member, counts > 0)


def test_core_rows_are_the_knn_entrys_counts_of_at_least_min_points(ctx):
    cube = _device_cloud(ctx, np.r_[_cube(61, 4000, side=0.5), raw_bits(62, 40)])
    frame = _sample1_frames(ctx)[0]
    assert frame.len() > 100000
    for cloud, radius in ((cube, 0.05), (frame, 0.01)):
        d_counts, _, _ = cloud.neighbor_distances(radius, 0)
        counts = ctx.to_host(d_counts, np.empty(cloud.len(), np.uint32))
        ctx.free(d_counts)
        for m in (1, 6):
            st, outs = _cluster(ctx, [cloud], radius, m)
            assert st == _abi.A3D_OK and outs[0]["clusters"] > 0
            _assert_consistent_with_counts(outs[0], counts, m)
            if cloud is cube:
                want = R.cluster(cloud.download()[0], radius, m, by_cell=True)
                assert np.array_equal(want.counts, counts)
                _assert_equal(outs[0], want)
    cube.free()


@pytest.mark.parametrize("m", (1, 2))
def test_two_chunks_per_tile(ctx, m):
    """More than 4096 chunks of 1024 rows: every tile takes two chunks.  Partners are half the cloud apart, and the ranking
    of the roots crosses every tile."""
    n = 4096 * 1024 + 1500
    points, _ = pairs_far_apart(n)
    cloud = _device_cloud(ctx, points)
    st, outs = _cluster(ctx, [cloud], 0.02, m)
    assert st == _abi.A3D_OK and outs[0]["dropped"] == 0
    _assert_construction(outs[0], *pairs_far_apart_expected(n, m))
    cloud.free()


def test_pairs_far_apart_small_and_all_noise(ctx):
    for n in (3001, 3000):
        cloud = _device_cloud(ctx, pairs_far_apart(n)[0])
        for m in (1, 2, 3):
            st, outs = _cluster(ctx, [cloud], 0.02, m)
            assert st == _abi.A3D_OK
            _assert_construction(outs[0], *pairs_far_apart_expected(n, m))
        cloud.free()


@pytest.mark.parametrize("knob,value", [("A3D_CLUSTER_LINK", "all"), ("A3D_CLUSTER_HALVING", "0")])
def test_the_forms_the_diagnostics_build_keeps_give_the_same_bits(ctx, diag_ctx, monkeypatch, knob, value):
    hosts = (np.r_[_cube(51, 3000, side=0.5), raw_bits(52, 30)], _cube(53, 65, side=0.2), chain(1025, "descending"))
    clouds, diag_clouds = [_device_cloud(ctx, p) for p in hosts], [_device_cloud(diag_ctx, p) for p in hosts]
    for radius, m in ((0.05, 1), (0.05, 5), (1e3, 3)):
        monkeypatch.delenv(knob, raising=False)
        st, outs = _cluster(ctx, clouds, radius, m)
        monkeypatch.setenv(knob, value)
        st2, diag = _cluster(diag_ctx, diag_clouds, radius, m)
        assert st == st2 == _abi.A3D_OK and outs[0]["clusters"] > 0
        for i in range(len(hosts)):
            for f in OUTPUTS + ("clusters", "noise", "dropped"):
                assert np.array_equal(outs[i][f], diag[i][f]), (radius, m, i, f)
    for c in clouds + diag_clouds:
        c.free()


def test_refusals_on_the_device_leave_everything_untouched(ctx):
    points = _cube(85, 300)
    cloud = _device_cloud(ctx, points, _cube(86, 300))
    out = ctx.malloc(300 * 4)
    found = (C.c_uint64 * 1)(777)

    def call(labels, row_sizes=None, radius=0.05, m=2):
        def one(p):
            return None if p is None else (C.c_void_p * 1)(p)
        return ctx.lib.a3d_point_clouds_cluster_device(ctx.handle, (_abi.PointCloudViewC * 1)(cloud.view()), 1, radius, m,
                                                       one(labels), one(row_sizes), None, None, found, None, None)

    assert call(cloud.d_points) == _abi.A3D_INVALID_PARAMETER
    assert call(C.c_void_p(cloud.d_normals.value + 3596)) == _abi.A3D_INVALID_PARAMETER  # on the normals' last word
    assert call(out, row_sizes=C.c_void_p(out.value + 1196)) == _abi.A3D_INVALID_PARAMETER
    assert call(out, m=0) == _abi.A3D_INVALID_PARAMETER and call(out, radius=0.0) == _abi.A3D_INVALID_PARAMETER
    assert found[0] == 777
    assert np.array_equal(_bits(cloud.download()[0]), _bits(points))
    assert call(out) == _abi.A3D_OK and found[0] == len(R.cluster(points, 0.05, 2).sizes)
    ctx.free(out)
    cloud.free()


# ---- the wrappers ------------------------------------------------------------------------------------------------------


def test_wrappers_equal_the_restatement_end_to_end(ctx):
    points, outlier, clump = floaters_cloud()
    rng = np.random.default_rng(95)
    normals = rng.normal(size=points.shape).astype(np.float32)
    colors = rng.integers(0, 256, size=points.shape).astype(np.uint8)
    full = _device_cloud(ctx, points, normals, colors)
    want = R.cluster(points, RADIUS, 1)
    d_labels, sizes, roots = full.cluster(RADIUS)
    assert sizes.dtype == roots.dtype == np.uint32
    assert np.array_equal(ctx.to_host(d_labels, np.empty(len(points), np.uint32)), want.labels)
    assert np.array_equal(sizes, want.sizes) and np.array_equal(roots, want.roots)
    one, index = full.select(d_labels, 3, 3, return_index=True)  # the label buffer goes to select as it is
    assert np.array_equal(index, np.flatnonzero(want.labels == 3)) and one.len() == want.sizes[3]
    one.free(), ctx.free(d_labels)

    def check(out, index, keep):
        assert np.array_equal(index, keep) and out.len() == len(keep)
        got_p, got_n = out.download()
        assert np.array_equal(_bits(got_p), _bits(points[keep])) and np.array_equal(_bits(got_n), _bits(normals[keep]))
        assert np.array_equal(out.download_colors(), colors[index])
        out.free()

    keep = R.remove_small_clusters(points, RADIUS, 1, 10)
    assert np.array_equal(keep, np.flatnonzero(~outlier & ~clump))  # the planted rows and the floating clumps go
    check(*full.remove_small_clusters(RADIUS, 1, 10, return_index=True), keep)
    check(*full.remove_small_clusters(RADIUS, 1, 2, 5, return_index=True), R.remove_small_clusters(points, RADIUS, 1, 2, 5))
    check(*full.remove_small_clusters(0.05, 8, 50, return_index=True), R.remove_small_clusters(points, 0.05, 8, 50))
    big = R.largest_cluster(points, RADIUS, 1)
    assert len(big) == 1000
    check(*full.largest_cluster(RADIUS, return_index=True), big)
    check(*full.largest_cluster(0.05, 8, return_index=True), R.largest_cluster(points, 0.05, 8))
    nothing = full.largest_cluster(1e-5, 2)  # no core row at all: an empty cloud
    assert nothing.len() == 0
    nothing.free()
    # the many forms over the batch, hostile and empty clouds included
    host = _batch_clouds()
    clouds = [_device_cloud(ctx, p) for p in host]
    outs, indexes = DevicePointCloud.remove_small_clusters_many(clouds, 0.05, 2, 4, return_index=True)
    for got, p in zip(indexes, host):
        assert np.array_equal(got, R.remove_small_clusters(p, 0.05, 2, 4))
    assert sum(o.len() for o in outs) > 1000
    labels, sizes, roots = DevicePointCloud.cluster_many(clouds, 0.05, 2)
    for d, s, r, p in zip(labels, sizes, roots, host):
        want = R.cluster(p, 0.05, 2)
        assert np.array_equal(s, want.sizes) and np.array_equal(r, want.roots)
        if len(p):
            assert np.array_equal(ctx.to_host(d, np.empty(len(p), np.uint32)), want.labels)
        ctx.free(d)
    for o in outs + clouds:
        o.free()
    with pytest.raises(A3dError):
        full.cluster(-1.0)
    with pytest.raises(A3dError):
        full.cluster(0.05, 0)
    with pytest.raises(A3dError):
        full.remove_small_clusters(0.05, 1, 0)
    full.free()
