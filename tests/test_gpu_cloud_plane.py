"""Plane segmentation of resident clouds on the GPU (a3d_point_clouds_segment_plane_device, DevicePointCloud.segment_plane /
split_plane / remove_plane).

Every comparison is np.array_equal on unsigned integer views, bit for bit, and the expected value is always the numpy
restatement of the rule (plane_restatement.py) or a construction, never the code under test.  The raw call writes its flags
and counts into buffers that are filled with a canary from end to end, with more of it on both sides; the words of counts
past the H candidates must still hold it.

The restatement is brute force over rows x candidates, so the sizes are what it can afford in a few seconds; the cloud of
four million rows has one candidate whose count and flags are known by construction."""
import ctypes as C

import numpy as np
import pytest

import plane_restatement as R
from align3d_amd import A3dError, DevicePointCloud, PointCloud, _abi
from plane_cases import (SCENE_H, SCENE_SEED, SCENE_T, all_degenerate, degenerate_cloud, exact_sheet, hostile_cloud, long_plane,
                         parallel_sheets, raw_bits, sheet_and_slab, tabletop_scene)
from test_gpu_cloud_normals import CANARY, SIZES, _bits, _Guarded, _sample1_frames
from test_gpu_cluster import _batch_clouds

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SPARE = 8  # words of the counts buffer past the candidates: they must stay untouched
HS = (1, 2, 63, 64, 65, 1000, 4096)
SENTINEL = 12345


def _device_cloud(ctx, points, normals=None, colors=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None, colors is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals, colors))


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _segment(ctx, clouds, triples, t, refine=0, counts=True):
    """The raw call into guarded buffers: (status, per cloud {flags [len], counts [H] or None, plane [4] f64, best, inliers,
    refit_rows}).  Asserts the guards and that counts is untouched past H."""
    n = len(clouds)
    triples = [np.ascontiguousarray(tr, np.uint32).reshape(-1, 3) for tr in triples]
    g_flags = [_Guarded(ctx, c.len(), 1) for c in clouds]
    g_counts = [_Guarded(ctx, len(tr) + SPARE, 1) for tr in triples] if counts else None
    planes = (C.c_double * (4 * n))(*[float(SENTINEL)] * (4 * n))
    words = [(C.c_uint64 * n)(*[SENTINEL] * n) for _ in range(3)]
    st = ctx.lib.a3d_point_clouds_segment_plane_device(
        ctx.handle, (_abi.PointCloudViewC * n)(*[c.view() for c in clouds]), n, t, refine,
        (C.c_void_p * n)(*[tr.ctypes.data if len(tr) else None for tr in triples]), (C.c_uint32 * n)(*[len(tr) for tr in triples]),
        (C.c_void_p * n)(*[g.ptr for g in g_flags]), (C.c_void_p * n)(*[g.ptr for g in g_counts]) if counts else None,
        planes, *words)
    outs = []
    for i in range(n):
        out = {"plane": np.array(planes[4 * i:4 * i + 4], np.float64), "best": int(words[0][i]), "inliers": int(words[1][i]),
               "refit_rows": int(words[2][i]), "counts": None}
        body, intact = g_flags[i].read()
        assert intact, "the call wrote outside its flags buffer"
        out["flags"] = body[:, 0]
        g_flags[i].free()
        if counts:
            body, intact = g_counts[i].read()
            assert intact, "the call wrote outside its counts buffer"
            assert (body[len(triples[i]):, 0] == CANARY).all(), "counts: words past the candidates were written"
            out["counts"] = body[:len(triples[i]), 0]
            g_counts[i].free()
        outs.append(out)
    return st, outs


def _assert_equal(out, want, n_rows):
    """One cloud's outputs against the restatement's Segmentation (an empty cloud's flags stay canary: there are none)."""
    if out["counts"] is not None:
        assert np.array_equal(out["counts"], want.counts)
    assert out["best"] == want.best
    assert np.array_equal(out["flags"], want.flags) and len(out["flags"]) == n_rows
    assert np.array_equal(_bits64(out["plane"]), _bits64(want.plane)), (out["plane"], want.plane)
    assert (out["inliers"], out["refit_rows"]) == (want.inliers, want.refit_rows)


def _grid_cloud(k, n):
    """n rows: a noisy sheet (two thirds) in a cube of clutter, shuffled."""
    rng = np.random.default_rng([500, k])
    on = (2 * n) // 3
    sheet = np.c_[rng.uniform(0.25, 0.75, size=(on, 2)), 0.5 + rng.normal(0, 0.01, on)]
    cube = rng.uniform(0.25, 0.75, size=(n - on, 3))
    return np.r_[sheet, cube].astype(np.float32)[rng.permutation(n)]


def test_size_grid(ctx):
    t = 0.03  # three sigma of the sheet's noise
    found = 0
    for k, n in enumerate(SIZES):
        points = _grid_cloud(k, n)
        cloud = _device_cloud(ctx, points)
        for H in HS if n else (0,):
            triples = R.hypotheses(1000 + H, n, H)
            for refine in ((0, 1, 3) if H in (0, 65) else (0,)):
                want = R.segment(points, triples, t, refine)
                st, outs = _segment(ctx, [cloud], [triples], t, refine)
                assert st == _abi.A3D_OK, (n, H, refine)
                _assert_equal(outs[0], want, n)
                found += want.best != NONE
                if n <= 2:
                    assert want.best == NONE  # no three distinct rows
                if n == 2049 and H == 4096:
                    assert want.inliers > 1300 and (want.counts > 0).sum() > 3500  # the sheet, and most candidates are good
        cloud.free()
    assert found > 30


SPLIT_EDGE_HS = (127, 128, 129, 255, 256, 257, 511, 512, 513)


@pytest.mark.parametrize("n", (300, 2049))
def test_candidate_counts_at_the_edges_of_the_score_split(ctx, n):
    """The product build splits the candidates of a score block's tile over grid.y = 1, 2, 4 or 8 blocks, doubling while
    the largest H of the call is at least 128 per split: H from 128 is split in 2, from 256 in 4, from 512 in 8, and a
    block's range is ceil(H / split) candidates, the last one shorter.  One H either side of each edge, against the
    restatement."""
    t = 0.03
    points = _grid_cloud(n, n)
    cloud = _device_cloud(ctx, points)
    for H in SPLIT_EDGE_HS:
        triples = R.hypotheses(2000 + H, n, H)
        want = R.segment(points, triples, t)
        assert want.best != NONE and (want.counts > 0).sum() > H // 2 and want.counts[-1] > 0 and len(np.unique(want.counts)) > 20
        st, outs = _segment(ctx, [cloud], [triples], t)
        assert st == _abi.A3D_OK, H
        _assert_equal(outs[0], want, n)
    cloud.free()


@pytest.mark.parametrize("Hs", ((700, 5, 130), (4096, 1, 257)))
def test_several_blocks_of_candidates_per_job_in_a_batch(ctx, Hs):
    """The candidates kernel takes ceil(max H / 256) blocks per job and finds its job from the block index; here that is
    3 and 16 blocks per job, for jobs of which two have fewer candidates than one block holds, and one has fewer
    candidates than the score grid has splits."""
    hosts = (np.r_[_grid_cloud(51, 3000), raw_bits(52, 30)], _grid_cloud(53, 65), _grid_cloud(54, 1025))
    triples = [R.hypotheses(10 * Hs[0] + i, len(p), H) for i, (p, H) in enumerate(zip(hosts, Hs))]
    clouds = [_device_cloud(ctx, p) for p in hosts]
    st, outs = _segment(ctx, clouds, triples, 0.03, 1)
    assert st == _abi.A3D_OK
    for i, p in enumerate(hosts):
        want = R.segment(p, triples[i], 0.03, 1)
        assert Hs[i] == 1 or want.best != NONE
        _assert_equal(outs[i], want, len(p))
    for c in clouds:
        c.free()


def test_rows_at_exactly_the_threshold_on_exact_coordinates(ctx):
    points, triples, t, flags = exact_sheet()
    assert 0 < flags.sum() < len(flags) and flags[np.abs(points[:, 2]) == t].all() and len(np.unique(np.abs(points[:, 2]))) == 7
    cloud = _device_cloud(ctx, points)
    for refine in (0, 2):
        st, outs = _segment(ctx, [cloud], [triples], t, refine)
        assert st == _abi.A3D_OK and outs[0]["best"] == 0 and outs[0]["counts"].tolist() == [int(flags.sum())]
        if refine == 0:
            assert np.array_equal(outs[0]["flags"], flags)  # by construction
        _assert_equal(outs[0], R.segment(points, triples, t, refine), len(points))
    cloud.free()


def test_ties_go_to_the_lower_candidate(ctx):
    points = _grid_cloud(77, 900)
    triples = R.hypotheses(5, 900, 1000)
    want = R.segment(points, triples, 0.02)
    winner = triples[want.best].copy()
    triples[:5] = np.arange(5)[:, None]  # (k, k, k): degenerate, so nothing before candidate 5 can tie with it
    triples[5] = triples[900] = winner  # the same triple twice
    want = R.segment(points, triples, 0.02)
    assert want.best == 5 and want.counts[5] == want.counts[900] == want.counts.max()
    cloud = _device_cloud(ctx, points)
    st, outs = _segment(ctx, [cloud], [triples], 0.02)
    assert st == _abi.A3D_OK and outs[0]["best"] == 5
    _assert_equal(outs[0], want, 900)
    cloud.free()
    for first in (0, 1):
        points, triples = parallel_sheets(first)
        cloud = _device_cloud(ctx, points)
        st, outs = _segment(ctx, [cloud], [triples], 0.25)
        assert st == _abi.A3D_OK and outs[0]["counts"].tolist() == [150, 150] and outs[0]["best"] == 0
        assert np.array_equal(np.flatnonzero(outs[0]["flags"]) // 150, np.full(150, first))  # the first candidate's sheet
        _assert_equal(outs[0], R.segment(points, triples, 0.25), 300)
        cloud.free()


def test_degenerate_candidates_count_nothing(ctx):
    points, triples, good = degenerate_cloud()
    cloud = _device_cloud(ctx, points)
    want = R.segment(points, triples, 0.05)
    st, outs = _segment(ctx, [cloud], [triples], 0.05)
    assert st == _abi.A3D_OK and (outs[0]["counts"][~good] == 0).all() and (outs[0]["counts"][good] >= 3).all()
    _assert_equal(outs[0], want, len(points))
    points, triples = all_degenerate()
    for refine in (0, 2):
        st, outs = _segment(ctx, [cloud], [triples], 0.05, refine)
        assert st == _abi.A3D_OK and outs[0]["best"] == NONE and not outs[0]["flags"].any() and not outs[0]["counts"].any()
        assert np.array_equal(_bits64(outs[0]["plane"]), np.zeros(4, np.uint64)) and outs[0]["inliers"] == outs[0]["refit_rows"] == 0
    st, outs = _segment(ctx, [cloud], [np.zeros((0, 3), np.uint32)], 0.05)  # no candidates at all
    assert st == _abi.A3D_OK and outs[0]["best"] == NONE and not outs[0]["flags"].any() and not outs[0]["plane"].any()
    cloud.free()


def test_hostile_rows_are_never_flagged(ctx):
    points = hostile_cloud()
    finite = np.isfinite(points).all(axis=1)
    assert 30 <= (~finite).sum() < 200
    triples = R.hypotheses(3, len(points), 300)
    cloud = _device_cloud(ctx, points)
    for refine in (0, 1):
        want = R.segment(points, triples, 0.02, refine)
        assert want.inliers > 600 and not want.flags[~finite].any() and (want.counts == 0).sum() > 5
        st, outs = _segment(ctx, [cloud], [triples], 0.02, refine)
        assert st == _abi.A3D_OK and not outs[0]["flags"][~finite].any()
        _assert_equal(outs[0], want, len(points))
    cloud.free()


def test_two_chunks_per_tile(ctx):
    """More than 4096 chunks of 1024 rows: every tile takes two chunks."""
    n = 4096 * 1024 + 1500
    points, triples, flags = sheet_and_slab(n)
    cloud = _device_cloud(ctx, points)
    st, outs = _segment(ctx, [cloud], [triples], 0.25)
    assert st == _abi.A3D_OK and outs[0]["best"] == 0
    assert outs[0]["counts"].tolist() == [int(flags.sum())] and outs[0]["inliers"] == outs[0]["refit_rows"] == int(flags.sum())
    assert np.array_equal(outs[0]["flags"], flags)
    assert abs(outs[0]["plane"][2]) == 1.0 and outs[0]["plane"][0] == outs[0]["plane"][1] == outs[0]["plane"][3] == 0.0
    cloud.free()


def test_inliers_beyond_the_lattice_are_left_out_of_the_refit(ctx):
    points, triples, t = long_plane()
    cloud = _device_cloud(ctx, points)
    for refine in (0, 2):
        want = R.segment(points, triples, t, refine)
        st, outs = _segment(ctx, [cloud], [triples], t, refine)
        assert st == _abi.A3D_OK and outs[0]["inliers"] > outs[0]["refit_rows"] > 0
        _assert_equal(outs[0], want, len(points))
    cloud.free()


def test_batch_of_unequal_clouds_each_as_if_alone(ctx):
    host = _batch_clouds()
    triples = [R.hypotheses(i, len(p), (i * 37) % 90 if len(p) and i % 5 else 0) for i, p in enumerate(host)]
    assert sum(1 for p in host if len(p) == 0) >= 4 and sum(1 for p, tr in zip(host, triples) if len(p) and not len(tr)) >= 2
    clouds = [_device_cloud(ctx, p) for p in host]
    for refine, counts in ((0, True), (2, True), (1, False)):
        st, outs = _segment(ctx, clouds, triples, 0.01, refine, counts)
        assert st == _abi.A3D_OK
        for i, p in enumerate(host):
            _assert_equal(outs[i], R.segment(p, triples[i], 0.01, refine), len(p))
        assert sum(o["best"] != NONE for o in outs) >= 8
    for c in clouds:
        c.free()


def test_batch_of_three_hundred_tiny_clouds(ctx):
    rng = np.random.default_rng(300)
    host = [rng.uniform(0.0, 0.12, size=(int(n), 3)).astype(np.float32) for n in rng.integers(0, 9, size=300)]
    triples = [R.hypotheses(i, len(p), 4 if len(p) else 0) for i, p in enumerate(host)]
    clouds = [_device_cloud(ctx, p) for p in host]
    st, outs = _segment(ctx, clouds, triples, 0.01, 1)
    assert st == _abi.A3D_OK
    for i, p in enumerate(host):
        _assert_equal(outs[i], R.segment(p, triples[i], 0.01, 1), len(p))
    assert 50 < sum(o["best"] != NONE for o in outs) < 250
    for c in clouds:
        c.free()


def test_two_runs_and_a_row_permutation(ctx):
    points = np.r_[_grid_cloud(41, 5000), raw_bits(42, 50)]
    triples = R.hypotheses(9, len(points), 500)
    perm = np.random.default_rng(43).permutation(len(points))
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))  # row r of the cloud is row inverse[r] of the shuffled one
    cloud, shuffled = _device_cloud(ctx, points), _device_cloud(ctx, points[perm])
    (st1, first), (st2, second) = (_segment(ctx, [cloud], [triples], 0.03, 2) for _ in range(2))
    st3, moved = _segment(ctx, [shuffled], [inverse[triples]], 0.03, 2)
    assert st1 == st2 == st3 == _abi.A3D_OK
    _assert_equal(first[0], R.segment(points, triples, 0.03, 2), len(points))
    for f in ("counts", "flags", "best", "inliers", "refit_rows"):
        assert np.array_equal(first[0][f], second[0][f]), f  # identical words
    assert np.array_equal(_bits64(first[0]["plane"]), _bits64(second[0]["plane"]))
    for f in ("counts", "best", "inliers", "refit_rows"):
        assert np.array_equal(first[0][f], moved[0][f]), f
    assert np.array_equal(first[0]["flags"][perm], moved[0]["flags"]) and first[0]["inliers"] > 2000
    assert np.array_equal(_bits64(first[0]["plane"]), _bits64(moved[0]["plane"]))
    cloud.free(), shuffled.free()


@pytest.mark.parametrize("knob,value", [("A3D_PLANE_ROWS", "1"), ("A3D_PLANE_ROWS", "2"), ("A3D_PLANE_ROWS", "8"),
                                        ("A3D_PLANE_SPLIT", "1"), ("A3D_PLANE_SPLIT", "3"), ("A3D_PLANE_SPLIT", "64"),
                                        ("A3D_PLANE_COUNTERS", "global")])
def test_the_forms_the_diagnostics_build_keeps_give_the_same_bits(ctx, diag_ctx, monkeypatch, knob, value):
    hosts = (np.r_[_grid_cloud(51, 3000), raw_bits(52, 30)], _grid_cloud(53, 65), _grid_cloud(54, 1025))
    triples = [R.hypotheses(i, len(p), H) for i, (p, H) in enumerate(zip(hosts, (700, 5, 130)))]
    clouds, diag_clouds = [_device_cloud(ctx, p) for p in hosts], [_device_cloud(diag_ctx, p) for p in hosts]
    monkeypatch.delenv(knob, raising=False)
    st, outs = _segment(ctx, clouds, triples, 0.03, 1)
    monkeypatch.setenv(knob, value)
    st2, diag = _segment(diag_ctx, diag_clouds, triples, 0.03, 1)
    assert st == st2 == _abi.A3D_OK and outs[0]["inliers"] > 1000
    for i in range(len(hosts)):
        for f in ("counts", "flags", "best", "inliers", "refit_rows"):
            assert np.array_equal(outs[i][f], diag[i][f]), (i, f)
        assert np.array_equal(_bits64(outs[i]["plane"]), _bits64(diag[i]["plane"]))
    for c in clouds + diag_clouds:
        c.free()


def test_refusals_on_the_device_leave_everything_untouched(ctx):
    points = _grid_cloud(85, 300)
    cloud = _device_cloud(ctx, points, _grid_cloud(86, 300))
    good = R.hypotheses(1, 300, 20)
    flags = _Guarded(ctx, 300, 1)
    counts = _Guarded(ctx, 64, 1)
    plane = (C.c_double * 4)(*[float(SENTINEL)] * 4)
    words = [(C.c_uint64 * 1)(SENTINEL) for _ in range(3)]

    def call(d_flags=flags.ptr, d_counts=counts.ptr, t=0.02, refine=0, triples=good):
        triples = np.ascontiguousarray(triples, np.uint32)
        return ctx.lib.a3d_point_clouds_segment_plane_device(
            ctx.handle, (_abi.PointCloudViewC * 1)(cloud.view()), 1, t, refine, (C.c_void_p * 1)(triples.ctypes.data),
            (C.c_uint32 * 1)(len(triples)), (C.c_void_p * 1)(d_flags), (C.c_void_p * 1)(d_counts), plane, *words)

    bad_index = good.copy()
    bad_index[7, 1] = 300
    refused = [dict(d_flags=cloud.d_points), dict(d_flags=C.c_void_p(cloud.d_normals.value + 3596)),
               dict(d_counts=C.c_void_p(flags.ptr.value + 1196)), dict(t=0.0), dict(t=float("nan")), dict(t=-0.02),
               dict(triples=np.zeros((4097, 3), np.uint32)), dict(triples=bad_index), dict(refine=9)]
    for change in refused:
        assert call(**change) == _abi.A3D_INVALID_PARAMETER, change
    assert list(plane) == [float(SENTINEL)] * 4 and all(w[0] == SENTINEL for w in words)
    for g in (flags, counts):
        body, intact = g.read()
        assert intact and (body == CANARY).all()
    got_p, got_n = cloud.download()
    assert np.array_equal(_bits(got_p), _bits(points)) and np.array_equal(_bits(got_n), _bits(_grid_cloud(86, 300)))
    want = R.segment(points, good, 0.02)
    assert call() == _abi.A3D_OK and words[0][0] == want.best and words[1][0] == want.inliers
    assert np.array_equal(flags.read()[0][:, 0], want.flags) and np.array_equal(counts.read()[0][:20, 0], want.counts)
    assert np.array_equal(_bits64(list(plane)), _bits64(want.plane))
    flags.free(), counts.free(), cloud.free()


# ---- the wrappers ------------------------------------------------------------------------------------------------------


def test_wrappers_equal_the_restatement_end_to_end(ctx):
    points, normals, colors, floor, box = tabletop_scene()
    triples = R.hypotheses(SCENE_SEED, len(points), SCENE_H)
    want = R.segment(points, triples, SCENE_T)
    assert floor[triples[want.best]].all() and np.array_equal(want.flags.astype(bool), floor)  # exactly the floor
    full = _device_cloud(ctx, points, normals, colors)
    plane, d_flags, inliers = full.segment_plane(SCENE_T, SCENE_H, seed=SCENE_SEED)
    assert plane.dtype == np.float64 and np.array_equal(_bits64(plane), _bits64(want.plane)) and inliers == 12000
    assert np.array_equal(ctx.to_host(d_flags, np.empty(len(points), np.uint32)), want.flags)
    ctx.free(d_flags)
    refined = R.segment(points, triples, SCENE_T, 2)
    plane, d_flags, inliers = full.segment_plane(SCENE_T, refine=2, triples=triples)  # the caller's own candidates
    assert np.array_equal(_bits64(plane), _bits64(refined.plane)) and inliers == refined.inliers
    ctx.free(d_flags)

    def check(out, index, keep):
        assert np.array_equal(index, keep) and out.len() == len(keep) and index.dtype == np.uint32
        got_p, got_n = out.download()
        assert np.array_equal(_bits(got_p), _bits(points[keep])) and np.array_equal(_bits(got_n), _bits(normals[keep]))
        assert np.array_equal(out.download_colors(), colors[keep])

    plane, on, off, on_index, off_index = full.split_plane(SCENE_T, SCENE_H, seed=SCENE_SEED, return_index=True)
    assert np.array_equal(_bits64(plane), _bits64(want.plane))
    check(on, on_index, np.flatnonzero(floor))
    check(off, off_index, np.flatnonzero(~floor))
    on.free(), off.free()
    plane, on, off = full.split_plane(SCENE_T, SCENE_H, seed=SCENE_SEED)
    assert (on.len(), off.len()) == (12000, 8000)
    on.free(), off.free()
    rest, rest_index = full.remove_plane(SCENE_T, SCENE_H, seed=SCENE_SEED, return_index=True)
    check(rest, rest_index, np.flatnonzero(~floor))
    # the case the feature exists for: the box stands on the floor, so the largest cluster of the scene is both ...
    radius = 0.08
    together, together_index = full.largest_cluster(radius, return_index=True)
    assert box[together_index].sum() == 6000 and floor[together_index].sum() > 11000
    together.free()
    # ... and with the plane gone it is the box
    alone, alone_index = rest.largest_cluster(radius, return_index=True)
    assert np.array_equal(rest_index[alone_index], np.flatnonzero(box))
    alone.free(), rest.free()
    # the many forms over the batch, hostile and empty clouds included
    host = _batch_clouds()
    clouds = [_device_cloud(ctx, p) for p in host]
    wants = [R.segment(p, R.hypotheses(7, len(p), 40 if len(p) else 0), 0.01, 1) for p in host]
    planes, flags, counts = DevicePointCloud.segment_plane_many(clouds, 0.01, 40, seed=7, refine=1)
    for w, pl, d, k, p in zip(wants, planes, flags, counts, host):
        assert np.array_equal(_bits64(pl), _bits64(w.plane)) and k == w.inliers
        if len(p):
            assert np.array_equal(ctx.to_host(d, np.empty(len(p), np.uint32)), w.flags)
        ctx.free(d)
    planes, ons, offs, on_indexes, off_indexes = DevicePointCloud.split_plane_many(clouds, 0.01, 40, seed=7, refine=1,
                                                                                 return_index=True)
    rests, rest_indexes = DevicePointCloud.remove_plane_many(clouds, 0.01, 40, seed=7, refine=1, return_index=True)
    for w, a, b, c in zip(wants, on_indexes, off_indexes, rest_indexes):
        assert np.array_equal(a, np.flatnonzero(w.flags == 1)) and np.array_equal(b, np.flatnonzero(w.flags == 0))
        assert np.array_equal(c, b)
    assert sum(o.len() for o in ons) > 100 and sum(o.len() for o in offs) > 100
    for o in ons + offs + rests + clouds:
        o.free()
    for bad in (dict(distance_threshold=-1.0), dict(distance_threshold=0.01, num_iterations=4097),
                dict(distance_threshold=0.01, refine=9), dict(distance_threshold=0.01, triples=[[0, 1, len(points)]]),
                dict(distance_threshold=0.01, triples=[[0, 1]]), dict(distance_threshold=float("nan"))):
        with pytest.raises(A3dError):
            full.segment_plane(**bad)
    with pytest.raises(A3dError):
        DevicePointCloud.segment_plane_many([full, full], 0.01, triples=[None])
    full.free()


def test_a_frame_of_sample1_is_consistent_with_its_best_candidate(ctx):
    frame = _sample1_frames(ctx)[0]
    n = frame.len()
    assert n > 100000
    points = frame.download()[0]
    t, H = 0.02, 512
    triples = R.hypotheses(0, n, H)
    st, outs = _segment(ctx, [frame], [triples], t)
    out = outs[0]
    assert st == _abi.A3D_OK and out["best"] != NONE
    assert out["counts"][out["best"]] == out["inliers"] == int(out["flags"].sum()) == out["counts"].max() > n // 20
    assert out["best"] == int(np.argmax(out["counts"]))  # the first of the largest
    normal, point, good = R.candidates(points, triples[out["best"]:out["best"] + 1])
    assert good[0]
    assert np.array_equal(out["flags"].astype(bool), R.inliers(points, normal[0], point[0], t))  # step 2, every row
    assert out["refit_rows"] <= out["inliers"] and abs(np.linalg.norm(out["plane"][:3]) - 1) < 1e-6 and out["plane"][3] >= 0
    # the refit minimises the sum of squared distances of the flagged rows (on a lattice of t / 64), and every one of them
    # is within t of the best candidate's plane: their root mean square distance to the refit cannot exceed t by more
    flagged = points[out["flags"] == 1].astype(np.float64)
    assert np.sqrt(np.mean((flagged @ out["plane"][:3] + out["plane"][3]) ** 2)) < 1.1 * t
