"""The three neighbourhood entries at ties and exact edges, on the GPU: the cases of neighbour_edge_cases.py (what each one is
and why stands there; test_neighbour_edge_cases_cpu.py proves it) through the raw calls into canary-guarded buffers.

Every comparison is on unsigned integer views, bit for bit.  The expected value is the numpy restatement of the rule and,
where the construction fixes a value (counts, Q, the statistics, axis normals with their zero signs, the curvature of three
equal eigenvalues, flags, clusters), that value as well.  Every case runs alone, with the other cases of its kernel as one
batch, and, where that leaves the coordinates as they are, as part of one cloud under a seeded row permutation; the tie and
witness cases run once more on the diagnostics build under each form it keeps.  Each test prints its wall time."""
import time

import numpy as np
import pytest

import cluster_restatement as CR
import neighbour_edge_cases as E
import normals_restatement as NR
import outlier_restatement as OR
import plane_restatement as PR
from align3d_amd import _abi
from test_gpu_cloud_normals import _assert_matches, _bits, _call, _device_cloud
from test_gpu_cloud_outliers import _assert_knn, _knn
from test_gpu_cloud_plane import _assert_equal as _assert_plane
from test_gpu_cloud_plane import _bits64, _segment
from test_gpu_cluster import _assert_construction, _cluster
from test_gpu_cluster import _assert_equal as _assert_clusters

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NORMALS_FORMS = (("A3D_NORMALS_ORDER", "input"), ("A3D_NORMALS_AHEAD", "1"), ("A3D_NORMALS_LDS", "1"))
KNN_FORMS = (("A3D_OUTLIERS_K", "32"), ("A3D_OUTLIERS_SELECT", "t"))
PLANE_FORMS = (("A3D_PLANE_ROWS", "1"), ("A3D_PLANE_ROWS", "2"), ("A3D_PLANE_ROWS", "8"))


@pytest.fixture(autouse=True)
def _wall_time(request):
    start = time.perf_counter()
    yield
    print(f"[wall time] {request.node.name}: {time.perf_counter() - start:.3f} s")


_memo = {}


def _once(key, build):
    """Builders and restatements are computed once and shared; nothing changes them."""
    if key not in _memo:
        _memo[key] = build()
    return _memo[key]


def _free(clouds):
    for c in clouds:
        c.free()


# ---- normals -----------------------------------------------------------------------------------------------------------


def _normals_jobs():
    """[(name, points, min_neighbors, eye, normals by construction or None, curvature bits or None, counts, valid)]: the
    tie cloud and every (degenerate case, viewpoint)."""
    def build():
        tie = E.normals_rint_ties()
        jobs = [(tie["name"], tie["points"], 3, np.asarray(tie["viewpoint"], np.float32), None, None, None, None)]
        for case in E.normals_degenerate():
            for view in case["views"]:
                jobs.append((case["name"], case["points"], case["min_neighbors"], view["eye"], view["normals"], case["curvature"],
                             case["counts"], case["valid"]))
        return jobs
    return _once("normals jobs", build)


def _normals_expected(i):
    name, points, m, eye, _, _, _, _ = _normals_jobs()[i]
    return _once(("normals expected", i), lambda: NR.estimate_normals(points, E.TIE_RADIUS, m, viewpoint=eye))


def _check_normals_job(i, out, valid, dropped):
    name, points, m, eye, normals, curvature, counts, ok = _normals_jobs()[i]
    _assert_matches(out, valid, dropped, _normals_expected(i), points, E.TIE_RADIUS)
    if counts is not None:  # by construction
        assert np.array_equal(out["counts"], counts) and valid == int(ok.sum()) and dropped == 0, name
        assert (out["normals"][~ok] == 0).all() and (out["curvature"][~ok] == 0).all(), name  # all-zero bits, count reported
    if normals is not None:
        assert np.array_equal(out["normals"], _bits(normals)), (name, eye)  # the zeros carry the sign
    if curvature is not None:
        assert (out["curvature"][ok] == curvature).all(), name


def _run_normals_jobs(ctx, which):
    """The jobs `which`, each alone, then as one batch per min_neighbors."""
    jobs = _normals_jobs()
    for i in which:
        cloud = _device_cloud(ctx, jobs[i][1])
        st, valid, dropped, outs = _call(ctx, [cloud], E.TIE_RADIUS, [jobs[i][3]], min_neighbors=jobs[i][2])
        assert st == _abi.A3D_OK
        _check_normals_job(i, outs[0], valid[0], dropped[0])
        cloud.free()
    for m in sorted({jobs[i][2] for i in which}):
        batch = [i for i in which if jobs[i][2] == m]
        clouds = [_device_cloud(ctx, jobs[i][1]) for i in batch]
        st, valid, dropped, outs = _call(ctx, clouds, E.TIE_RADIUS, [jobs[i][3] for i in batch], min_neighbors=m)
        assert st == _abi.A3D_OK
        for at, i in enumerate(batch):
            _check_normals_job(i, outs[at], valid[at], dropped[at])
        _free(clouds)


def test_normals_rint_ties(ctx):
    _run_normals_jobs(ctx, [0])
    # the rows permuted: every row keeps its bits
    tie = E.normals_rint_ties()
    perm = np.random.default_rng(3).permutation(len(tie["points"]))
    cloud = _device_cloud(ctx, tie["points"][perm])
    st, valid, dropped, outs = _call(ctx, [cloud], E.TIE_RADIUS, [tie["viewpoint"]])
    want = _normals_expected(0)
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], valid[0], dropped[0], tuple(a[perm] for a in want), tie["points"][perm], E.TIE_RADIUS)
    cloud.free()


def test_normals_degenerate_alone_and_as_batches(ctx):
    jobs = _normals_jobs()
    assert len(jobs) > 40
    _run_normals_jobs(ctx, range(1, len(jobs)))
    octahedron = [j for j in jobs if j[0] == "octahedron"][0]  # the issue's statement of it, word for word
    assert np.array_equal(octahedron[4], np.tile(np.float32([-1.0, -0.0, -0.0]), (7, 1))) and octahedron[5] == 0x3EAAAAAB
    assert np.array_equal(_bits(octahedron[4])[0], [0xBF800000, 0x80000000, 0x80000000])


def _all_normals_cases():
    parts = [E.normals_rint_ties()["points"]] + [c["points"] for c in E.normals_degenerate()]
    return np.concatenate(parts), np.cumsum([len(p) for p in parts])[:-1]


def test_normals_cases_concatenated_and_permuted(ctx):
    points, splits = _all_normals_cases()
    perm = np.random.default_rng(4).permutation(len(points))
    shuffled = points[perm]
    eye = np.float32(E.EYE)
    want = _once("normals concatenated", lambda: NR.estimate_normals(shuffled, E.TIE_RADIUS, viewpoint=eye))
    cloud = _device_cloud(ctx, shuffled)
    st, valid, dropped, outs = _call(ctx, [cloud], E.TIE_RADIUS, [eye])
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], valid[0], dropped[0], want, shuffled, E.TIE_RADIUS)
    # no case is a neighbour of another: every row has the count it has in its own cloud
    alone = np.concatenate([NR.estimate_normals(p, E.TIE_RADIUS)[2] for p in np.split(points, splits)])
    assert np.array_equal(outs[0]["counts"], alone[perm])
    cloud.free()


@pytest.mark.parametrize("knob,value", NORMALS_FORMS)
def test_normals_cases_on_the_forms_the_diagnostics_build_keeps(diag_ctx, monkeypatch, knob, value):
    monkeypatch.setenv(knob, value)
    jobs = _normals_jobs()
    _run_normals_jobs(diag_ctx, [i for i in range(len(jobs)) if jobs[i][2] == 3])
    case = E.normals_orient_cases()[0]
    cloud = _device_cloud(diag_ctx, case["points"], case["old_normals"])
    st, valid, dropped, outs = _call(diag_ctx, [cloud], case["radius"], orient=1)
    assert st == _abi.A3D_OK and np.array_equal(outs[0]["normals"], _bits(case["normals"]))
    cloud.free()


def test_normals_orient_cases_raw_and_in_place(ctx):
    cases = E.normals_orient_cases()
    wants = [NR.estimate_normals(c["points"], c["radius"], old_normals=c["old_normals"]) for c in cases]
    clouds = [_device_cloud(ctx, c["points"], c["old_normals"]) for c in cases]
    for which in ([0], [1], [0, 1]):  # alone and as a batch
        st, valid, dropped, outs = _call(ctx, [clouds[i] for i in which], E.TIE_RADIUS, orient=1)
        assert st == _abi.A3D_OK
        for at, i in enumerate(which):
            _assert_matches(outs[at], valid[at], dropped[at], wants[i], cases[i]["points"], E.TIE_RADIUS)
            assert valid[at] == 9
            if cases[i]["normals"] is not None:
                assert np.array_equal(outs[at]["normals"], _bits(cases[i]["normals"]))
            for row, kind in enumerate(cases[i]["kinds"]):  # which side of the plane each row ends on
                side = float(outs[at]["normals"][row].view(np.float32).astype(np.float64) @ cases[i]["unit"])
                assert (side < 0) == (kind == "against") or kind not in ("along", "against")
    _free(clouds)
    # one cloud of both planes, permuted, through the wrapper, in place over the old normals
    points = np.concatenate([c["points"] for c in cases])
    old = np.concatenate([c["old_normals"] for c in cases])
    perm = np.random.default_rng(5).permutation(len(points))
    points, old = points[perm], old[perm]
    want = NR.estimate_normals(points, E.TIE_RADIUS, old_normals=old)
    assert np.array_equal(_bits(want[0]), _bits(np.concatenate([w[0] for w in wants])[perm]))  # the planes are not neighbours
    cloud = _device_cloud(ctx, points, old)
    assert cloud.estimate_normals(E.TIE_RADIUS, orient="normals") == 18
    got_points, got = cloud.download()
    assert np.array_equal(_bits(got_points), _bits(points)) and np.array_equal(_bits(got), _bits(want[0]))
    cloud.free()


# ---- knn and cluster ---------------------------------------------------------------------------------------------------


def _knn_expected(name, points, radius, k):
    return _once(("knn", name, k), lambda: OR.knn_distance(points, radius, k))


def _check_tie_cloud(case, k, out, stats, dropped):
    _assert_knn(out, stats, dropped, case["points"], case["radius"], k, _knn_expected(case["name"], case["points"], case["radius"], k))
    assert (out["counts"] == len(case["points"])).all() and int(out["qsum"][0]) == case["centre_q"][k], (case["name"], k)
    if case["rows_q"] is not None:
        assert out["qsum"].tolist() == case["rows_q"][k] and stats == case["stats"][k], (case["name"], k)


def _run_tie_clouds(ctx, k):
    cases = [c for c in E.knn_rint_ties() if k in c["centre_q"]]
    clouds = [_device_cloud(ctx, c["points"]) for c in cases]
    for case, cloud in zip(cases, clouds):
        st, stats, dropped, outs = _knn(ctx, [cloud], case["radius"], k)
        assert st == _abi.A3D_OK
        _check_tie_cloud(case, k, outs[0], stats[0], dropped[0])
    st, stats, dropped, outs = _knn(ctx, clouds, E.TIE_RADIUS, k)
    assert st == _abi.A3D_OK
    for i, case in enumerate(cases):
        _check_tie_cloud(case, k, outs[i], stats[i], dropped[i])
    _free(clouds)
    return cases


@pytest.mark.parametrize("k", E.KNN_KS + (10,))
def test_knn_rint_ties(ctx, k):
    cases = _run_tie_clouds(ctx, k)
    assert len(cases) == (1 if k == 10 else 5 if k < 10 else 4)  # (the cloud of ten others has no k above 10)
    if k == 10:
        assert cases[0]["centre_q"][10] == 4318
        return
    # the clouds with a centre of their own as one cloud, permuted: every row keeps its Q, the statistics add up
    parts = [c for c in cases if c["name"] != "knn ties, ten others along +x"]
    points = np.concatenate([c["points"] for c in parts])
    perm = np.random.default_rng(6).permutation(len(points))
    want = _knn_expected("tie clouds concatenated", points[perm], E.TIE_RADIUS, k)
    alone = np.concatenate([_knn_expected(c["name"], c["points"], c["radius"], k)[1] for c in parts])
    assert np.array_equal(want[1], alone[perm]) and want[2] == OR.stats_of(alone)
    cloud = _device_cloud(ctx, points[perm])
    st, stats, dropped, outs = _knn(ctx, [cloud], E.TIE_RADIUS, k)
    assert st == _abi.A3D_OK
    _assert_knn(outs[0], stats[0], dropped[0], points[perm], E.TIE_RADIUS, k, want)
    cloud.free()


def test_knn_equal_kth_and_its_clusters(ctx):
    case = E.knn_equal_kth()
    points = case["points"]
    perm = np.random.default_rng(7).permutation(len(points))
    clouds = [_device_cloud(ctx, points), _device_cloud(ctx, points[perm])]
    for k, q in case["centre_q"].items():
        want = OR.knn_distance(points, case["radius"], k)
        for which in ([0], [0, 1]):
            st, stats, dropped, outs = _knn(ctx, [clouds[i] for i in which], case["radius"], k)
            assert st == _abi.A3D_OK
            _assert_knn(outs[0], stats[0], dropped[0], points, case["radius"], k, want)
            assert int(outs[0]["qsum"][0]) == q and outs[0]["counts"][0] == case["centre_count"]
            if len(which) == 2:
                assert np.array_equal(outs[1]["qsum"], want[1][perm]) and stats[1] == want[2]
    # the row at d2 == r2 is a neighbour of the centre: one cluster of all 47 rows from min_points 1 up to the least count
    for m in (1, int(OR.knn_distance(points, case["radius"], 0)[0].min()), 47, 48):
        want = CR.cluster(points, case["radius"], m)
        st, outs = _cluster(ctx, [clouds[0]], case["radius"], m)
        assert st == _abi.A3D_OK
        _assert_clusters(outs[0], want)
    st, outs = _cluster(ctx, [clouds[0]], case["radius"], 1)
    _assert_construction(outs[0], np.zeros(47, np.uint32), [47], [0])
    _free(clouds)
    # every knn case of this radius as one batch: the tie clouds, this cloud, the witness clouds at the origin
    hosts = [(c["name"], c["points"]) for c in E.knn_rint_ties()] + [(case["name"], points)]
    hosts += [(("origin", E.TIE_RADIUS, i), p) for i, p in enumerate(_witnesses(E.TIE_RADIUS)["origin"]["clouds"])]
    clouds = [_device_cloud(ctx, p) for _, p in hosts]
    for k in (2, 8):
        st, stats, dropped, outs = _knn(ctx, clouds, E.TIE_RADIUS, k)
        st2, labelled = _cluster(ctx, clouds, E.TIE_RADIUS, k)
        assert st == st2 == _abi.A3D_OK and len(clouds) > 40
        for i, (key, p) in enumerate(hosts):
            _assert_knn(outs[i], stats[i], dropped[i], p, E.TIE_RADIUS, k, _knn_expected(key, p, E.TIE_RADIUS, k))
            _assert_clusters(labelled[i], _once(("cluster", key, k), lambda: CR.cluster(p, E.TIE_RADIUS, k)))
    _free(clouds)


def _witness_labels(pairs):
    """(labels, sizes, roots) of min_points = 1 for rows [p_i, p_j, helper] per pair, by construction."""
    labels, sizes, roots = [], [], []
    for i, pr in enumerate(pairs):
        c = len(sizes)
        if pr["inside"]:
            labels += [c, c, c]
            sizes += [3]
            roots += [3 * i]
        else:
            labels += [c, c + 1, c]
            sizes += [2, 1]
            roots += [3 * i, 3 * i + 1]
    return np.asarray(labels, np.uint32), sizes, roots


def _witness_counts(pairs):
    inside = np.asarray([pr["inside"] for pr in pairs])
    return np.stack([2 + inside, 1 + inside, np.full(len(pairs), 2)], axis=1).reshape(-1).astype(np.uint32), inside


ENTRIES = ("knn", "cluster", "normals")


def _check_witness_clouds(ctx, entry, clouds, hosts, radius, pairs_of, keys):
    """One call of one entry on resident clouds of rows [p_i, p_j, helper] per pair, against the restatement and the
    construction.  knn: k = 0, 1, 2.  cluster: min_points 1 (by construction) and 3 (the p_i of inside pairs are the core
    rows).  normals: min_neighbors 3, so p_i is valid iff the pair is inside; its count says the same."""
    built = [_witness_counts(pairs) for pairs in pairs_of]
    if entry == "knn":
        for k in (0, 1, 2):
            st, stats, dropped, outs = _knn(ctx, clouds, radius, k)
            assert st == _abi.A3D_OK
            for i, (counts, inside) in enumerate(built):
                _assert_knn(outs[i], stats[i], dropped[i], hosts[i], radius, k, _knn_expected(keys[i], hosts[i], radius, k))
                assert np.array_equal(outs[i]["counts"], counts)
                if k:  # p_j has an other iff the pair is inside; p_i has two iff it is
                    assert np.array_equal(outs[i]["qsum"].reshape(-1, 3)[:, 2 - k] != NONE, inside)
    elif entry == "cluster":
        for m in (1, 3):
            st, outs = _cluster(ctx, clouds, radius, m)
            assert st == _abi.A3D_OK
            for i, pairs in enumerate(pairs_of):
                if m == 1:
                    _assert_construction(outs[i], *_witness_labels(pairs))
                _assert_clusters(outs[i], _once(("cluster", keys[i], m), lambda: CR.cluster(hosts[i], radius, m)))
    else:
        st, valid, dropped, outs = _call(ctx, clouds, radius)
        assert st == _abi.A3D_OK
        for i, (counts, inside) in enumerate(built):
            want = _once(("normals", keys[i]), lambda: NR.estimate_normals(hosts[i], radius))
            _assert_matches(outs[i], valid[i], dropped[i], want, hosts[i], radius)
            assert np.array_equal(outs[i]["counts"], counts) and valid[i] == int(inside.sum())
            assert np.array_equal(outs[i]["normals"].any(axis=1).reshape(-1, 3)[:, 0], inside)  # p_i alone has a normal
            assert not outs[i]["normals"].reshape(-1, 3, 3)[:, 1:].any()


def _witnesses(radius):
    return _once(("witnesses", radius), lambda: E.d2_witnesses(radius))


@pytest.mark.parametrize("radius", E.WITNESS_RADII)
@pytest.mark.parametrize("entry", ENTRIES)
def test_d2_witnesses(ctx, entry, radius):
    w = _witnesses(radius)
    print(f"witnesses at r = {radius}: {w['found']}")
    # at the origin: every cloud alone, then all of them as one batch
    pairs, hosts = w["origin"]["pairs"], w["origin"]["clouds"]
    keys = [("origin", radius, i) for i in range(len(hosts))]
    clouds = [_device_cloud(ctx, p) for p in hosts]
    for i, cloud in enumerate(clouds):
        _check_witness_clouds(ctx, entry, [cloud], [hosts[i]], radius, [[pairs[i]]], [keys[i]])
    _check_witness_clouds(ctx, entry, clouds, hosts, radius, [[pr] for pr in pairs], keys)
    _free(clouds)
    # in place: the one cloud as it stands
    points, pairs = w["in place"]["points"], w["in place"]["pairs"]
    cloud = _device_cloud(ctx, points)
    _check_witness_clouds(ctx, entry, [cloud], [points], radius, [pairs], [("in place", radius)])
    cloud.free()
    if entry != "knn":
        return
    # and under a row permutation: every row keeps its count and its Q
    perm = np.random.default_rng(8).permutation(len(points))
    cloud = _device_cloud(ctx, points[perm])
    for k in (1, 2):
        want = _knn_expected(("in place", radius), points, radius, k)
        st, stats, dropped, outs = _knn(ctx, [cloud], radius, k)
        assert st == _abi.A3D_OK and stats[0] == want[2]
        assert np.array_equal(outs[0]["counts"], want[0][perm]) and np.array_equal(outs[0]["qsum"], want[1][perm])
    cloud.free()


@pytest.mark.parametrize("knob,value", KNN_FORMS + (("A3D_CLUSTER_LINK", "all"),) + NORMALS_FORMS)
def test_witnesses_and_knn_ties_on_the_forms_the_diagnostics_build_keeps(diag_ctx, monkeypatch, knob, value):
    monkeypatch.setenv(knob, value)
    entry = "cluster" if knob == "A3D_CLUSTER_LINK" else "normals" if knob.startswith("A3D_NORMALS") else "knn"
    if entry == "knn":
        for k in E.KNN_KS:
            _run_tie_clouds(diag_ctx, k)
    for radius in E.WITNESS_RADII:
        w = _witnesses(radius)
        points, pairs = w["in place"]["points"], w["in place"]["pairs"]
        cloud = _device_cloud(diag_ctx, points)
        _check_witness_clouds(diag_ctx, entry, [cloud], [points], radius, [pairs], [("in place", radius)])
        cloud.free()
        hosts = w["origin"]["clouds"]
        clouds = [_device_cloud(diag_ctx, p) for p in hosts]
        _check_witness_clouds(diag_ctx, entry, clouds, hosts, radius, [[pr] for pr in w["origin"]["pairs"]],
                              [("origin", radius, i) for i in range(len(hosts))])
        _free(clouds)


def test_statistical_filter_on_the_tie_cloud(ctx):
    case = E.knn_rint_ties()[4]  # others in all directions
    points = case["points"]
    for k, ratio in ((8, 0.5), (32, 0.0), (17, 0.25)):
        keep, t = OR.remove_statistical_outliers(points, case["radius"], k, ratio)
        _, qsum, stats = OR.knn_distance(points, case["radius"], k)
        assert 0 < len(keep) < len(points) and t == OR.threshold(stats, ratio)
        cloud = _device_cloud(ctx, points)
        out, index = cloud.remove_statistical_outliers(case["radius"], k, ratio, return_index=True)
        assert np.array_equal(index, keep) and np.array_equal(_bits(out.download()[0]), _bits(points[keep]))
        d_counts, d_qsum, got_stats = cloud.neighbor_distances(case["radius"], k)
        assert got_stats == (stats[0], stats[1], stats[2] + (stats[3] << 32)) and type(cloud).knn_distance_threshold(got_stats, ratio) == t
        ctx.free(d_counts), ctx.free(d_qsum)
        out.free(), cloud.free()


# ---- plane -------------------------------------------------------------------------------------------------------------


def _plane_expected(case, refine):
    return _once(("plane", case["name"], refine), lambda: PR.segment(case["points"], case["triples"], case["t"], refine))


def _check_plane(case, refine, out):
    want = _plane_expected(case, refine)
    _assert_plane(out, want, len(case["points"]))
    if refine == 0 and "flags" in case:
        assert np.array_equal(out["flags"], case["flags"]) and out["counts"].tolist() == [int(case["flags"].sum())] and out["best"] == 0
    if refine == 0 and "record" in case:  # the plane of the integers known by construction
        normal, _, _ = PR.candidates(case["points"], case["triples"])
        plane, valid, _ = PR.plane_from_moments(case["record"], case["points"][0], case["t"], normal[0])
        assert valid and np.array_equal(_bits64(out["plane"]), _bits64(plane)) and out["refit_rows"] == case["record"][0] == 9
    if "good" in case:
        assert (out["best"] == 0) == case["good"] and out["counts"].tolist() == [3 if case["good"] else 0]
        if not case["good"]:
            assert out["best"] == NONE and not out["flags"].any() and np.array_equal(_bits64(out["plane"]), np.zeros(4, np.uint64))


def _run_plane_cases(ctx, cases, refines=(0, 1)):
    """Each case alone, then all of them (they share t) as one batch, at every refine."""
    clouds = [_device_cloud(ctx, c["points"]) for c in cases]
    for refine in refines:
        for case, cloud in zip(cases, clouds):
            st, outs = _segment(ctx, [cloud], [case["triples"]], case["t"], refine)
            assert st == _abi.A3D_OK
            _check_plane(case, refine, outs[0])
        if len(cases) > 1:
            assert len({c["t"] for c in cases}) == 1
            st, outs = _segment(ctx, clouds, [c["triples"] for c in cases], cases[0]["t"], refine)
            assert st == _abi.A3D_OK
            for case, out in zip(cases, outs):
                _check_plane(case, refine, out)
    _free(clouds)


def _permuted(case, seed):
    """The case with its rows permuted and its triple renumbered (values by construction follow the rows)."""
    perm = np.random.default_rng(seed).permutation(len(case["points"]))
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    moved = {"name": case["name"] + ", permuted", "points": case["points"][perm], "t": case["t"],
             "triples": inverse[case["triples"].astype(np.int64)].astype(np.uint32)}
    if "flags" in case:
        moved["flags"] = case["flags"][perm]
    return moved, perm


def test_plane_rint_ties(ctx):
    cases = _once("plane ties", E.plane_rint_ties)
    _run_plane_cases(ctx, cases)
    moved, perm = _permuted(cases[3], 9)
    _run_plane_cases(ctx, [moved])
    for refine in (0, 1):  # integer moments: the plane does not depend on the order of the rows
        assert np.array_equal(_bits64(_plane_expected(moved, refine).plane), _bits64(_plane_expected(cases[3], refine).plane))


def test_plane_threshold_witnesses_and_degenerate_cut(ctx):
    w = _once("plane witnesses", E.plane_threshold_witnesses)
    cut = _once("plane cut", E.plane_degenerate_cut)
    print(f"plane threshold witnesses: {w['found']}")
    _run_plane_cases(ctx, [w] + cut)  # one t: alone and as one batch
    moved, perm = _permuted(w, 10)
    _run_plane_cases(ctx, [moved])


@pytest.mark.parametrize("knob,value", PLANE_FORMS)
def test_plane_cases_on_the_forms_the_diagnostics_build_keeps(diag_ctx, monkeypatch, knob, value):
    monkeypatch.setenv(knob, value)
    _run_plane_cases(diag_ctx, _once("plane ties", E.plane_rint_ties))
    _run_plane_cases(diag_ctx, [_once("plane witnesses", E.plane_threshold_witnesses)] + _once("plane cut", E.plane_degenerate_cut))
