"""Every case of neighbour_edge_cases.py is what it claims to be (no GPU): the products that must be ties are ties in
exact rationals, the integers known by construction are the restatement's, another rounding or the fused form gives another
answer on them, the degenerate matrices have the zeros claimed, and every dot product that must be a zero or a NaN is one."""
from fractions import Fraction

import numpy as np

import cluster_restatement as CR
import neighbour_edge_cases as E
import normals_restatement as NR
import outlier_restatement as OR
import plane_restatement as PR

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _eig(points, radius):
    """Steps 1 to 6 of the normals rule up to the sign, from the restatement's own pieces:
    (B [n, 3, 3] f32, lam [n, 3], V [n, 3, 3], winner [n], raw unit normal [n, 3] f32); rows with mx == 0 must not be asked."""
    _, N, S, M = NR.moments(points, radius)
    A, mx = NR.scatter_matrix(N, S, M)
    assert (mx > 0).all()
    _, e = np.frexp(mx)
    B = np.ldexp(A, -e[:, None, None]).astype(F)
    lam, V = NR.jacobi(B)
    m = np.argmin(lam, axis=1)
    nv = V[np.arange(len(B)), :, m]
    nv = nv / np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])[:, None]
    assert nv.dtype == F
    return B, lam, V, m, nv


def _dot(n, w):
    with np.errstate(all="ignore"):
        d = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
    assert d.dtype == F
    return d


def _group_distance(points, groups):
    """The least distance between rows of different groups (f64)."""
    p = np.asarray(points, np.float64)
    least = np.inf
    for a in range(len(groups)):
        for b in range(a + 1, len(groups)):
            d = p[groups[a]][:, None, :] - p[groups[b]][None, :, :]
            least = min(least, np.sqrt((d * d).sum(axis=2)).min())
    return least


def test_the_exact_rounding_helpers_agree_with_numpy():
    rng = np.random.default_rng(1)
    for _ in range(300):
        a, b = rng.normal(size=3).astype(F), (rng.normal(size=3) * 10.0 ** rng.integers(-3, 3)).astype(F)
        want = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        assert E.sum3_unfused(a, b) == E.frac(want)
    x = np.asarray([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 16000.5, -16001.5, 0.25, -0.75], F)
    assert np.rint(x).tolist() == [0, 2, 2, -0, -2, -2, 16000, -16002, 0, -1]
    assert E.half_away(x).tolist() == [1, 2, 3, -1, -2, -3, 16001, -16002, 0, -1]
    assert E.half_up(x).tolist() == [1, 2, 3, 0, -1, -2, 16001, -16001, 0, -1]
    assert [E.half_even(k) for k in (0, 1, 2, 3, -1, -2, -3, -4)] == [0, 2, 2, 4, 0, -2, -2, -4]
    assert E.round_f32(Fraction(1, 3)) == E.frac(F(1) / F(3)) and E.frac(np.uint32(E.THIRD).view(F)) == E.round_f32(Fraction(1, 3))


# ---- normals -----------------------------------------------------------------------------------------------------------


def test_normals_rint_ties():
    case = E.normals_rint_ties()
    p, r, s = case["points"], F(case["radius"]), F(32768.0) / F(case["radius"])
    assert s == E.TIE_S and len(case["groups"]) == E.NORMALS_TIE_GROUPS and len(p) < 100
    seen_k = set()
    for g in case["groups"]:
        ctr = p[g["centre"]]
        for row, ks in zip(g["rows"][1:], g["ks"]):
            prod = (p[row] - ctr) * s  # as the kernel forms it
            assert prod.dtype == F and [E.frac(v) for v in prod] == [Fraction(2 * k + 1, 2) for k in ks]
            seen_k.update(ks)
    assert seen_k == set(E.TIE_KS)  # both signs, both parities, small and near 16000
    kept, N, S, M = NR.moments(p, r)
    for g in case["groups"]:
        i = g["centre"]
        assert kept[g["rows"]].all() and N[i] == g["N"] and S[i].tolist() == g["S"] and M[i].tolist() == g["M"]
    assert _group_distance(p, [g["rows"] for g in case["groups"]]) >= 4 * float(r)
    _, cell = NR.cells(p, r)
    assert (cell < 0).any(axis=0).all() and (cell > 0).any(axis=0).all()  # cells of both signs on every axis
    want = NR.estimate_normals(p, r, viewpoint=case["viewpoint"])
    assert want[3].all()
    for name, rounding in E.ALTERNATIVE_ROUNDINGS.items():
        other = NR.estimate_normals(p, r, viewpoint=case["viewpoint"], rint=rounding)
        changed = sum(1 for g in case["groups"]
                      if not np.array_equal(_bits(other[0][g["centre"]]), _bits(want[0][g["centre"]]))
                      or _bits(other[1])[g["centre"]] != _bits(want[1])[g["centre"]])
        assert 2 * changed >= len(case["groups"]), (name, changed)
        _, _, S2, M2 = NR.moments(p, r, rint=rounding)  # (the integers differ in every group)
        assert all(S2[g["centre"]].tolist() != g["S"] or M2[g["centre"]].tolist() != g["M"] for g in case["groups"]), name


DEGENERATE_NAMES = ["octahedron", "cube corners", "five identical points", "groups of 2, 3, 4 at min_neighbors 3",
                    "groups of 3, 4, 5 at min_neighbors 4", "groups of 8, 9, 10 at min_neighbors 9", "line along axis 0",
                    "line along axis 1", "line along axis 2", "line along (1, 2, 0)", "plane z = c", "plane x = y"]


def test_normals_degenerate():
    cases = E.normals_degenerate()
    assert [c["name"] for c in cases] == DEGENERATE_NAMES
    assert _group_distance(np.concatenate([c["points"] for c in cases]),
                           np.split(np.arange(sum(len(c["points"]) for c in cases)), np.cumsum([len(c["points"]) for c in cases])[:-1])
                           ) >= 4 * E.TIE_RADIUS
    for case in cases:
        p, r, m = case["points"], case["radius"], case["min_neighbors"]
        for view in case["views"]:
            normals, curvature, counts, valid = NR.estimate_normals(p, r, m, viewpoint=view["eye"])
            assert np.array_equal(counts, case["counts"]) and np.array_equal(valid, case["valid"]), case["name"]
            if view["normals"] is not None:
                assert np.array_equal(_bits(normals), _bits(view["normals"])), (case["name"], view["eye"])
            if case["curvature"] is not None:
                assert (_bits(curvature)[valid] == case["curvature"]).all(), case["name"]
            assert (_bits(normals)[~valid] == 0).all() and (_bits(curvature)[~valid] == 0).all()
        claim = case["claim"]
        if claim == "zero":
            _, N, S, M = NR.moments(p, r)
            assert (NR.scatter_matrix(N, S, M)[1] == 0).all() and (N == 5).all()
            continue
        if claim is None:
            assert sorted(set(case["counts"].tolist())) == [m - 1, m, m + 1] and 0 < case["valid"].sum() < len(p)
            continue
        B, lam, V, winner, nv = _eig(p, r)
        off = np.stack([B[:, 0, 1], B[:, 0, 2], B[:, 1, 2]], axis=1)
        diag = np.stack([B[:, 0, 0], B[:, 1, 1], B[:, 2, 2]], axis=1)
        assert (winner == case["winner"]).all(), case["name"]
        identity = np.broadcast_to(np.eye(3, dtype=F), V.shape)
        if claim == "isotropic":
            assert (off == 0).all() and (diag[:, 0] == diag[:, 1]).all() and (diag[:, 1] == diag[:, 2]).all() and (diag > 0).all()
            assert np.array_equal(V, identity) and np.array_equal(lam, diag)  # every pair skipped
        elif claim == "line":
            axis = int(np.argmax(diag[0]))
            assert (off == 0).all() and (np.delete(diag, axis, axis=1) == 0).all() and (diag[:, axis] > 0).all()
            assert np.array_equal(V, identity) and case["winner"] == min(set(range(3)) - {axis})  # the lower of the two zeros
        elif claim == "plane":
            assert (off == 0).all() and (diag[:, 2] == 0).all() and (diag[:, :2] > 0).all() and np.array_equal(V, identity)
        elif claim == "line (1, 2, 0)":
            assert (B[:, 0, 2] == 0).all() and (B[:, 1, 2] == 0).all() and (B[:, 2, 2] == 0).all() and (B[:, 0, 1] > 0).all()
            assert (_bits(lam[:, 0]) == 0).all() and (_bits(lam[:, 2]) == 0).all() and (lam[:, 1] > 0).all()  # 0 ties with 2
            assert (nv[:, 2] == 0).all() and (np.abs(nv[:, 0] / nv[:, 1] + 2) < 1e-6).all()  # across the line, in its plane
        elif claim == "plane x = y":
            assert (B[:, 0, 0] == B[:, 1, 1]).all() and (B[:, 0, 0] == B[:, 0, 1]).all() and (B[:, 0, 2] == 0).all()
            assert (B[:, 1, 2] == 0).all() and (B[:, 2, 2] > 0).all() and (_bits(lam[:, 0]) == 0).all()
            assert (_bits(nv[:, 0]) == _bits(-nv[:, 1])).all() and (_bits(nv[:, 2]) == 0).all() and (nv[:, 0] > 0.7).all()
        else:
            raise AssertionError(claim)
        # the viewpoints: where the construction says the dot product is a zero it is one, bit for bit
        zero_rows = 0
        for view in case["views"]:
            w = view["eye"][None, :] - p
            dot = _dot(nv, w)
            if view.get("dot") == "zero":
                assert (dot == 0).all()
            elif view.get("dot"):
                assert ((dot > 0) if view["dot"] == "positive" else (dot < 0)).all()
            if view["normals"] is not None:
                flipped = np.signbit(view["normals"][:, case["winner"]])
                assert np.array_equal(flipped, dot < 0) and (np.isin(_bits(dot[~flipped & ~(dot > 0)]), (0, 0x80000000))).all()
            zero_rows += int((dot == 0).sum())
            assert np.array_equal(_bits(NR.estimate_normals(p, r, m, viewpoint=view["eye"])[0]), _bits(np.where((dot < 0)[:, None], -nv, nv)))
        assert zero_rows >= (len(p) if "plane" in claim or claim == "line" else 1), case["name"]
        assert any((_dot(nv, v["eye"][None, :] - p) < 0).any() for v in case["views"]) or claim == "line (1, 2, 0)"


def test_normals_orient_cases():
    cases = E.normals_orient_cases()
    assert len(cases) == 2
    for case in cases:
        p, old = case["points"], case["old_normals"]
        assert set(case["kinds"]) == set(E.ORIENT_KINDS)
        _, _, _, _, nv = _eig(p, case["radius"])
        dot = _dot(nv, old)
        got = NR.estimate_normals(p, case["radius"], old_normals=old)
        assert got[3].all() and np.array_equal(_bits(got[0]), _bits(np.where((dot < 0)[:, None], -nv, nv)))
        if case["normals"] is not None:
            assert np.array_equal(_bits(got[0]), _bits(case["normals"]))
        along = (nv.astype(np.float64) @ case["unit"]) > 0  # the raw normal's side of `unit`, one for all rows
        assert along.all() or not along.any()
        for row, kind in enumerate(case["kinds"]):
            b = int(_bits(dot)[row])
            if kind in ("along", "against"):
                assert (dot[row] > 0) == ((kind == "along") == bool(along[0])) and dot[row] != 0
                assert ((got[0][row].astype(np.float64) @ case["unit"]) > 0) == (kind == "along")
            elif kind in ("nan", "nan in one"):
                assert np.isnan(dot[row]) and np.array_equal(_bits(got[0][row]), _bits(nv[row]))
            else:
                assert b in (0, 0x80000000) and np.array_equal(_bits(got[0][row]), _bits(nv[row])), (kind, dot[row])
        zeros = {int(_bits(dot)[row]) for row, kind in enumerate(case["kinds"]) if kind in ("perpendicular", "+0", "-0")}
        assert 0x80000000 in zeros or case["normals"] is None  # a dot product of -0 occurs (it is not < 0)


# ---- knn and cluster ---------------------------------------------------------------------------------------------------


def test_knn_rint_ties():
    cases = E.knn_rint_ties()
    assert len(cases) == 5
    s = F(32768.0) / F(E.TIE_RADIUS)
    changed = {name: 0 for name in E.ALTERNATIVE_ROUNDINGS}
    groups = 0
    for case in cases:
        p = case["points"]
        d = p[1:] - p[0]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        prod = np.sqrt(d2) * s
        assert prod.dtype == F and [E.frac(v) for v in prod] == [Fraction(L, 2) for L in case["halves"]]
        directions = {tuple(np.sign(v).astype(int)) for v in d}
        if not case["exact_rows"]:
            assert len(directions) >= 14 and sum(1 for v in d if np.count_nonzero(v) == 2) == 20  # six axes, 3-4-5 in 8+ quadrants
        for k, q in case["centre_q"].items():
            counts, qsum, stats = OR.knn_distance(p, case["radius"], k)
            assert (counts == len(p)).all() and int(qsum[0]) == q
            if case["rows_q"] is not None:
                assert qsum.tolist() == case["rows_q"][k] and stats == case["stats"][k]
            ts = sorted(L // 2 for L in case["halves"])  # the n of n + 0.5, ascending
            if k < len(ts):
                assert ts[k - 1] <= ts[k]  # the k-th place lies between two ties (or on equal ones)
            groups += 1
            for name, rounding in E.ALTERNATIVE_ROUNDINGS.items():
                changed[name] += int(OR.knn_distance(p, case["radius"], k, rint=rounding)[1][0]) != q
    assert all(2 * c >= groups for c in changed.values()), (changed, groups)
    issue = cases[3]
    assert issue["centre_q"][10] == 4318 and OR.knn_distance(issue["points"], 0.0625, 10, rint=E.half_away)[1][0] == 4323
    _, N, S, M = NR.moments(issue["points"], 0.0625)
    assert N[0] == 11 and S[0, 0] == 4318 and M[0, 0, 0] == 8400948


def test_knn_equal_kth():
    case = E.knn_equal_kth()
    p = case["points"]
    d = p - p[0]
    d2 = _bits((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    r2 = _bits(F(case["radius"]) * F(case["radius"]))
    values, counts = np.unique(d2, return_counts=True)
    assert counts.tolist() == [2, 4, 40, 1] and values[3] == r2 and values[0] == 0  # one bit pattern for the forty
    t = np.rint(np.sqrt(values.view(F)) * (F(32768.0) / F(case["radius"])))
    assert t.tolist() == [0, E.EQUAL_T_NEAR, E.EQUAL_T_SHELL, E.EQUAL_T_EDGE]
    for k, q in case["centre_q"].items():
        counts, qsum, _ = OR.knn_distance(p, case["radius"], k)
        assert counts[0] == case["centre_count"] == len(p) and int(qsum[0]) == q
    assert case["centre_q"][8] == 4 * 1536 + 3 * 3584 and case["centre_q"][32] == 4 * 1536 + 27 * 3584
    assert {8, 16, 32} <= set(case["centre_q"])  # the k-th place inside the forty at every width


def test_d2_witnesses():
    for radius in E.WITNESS_RADII:
        w = E.d2_witnesses(radius)
        r = F(radius)
        r2 = r * r
        print(f"r = {radius}: samples met by the search {dict(zip(E.KINDS, w['found']['origin']))} at the origin, "
              f"{dict(zip(E.KINDS, w['found']['in place']))} in place")
        layouts = {"origin": (w["origin"]["pairs"], np.concatenate(w["origin"]["clouds"])),
                   "in place": (w["in place"]["pairs"], w["in place"]["points"])}
        for layout, (pairs, rows) in layouts.items():
            assert all(sum(1 for pr in pairs if pr["kind"] == q) >= 8 for q in range(4)), (radius, layout)
            assert len(rows) == 3 * len(pairs) < 3000
            for i, pr in enumerate(pairs):
                p_i, p_j = rows[3 * i], rows[3 * i + 1]
                d = p_j - p_i
                assert np.array_equal(_bits(d), _bits(pr["d"]))
                unfused, fused = E.sum3_unfused(d, d), E.sum3_fused(d, d)
                assert unfused == E.frac((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])  # the rationals follow numpy
                inside, inside_fused = unfused <= E.frac(r2), fused <= E.frac(r2)
                assert inside == pr["inside"]
                if pr["kind"] == 0:
                    assert inside and not inside_fused
                elif pr["kind"] == 1:
                    assert inside_fused and not inside
                elif pr["kind"] == 2:
                    assert unfused == E.frac(r2) and any(E.round_f32(E.frac(v) ** 2) != E.frac(v) ** 2 for v in d)  # off the lattice
                else:
                    assert unfused == E.frac(np.nextafter(r2, F(np.inf)))
                if layout == "origin":
                    assert not p_i.any()
        # by construction: the counts, who has an other, the clusters
        for layout, (pairs, rows) in layouts.items():
            clouds = [rows[3 * i:3 * i + 3] for i in range(len(pairs))] if layout == "origin" else [rows]
            per_cloud = [[pr] for pr in pairs] if layout == "origin" else [pairs]
            for cloud, prs in zip(clouds, per_cloud):
                inside = np.asarray([pr["inside"] for pr in prs])
                want_counts = np.stack([2 + inside, 1 + inside, np.full(len(prs), 2)], axis=1).reshape(-1)
                counts, q1, _ = OR.knn_distance(cloud, radius, 1)
                _, q2, _ = OR.knn_distance(cloud, radius, 2)
                assert np.array_equal(counts, want_counts)
                assert np.array_equal(q1.reshape(-1, 3)[:, 1] != OR.NONE, inside) and np.array_equal(q2.reshape(-1, 3)[:, 0] != OR.NONE, inside)
                _, _, n_counts, n_valid = NR.estimate_normals(cloud, radius)  # min_neighbors 3: p_i is valid iff inside
                assert np.array_equal(n_counts, want_counts) and np.array_equal(n_valid.reshape(-1, 3)[:, 0], inside)
                assert not n_valid.reshape(-1, 3)[:, 1:].any()
                got = CR.cluster(cloud, radius, 1)
                assert len(got.sizes) == len(prs) + int((~inside).sum())
                labels = got.labels.reshape(-1, 3)
                assert np.array_equal(labels[:, 0] == labels[:, 1], inside) and (labels[:, 0] == labels[:, 2]).all()
        # the bases of the one cloud are at least 4 r apart, and no row of a pair is near a row of another pair
        rows, n_pairs = w["in place"]["points"], len(w["in place"]["pairs"])
        assert _group_distance(rows, [[3 * i] for i in range(n_pairs)]) >= 4 * float(r)
        assert _group_distance(rows, [list(range(3 * i, 3 * i + 3)) for i in range(n_pairs)]) >= 2 * float(r)


# ---- plane -------------------------------------------------------------------------------------------------------------


def test_plane_rint_ties():
    cases = E.plane_rint_ties()
    assert len(cases) == E.PLANE_TIE_GROUPS
    changed = {name: 0 for name in E.ALTERNATIVE_ROUNDINGS}
    seen = set()
    for case in cases:
        p, t = case["points"], case["t"]
        s = F(64.0) / F(t)
        assert s == E.PLANE_TIE_S
        normal, point, good = PR.candidates(p, case["triples"])
        assert good[0] and np.array_equal(_bits(normal[0]), _bits([0, 0, 1])) and np.array_equal(point[0], p[0])
        for row, ks in zip(case["tie_rows"], case["ks"]):
            prod = (p[row] - p[0]) * s
            assert prod.dtype == F and [E.frac(v) for v in prod] == [Fraction(2 * k + 1, 2) for k in ks]
            seen.update(ks)
        for refine in (0, 1):
            want = PR.segment(p, case["triples"], t, refine)
            assert want.best == 0 and want.moments[0] == case["record"] and want.counts.tolist() == [9]
            if refine == 0:
                assert np.array_equal(want.flags, case["flags"]) and want.refit_rows == 9
                plane, valid, _ = PR.plane_from_moments(case["record"], p[0], t, normal[0])
                assert valid and np.array_equal(_bits64(plane), _bits64(want.plane))
            for name, rounding in E.ALTERNATIVE_ROUNDINGS.items():
                other = PR.segment(p, case["triples"], t, refine, rint=rounding)
                if refine == 0:
                    assert other.moments[0] != case["record"]
                    changed[name] += not np.array_equal(_bits64(other.plane), _bits64(want.plane))
    assert set(E.TIE_KS) <= seen and all(2 * c >= len(cases) for c in changed.values()), changed


def test_plane_threshold_witnesses():
    w = E.plane_threshold_witnesses()
    print(f"plane threshold: samples met by the search {dict(zip(E.KINDS, w['found']))}")
    p, t = w["points"], F(w["t"])
    normal, point, good = PR.candidates(p, w["triples"])
    assert good[0] and np.array_equal(_bits(normal[0]), _bits(w["normal"])) and np.count_nonzero(normal[0]) == 3
    assert sum(1 for q in w["kinds"] if q == 0) >= 8 and sum(1 for q in w["kinds"] if q == 1) >= 8
    for row, q in enumerate(w["kinds"]):
        e = p[row] - p[0]
        unfused, fused = abs(E.sum3_unfused(normal[0], e)), abs(E.sum3_fused(normal[0], e))
        if q == 0:
            assert unfused <= E.frac(t) < fused
        elif q == 1:
            assert fused <= E.frac(t) < unfused
        else:  # far from the face: no rounding decides
            assert (unfused <= E.frac(t)) == (fused <= E.frac(t)) == bool(w["flags"][row])
            assert abs(float(unfused) - float(t)) > 0.1 * float(t)
    want = PR.segment(p, w["triples"], float(t))
    assert np.array_equal(want.flags, w["flags"]) and want.counts.tolist() == [int(w["flags"].sum())] and want.best == 0


def test_plane_degenerate_cut():
    cases = E.plane_degenerate_cut()
    assert all(sum(1 for c in cases if c["kind"] == q) >= 4 for q in range(3))
    assert len({c["name"] for c in cases}) >= 12  # the triples differ
    r64 = lambda x: E.round_f32(x, 53, -1022)
    for case in cases:
        a, b, c = ([E.frac(v) for v in row] for row in case["points"])
        u, v = [y - x for x, y in zip(a, b)], [y - x for x, y in zip(a, c)]  # exact in f64: p_a is the origin
        cross = lambda p, q, i, j: r64(r64(p[i] * q[j]) - r64(p[j] * q[i]))
        m = [cross(u, v, 1, 2), cross(u, v, 2, 0), cross(u, v, 0, 1)]
        sq = lambda w: r64(r64(r64(w[0] * w[0]) + r64(w[1] * w[1])) + r64(w[2] * w[2]))
        L, cut = sq(m), r64(r64(sq(u) * sq(v)) * Fraction(1, 1 << 20))
        got_L, got_cut = E.cut_terms(*case["points"])
        assert (L, cut) == (E.frac(got_L), E.frac(got_cut))  # the rationals follow numpy
        above, below = E.frac(np.nextafter(got_cut, np.inf)), E.frac(np.nextafter(got_cut, -np.inf))
        assert L == (cut, above, below)[case["kind"]] and case["good"] == (L > cut)
        _, _, good = PR.candidates(case["points"], case["triples"])
        want = PR.segment(case["points"], case["triples"], case["t"])
        assert bool(good[0]) == case["good"] and (want.best == 0) == case["good"] and want.counts.tolist() == [3 if case["good"] else 0]
