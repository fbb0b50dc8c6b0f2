"""Clustering of resident clouds (a3d_point_clouds_cluster_device) without a GPU: the C ABI (exported symbol, the header,
the ctypes mirror, the Rust bindings, every refusal that is decided on the host, with made-up device addresses: nothing is
dereferenced), and the numpy restatement (cluster_restatement.py, the expected value of the GPU tests) against
connected components, against a textbook sequential DBSCAN, against clouds whose clusters are known by construction and
against what the feature is for; and the clouds of test_gpu_cluster_contention.py (cluster_cases.py) against the clusters
they have by construction, with the restatement's hooking components, which are shown equal to the quick-find's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import cluster_restatement as R
import outlier_restatement as OR
from align3d_amd import DevicePointCloud, PointCloud, _abi
from cluster_cases import (CLUMP, COMB_TEETH, COMB_TOOTH, N_CLUMPS, NOISE_SET, R_CONTENTION, SHEET_SIDE, border_ties, bridge,
                           chain, chain_sets, comb, exact_chain, floaters_cloud, interleaved_lines, labels_of_sets,
                           lattice_sheet, pairs_far_apart, pairs_far_apart_expected, raw_bits)
from outlier_cases import N_OUTLIERS, RADIUS, effectiveness_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER = "a3d_point_clouds_cluster_device"
SENTINEL = 0x7777
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


# ---- the ABI, without a device -----------------------------------------------------------------------------------------


def test_symbol_is_exported_declared_mirrored_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    assert hasattr(lib, CLUSTER) and hasattr(diag, CLUSTER)
    assert re.search(r"a3d_status\s+%s\s*\(" % CLUSTER, header) and CLUSTER in section
    assert section.index("a3d_knn_distance_threshold(") < section.index(CLUSTER + "(")  # after the outlier entries
    assert CLUSTER in _abi.SIGNATURES and len(_abi.SIGNATURES[CLUSTER][1]) == 12
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys

    text = open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    assert text == gen_rust_sys.generate() and "pub fn %s(" % CLUSTER in text
    for method in ("cluster", "cluster_many", "remove_small_clusters", "remove_small_clusters_many", "largest_cluster"):
        assert callable(getattr(DevicePointCloud, method))


def test_the_rule_stands_verbatim_in_the_kernel_file_and_the_restatement():
    def rule(text, strip):
        lines = [ln.strip().lstrip(strip).strip() for ln in text.splitlines()]
        joined = " ".join(" ".join(lines).split())
        return joined[joined.index("The rule of the cluster call."):joined.index("the same on every run.")]

    hip = open(os.path.join(ROOT, "align3d_amd", "csrc", "cloud_outliers.hip")).read()
    assert rule(hip, "/") == rule(R.__doc__, "")
    assert "6. Labels." in rule(hip, "/") and "bits(d2) << 32 | j" in rule(hip, "/")


def test_product_library_has_no_knob_for_the_feature():
    assert b"A3D_CLUSTER" not in open(_abi.LIB_PATH, "rb").read()
    diag = open(_abi.DIAG_LIB_PATH, "rb").read()
    assert b"A3D_CLUSTER_LINK" in diag and b"A3D_CLUSTER_HALVING" in diag


OUTPUTS = ("labels", "row_sizes", "sizes", "roots")


class _Args:
    """Two clouds of 4 rows at made-up, disjoint device addresses (cloud 0 with normals), a made-up context and
    sentinel-filled host outputs: the checks under test fail before anything is dereferenced."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, None, 4
        self.ctx = C.c_void_p(0x900000)
        self.labels = (C.c_void_p * 2)(0x40000, 0x41000)
        self.row_sizes = (C.c_void_p * 2)(0x50000, None)
        self.sizes = (C.c_void_p * 2)(0x60000, 0x61000)
        self.roots = (C.c_void_p * 2)(None, 0x71000)
        self.clusters = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.noise = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.dropped = (C.c_uint64 * 2)(SENTINEL, SENTINEL)

    def call(self, lib, **override):
        a = dict(ctx=self.ctx, views=self.views, n=2, radius=0.05, m=3, labels=self.labels, row_sizes=self.row_sizes,
                 sizes=self.sizes, roots=self.roots, clusters=self.clusters, noise=self.noise, dropped=self.dropped)
        a.update(override)
        return getattr(lib, CLUSTER)(a["ctx"], a["views"], a["n"], a["radius"], a["m"], a["labels"], a["row_sizes"],
                                     a["sizes"], a["roots"], a["clusters"], a["noise"], a["dropped"])

    def untouched(self):
        return all(list(w) == [SENTINEL] * 2 for w in (self.clusters, self.noise, self.dropped))


def test_empty_batch_is_ok_and_nulls_are_invalid(lib):
    assert getattr(lib, CLUSTER)(None, None, 0, 0.0, 0, None, None, None, None, None, None, None) == _abi.A3D_OK
    a = _Args()
    assert a.call(lib, n=0, radius=float("nan")) == _abi.A3D_OK and a.untouched()
    for name in ("ctx", "views", "labels"):
        a = _Args()
        assert a.call(lib, **{name: None}) == _abi.A3D_INVALID_PARAMETER, name
        assert a.untouched(), name
    a = _Args()
    a.labels[1] = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    a = _Args()
    a.views[1].points = None
    assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()


@pytest.mark.parametrize("radius", [0.0, -0.0, -0.05, float("nan"), float("inf"), float("-inf"), 1e-30])
def test_bad_radius_is_invalid(lib, radius):
    for m in (1, 8):
        a = _Args()
        assert a.call(lib, radius=radius, m=m) == _abi.A3D_INVALID_PARAMETER
        assert a.untouched()


def test_min_points_zero_and_huge_clouds_are_invalid(lib):
    a = _Args()
    assert a.call(lib, m=0) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    for big in (1 << 32, 1 << 40, (1 << 32) - 1, (1 << 32) - 1000):
        for i in (0, 1):
            a = _Args()
            a.views[i].len = big
            assert a.call(lib) == _abi.A3D_INVALID_PARAMETER and a.untouched()


def test_every_overlap_is_invalid(lib):
    """4 rows = 48 bytes of points or normals, 16 of each output.  Every output on the points, on the normals' last byte,
    and on every other output's last word."""
    bases = {"labels": (0x40000, 0x41000), "row_sizes": (0x50000, None), "sizes": (0x60000, 0x61000), "roots": (None, 0x71000)}
    cases = []
    for field in OUTPUTS:
        i = 0 if bases[field][0] else 1
        cases += [(field, i, 0x10000), (field, i, 0x10000 + 47), (field, i, 0x30000 + 44), (field, i, 0x20000 + 47),
                  (field, i, 0x20000 - 15)]
        for other in OUTPUTS:
            for k in (0, 1):
                if bases[other][k] and (other, k) != (field, i):
                    cases += [(field, i, bases[other][k] + 15), (field, i, bases[other][k] - 15)]
    assert len(cases) > 50
    for field, i, address in cases:
        a = _Args()
        getattr(a, field)[i] = address
        assert a.call(lib) == _abi.A3D_INVALID_PARAMETER, (field, i, hex(address))
        assert a.untouched()


def test_python_wrappers_refuse_host_clouds_and_an_empty_list_is_empty():
    assert DevicePointCloud.cluster_many([], 0.05) == ([], [], [])
    assert DevicePointCloud.remove_small_clusters_many([], 0.05, 1, 10) == []
    assert DevicePointCloud.remove_small_clusters_many([], 0.05, 1, 10, return_index=True) == ([], [])
    host = PointCloud([[1.0, 2.0, 3.0]])
    with pytest.raises(TypeError):
        DevicePointCloud.cluster_many([host], 0.05)
    with pytest.raises(TypeError):
        DevicePointCloud.remove_small_clusters_many([host], 0.05, 1, 1)
    with pytest.raises(_abi.InvalidParameter):
        DevicePointCloud.remove_small_clusters_many([host], 0.05, 1, 0)  # min_size >= 1, decided before the clouds are looked at
    assert not hasattr(PointCloud, "cluster")


# ---- the restatement ---------------------------------------------------------------------------------------------------


def _partition(labels, rows):
    """The partition of `rows` that the labels induce, as a sorted list of sorted tuples."""
    groups = {}
    for r in rows:
        groups.setdefault(int(labels[r]), []).append(int(r))
    return sorted(tuple(g) for g in groups.values())


def test_effectiveness_cloud_clusters_and_connected_components():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    points, outlier = effectiveness_cloud()
    n = len(points)
    pairs = R.pairs_brute(points, RADIUS)
    c = R.cluster_pairs(pairs, 1)
    assert sorted(c.sizes.tolist(), reverse=True) == [1000, 500] + [1] * N_OUTLIERS
    assert not c.noise.any() and not c.border.any() and c.core.all()
    graph = coo_matrix((np.ones(len(pairs.i)), (pairs.i, pairs.j)), shape=(n, n))
    count, comp = connected_components(graph, directed=False)
    assert count == 32 and _partition(comp, range(n)) == _partition(c.labels, range(n))
    assert (np.diff(c.roots.astype(np.int64)) > 0).all()
    assert np.array_equal(c.roots, [np.flatnonzero(c.labels == k)[0] for k in range(32)])  # the root is the lowest row
    assert np.array_equal(c.counts, OR.knn_distance(points, RADIUS, 0)[0])  # rule 2: that entry's counts
    c = R.cluster_pairs(pairs, 5)
    assert sorted(c.sizes.tolist()) == [500, 1000] and np.array_equal(c.noise, outlier) and not c.border.any()
    c = R.cluster(points, 0.05, 8)
    print(f"r = 0.05, m = 8: {len(c.sizes)} clusters, {c.noise.sum()} noise rows, {c.border.sum()} border rows")
    assert len(c.sizes) == 14 and c.noise.sum() == 625 and c.border.sum() == 277
    assert c.noise.sum() >= 100 and c.border.sum() >= 100
    assert np.array_equal(c.row_sizes[~c.noise], c.sizes[c.labels[~c.noise]]) and (c.row_sizes[c.noise] == 0).all()
    assert c.sizes.sum() == n - c.noise.sum() and (c.labels[c.noise] == NONE).all()


def _textbook_dbscan(points, radius, m):
    """DBSCAN as published (Ester, Kriegel, Sander, Xu 1996; the form of the 2017 revisit): rows in order, a queue per
    cluster, a border row goes to the first cluster that reaches it.  Neighbours are rule 1's, from a list of sets.
    Returns (labels with -1 for noise, neighbour sets)."""
    pairs = R.pairs_brute(points, radius)
    n = len(points)
    nbrs = [[] for _ in range(n)]
    for i, j in zip(pairs.i.tolist(), pairs.j.tolist()):
        nbrs[i].append(j)
    UNSEEN, NOISE = -2, -1
    labels = [UNSEEN] * n
    c = -1
    for p in range(n):
        if labels[p] != UNSEEN:
            continue
        if len(nbrs[p]) < m:
            labels[p] = NOISE
            continue
        c += 1
        labels[p] = c
        queue = [q for q in nbrs[p] if q != p]
        while queue:
            q = queue.pop(0)
            if labels[q] == NOISE:
                labels[q] = c  # a border row
            if labels[q] != UNSEEN:
                continue
            labels[q] = c
            if len(nbrs[q]) >= m:
                queue.extend(nbrs[q])
    return np.array(labels), nbrs


@pytest.mark.parametrize("radius,m", [(0.05, 8), (0.08, 12), (RADIUS, 5), (RADIUS, 1)])
def test_restatement_against_a_textbook_sequential_dbscan(radius, m):
    points, _ = effectiveness_cloud()
    points = np.r_[points, raw_bits(3, 20)]
    book, nbrs = _textbook_dbscan(points, radius, m)
    c = R.cluster(points, radius, m)
    assert c.dropped > 5
    core = np.flatnonzero(c.core)
    assert np.array_equal(c.labels[core], book[core].astype(np.uint32))  # both number clusters by their lowest core row
    assert np.array_equal(c.noise, book == -1)
    for b in np.flatnonzero(c.border):
        assert int(c.labels[b]) in {int(c.labels[q]) for q in nbrs[b] if c.core[q]}
    moved = sum(int(c.labels[b]) != book[b] for b in np.flatnonzero(c.border))
    print(f"r = {radius}, m = {m}: {c.border.sum()} border rows, {moved} of them in another cluster than first-come puts them")


def test_floaters_the_radius_filter_keeps_them_and_the_cluster_filter_removes_them():
    points, outlier, clump = floaters_cloud()
    assert len(points) == 1530 + N_CLUMPS * CLUMP and clump.sum() == N_CLUMPS * CLUMP
    kept = OR.remove_radius_outliers(points, RADIUS, 2)
    assert set(np.flatnonzero(clump)) <= set(kept.tolist())  # every clump row has four neighbours
    assert not outlier[kept].any()
    kept = R.remove_small_clusters(points, RADIUS, 1, 10)
    assert np.array_equal(kept, np.flatnonzero(~outlier & ~clump)) and len(kept) == 1500
    big = R.largest_cluster(points, RADIUS, 1)
    assert len(big) == 1000 and not (outlier | clump)[big].any()
    assert len(R.remove_small_clusters(points, RADIUS, 1, 1, 5)) == N_OUTLIERS + N_CLUMPS * CLUMP  # max_size


def test_bridge_border_ties_chains_and_pairs_by_construction():
    points, row, m = bridge()
    c = R.cluster(points, 0.05, m)
    assert len(c.sizes) == 2 and c.border[row] and c.border.sum() == 1 and not c.noise.any() and c.counts[row] == 3
    assert sorted(c.sizes.tolist()) == [41, 42]
    assert len(R.cluster(points, 0.05, 3).sizes) == 1  # the midway row as a core row links the two
    points, radius, m, want = border_ties()
    c = R.cluster(points, radius, m)
    assert np.array_equal(c.labels, want) and c.border.tolist() == [False] * 10 + [True, True]
    assert np.array_equal(c.sizes, [6, 6]) and np.array_equal(c.roots, [0, 5])
    for order in ("ascending", "descending", "shuffled"):
        assert R.cluster(chain(65, order), 0.05, 1).sizes.tolist() == [65]
        assert sorted(R.cluster(chain(65, order, stretch=(30, 1.001)), 0.05, 1).sizes.tolist()) == [31, 34]
        c = R.cluster(chain(65, order), 0.05, 3)
        assert c.sizes.tolist() == [65] and c.border.sum() == 2  # the two ends
    assert R.cluster(exact_chain(10, 4), 0.25, 1).labels.tolist() == [0] * 5 + [1] * 5  # <= at exactly r; just above r
    for n in (3001, 3000):
        points, _ = pairs_far_apart(n)
        for m in (1, 2, 3):
            c = R.cluster(points, 0.02, m, by_cell=True)
            labels, sizes, roots = pairs_far_apart_expected(n, m)
            assert np.array_equal(c.labels, labels) and np.array_equal(c.sizes, sizes) and np.array_equal(c.roots, roots)


def test_brute_force_and_cell_sorted_enumeration_agree():
    rng = np.random.default_rng(11)
    points = np.r_[rng.uniform(-0.4, 0.4, size=(1500, 3)).astype(np.float32), raw_bits(12, 80),
                   (rng.integers(-3, 3, size=(300, 3)) * np.float32(0.0625)).astype(np.float32)][rng.permutation(1880)]
    for radius in (0.0625, 0.11):
        a, b = R.pairs_brute(points, radius), R.pairs_by_cell(points, radius)
        assert np.array_equal(a.kept, b.kept) and (~a.kept).sum() > 30
        for x, y in zip(R.sorted_pairs(a), R.sorted_pairs(b)):
            assert np.array_equal(x, y)
        assert len(a.i) > 5000
        for m in (1, 6):
            for x, y in zip(R.cluster_pairs(a, m), R.cluster_pairs(b, m)):
                assert np.array_equal(x, y)


def test_a_row_permutation_keeps_the_core_partition_the_noise_and_the_sizes():
    """A cloud with border rows.  Rule 4 depends on the row order only where two core rows of different clusters are at
    bit-equal d2 from one border row; this seeded cloud has no such row (the multiset of sizes would show it)."""
    points, _ = effectiveness_cloud()
    c = R.cluster(points, 0.05, 8)
    perm = np.random.default_rng(21).permutation(len(points))
    moved = R.cluster(points[perm], 0.05, 8)
    assert c.border.sum() >= 100
    assert np.array_equal(moved.core, c.core[perm]) and np.array_equal(moved.noise, c.noise[perm])
    core = np.flatnonzero(c.core[perm])
    assert _partition(moved.labels, core) == sorted(tuple(sorted(int(np.flatnonzero(perm == r)[0]) for r in g))
                                                    for g in _partition(c.labels, np.flatnonzero(c.core)))
    assert sorted(moved.sizes.tolist()) == sorted(c.sizes.tolist())


# ---- the clouds of test_gpu_cluster_contention.py, and the components routine that scales to them ------------------------


def _same_clusters(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_hooking_components_give_the_quick_finds_clusters_on_every_cloud_of_this_file():
    base, _ = effectiveness_cloud()
    rng = np.random.default_rng(11)
    mixed = np.r_[rng.uniform(-0.4, 0.4, size=(1500, 3)).astype(np.float32), raw_bits(12, 80),
                  (rng.integers(-3, 3, size=(300, 3)) * np.float32(0.0625)).astype(np.float32)][rng.permutation(1880)]
    cases = [(base, RADIUS, (1, 5)), (base, 0.05, (8,)), (np.r_[base, raw_bits(3, 20)], 0.05, (8,)),
             (np.r_[base, raw_bits(3, 20)], 0.08, (12,)), (np.r_[base, raw_bits(3, 20)], RADIUS, (5, 1)),
             (floaters_cloud()[0], RADIUS, (1,)), (bridge()[0], 0.05, (10, 3)), (border_ties()[0], 1.0, (5,)),
             (exact_chain(10, 4), 0.25, (1,)), (mixed, 0.0625, (1, 6)), (mixed, 0.11, (1, 6)),
             (base[np.random.default_rng(21).permutation(len(base))], 0.05, (8,))]
    for order in ("ascending", "descending", "shuffled"):
        cases += [(chain(65, order), 0.05, (1, 3)), (chain(65, order, stretch=(30, 1.001)), 0.05, (1,))]
    cases += [(pairs_far_apart(n)[0], 0.02, (1, 2, 3)) for n in (3001, 3000)]
    unions = 0
    for points, radius, ms in cases:
        pairs = R.pairs_by_cell(points, radius)
        for m in ms:
            quick, hooked = R.cluster_pairs(pairs, m), R.cluster_pairs(pairs, m, components="hooking")
            assert _same_clusters(quick, hooked), (len(points), radius, m)
            unions += int(quick.core.sum()) - len(quick.sizes)
    assert unions > 10000
    c = R.cluster(base, 0.05, 8, by_cell=True, components="hooking")  # the keyword of cluster()
    assert _same_clusters(c, R.cluster(base, 0.05, 8)) and len(c.sizes) == 14
    with pytest.raises(KeyError):
        R.cluster(base, 0.05, 8, components="none")


def _contention(points, m):
    return R.cluster(points, R_CONTENTION, m, by_cell=True, components="hooking")


def _is_construction(c, labels, sizes, roots):
    return np.array_equal(c.labels, labels) and np.array_equal(c.sizes, sizes) and np.array_equal(c.roots, roots)


def test_labels_of_sets_numbers_the_sets_by_their_lowest_core_row():
    labels, sizes, roots = labels_of_sets([2, 0, NOISE_SET, 2, 0, 1, 1], core=[0, 1, 0, 1, 1, 0, 1])
    assert labels.tolist() == [1, 0, NONE, 1, 0, 2, 2] and sizes.tolist() == [2, 2, 2] and roots.tolist() == [1, 3, 6]
    labels, sizes, roots = labels_of_sets(np.full(3, NOISE_SET))
    assert labels.tolist() == [NONE] * 3 and len(sizes) == len(roots) == 0


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_long_chains_are_one_cluster_and_two_at_a_stretched_link(order):
    n = 70001
    c = _contention(chain(n, order), 1)
    assert c.sizes.tolist() == [n] and c.roots.tolist() == [0] and c.counts.max() == 3 and not c.labels.any()
    k = n // 3
    c = _contention(chain(n, order, stretch=(k, 1.001)), 1)
    sets = chain_sets(n, order, k)
    assert _is_construction(c, *labels_of_sets(sets)) and sorted(c.sizes.tolist()) == [k + 1, n - k - 1]
    if order != "shuffled":  # row 0 is the chain's first point, or its last
        assert c.roots.tolist() == ([0, k + 1] if order == "ascending" else [0, n - k - 1])


@pytest.mark.parametrize("K", (2, 3, 64, 65, 1000))
def test_interleaved_lines_are_one_cluster_a_line(K):
    n = 20007
    for descending in (False, True):
        points, line, ends = interleaved_lines(n, K, descending)
        assert np.array_equal(line, np.arange(n) % K) and ends.sum() == 2 * K
        lengths = np.bincount(line)
        c = _contention(points, 1)
        assert np.array_equal(c.labels, line) and np.array_equal(c.roots, np.arange(K)) and np.array_equal(c.sizes, lengths)
        assert c.counts.max() == 3 and np.array_equal(c.counts == 2, ends)
        # min_points = 3: the two ends of a line are border rows of that line; the root is the lowest row that is no end
        c = _contention(points, 3)
        assert np.array_equal(c.labels, line) and np.array_equal(c.sizes, lengths) and np.array_equal(c.border, ends)
        assert _is_construction(c, *labels_of_sets(line, ~ends)) and np.array_equal(c.roots, np.arange(K) + K)
        c = _contention(points, 4)
        assert c.noise.all() and len(c.sizes) == 0 and _is_construction(c, *labels_of_sets(np.full(n, NOISE_SET)))


@pytest.mark.parametrize("side", (150, SHEET_SIDE))
def test_lattice_sheet_counts_five_four_and_three(side):
    points, kind = lattice_sheet(side)
    n = side * side
    assert (kind == 2).sum() == 4 and (kind == 3).sum() == 4 * (side - 2)
    c = _contention(points, 1)
    assert np.array_equal(c.counts, kind + 1) and c.sizes.tolist() == [n] and c.roots.tolist() == [0]
    c = _contention(points, 5)
    assert c.sizes.tolist() == [n - 4] and c.noise.sum() == 4 and c.border.sum() == 4 * (side - 2)
    assert np.array_equal(c.noise, kind == 2) and np.array_equal(c.border, kind == 3)
    assert c.roots.tolist() == [int(np.flatnonzero(kind == 4)[0])]  # the lowest interior row
    assert _is_construction(c, *labels_of_sets(np.where(kind == 2, NOISE_SET, 0), kind == 4))
    if side == 150:
        assert c.sizes.tolist() == [22496] and c.border.sum() == 592
    pairs = R.pairs_by_cell(points, R_CONTENTION)  # a border row has exactly one core neighbour
    core_neighbours = np.bincount(pairs.i[c.core[pairs.j]], minlength=n)
    assert (core_neighbours[c.border] == 1).all()
    assert _contention(points, 6).noise.all()


@pytest.mark.parametrize("shuffled", (False, True))
def test_comb_is_one_cluster_and_two_without_one_spine_point(shuffled):
    points, sets = comb(None, shuffled)
    assert len(points) == COMB_TEETH * COMB_TOOTH + 2 * COMB_TEETH - 1
    c = _contention(points, 1)
    assert c.sizes.tolist() == [len(points)] and c.roots.tolist() == [0] and c.counts.max() == 4
    cut = 40
    points, sets = comb(cut, shuffled)
    c = _contention(points, 1)
    assert _is_construction(c, *labels_of_sets(sets)) and len(c.sizes) == 2
    assert sorted(c.sizes.tolist()) == sorted([(cut + 1) * COMB_TOOTH + 2 * cut + 1,
                                               (COMB_TEETH - cut - 1) * COMB_TOOTH + 2 * (COMB_TEETH - cut - 1) - 1])
    if not shuffled:
        assert c.roots.tolist() == [0, (cut + 1) * COMB_TOOTH]


def test_hooking_partition_is_scipys_connected_components_on_the_sheet_and_the_comb():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    for points, m in ((lattice_sheet(SHEET_SIDE)[0], 5), (comb(40, True)[0], 1), (comb(None, True)[0], 1)):
        n = len(points)
        pairs = R.pairs_by_cell(points, R_CONTENTION)
        c = R.cluster_pairs(pairs, m, components="hooking")
        link = c.core[pairs.i] & c.core[pairs.j]
        graph = coo_matrix((np.ones(int(link.sum())), (pairs.i[link], pairs.j[link])), shape=(n, n))
        count, comp = connected_components(graph, directed=False)
        core = np.flatnonzero(c.core)
        assert count - (n - len(core)) == len(c.sizes)  # a row that is not core is a component of its own in the graph
        both = np.unique(np.stack([comp[core], c.labels[core].astype(np.int64)], axis=1), axis=0)  # a bijection
        assert len(both) == len(np.unique(both[:, 0])) == len(np.unique(both[:, 1])) == len(c.sizes)
