"""The lock-free union-find of the cluster call (cluster_union, cluster_find and the flatten pass's run carry in
align3d_amd/csrc/cloud_outliers.hip) under contention, on the GPU: clouds of more than 64 tiles whose clusters are ONE
big tree each, built by CAS hooks that collide across every tile.

The clouds are cluster_cases.py's: chains of 70 001 rows (a union tree as deep as the cloud before halving), lines
interleaved row by row (K roots alternating in every wave of the flatten pass, every root in the first tile), a lattice
sheet (a two-dimensional component with border rows all round it) and a comb (66 trees of one tile each, joined late from
the highest rows).  Their labels, sizes and roots are known by construction (labels_of_sets), and test_cluster_cpu.py
shows without a GPU that the restatement agrees with every one of them.  A band of 70 000 rows of a recorded frame is
compared with the full restatement, whose components come from its hooking routine.

Every comparison is np.array_equal on uint32; every call must return A3D_OK (a fault word that a union-find bound sets
makes it A3D_HIP_ERROR).  The forms of the diagnostics build are not run here: without halving a chain of 70 001 rows is
quadratic.  Every test prints its wall time."""
import time

import numpy as np
import pytest

import cluster_restatement as R
from align3d_amd import _abi
from cluster_cases import (COMB_TEETH, COMB_TOOTH, NOISE_SET, R_CONTENTION, SHEET_SIDE, chain, chain_sets, comb,
                           interleaved_lines, labels_of_sets, lattice_sheet)
from test_gpu_cloud_normals import _sample1_frames
from test_gpu_cluster import OUTPUTS, _assert_construction, _assert_equal, _cluster, _device_cloud

pytestmark = pytest.mark.gpu

BAND_ROWS, BAND_RADIUS = 70000, 0.01
BAND_M2 = 12  # chosen on the restatement of the band: see test_a_band_of_a_recorded_frame_against_the_full_restatement


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"[wall time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


def _run(ctx, cloud, m, label, radius=R_CONTENTION):
    t0 = time.perf_counter()
    st, outs = _cluster(ctx, [cloud], radius, m)
    print(f"[cluster call and read-back] {label}, {cloud.len()} rows, min_points {m}: {time.perf_counter() - t0:.3f} s")
    assert st == _abi.A3D_OK, (label, m, st)
    assert radius != R_CONTENTION or outs[0]["dropped"] == 0  # the constructions have no row to drop
    return outs[0]


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_chain_of_seventy_thousand_rows_is_one_cluster(ctx, order):
    n = 70001
    cloud = _device_cloud(ctx, chain(n, order))
    _assert_construction(_run(ctx, cloud, 1, f"chain {order}"), np.zeros(n, np.uint32), [n], [0])
    cloud.free()


def test_shuffled_chain_with_one_link_stretched_is_two_clusters(ctx):
    n = 70001
    k = n // 3
    cloud = _device_cloud(ctx, chain(n, "shuffled", stretch=(k, 1.001)))
    labels, sizes, roots = labels_of_sets(chain_sets(n, "shuffled", k))
    assert sorted(sizes.tolist()) == [k + 1, n - k - 1]
    _assert_construction(_run(ctx, cloud, 1, "chain shuffled, stretched"), labels, sizes, roots)
    cloud.free()


@pytest.mark.parametrize("K,descending", [(2, False), (3, False), (64, False), (65, False), (1000, False), (65, True)])
def test_interleaved_lines(ctx, K, descending):
    n = 20007
    points, line, ends = interleaved_lines(n, K, descending)
    cloud = _device_cloud(ctx, points)
    label = f"lines K = {K}" + (" descending" if descending else "")
    labels, sizes, roots = labels_of_sets(line)
    assert np.array_equal(labels, np.arange(n) % K) and np.array_equal(roots, np.arange(K))
    _assert_construction(_run(ctx, cloud, 1, label), labels, sizes, roots)
    # min_points = 3: the two ends of a line have 2 neighbours and are border rows of that line (its only core rows within
    # reach), so the labels and sizes stay; the root is the line's lowest CORE row, its second row
    labels3, sizes3, roots3 = labels_of_sets(line, ~ends)
    assert np.array_equal(labels3, labels) and np.array_equal(sizes3, sizes) and np.array_equal(roots3, np.arange(K) + K)
    _assert_construction(_run(ctx, cloud, 3, label), labels3, sizes3, roots3)
    _assert_construction(_run(ctx, cloud, 4, label), *labels_of_sets(np.full(n, NOISE_SET)))
    cloud.free()


def test_lattice_sheet(ctx):
    side = SHEET_SIDE
    points, kind = lattice_sheet(side)
    n = side * side
    cloud = _device_cloud(ctx, points)
    _assert_construction(_run(ctx, cloud, 1, "sheet"), np.zeros(n, np.uint32), [n], [0])
    labels, sizes, roots = labels_of_sets(np.where(kind == 2, NOISE_SET, 0), kind == 4)
    assert sizes.tolist() == [n - 4] and roots.tolist() == [int(np.flatnonzero(kind == 4)[0])]
    out = _run(ctx, cloud, 5, "sheet")
    _assert_construction(out, labels, sizes, roots)
    assert out["noise"] == 4
    _assert_construction(_run(ctx, cloud, 6, "sheet"), *labels_of_sets(np.full(n, NOISE_SET)))
    cloud.free()


@pytest.mark.parametrize("shuffled", (False, True), ids=("in row order", "shuffled"))
@pytest.mark.parametrize("cut", (None, 40), ids=("uncut", "cut"))
def test_comb(ctx, cut, shuffled):
    points, sets = comb(cut, shuffled)
    labels, sizes, roots = labels_of_sets(sets)
    if not shuffled:
        assert roots.tolist() == ([0] if cut is None else [0, (cut + 1) * COMB_TOOTH])
    assert len(points) == COMB_TEETH * COMB_TOOTH + 2 * COMB_TEETH - 1 - (cut is not None)
    cloud = _device_cloud(ctx, points)
    first = _run(ctx, cloud, 1, f"comb cut {cut} shuffled {shuffled}")
    _assert_construction(first, labels, sizes, roots)
    if shuffled:  # a second run: identical words
        second = _run(ctx, cloud, 1, f"comb cut {cut} shuffled {shuffled}, again")
        for f in OUTPUTS + ("clusters", "noise", "dropped"):
            assert np.array_equal(first[f], second[f]), f
    cloud.free()


def test_a_band_of_a_recorded_frame_against_the_full_restatement(ctx):
    """The first 70 000 rows of frame 0 of sample1 at r = 0.01.  BAND_M2 was chosen on the restatement so that the band
    has at least 10 clusters, 100 border rows and 100 noise rows."""
    frame = _sample1_frames(ctx)[0]
    assert frame.len() > BAND_ROWS
    points = np.ascontiguousarray(frame.download()[0][:BAND_ROWS])
    cloud = _device_cloud(ctx, points)
    t0 = time.perf_counter()
    pairs = R.pairs_by_cell(points, BAND_RADIUS)
    print(f"[restatement] {len(pairs.i)} pairs of {BAND_ROWS} rows: {time.perf_counter() - t0:.2f} s")
    for m in (1, BAND_M2):
        t0 = time.perf_counter()
        want = R.cluster_pairs(pairs, m, components="hooking")
        print(f"[restatement] min_points {m}: {len(want.sizes)} clusters, {int(want.border.sum())} border rows, "
              f"{int(want.noise.sum())} noise rows, the largest of {int(want.sizes.max())} rows: {time.perf_counter() - t0:.2f} s")
        if m == BAND_M2:
            assert len(want.sizes) >= 10 and want.border.sum() >= 100 and want.noise.sum() >= 100
        _assert_equal(_run(ctx, cloud, m, "band", BAND_RADIUS), want)
    cloud.free()
