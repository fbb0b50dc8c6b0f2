"""What test_gpu_scene_batch_many_jobs.py feeds the four scene entries (knn_distance, select, cluster, segment_plane) over
batches of 65, 129 and 1000 clouds, and the conditions those inputs have to meet, checked without a GPU.

The clouds are the recipe of test_cloud_batch_recipe_cpu.py; this file adds what the four entries take per cloud (the
values and bounds of the select, its colours, the number of plane candidates) as functions of the cloud index alone, and
restates the host's choice of the plane score's launch geometry.  The tests below are conditions on those inputs: they say
that the batches reach the paths the GPU tests are there for (jobs past index 63 that drop rows and keep rows, border rows
and roots beyond a cloud's first tile, more than one block of candidates per job, a split score grid)."""
import numpy as np

import cluster_restatement as CR
import outlier_restatement as OR
import plane_restatement as PR
from test_cloud_batch_recipe_cpu import BATCHES, BIG_AT, SEED, TILE_VOXEL, VOXEL, batch_lengths, is_raw, plan, recipe

RADIUS = VOXEL
KNN_KS = (0, 17)
MIN_POINTS = (1, 4)
PLANE_T = 0.02
PLANE_HS = (0, 1, 3, 64, 130, 257, 700)
PLANE_THREADS = 256  # candidates of a block of the candidates kernel
TILE_SCENE = TILE_VOXEL  # rows of a tile of all four entries


def select_values(i, n):
    """[n] u32 in 0 .. 3 for cloud i."""
    return np.random.default_rng([SEED + 2, i]).integers(0, 4, n).astype(np.uint32)


def select_bounds(i):
    """(lo, hi) of cloud i: 1 .. 2 or 2 .. 3."""
    return 1 + i % 2, 2 + i % 2


def has_colors(i):
    """Every second cloud has colours, and an index output."""
    return i % 2 == 1


def select_colors(i, n):
    return np.random.default_rng([SEED + 3, i]).integers(0, 256, size=(n, 3)).astype(np.uint8)


def plane_h(i, n):
    """The number of candidates of cloud i with n rows: the cycle of PLANE_HS by cloud index, entered at its end so that
    the clouds BIG_AT get 700; no candidate for a cloud of fewer than 3 rows."""
    return PLANE_HS[(i + len(PLANE_HS) - 1) % len(PLANE_HS)] if n >= 3 else 0


def plane_triples(i, n):
    return PR.hypotheses(i, n, plane_h(i, n))


def plane_geometry(lengths, hs):
    """(per, split) of a segment_plane call, restating the host: `per` blocks of PLANE_THREADS candidates per job for the
    largest H of the call; the score grid's second dimension doubles while it is below 8, the grid is below 2048 blocks and
    every split still has at least 64 of the largest H."""
    tiles = sum(count for _, _, count, _ in plan(lengths, TILE_SCENE, 4096))
    cand_max = max(hs) if len(hs) else 0
    split = 1
    while split < 8 and tiles * split < 2048 and cand_max // (2 * split) >= 64:
        split *= 2
    return (cand_max + PLANE_THREADS - 1) // PLANE_THREADS, split


def kept_rows(i, points):
    return OR.select(select_values(i, len(points)), *select_bounds(i))


def test_the_per_cloud_inputs_depend_on_the_cloud_index_alone():
    assert np.array_equal(select_values(5, 64), select_values(5, 64)) and set(select_values(5, 4097).tolist()) == {0, 1, 2, 3}
    assert not np.array_equal(select_values(5, 64), select_values(6, 64))
    assert [select_bounds(i) for i in (0, 1, 70, 999)] == [(1, 2), (2, 3), (1, 2), (2, 3)]
    assert select_colors(3, 10).shape == (10, 3) and select_colors(3, 10).dtype == np.uint8
    assert [plane_h(i, 100) for i in range(8)] == [700, 0, 1, 3, 64, 130, 257, 700] and plane_h(6, 2) == 0 and plane_h(6, 3) == 257
    assert all(plane_h(i, 70001) == 700 for i in BIG_AT)  # the two clouds of 69 tiles are scored against the most candidates
    tr = plane_triples(70, 70001)
    assert tr.shape == (700, 3) and tr.max() < 70001 and tr.max() > 60000


def test_late_jobs_drop_rows_keep_rows_and_overflow_where_the_gpu_test_cuts():
    for n in BATCHES:
        clouds = recipe(n)
        lengths = batch_lengths(n)
        kept = [len(kept_rows(i, p)) for i, (p, _, _) in enumerate(clouds)]
        # a non-zero kept count on both sides of index 64 and in the last job; the job whose capacity is cut keeps rows
        assert kept[63] > 0 and kept[64] > 0 and kept[n - 1] > 0
        cut = 70 if n > 70 else max(i for i in range(n) if lengths[i])
        assert cut > 63 and kept[cut] >= 2
        assert all((kept[i] > 0) == (lengths[i] > 0) for i in range(n) if lengths[i] != 1)
        # the normals of the select: the recipe's bare third has none
        late = clouds[64:] if n > 70 else clouds
        assert any(nrm is None for _, nrm, _ in late) and any(nrm is not None and len(p) for p, nrm, _ in late)
        assert any(has_colors(i) and lengths[i] for i in range(64 if n > 70 else 0, n)) and not has_colors(70)
        # jobs at an index above 63 that drop rows, and keep some: the raw-bit clouds
        dropping = []
        for i in range(64, n):
            if is_raw(i) and lengths[i]:
                counts, _, _ = OR.knn_distance(clouds[i][0], RADIUS, 0)
                dropping.append((i, int((counts == 0).sum()), int((counts > 0).sum())))
        assert all(d > 0 for _, d, _ in dropping) and sum(1 for _, _, k in dropping if k > 0) >= (1 if n == 65 else 2), dropping
        assert len({(d, k) for _, d, k in dropping}) == len(dropping) or n == 1000  # counts that an index mix-up cannot reproduce
        print(f"N = {n}: (cloud, dropped, kept) of the raw-bit clouds past 63: {dropping[:6]}")
        assert lengths.index(0) == 1  # job index != cloud index from cloud 2 on


def test_clusters_have_border_rows_and_roots_beyond_the_first_tile():
    """In every batch size: a tame cloud is one big cluster and, at min_points 1, a few single rows off its surface, some
    of them beyond row 1023 (clouds 0 and 29 lie in the batch of 65, 70, 73 and 104 past index 63); at min_points 4 those
    rows are noise and the rows of the surface are border rows."""
    clouds = recipe(129)
    border, far_roots, noise = {}, {}, {}
    for i in (0, 5, 29, 70, 73, 104, 128):  # 70 001, 511, 4097, 70 001, 2049 and 4097 tame rows; 1023 raw-bit rows
        for m in MIN_POINTS:
            c = CR.cluster(clouds[i][0], RADIUS, m, by_cell=True, components="hooking")
            border[(i, m)], noise[(i, m)] = int(c.border.sum()), int(c.noise.sum())
            far_roots[(i, m)] = int((c.roots >= TILE_SCENE).sum())
            assert c.sizes.max() > 0.9 * (len(clouds[i][0]) - c.dropped) or is_raw(i)
    print(f"border rows {border}\nroots beyond the first tile {far_roots}\nnoise rows {noise}")
    assert all(border[(i, 4)] > 0 for i in (0, 5, 29, 70, 73, 104)) and not any(border[(i, 1)] for i in (0, 5, 29, 70, 73, 104, 128))
    assert all(far_roots[(i, 1)] > 0 for i in (0, 29, 70, 73, 104))  # a cluster whose root is past row 1023
    assert noise[(128, 1)] > 0 and noise[(128, 4)] > noise[(128, 1)]  # the dropped rows; kept rows far from every other
    assert all(noise[(i, 4)] > noise[(i, 1)] == 0 for i in (0, 29, 70, 73, 104))


def test_plane_batches_take_several_blocks_of_candidates_and_a_split_score_grid():
    for n in BATCHES:
        lengths = batch_lengths(n)
        hs = [plane_h(i, k) for i, k in enumerate(lengths)]
        per, split = plane_geometry(lengths, hs)
        print(f"N = {n}: {per} blocks of candidates per job, score grid split {split}")
        assert max(hs) == 700 and per == 3 > 1
        assert n == 1000 or split > 1  # 65 and 129 clouds are few enough tiles for the candidates to be split
        if n > 70:  # every H of the cycle occurs at an index above 63
            assert {hs[i] for i in range(64, n)} == set(PLANE_HS)
        assert sum(1 for i in range(n) if lengths[i] >= 3 and not hs[i]) >= 5  # clouds without a candidate: no plane
        assert all(h == 0 for h, k in zip(hs, lengths) if k < 3) and any(0 < k < 3 for k in lengths)
    # alone, the clouds of the singled-out set run with split 1, 2, 4 and 8 by their own H
    assert {plane_geometry([1025], [h])[1] for h in PLANE_HS} == {1, 2, 4, 8}
    assert plane_geometry(batch_lengths(65), [5] * 65) == (1, 1) and plane_geometry(batch_lengths(65), [130] * 65) == (1, 2)
    assert BIG_AT == (0, 70)
