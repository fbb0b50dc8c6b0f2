"""The four scene entries (csrc/cloud_outliers.hip: knn_distance, select, cluster; csrc/cloud_plane.hip: segment_plane) over
batches of 65, 129 and 1000 clouds on the GPU, through the raw ABI calls.

What a batch of this size reaches and no smaller one does: the second trip of the loops over jobs (k += 64: the select's
capacity scan over all jobs), a find_job search of ten levels, per-job words (lens, the four statistics, dropped,
clusters, noise, best, inliers) that travel back through cloud_of_job at indices past 63 with empty clouds in between,
clouds of 69 tiles at a high first_tile, and several blocks of plane candidates per job.  The clouds are the seeded
recipe of test_cloud_batch_recipe_cpu.py, resident in one allocation as in test_gpu_cloud_batch_many_jobs.py; what each
entry takes per cloud is test_scene_batch_recipe_cpu.py's, whose CPU tests state what the inputs have to contain.

All device outputs of a call lie in one canary-filled allocation (_Arena), and every check compares the WHOLE allocation
with the expectation laid out the same way: what the call did not have to write must still hold the canary.  Per-cloud
host arrays start at UNSET.  Every comparison is on integer words, or on the u64 bits of the plane's doubles; no tolerance
appears.  The expected value is the numpy restatement (outlier_restatement.py, cluster_restatement.py by cell with its
hooking components, plane_restatement.py), never the library.  Every cloud of every batch is restated, the batch of 1000
included, with one exception, the precedent of the 20 000-point test of test_gpu_cloud_outliers.py: the distance sums of
the two clouds of 70 001 rows are restated on 512 seeded rows, and their statistics are those of the sums read back.

Every test prints its wall time."""
import ctypes as C
import time

import numpy as np
import pytest

import cluster_restatement as CR
import outlier_restatement as OR
import plane_restatement as PR
from align3d_amd import _abi
from test_cloud_batch_recipe_cpu import BATCHES, BIG_AT
from test_gpu_cloud_batch_many_jobs import UNSET, _Arena, _assert_words, _bits, _Clouds, _singled_out, _wall_time  # noqa: F401
from test_scene_batch_recipe_cpu import (KNN_KS, MIN_POINTS, PLANE_T, RADIUS, has_colors, plane_triples, select_bounds,
                                         select_colors, select_values)

pytestmark = pytest.mark.gpu

SAMPLED_ROWS = 512
COLOR_OFFSET = 1  # a colour output starts this many bytes past a 4-byte boundary
REFINES = (0, 2)


class _Scene:
    """The clouds of recipe(n) resident on the device (_Clouds: one allocation, the views of the bare third without
    normals), the select's values and colours resident in one allocation each, and what the host expects of every entry,
    each expectation computed once and left unchanged."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.w = _Clouds(ctx, n)
        self.lens, self.points = self.w.lens, self.w.points
        self.normals = [None if self.w.bare[i] else self.w.normals[i] for i in range(n)]
        self.values = [select_values(i, k) for i, k in enumerate(self.lens)]
        self.bounds = [select_bounds(i) for i in range(n)]
        self.colors = [select_colors(i, k) if has_colors(i) else None for i, k in enumerate(self.lens)]
        self.keeps = [OR.select(v, lo, hi) for v, (lo, hi) in zip(self.values, self.bounds)]
        self.v_off = [int(x) for x in np.cumsum([0] + self.lens[:-1])]
        self.d_values = ctx.to_device(np.concatenate(self.values + [np.zeros(1, np.uint32)]))
        sizes = [3 * k if has_colors(i) else 0 for i, k in enumerate(self.lens)]
        self.c_off = [int(x) for x in np.cumsum([0] + sizes[:-1])]
        self.d_colors = ctx.to_device(np.concatenate([c.reshape(-1) for c in self.colors if c is not None] + [np.zeros(4, np.uint8)]))
        self.triples = [plane_triples(i, k) for i, k in enumerate(self.lens)]
        self._pairs, self._knn, self._cluster, self._plane = {}, {}, {}, {}

    def views(self, which):
        return self.w.views(which, bare=True)

    def pairs(self, i):
        if i not in self._pairs:
            self._pairs[i] = CR.pairs_by_cell(self.points[i], RADIUS)
        return self._pairs[i]

    def knn(self, i, k):
        """(counts, qsum or None, stats or None, rows or None): rows are the restated rows of a cloud of BIG_AT, whose
        counts come from the neighbour pairs of the cluster restatement (rule 2: the same bits) and whose statistics are
        not restated."""
        if (i, k) not in self._knn:
            if i in BIG_AT:
                rows = np.sort(np.random.default_rng([78, i]).choice(self.lens[i], size=SAMPLED_ROWS, replace=False))
                counts = np.bincount(self.pairs(i).i, minlength=self.lens[i]).astype(np.uint32)
                sampled, qsum, _ = OR.knn_distance(self.points[i], RADIUS, k, rows=rows)
                assert np.array_equal(sampled[rows], counts[rows])  # the two restatements of the count agree
                self._knn[(i, k)] = (counts, qsum, None, rows)
            else:
                self._knn[(i, k)] = (*OR.knn_distance(self.points[i], RADIUS, k), None)
        return self._knn[(i, k)]

    def cluster(self, i, m):
        if (i, m) not in self._cluster:
            self._cluster[(i, m)] = CR.cluster_pairs(self.pairs(i), m, components="hooking")
        return self._cluster[(i, m)]

    def plane(self, i, refine):
        if (i, refine) not in self._plane:
            self._plane[(i, refine)] = PR.segment(self.points[i], self.triples[i], PLANE_T, refine)
        return self._plane[(i, refine)]

    def free(self):
        self.w.free(), self.ctx.free(self.d_values), self.ctx.free(self.d_colors)


class _Scenes:
    def __init__(self, ctx):
        self.ctx, self._scenes = ctx, {}

    def get(self, n):
        if n not in self._scenes:
            self._scenes[n] = _Scene(self.ctx, n)
        return self._scenes[n]

    def free(self):
        for s in self._scenes.values():
            s.free()


@pytest.fixture(scope="module")
def scenes(ctx):
    s = _Scenes(ctx)
    yield s
    s.free()


def _table(arena, which, per_cloud, plane, present=lambda i: True, offset=0):
    """The [len(which)] pointer array of segment `plane` of every cloud; null where the cloud has no such output."""
    return (C.c_void_p * len(which))(*[arena.ptr(per_cloud * k + plane) + offset if present(i) else None
                                       for k, i in enumerate(which)])


def _unset(count):
    return (C.c_uint64 * count)(*[UNSET] * count)


# ---- the raw calls: (arena words, host words) of a run, and their expectation ---------------------------------------------

def _knn(s, which, k):
    """Segments per cloud: counts [len], qsum [len] (handed over for k == 0 as well: it must stay untouched)."""
    m = len(which)
    arena = _Arena(s.ctx, [s.lens[i] for i in which for _ in range(2)])
    stats, dropped = _unset(4 * m), _unset(m)
    st = s.ctx.lib.a3d_point_clouds_knn_distance_device(s.ctx.handle, s.views(which), m, RADIUS, k, _table(arena, which, 2, 0),
                                                        _table(arena, which, 2, 1), stats, dropped)
    assert st == _abi.A3D_OK
    got = arena.read()
    arena.free()
    return arena, got, {"stats": [tuple(int(v) for v in stats[4 * j:4 * j + 4]) for j in range(m)], "dropped": list(dropped)}


def _knn_expectation(s, which, k, arena, got):
    canvas, stats, dropped = arena.blank(), [], []
    for j, i in enumerate(which):
        counts, qsum, st, rows = s.knn(i, k)
        arena.put(canvas, 2 * j, counts)
        dropped.append(int((counts == 0).sum()))
        if k and rows is None:
            arena.put(canvas, 2 * j + 1, qsum)
        elif k:  # a cloud of BIG_AT: the sampled rows are restated; the statistics are those of the sums read back
            read_back = arena.segment(got, 2 * j + 1).copy()
            st = OR.stats_of(read_back)
            # (about 17 rows to a ball of this radius: rows with 17 others and rows without, both among the sampled ones)
            assert st[0] > len(read_back) // 10 and min((qsum[rows] != OR.NONE).sum(), (qsum[rows] == OR.NONE).sum()) > 10
            read_back[rows] = qsum[rows]
            arena.put(canvas, 2 * j + 1, read_back)
        stats.append(st if k else (0, 0, 0, 0))
    return canvas, {"stats": stats, "dropped": dropped}


def _select(s, which, capacities=None):
    """Segments per cloud: points [cap][3], normals [cap][3] (clouds with normals), colours 3 cap bytes from byte
    COLOR_OFFSET on, index [cap] (clouds with colours).  Returns (status, arena, words, lens)."""
    m = len(which)
    caps = [len(s.keeps[i]) for i in which] if capacities is None else list(capacities)
    sizes = []
    for i, cap in zip(which, caps):
        sizes += [3 * cap, 3 * cap if s.normals[i] is not None else 0, (3 * cap + COLOR_OFFSET + 3) // 4 if has_colors(i) else 0,
                  cap if has_colors(i) else 0]
    arena = _Arena(s.ctx, sizes)
    lens = _unset(m)
    lo, hi = (C.c_uint32 * m)(*[s.bounds[i][0] for i in which]), (C.c_uint32 * m)(*[s.bounds[i][1] for i in which])
    d_colors = (C.c_void_p * m)(*[s.d_colors.value + s.c_off[i] if has_colors(i) else None for i in which])
    d_values = (C.c_void_p * m)(*[s.d_values.value + 4 * s.v_off[i] for i in which])
    st = s.ctx.lib.a3d_point_clouds_select_device(
        s.ctx.handle, s.views(which), d_colors, m, d_values, lo, hi, _table(arena, which, 4, 0),
        _table(arena, which, 4, 1, lambda i: s.normals[i] is not None), _table(arena, which, 4, 2, has_colors, COLOR_OFFSET),
        _table(arena, which, 4, 3, has_colors), (C.c_uint64 * m)(*caps), lens)
    got = arena.read()
    arena.free()
    return st, arena, got, list(lens)


def _select_expectation(s, which, arena):
    canvas = arena.blank()
    for j, i in enumerate(which):
        keep = s.keeps[i]
        arena.put(canvas, 4 * j, _bits(s.points[i][keep]))
        if s.normals[i] is not None:
            arena.put(canvas, 4 * j + 1, _bits(s.normals[i][keep]))
        if has_colors(i):
            at = 4 * arena.offsets[4 * j + 2] + COLOR_OFFSET
            canvas.view(np.uint8)[at:at + 3 * len(keep)] = s.colors[i][keep].reshape(-1)
            arena.put(canvas, 4 * j + 3, keep)
    return canvas, [len(s.keeps[i]) for i in which]


def _cluster(s, which, m):
    """Segments per cloud: labels, row_sizes, sizes, roots, [len] each."""
    k = len(which)
    arena = _Arena(s.ctx, [s.lens[i] for i in which for _ in range(4)])
    words = [_unset(k) for _ in range(3)]
    st = s.ctx.lib.a3d_point_clouds_cluster_device(s.ctx.handle, s.views(which), k, RADIUS, m, *[_table(arena, which, 4, f) for f in range(4)],
                                                   *words)
    assert st == _abi.A3D_OK
    got = arena.read()
    arena.free()
    return arena, got, {"clusters": list(words[0]), "noise": list(words[1]), "dropped": list(words[2])}


def _cluster_expectation(s, which, m, arena):
    canvas, words = arena.blank(), {"clusters": [], "noise": [], "dropped": []}
    for j, i in enumerate(which):
        want = s.cluster(i, m)
        for f, field in enumerate((want.labels, want.row_sizes, want.sizes, want.roots)):  # sizes, roots: the first C words
            arena.put(canvas, 4 * j + f, field)
        words["clusters"].append(len(want.sizes)), words["noise"].append(int(want.noise.sum())), words["dropped"].append(want.dropped)
    return canvas, words


def _plane(s, which, refine):
    """Segments per cloud: flags [len], counts [H]."""
    k = len(which)
    arena = _Arena(s.ctx, [x for i in which for x in (s.lens[i], len(s.triples[i]))])
    planes = (C.c_double * (4 * k))(*[float(UNSET)] * (4 * k))
    words = [_unset(k) for _ in range(3)]
    triples = [np.ascontiguousarray(s.triples[i], np.uint32) for i in which]
    st = s.ctx.lib.a3d_point_clouds_segment_plane_device(
        s.ctx.handle, s.views(which), k, PLANE_T, refine, (C.c_void_p * k)(*[tr.ctypes.data if len(tr) else None for tr in triples]),
        (C.c_uint32 * k)(*[len(tr) for tr in triples]), _table(arena, which, 2, 0), _table(arena, which, 2, 1), planes, *words)
    assert st == _abi.A3D_OK
    got = arena.read()
    arena.free()
    return arena, got, {"planes": np.array(planes[:], np.float64).view(np.uint64).tolist(), "best": list(words[0]),
                        "inliers": list(words[1]), "refit_rows": list(words[2])}


def _plane_expectation(s, which, refine, arena):
    canvas, words = arena.blank(), {"planes": [], "best": [], "inliers": [], "refit_rows": []}
    for j, i in enumerate(which):
        want = s.plane(i, refine)
        arena.put(canvas, 2 * j, want.flags)
        arena.put(canvas, 2 * j + 1, want.counts)
        words["planes"] += np.ascontiguousarray(want.plane, np.float64).view(np.uint64).tolist()
        words["best"].append(want.best), words["inliers"].append(want.inliers), words["refit_rows"].append(want.refit_rows)
    return canvas, words


def _alone_and_again(s, n, run, per_cloud, per_word, first, label):
    """A second run of the batch gives identical words; each cloud of _singled_out passed alone gives the words it got in
    the batch.  first = (arena, words, host words) of the first run; per_word: host words per cloud, by name."""
    arena, got, host = first
    _, again, host_again = run(list(range(n)))
    _assert_words(again, got, f"{label}: two runs of {n}")
    assert host_again == host, label
    for i in _singled_out(n):
        single, words, single_host = run([i])
        for plane in range(per_cloud):
            _assert_words(single.segment(words, plane), arena.segment(got, per_cloud * i + plane), f"{label}: cloud {i} alone, segment {plane}")
        for name, width in per_word.items():
            assert single_host[name] == host[name][width * i:width * (i + 1)], (label, i, name)


# ---- 1. knn_distance ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KNN_KS)
@pytest.mark.parametrize("n", BATCHES)
def test_knn_distance_of_every_job(scenes, n, k):
    s = scenes.get(n)
    which = list(range(n))
    arena, got, host = _knn(s, which, k)
    canvas, want = _knn_expectation(s, which, k, arena, got)
    assert host == want
    assert all((host["stats"][i], host["dropped"][i]) == ((0, 0, 0, 0), 0) for i in which if s.lens[i] == 0)
    assert sum(1 for i in which[64:] if host["dropped"][i] and host["dropped"][i] < s.lens[i]) >= (3 if n == 1000 else 1)
    _assert_words(got, canvas, f"knn_distance of {n}, k = {k}")
    _alone_and_again(s, n, lambda w: _knn(s, w, k), 2, {"stats": 1, "dropped": 1}, (arena, got, host), f"knn_distance k = {k}")


# ---- 2. select -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
def test_select_of_every_job_with_exact_capacities(scenes, n):
    s = scenes.get(n)
    which = list(range(n))
    st, arena, got, lens = _select(s, which)
    canvas, want_lens = _select_expectation(s, which, arena)
    assert st == _abi.A3D_OK and lens == want_lens
    assert want_lens[63] > 0 and want_lens[64] > 0 and want_lens[n - 1] > 0 and sum(1 for x in want_lens if x == 0) >= n // 15
    _assert_words(got, canvas, f"select of {n}")

    def run(w):
        st, arena, got, lens = _select(s, w)
        assert st == _abi.A3D_OK
        return arena, got, {"lens": lens}

    _alone_and_again(s, n, run, 4, {"lens": 1}, (arena, got, {"lens": lens}), "select")


@pytest.mark.parametrize("n", BATCHES)
def test_select_capacity_one_short_in_a_late_job(scenes, n):
    s = scenes.get(n)
    which = list(range(n))
    counts = [len(s.keeps[i]) for i in which]
    short = 70 if n > 70 else max(i for i in which if s.lens[i])
    assert short > 63 and counts[short] >= 2
    caps = list(counts)
    caps[short] -= 1
    st, arena, got, lens = _select(s, which, capacities=caps)
    assert st == _abi.A3D_INVALID_PARAMETER
    assert lens == counts
    _assert_words(got, arena.blank(), f"a select one short in cloud {short} of {n} wrote")


# ---- 3. cluster ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MIN_POINTS)
@pytest.mark.parametrize("n", BATCHES)
def test_cluster_of_every_job(scenes, n, m):
    s = scenes.get(n)
    which = list(range(n))
    arena, got, host = _cluster(s, which, m)
    canvas, want = _cluster_expectation(s, which, m, arena)
    assert host == want
    assert all(host[f][i] == 0 for f in host for i in which if s.lens[i] == 0)
    assert sum(1 for i in which[64:] if 0 < host["dropped"][i] < s.lens[i]) >= (3 if n == 1000 else 1)
    _assert_words(got, canvas, f"cluster of {n}, min_points {m}")
    _alone_and_again(s, n, lambda w: _cluster(s, w, m), 4, {"clusters": 1, "noise": 1, "dropped": 1}, (arena, got, host),
                     f"cluster min_points {m}")


# ---- 4. segment_plane ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("n", BATCHES)
def test_segment_plane_of_every_job(scenes, n, refine):
    s = scenes.get(n)
    which = list(range(n))
    arena, got, host = _plane(s, which, refine)
    canvas, want = _plane_expectation(s, which, refine, arena)
    assert host == want
    assert n <= 70 or sum(1 for i in which[64:] if host["best"][i] != PR.NONE) >= 20  # (cloud 64 has no candidate)
    assert all(host["best"][i] != PR.NONE and host["inliers"][i] > 1000 for i in BIG_AT if i < n)
    assert all(host["best"][i] == PR.NONE and host["planes"][4 * i:4 * i + 4] == [0] * 4 for i in which if len(s.triples[i]) == 0)
    _assert_words(got, canvas, f"segment_plane of {n}, refine {refine}")
    _alone_and_again(s, n, lambda w: _plane(s, w, refine), 2, {"planes": 4, "best": 1, "inliers": 1, "refit_rows": 1},
                     (arena, got, host), f"segment_plane refine {refine}")
