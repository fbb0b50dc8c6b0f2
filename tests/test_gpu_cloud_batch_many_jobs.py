"""The job-table kernels (csrc/cloud_batch.hpp) over batches of 65, 129 and 1000 clouds on the GPU: point clouds from
images, transform, merge, voxel downsample and voxel-map insert, through the raw ABI calls.

What a batch of this size reaches and no smaller one does: the second trip of the write passes' loops over jobs
(k += 64: the capacity scan over all jobs, the sum of a job's earlier tile counts), a find_job search of ten levels, and
per-job words (lens, dropped) that travel back through cloud_of_job at indices past 63 with empty clouds in between.  The
inputs are the seeded recipe of test_cloud_batch_recipe_cpu.py, whose CPU tests state what it has to contain.

All clouds of a batch are views into ONE device allocation, back to back (the points of cloud 0, of cloud 1, ..., then
the normals in the same order), so most arrays start at a 4-byte-aligned address that is not 16-byte aligned: the layout
of a buffer sliced into clouds (images are handles that own their arrays: they are uploaded one by one).  All outputs of a call lie in one canary-filled allocation (_Arena) with CANARY_WORDS of canary
before, between and behind them, and every check compares the WHOLE allocation with the expectation laid out the same
way: what the call did not have to write must still hold the canary.

Every comparison is on uint32 views, bit for bit; no tolerance appears.  The expected value is the oracle's
orc_transform_points / orc_transform_normals, the numpy restatement of the downsample (voxel_restatement.py) or the host
path PointCloud.from_range_image, never the library.  The one exception is the one of test_gpu_cloud_transform.py: where
the oracle COMPUTES a NaN (a raw-bits point under a pose), the GPU must have a NaN too, and its payload and sign, which
differ between x86 and the GPU by design, are not compared.  Verbatim copies keep every NaN payload and are compared in
full.

Every test prints its wall time."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as O
import voxel_restatement as V
from align3d_amd import CameraIntrinsics, DevicePointCloud, DeviceVoxelMap, PointCloud, RangeImage, Transform, _abi
from align3d_amd._abi import PointCloudViewC, PoseC
from align3d_amd.range_image import DeviceRangeImage
from test_cloud_batch_recipe_cpu import BATCHES, VOXEL, image_recipe, recipe

pytestmark = pytest.mark.gpu

CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)
ORIGINS = (None, (0.013, -0.4, 7.5))
UNSET = 12345  # what the per-cloud result arrays hold before a call
SPARE_ROWS = 3  # rows of capacity beyond a map's cells: they must stay canary


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _singled_out(n):
    """The clouds passed alone and the ones whose capacity is cut: both sides of the 64-job stride, the long job at a
    high first_tile, and the last."""
    return sorted({i for i in (0, 63, 64, 65, 70, n - 1) if i < n})


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"[wall time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


class _Arena:
    """One device allocation for the outputs of a call: segment k has sizes[k] words, with CANARY_WORDS of canary before
    the first segment, between neighbours and behind the last; filled with the canary from end to end."""

    def __init__(self, ctx, sizes):
        self.ctx, self.sizes, self.offsets = ctx, [int(s) for s in sizes], []
        at = CANARY_WORDS
        for s in self.sizes:
            self.offsets.append(at)
            at += s + CANARY_WORDS
        self.words = at
        self._fill = np.full(self.words, CANARY, np.uint32)
        self.base = ctx.to_device(self._fill)

    def ptr(self, k):
        return self.base.value + 4 * self.offsets[k]

    def reset(self):
        _abi.check(self.ctx.lib.a3d_memcpy_h2d(self.ctx.handle, self.base, _abi.ptr(self._fill), self._fill.nbytes))

    def read(self):
        return self.ctx.to_host(self.base, np.empty(self.words, np.uint32))

    def blank(self):
        """The allocation as it is before a call, on the host: the canvas of an expectation."""
        return self._fill.copy()

    def put(self, canvas, k, words):
        words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
        assert words.size <= self.sizes[k]
        canvas[self.offsets[k]:self.offsets[k] + words.size] = words

    def segment(self, buffer, k, count=None):
        count = self.sizes[k] if count is None else count
        return buffer[self.offsets[k]:self.offsets[k] + count]

    def free(self):
        self.ctx.free(self.base)


def _assert_words(got, want, label, computed=False):
    """got == want word for word.  computed: the words are a transform's results, so where the expectation is a NaN the
    result has to be a NaN and its payload is not compared (the canary is no NaN)."""
    if computed:
        nan = np.isnan(want.view(np.float32))
        assert np.isnan(got.view(np.float32)[nan]).all(), f"{label}: a NaN of the oracle is no NaN here"
        got = np.where(nan, want, got)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{label}: {bad.size} of {want.size} words differ, the first at word {bad[0]}: "
                             f"got {int(got[bad[0]]):#010x}, expected {int(want[bad[0]]):#010x}")


def _pose_c(pose):
    p = PoseC()
    p.t[:] = [float(x) for x in pose[0]]
    p.q[:] = [float(x) for x in pose[1]]
    return p


def _oracle(pose_c, points, normals):
    """(orc_transform_points, orc_transform_normals) of host arrays under a PoseC."""
    if len(points) == 0:
        return points, normals
    out_n = np.empty_like(normals)
    O.load().orc_transform_normals(C.byref(pose_c), _abi.ptr(normals), normals.size // 3, _abi.ptr(out_n))
    return O.transform_points(pose_c, points), out_n


class _Clouds:
    """The clouds of recipe(n) resident in one allocation, and what the host expects of them (each expectation computed
    once and left unchanged).  Every cloud has normals in the allocation; a view of a `bare` cloud does not show them."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        full = recipe(n, bare_third=False)
        self.points = [p for p, _, _ in full]
        self.normals = [nrm for _, nrm, _ in full]
        self.bare = [nrm is None for _, nrm, _ in recipe(n)]
        self.pose_c = [_pose_c(pose) for _, _, pose in full]
        self.lens = [len(p) for p in self.points]
        assert 0 in self.lens[:2] and any(self.bare) and not all(self.bare)
        # the points of all clouds back to back, then their normals: an array starts 12 * (points before it) bytes in
        total = sum(self.lens)
        self.p_off = [3 * int(x) for x in np.cumsum([0] + self.lens[:-1])]
        self.n_off = [3 * total + o for o in self.p_off]
        self.flat = np.concatenate([_bits(a).reshape(-1) for a in (*self.points, *self.normals)])
        assert self.flat.size == 6 * total
        self.d_in = ctx.to_device(self.flat)
        starts = np.asarray([self.d_in.value + 4 * o for off in (self.p_off, self.n_off) for o, k in zip(off, self.lens) if k])
        assert (starts % 16 != 0).sum() > len(starts) // 2  # most arrays start off a 16-byte boundary
        self._transformed, self._downsampled, self._map = None, {}, None

    def has_normals(self, i, bare):
        return not (bare and self.bare[i])

    def views(self, which, bare, base=None):
        base = self.d_in.value if base is None else base
        arr = (PointCloudViewC * len(which))()
        for k, i in enumerate(which):
            arr[k].points = base + 4 * self.p_off[i]
            arr[k].normals = base + 4 * self.n_off[i] if self.has_normals(i, bare) else None
            arr[k].len = self.lens[i]
        return arr

    def poses(self, which):
        return (PoseC * len(which))(*[self.pose_c[i] for i in which])

    def outputs(self, which, bare, index=False):
        """An arena of three segments per cloud of `which`: points, normals, indices.  A plane the call does not write
        has no words (its pointer is null: pointers())."""
        sizes = []
        for i in which:
            sizes += [3 * self.lens[i], 3 * self.lens[i] if self.has_normals(i, bare) else 0, self.lens[i] if index else 0]
        return _Arena(self.ctx, sizes)

    def pointers(self, arena, which, bare, plane):
        """The [len(which)] pointer array of plane 0 (points), 1 (normals: null for a cloud viewed without) or 2."""
        return (C.c_void_p * len(which))(*[arena.ptr(3 * k + plane) if plane != 1 or self.has_normals(i, bare) else None
                                           for k, i in enumerate(which)])

    def transformed(self):
        """Per cloud (points, normals) under its own pose, through the oracle."""
        if self._transformed is None:
            self._transformed = [_oracle(pc, p, nrm) for pc, p, nrm in zip(self.pose_c, self.points, self.normals)]
        return self._transformed

    def downsampled(self, origin):
        """Per cloud (points, normals, index, dropped) of the restatement at VOXEL."""
        if origin not in self._downsampled:
            self._downsampled[origin] = [V.voxel_downsample_cloud(p, nrm, VOXEL, origin)
                                         for p, nrm in zip(self.points, self.normals)]
        return self._downsampled[origin]

    def mapped(self):
        """((points, normals, index, dropped) of the restatement over the merged, oracle-transformed clouds, dropped per
        cloud)."""
        if self._map is None:
            parts = self.transformed()
            merged_p = np.concatenate([p for p, _ in parts])
            merged_n = np.concatenate([nrm for _, nrm in parts])
            kept, _, _ = V.voxel_keys(merged_p, VOXEL)
            ends = np.cumsum(self.lens)
            dropped = [int((~kept[e - k:e]).sum()) for k, e in zip(self.lens, ends)]
            self._map = (V.voxel_downsample_cloud(merged_p, merged_n, VOXEL), dropped)
        return self._map

    def free(self):
        self.ctx.free(self.d_in)


class _Images:
    """The images of image_recipe(n) resident on the device, their host forms and the host path's clouds."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.hosts = [RangeImage(p, m, CameraIntrinsics(500.0, 500.0, m.shape[1] / 2, m.shape[0] / 2, m.shape[1], m.shape[0]),
                                 normals=nrm) for p, m, nrm in image_recipe(n)]
        self.pixels = [h.len() for h in self.hosts]
        self.with_normals = [h.normals is not None for h in self.hosts]
        self.expected = [PointCloud.from_range_image(h) for h in self.hosts]
        self.kept = [e.len() for e in self.expected]
        assert 0 in self.kept and not all(self.with_normals) and any(self.with_normals)
        self.devs = [DeviceRangeImage(ctx, h) for h in self.hosts]

    def outputs(self, which):
        sizes = []
        for i in which:
            sizes += [3 * self.pixels[i], 3 * self.pixels[i] if self.with_normals[i] else 0]
        return _Arena(self.ctx, sizes)

    def free(self):
        for d in self.devs:
            d.free()


class _Worlds:
    def __init__(self, ctx):
        self.ctx, self._clouds, self._images = ctx, {}, {}

    def clouds(self, n):
        if n not in self._clouds:
            self._clouds[n] = _Clouds(self.ctx, n)
        return self._clouds[n]

    def images(self, n):
        if n not in self._images:
            self._images[n] = _Images(self.ctx, n)
        return self._images[n]

    def free(self):
        for w in (*self._clouds.values(), *self._images.values()):
            w.free()


@pytest.fixture(scope="module")
def worlds(ctx):
    w = _Worlds(ctx)
    yield w
    w.free()


# ---- the raw calls ------------------------------------------------------------------------------------------------------

def _transform(w, which, arena, with_poses, bare=True):
    return w.ctx.lib.a3d_point_clouds_transform_device(
        w.ctx.handle, w.views(which, bare), w.poses(which) if with_poses else None, len(which),
        w.pointers(arena, which, bare, 0), w.pointers(arena, which, bare, 1))


def _transform_expectation(w, which, arena, with_poses, bare=True):
    canvas = arena.blank()
    for k, i in enumerate(which):
        p, nrm = w.transformed()[i] if with_poses else (w.points[i], w.normals[i])
        arena.put(canvas, 3 * k, _bits(p))
        if w.has_normals(i, bare):
            arena.put(canvas, 3 * k + 1, _bits(nrm))
    return canvas


def _downsample(w, which, arena, origin, want_index, capacities=None, bare=True):
    """(status, lens, dropped) of the raw call over the clouds `which` into `arena` (outputs(which, bare, want_index))."""
    m = len(which)
    caps = [w.lens[i] for i in which] if capacities is None else list(capacities)
    lens, dropped = (C.c_uint64 * m)(*[UNSET] * m), (C.c_uint64 * m)(*[UNSET] * m)
    st = w.ctx.lib.a3d_point_clouds_voxel_downsample_device(
        w.ctx.handle, w.views(which, bare), m, VOXEL, None if origin is None else (C.c_float * 3)(*origin),
        w.pointers(arena, which, bare, 0), w.pointers(arena, which, bare, 1),
        w.pointers(arena, which, bare, 2) if want_index else None, (C.c_uint64 * m)(*caps), lens, dropped)
    return st, list(lens), list(dropped)


def _downsample_expectation(w, which, arena, origin, want_index, bare=True):
    """(canvas, lens, dropped)."""
    canvas, expected = arena.blank(), w.downsampled(origin)
    for k, i in enumerate(which):
        p, nrm, index, _ = expected[i]
        arena.put(canvas, 3 * k, _bits(p))
        if w.has_normals(i, bare):
            arena.put(canvas, 3 * k + 1, _bits(nrm))
        if want_index:
            arena.put(canvas, 3 * k + 2, index)
    return canvas, [len(expected[i][2]) for i in which], [expected[i][3] for i in which]


def _from_images(w, which, arena, capacities=None):
    """(status, lens) of the raw call over the images `which` into `arena` (outputs(which))."""
    m = len(which)
    caps = [w.pixels[i] for i in which] if capacities is None else list(capacities)
    lens = (C.c_uint64 * m)(*[UNSET] * m)
    d_normals = (C.c_void_p * m)(*[arena.ptr(2 * k + 1) if w.with_normals[i] else None for k, i in enumerate(which)])
    assert any(p is None for p in d_normals) or m < 3
    st = w.ctx.lib.a3d_range_image_to_point_clouds(
        (C.c_void_p * m)(*[w.devs[i].handle for i in which]), m, (C.c_void_p * m)(*[arena.ptr(2 * k) for k in range(m)]),
        d_normals, (C.c_uint64 * m)(*caps), lens)
    return st, list(lens)


def _from_images_expectation(w, which, arena):
    canvas = arena.blank()
    for k, i in enumerate(which):
        arena.put(canvas, 2 * k, _bits(w.expected[i].points))
        if w.with_normals[i]:
            arena.put(canvas, 2 * k + 1, _bits(w.expected[i].normals))
    return canvas


def _map_insert(w, m, which):
    """The raw insert of the clouds `which` under their poses; returns their dropped counts."""
    k = len(which)
    dropped, cells = (C.c_uint64 * k)(*[UNSET] * k), C.c_uint64(UNSET)
    st = w.ctx.lib.a3d_voxel_map_insert(m.handle, w.views(which, bare=False), w.poses(which), k, dropped, C.byref(cells))
    assert st == _abi.A3D_OK and cells.value == m.cells()
    return list(dropped)


def _map_extract(ctx, m, cells):
    """The raw extract into an arena with SPARE_ROWS rows to spare: (the arena, freed: its layout lays out the
    expectation; its words after the call)."""
    capacity = cells + SPARE_ROWS
    arena = _Arena(ctx, [3 * capacity, 3 * capacity, capacity])
    n_out = C.c_uint64(UNSET)
    st = ctx.lib.a3d_voxel_map_extract(m.handle, arena.ptr(0), arena.ptr(1), arena.ptr(2), capacity, C.byref(n_out))
    assert st == _abi.A3D_OK and n_out.value == cells
    got = arena.read()
    arena.free()
    return arena, got


# ---- 1. transform -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
def test_transform_under_a_pose_per_job_verbatim_in_place_and_refused(worlds, n):
    w, ctx = worlds.clouds(n), worlds.ctx
    which = list(range(n))
    arena = w.outputs(which, bare=True)
    assert _transform(w, which, arena, with_poses=True) == _abi.A3D_OK
    _assert_words(arena.read(), _transform_expectation(w, which, arena, True), f"transform of {n}", computed=True)
    # poses_host = NULL: a verbatim copy, NaN payloads included
    arena.reset()
    assert _transform(w, which, arena, with_poses=False) == _abi.A3D_OK
    _assert_words(arena.read(), _transform_expectation(w, which, arena, False), f"verbatim copy of {n}")
    # in place: out[i] == in[i] on a second copy of the allocation (the normals of a bare view stay as they are)
    d_copy = ctx.to_device(w.flat)
    views = w.views(which, True, base=d_copy.value)
    st = ctx.lib.a3d_point_clouds_transform_device(ctx.handle, views, w.poses(which), n,
                                                   (C.c_void_p * n)(*[v.points for v in views]),
                                                   (C.c_void_p * n)(*[v.normals for v in views]))
    assert st == _abi.A3D_OK
    want = w.flat.copy()
    for i, (p, nrm) in enumerate(w.transformed()):
        want[w.p_off[i]:w.p_off[i] + 3 * w.lens[i]] = _bits(p).reshape(-1)
        if not w.bare[i]:
            want[w.n_off[i]:w.n_off[i] + 3 * w.lens[i]] = _bits(nrm).reshape(-1)
    _assert_words(ctx.to_host(d_copy, np.empty_like(w.flat)), want, f"in-place transform of {n}", computed=True)
    ctx.free(d_copy)
    if n > 700:
        # the output of cloud 700 (1025 points) on the input of cloud 3: refused, nothing written anywhere
        assert w.lens[700] > w.lens[3] > 0
        arena.reset()
        out_points = w.pointers(arena, which, True, 0)
        out_points[700] = w.d_in.value + 4 * w.p_off[3]
        st = ctx.lib.a3d_point_clouds_transform_device(ctx.handle, w.views(which, True), w.poses(which), n, out_points,
                                                       w.pointers(arena, which, True, 1))
        assert st == _abi.A3D_INVALID_PARAMETER
        _assert_words(arena.read(), arena.blank(), "a refused transform wrote into its outputs")
        _assert_words(ctx.to_host(w.d_in, np.empty_like(w.flat)), w.flat, "a refused transform wrote into its inputs")
    arena.free()


# ---- 2. merge -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
def test_merge_with_and_without_the_normals_plane_and_one_short(worlds, n):
    w, ctx = worlds.clouds(n), worlds.ctx
    which = list(range(n))
    total = sum(w.lens)
    parts = w.transformed()
    want_p = _bits(np.concatenate([p for p, _ in parts]))
    want_n = _bits(np.concatenate([nrm for _, nrm in parts]))
    arena = _Arena(ctx, [3 * total, 3 * total])
    for normals_plane in (True, False):
        arena.reset()
        n_out = C.c_uint64(UNSET)
        # (without the normals plane the clouds may lack normals: the views of the bare third do)
        st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, w.views(which, bare=not normals_plane), w.poses(which), n,
                                                   arena.ptr(0), arena.ptr(1) if normals_plane else None, total, C.byref(n_out))
        assert st == _abi.A3D_OK and n_out.value == total
        canvas = arena.blank()
        arena.put(canvas, 0, want_p)
        if normals_plane:
            arena.put(canvas, 1, want_n)
        _assert_words(arena.read(), canvas, f"merge of {n}, normals plane {normals_plane}", computed=True)
    # capacity = total - 1 reports the total and writes nothing
    arena.reset()
    n_out = C.c_uint64(UNSET)
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, w.views(which, False), w.poses(which), n, arena.ptr(0), arena.ptr(1),
                                               total - 1, C.byref(n_out))
    assert st == _abi.A3D_INVALID_PARAMETER and n_out.value == total
    _assert_words(arena.read(), arena.blank(), "a merge one short wrote")
    arena.free()


# ---- 3. voxel downsample --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("origin", ORIGINS, ids=["no origin", "origin"])
@pytest.mark.parametrize("n", BATCHES)
def test_voxel_downsample_of_every_job(worlds, n, origin):
    w = worlds.clouds(n)
    which = list(range(n))
    want_index = n % 2 == 1
    arena = w.outputs(which, bare=True, index=want_index)
    st, lens, dropped = _downsample(w, which, arena, origin, want_index)
    canvas, want_lens, want_dropped = _downsample_expectation(w, which, arena, origin, want_index)
    assert st == _abi.A3D_OK
    assert lens == want_lens and dropped == want_dropped
    assert all((lens[i], dropped[i]) == (0, 0) for i in which if w.lens[i] == 0)
    if n > 64 and origin is None:
        assert sum(1 for i in which[64:] if dropped[i] and lens[i]) >= (3 if n == 1000 else 1)
    _assert_words(arena.read(), canvas, f"voxel downsample of {n}, origin {origin}")
    arena.free()


# ---- 4. point clouds from images --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
def test_point_clouds_from_images_of_every_job(worlds, n):
    w = worlds.images(n)
    which = list(range(n))
    arena = w.outputs(which)
    st, lens = _from_images(w, which, arena)
    assert st == _abi.A3D_OK and lens == w.kept
    _assert_words(arena.read(), _from_images_expectation(w, which, arena), f"point clouds from {n} images")
    arena.free()


# ---- 5. voxel-map insert ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
def test_voxel_map_insert_in_one_call_and_in_calls_of_64_1_and_the_rest(worlds, n):
    w, ctx = worlds.clouds(n), worlds.ctx
    (exp_p, exp_n, exp_i, _), exp_dropped = w.mapped()
    cells = len(exp_i)
    assert 0 < cells < sum(w.lens) - sum(exp_dropped)  # cells are shared
    assert n == 65 or exp_i.max() >= sum(w.lens[:64])  # a winner's index counts the points of more than 64 clouds
    which = list(range(n))
    one = DeviceVoxelMap(ctx, VOXEL)
    assert _map_insert(w, one, which) == exp_dropped
    s = one.stats()
    assert (s["cells"], s["total"], s["dropped_total"]) == (cells, sum(w.lens), sum(exp_dropped))
    arena, got = _map_extract(ctx, one, cells)
    canvas = arena.blank()
    arena.put(canvas, 0, _bits(exp_p))
    arena.put(canvas, 1, _bits(exp_n))
    arena.put(canvas, 2, exp_i)
    _assert_words(got, canvas, f"voxel map of {n} clouds in one call")
    one.free()
    grouped = DeviceVoxelMap(ctx, VOXEL)
    dropped = []
    for group in (which[:64], which[64:65], which[65:]):
        if group:
            dropped += _map_insert(w, grouped, group)
    assert dropped == exp_dropped
    s = grouped.stats()
    assert (s["cells"], s["total"], s["dropped_total"]) == (cells, sum(w.lens), sum(exp_dropped))
    _, got_grouped = _map_extract(ctx, grouped, cells)
    _assert_words(got_grouped, got, f"voxel map of {n} clouds in calls of 64, 1 and {n - 65}")
    grouped.free()


# ---- 6. capacity one short in a late job --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (129, 1000))
def test_voxel_downsample_capacity_one_short_in_a_late_job(worlds, n):
    w = worlds.clouds(n)
    which = list(range(n))
    want_index = n % 2 == 1
    arena = w.outputs(which, bare=True, index=want_index)
    canvas, counts, want_dropped = _downsample_expectation(w, which, arena, None, want_index)
    for short in (0, 63, 64, 65, n - 1):
        assert counts[short] >= 1
        caps = list(w.lens)
        caps[short] = counts[short] - 1
        st, lens, dropped = _downsample(w, which, arena, None, want_index, capacities=caps)
        assert st == _abi.A3D_INVALID_PARAMETER, short
        assert lens == counts and dropped == want_dropped, short
        _assert_words(arena.read(), arena.blank(), f"a downsample one short in cloud {short} of {n} wrote")
    st, lens, dropped = _downsample(w, which, arena, None, want_index, capacities=counts)  # exactly enough is enough
    assert st == _abi.A3D_OK and lens == counts and dropped == want_dropped
    _assert_words(arena.read(), canvas, f"voxel downsample of {n} with exact capacities")
    arena.free()


@pytest.mark.parametrize("n", (129, 1000))
def test_point_clouds_from_images_capacity_one_short_in_a_late_job(worlds, n):
    w = worlds.images(n)
    which = list(range(n))
    arena = w.outputs(which)
    for short in (0, 63, 64, 65, n - 1):
        assert w.kept[short] >= 1
        caps = list(w.pixels)
        caps[short] = w.kept[short] - 1
        st, lens = _from_images(w, which, arena, capacities=caps)
        assert st == _abi.A3D_INVALID_PARAMETER, short
        assert lens == w.kept, short
        _assert_words(arena.read(), arena.blank(), f"a conversion one short in image {short} of {n} wrote")
    st, lens = _from_images(w, which, arena, capacities=w.kept)  # exactly enough is enough
    assert st == _abi.A3D_OK and lens == w.kept
    _assert_words(arena.read(), _from_images_expectation(w, which, arena), f"point clouds from {n} images, exact capacities")
    arena.free()


# ---- 7. a job alone equals the job in the batch; two runs of the batch are identical ------------------------------------------

def _alone(batch_arena, batch_words, per_cloud, i, single_arena, single_words, label):
    for plane in range(per_cloud):
        _assert_words(single_arena.segment(single_words, plane), batch_arena.segment(batch_words, per_cloud * i + plane),
                      f"{label}: cloud {i} alone, plane {plane}")


@pytest.mark.parametrize("n", BATCHES)
def test_transform_alone_equals_in_the_batch_and_runs_are_identical(worlds, n):
    w = worlds.clouds(n)
    which = list(range(n))
    arena = w.outputs(which, bare=True)
    runs = []
    for _ in range(2):
        arena.reset()
        assert _transform(w, which, arena, with_poses=True) == _abi.A3D_OK
        runs.append(arena.read())
    _assert_words(runs[1], runs[0], f"two transforms of {n}")
    for i in _singled_out(n):
        single = w.outputs([i], bare=True)
        assert _transform(w, [i], single, with_poses=True) == _abi.A3D_OK
        _alone(arena, runs[0], 3, i, single, single.read(), "transform")
        single.free()
    arena.free()


@pytest.mark.parametrize("n", BATCHES)
def test_voxel_downsample_alone_equals_in_the_batch_and_runs_are_identical(worlds, n):
    w = worlds.clouds(n)
    which = list(range(n))
    arena = w.outputs(which, bare=True, index=True)
    runs = []
    for _ in range(2):
        arena.reset()
        st, lens, dropped = _downsample(w, which, arena, ORIGINS[1], True)
        assert st == _abi.A3D_OK
        runs.append((arena.read(), lens, dropped))
    _assert_words(runs[1][0], runs[0][0], f"two downsamples of {n}")
    assert runs[1][1:] == runs[0][1:]
    for i in _singled_out(n):
        single = w.outputs([i], bare=True, index=True)
        st, lens, dropped = _downsample(w, [i], single, ORIGINS[1], True)
        assert st == _abi.A3D_OK and (lens[0], dropped[0]) == (runs[0][1][i], runs[0][2][i])
        _alone(arena, runs[0][0], 3, i, single, single.read(), "voxel downsample")
        single.free()
    arena.free()


@pytest.mark.parametrize("n", BATCHES)
def test_point_clouds_from_images_alone_equals_in_the_batch_and_runs_are_identical(worlds, n):
    w = worlds.images(n)
    which = list(range(n))
    arena = w.outputs(which)
    runs = []
    for _ in range(2):
        arena.reset()
        st, lens = _from_images(w, which, arena)
        assert st == _abi.A3D_OK
        runs.append((arena.read(), lens))
    _assert_words(runs[1][0], runs[0][0], f"two conversions of {n} images")
    assert runs[1][1] == runs[0][1]
    for i in _singled_out(n):
        single = w.outputs([i])
        st, lens = _from_images(w, [i], single)
        assert st == _abi.A3D_OK and lens[0] == runs[0][1][i]
        _alone(arena, runs[0][0], 2, i, single, single.read(), "point clouds from images")
        single.free()
    arena.free()


# ---- 8. the Python forms ----------------------------------------------------------------------------------------------------

def _view_cloud(w, i, bare):
    """Cloud i of the shared allocation as a DevicePointCloud that owns nothing (it is never freed)."""
    c = DevicePointCloud.__new__(DevicePointCloud)
    c.ctx, c.n = w.ctx, w.lens[i]
    c.d_points = C.c_void_p(w.d_in.value + 4 * w.p_off[i])
    c.d_normals = C.c_void_p(w.d_in.value + 4 * w.n_off[i]) if w.has_normals(i, bare) else None
    return c


def _assert_cloud(cloud, want_points, want_normals, label):
    """A resident cloud against [len, 3] uint32 rows (want_normals None: the cloud has no normals)."""
    got_p, got_n = cloud.download()
    assert 3 * cloud.len() == want_points.size, label
    _assert_words(_bits(got_p).reshape(-1), want_points.reshape(-1), f"{label}: points")
    assert (got_n is None) == (want_normals is None) == (cloud.d_normals is None), label
    if want_normals is not None:
        _assert_words(_bits(got_n).reshape(-1), want_normals.reshape(-1), f"{label}: normals")


def test_python_forms_return_what_the_raw_calls_return(worlds):
    n = 129
    w, im, ctx = worlds.clouds(n), worlds.images(n), worlds.ctx
    which = list(range(n))
    transforms = [Transform.from_c(p) for p in w.pose_c]
    bare_views = [_view_cloud(w, i, True) for i in which]
    full_views = [_view_cloud(w, i, False) for i in which]
    # DevicePointCloud.from_range_images
    arena = im.outputs(which)
    st, lens = _from_images(im, which, arena)
    assert st == _abi.A3D_OK
    raw = arena.read()
    clouds = DevicePointCloud.from_range_images(im.devs)
    assert len(clouds) == n
    for i, c in enumerate(clouds):
        _assert_cloud(c, arena.segment(raw, 2 * i, 3 * lens[i]), arena.segment(raw, 2 * i + 1, 3 * lens[i])
                      if im.with_normals[i] else None, f"from_range_images[{i}]")
        c.free()
    arena.free()
    # transform_many
    arena = w.outputs(which, bare=True)
    assert _transform(w, which, arena, with_poses=True) == _abi.A3D_OK
    raw = arena.read()
    moved = DevicePointCloud.transform_many(bare_views, transforms)
    assert len(moved) == n
    for i, c in enumerate(moved):
        _assert_cloud(c, arena.segment(raw, 3 * i), None if w.bare[i] else arena.segment(raw, 3 * i + 1), f"transform_many[{i}]")
        c.free()
    arena.free()
    # merge
    total = sum(w.lens)
    arena = _Arena(ctx, [3 * total, 3 * total])
    n_out = C.c_uint64(UNSET)
    st = ctx.lib.a3d_point_clouds_merge_device(ctx.handle, w.views(which, False), w.poses(which), n, arena.ptr(0), arena.ptr(1),
                                               total, C.byref(n_out))
    assert st == _abi.A3D_OK and n_out.value == total
    raw = arena.read()
    merged = DevicePointCloud.merge(full_views, transforms)
    _assert_cloud(merged, arena.segment(raw, 0), arena.segment(raw, 1), "merge")
    merged.free()
    arena.free()
    # voxel_downsample_many
    arena = w.outputs(which, bare=True)
    st, lens, _ = _downsample(w, which, arena, ORIGINS[1], False)
    assert st == _abi.A3D_OK
    raw = arena.read()
    thinned = DevicePointCloud.voxel_downsample_many(bare_views, VOXEL, ORIGINS[1])
    assert len(thinned) == n
    for i, c in enumerate(thinned):
        _assert_cloud(c, arena.segment(raw, 3 * i, 3 * lens[i]), None if w.bare[i] else arena.segment(raw, 3 * i + 1, 3 * lens[i]),
                      f"voxel_downsample_many[{i}]")
        c.free()
    arena.free()
    # DeviceVoxelMap.insert_many
    raw_map, py_map = DeviceVoxelMap(ctx, VOXEL), DeviceVoxelMap(ctx, VOXEL)
    raw_dropped = _map_insert(w, raw_map, which)
    cells = raw_map.cells()
    arena, raw = _map_extract(ctx, raw_map, cells)
    py_dropped = py_map.insert_many(full_views, transforms)
    assert len(py_dropped) == n and py_dropped == raw_dropped and py_map.stats() == raw_map.stats()
    cloud, index = py_map.extract(return_index=True)
    _assert_cloud(cloud, arena.segment(raw, 0, 3 * cells), arena.segment(raw, 1, 3 * cells), "insert_many, extract")
    assert np.array_equal(index, arena.segment(raw, 2, cells))
    cloud.free(), raw_map.free(), py_map.free()
