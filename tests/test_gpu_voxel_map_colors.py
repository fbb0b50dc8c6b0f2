"""Colours in the persistent voxel map (a3d_voxel_map_new_rgb / _insert_rgb / _extract_rgb, DeviceVoxelMap(colors=True))
on the GPU.

The contract under test extends the map's word for word: after any sequence of inserts, extract equals merge of
everything inserted followed by voxel_downsample — points, normals, COLOURS, order and indices — however the inserts were
grouped and whatever the table's size history was; after a retain the map is a new map into which the surviving rows,
colours too, went as one cloud.  The expected value is always the numpy restatement (voxel_restatement.py) applied to
the concatenation of the ORACLE-transformed host clouds, as test_gpu_voxel_map.py does; a colour is a pure function of
position, so the expected colour of a row is colors_in[index].  Input colours identify their row (colors_util.row_colors)
and extracts go into canary-filled buffers with byte-granular guards (colors_util.Guarded)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import voxel_restatement as V
from align3d_amd import (A3dError, DevicePointCloud, DeviceVoxelMap, IcpParams, PointCloud, RangeImageBuilder,
                         SlamTbDataset, Transform, _abi)
from colors_util import Guarded, check_rows, row_colors, untouched
from gpu_util import oracle_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.5
SIZES = (2049, 2047, 65)  # seeds 1, 2, 3
SPARE_ROWS = 3
OK, INVALID, MISSING = _abi.A3D_OK, _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD


def _uniform(seed, n):
    """([n, 3] seeded points in the 3 m cube [0.25, 3.25)^3, [n, 3] 'normals'): the recipe of test_gpu_voxel_map.py."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.25, 3.25, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def _transformed(pose_c, points, normals):
    """The oracle's (transform_vectors, transform_normals) of host arrays under a PoseC; None = verbatim."""
    if pose_c is None or len(points) == 0:
        return points, normals
    out_n = np.empty_like(normals)
    O.load().orc_transform_normals(C.byref(pose_c), _abi.ptr(np.ascontiguousarray(normals)), normals.size // 3, _abi.ptr(out_n))
    return O.transform_points(pose_c, points), out_n


class _Model:
    """The expected map by the restatement alone: the rows of everything offered since the last retain (the survivors of
    that retain first), colours beside them."""

    def __init__(self, voxel=VOXEL):
        self.voxel = voxel
        self.p, self.n, self.c = np.empty((0, 3), np.float32), np.empty((0, 3), np.float32), np.empty((0, 3), np.uint8)

    def insert(self, hosts, poses=None):
        for i, (p, n, c) in enumerate(hosts):
            tp, tn = _transformed(None if poses is None else poses[i], p, n)
            self.p, self.n, self.c = np.concatenate([self.p, tp]), np.concatenate([self.n, tn]), np.concatenate([self.c, c])

    def expected(self):
        """(points, normals, colours, index) of the map's extract."""
        p, n, index, _ = V.voxel_downsample_cloud(self.p, self.n, self.voxel)
        return p, n, self.c[index], index

    def retain(self, box=None, min_seq=0):
        """The survivors become the model's only rows; returns the number removed."""
        p, n, c, index = self.expected()
        keep = index >= min_seq
        if box is not None:
            lo, hi = np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)
            keep &= ((p >= lo) & (p <= hi)).all(axis=1)
        self.p, self.n, self.c = p[keep], n[keep], c[keep]
        return int(len(index) - keep.sum())


def _extract(ctx, m, capacity, colors=True, rgb=True):
    """The raw extract into guarded buffers: (status, out_len, points, normals, colours, index bufs)."""
    gp, gn, gi = Guarded(ctx, 12 * capacity), Guarded(ctx, 12 * capacity), Guarded(ctx, 4 * capacity)
    gc = Guarded(ctx, 3 * capacity) if colors else None
    n = C.c_uint64(12345)
    if rgb:
        st = ctx.lib.a3d_voxel_map_extract_rgb(m.handle, gp.ptr, gn.ptr, gc.ptr if gc else None, gi.ptr, capacity, C.byref(n))
    else:
        st = ctx.lib.a3d_voxel_map_extract(m.handle, gp.ptr, gn.ptr, gi.ptr, capacity, C.byref(n))
    return st, int(n.value), gp, gn, gc, gi


def _assert_map_equals(ctx, m, model, label=""):
    exp_p, exp_n, exp_c, exp_i = model.expected()
    cells = len(exp_i)
    assert m.cells() == cells and m.total() == len(model.p), label
    st, n, gp, gn, gc, gi = _extract(ctx, m, cells + SPARE_ROWS)
    assert st == OK and n == cells, label
    check_rows(gp, cells, exp_p, 12, f"{label} points")
    check_rows(gn, cells, exp_n, 12, f"{label} normals")
    check_rows(gc, cells, exp_c, 3, f"{label} colours")
    check_rows(gi, cells, exp_i, 4, f"{label} index")
    return exp_p, exp_n, exp_c, exp_i


@pytest.fixture(scope="module")
def world(ctx):
    """The three seeded clouds with row colours, resident with and without them, and their oracle poses."""
    hosts = [_uniform(seed, n) + (row_colors(j, n),) for j, (seed, n) in enumerate(zip((1, 2, 3), SIZES))]
    rng = np.random.default_rng(17)
    poses = [O.exp_se3((rng.uniform(-1.0, 1.0, size=6) * [0.1, 0.1, 0.1, 0.05, 0.05, 0.05]).astype(np.float32)) for _ in SIZES]
    clouds = [DevicePointCloud(ctx, PointCloud(*h)) for h in hosts]
    bare = [DevicePointCloud(ctx, PointCloud(h[0], h[1])) for h in hosts]
    yield dict(hosts=hosts, poses=poses, transforms=[Transform.from_c(p) for p in poses], clouds=clouds, bare=bare)
    for c in (*clouds, *bare):
        c.free()


def test_replaced_winners_and_a_growth_carry_the_new_winners_colour(ctx, world):
    """The three clouds one per call, each under its pose: cells change hands and the extract shows the new winner's
    colour.  With reserve_cells = 0 the first table already has 8192 slots (2 * 2049 = 4098 > 4096) and 2 * (cells + 65)
    stays below that, so this order never grows the table; the growth (256 -> 8192 slots, the rehash that moves the
    colour plane) is taken from the same clouds inserted in reverse order."""
    hosts, poses, transforms, clouds = world["hosts"], world["poses"], world["transforms"], world["clouds"]
    # the figures of the clouds without a pose, read off the restatement
    bare_first, _ = V.voxel_downsample(hosts[0][0], VOXEL)
    bare_final, _ = V.voxel_downsample(np.concatenate([h[0] for h in hosts]), VOXEL)
    ends = np.cumsum(SIZES)
    winners = [int(((bare_final >= e - n) & (bare_final < e)).sum()) for n, e in zip(SIZES, ends)]
    print(f"without poses: {len(bare_first)} cells after the first cloud, {len(bare_final)} at the end, winners {winners}")
    assert len(bare_first) - winners[0] >= len(bare_first) / 4
    # from the restatement, before the GPU is touched: at least a quarter of the first insert's cells change their winner
    model = _Model()
    model.insert(hosts[:1], poses[:1])
    first = model.expected()[3]
    model.insert(hosts[1:], poses[1:])
    final = model.expected()[3]
    changed = len(first) - int((final < SIZES[0]).sum())
    print(f"{len(first)} cells after the first cloud, {len(final)} at the end, {changed} of the first change hands")
    assert changed >= len(first) / 4
    m = DeviceVoxelMap(ctx, VOXEL, colors=True)
    model = _Model()
    for k in range(3):
        assert m.insert(clouds[k], transforms[k]) == 0
        model.insert(hosts[k:k + 1], poses[k:k + 1])
        _assert_map_equals(ctx, m, model, f"after cloud {k}")
    assert m.stats()["slots"] == 8192
    # the wrapper's extract: a cloud with colours
    got, index = m.extract(return_index=True)
    exp_p, exp_n, exp_c, exp_i = model.expected()
    assert got.has_colors() and np.array_equal(index, exp_i) and np.array_equal(got.download_colors(), exp_c)
    assert np.array_equal(got.download()[0].view(np.uint32), exp_p.view(np.uint32))
    got.free(), m.free()
    # the same clouds, the smallest first: the second insert moves the table, colour plane included
    m = DeviceVoxelMap(ctx, VOXEL, colors=True)
    model = _Model()
    for k in (2, 1, 0):
        assert m.insert(clouds[k], transforms[k]) == 0
        model.insert(hosts[k:k + 1], poses[k:k + 1])
        _assert_map_equals(ctx, m, model, f"reverse order, after cloud {k}")
        if k == 2:
            assert m.stats()["slots"] == 256 and m.stats()["growths"] == 0
    assert m.stats()["growths"] >= 1 and m.stats()["slots"] == 8192
    m.free()


def test_grouping_does_not_change_the_extract(ctx, world):
    hosts, poses, transforms, clouds = world["hosts"], world["poses"], world["transforms"], world["clouds"]
    model = _Model()
    model.insert(hosts, poses)
    one = DeviceVoxelMap(ctx, VOXEL, colors=True)
    assert one.insert_many(clouds, transforms) == [0, 0, 0]
    _assert_map_equals(ctx, one, model, "one call")
    three = DeviceVoxelMap(ctx, VOXEL, colors=True)
    for c, t in zip(clouds, transforms):
        three.insert(c, t)
    _assert_map_equals(ctx, three, model, "three calls")
    halves, half_t = [], []
    for (p, n, c), t in zip(hosts, transforms):
        cut = len(p) // 2
        halves += [DevicePointCloud(ctx, PointCloud(p[:cut], n[:cut], c[:cut])), DevicePointCloud(ctx, PointCloud(p[cut:], n[cut:], c[cut:]))]
        half_t += [t, t]
    six = DeviceVoxelMap(ctx, VOXEL, colors=True)
    for c, t in zip(halves, half_t):
        six.insert(c, t)
    _assert_map_equals(ctx, six, model, "six halves")
    assert six.stats()["growths"] >= 1 and three.stats()["growths"] == 0  # a different size history, the same extract
    for x in (one, three, six, *halves):
        x.free()


@pytest.mark.parametrize("rule", ["box", "min_seq", "compact"])
def test_retain_keeps_the_survivors_colours(ctx, world, rule):
    hosts, poses, transforms, clouds = world["hosts"], world["poses"], world["transforms"], world["clouds"]
    m = DeviceVoxelMap(ctx, VOXEL, colors=True)
    model = _Model()
    m.insert_many(clouds[:2], transforms[:2])
    model.insert(hosts[:2], poses[:2])
    before = _assert_map_equals(ctx, m, model, "before")
    cells = len(before[3])
    if rule == "box":
        box = (np.float32([-10.0, -10.0, -10.0]), np.float32([1.75, 10.0, 10.0]))
        removed = model.retain(box=box)
        assert cells / 3 < removed < 2 * cells / 3  # the box keeps about half
        assert m.retain(box=box) == removed
    elif rule == "min_seq":
        removed = model.retain(min_seq=SIZES[0])  # the second cloud's mark: the cells the first cloud still holds go
        assert 0 < removed < cells
        assert m.retain(min_seq=SIZES[0]) == removed
    else:
        removed = model.retain()
        assert removed == 0 and m.compact() == 0
    exp = _assert_map_equals(ctx, m, model, f"after {rule}")
    k = cells - removed
    assert np.array_equal(exp[3], np.arange(k, dtype=np.uint32)) and m.stats()["cells"] == m.stats()["total"] == k
    # a later insert still follows the contract
    assert m.insert(clouds[2], transforms[2]) == 0
    model.insert(hosts[2:], poses[2:])
    _assert_map_equals(ctx, m, model, f"after {rule} and an insert")
    # clear, then everything again: the first extract
    m.clear()
    assert m.cells() == 0 and m.total() == 0
    again = _Model()
    m.insert_many(clouds[:2], transforms[:2])
    again.insert(hosts[:2], poses[:2])
    got = _assert_map_equals(ctx, m, again, "after clear")
    for a, b in zip(got, before):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m.free()


def test_refusals_on_the_device_path(ctx, world):
    hosts, poses, transforms, clouds, bare = (world[k] for k in ("hosts", "poses", "transforms", "clouds", "bare"))
    m = DeviceVoxelMap(ctx, VOXEL, colors=True)
    model = _Model()
    m.insert(clouds[0], transforms[0])
    model.insert(hosts[:1], poses[:1])
    stats = m.stats()
    # a cloud without colours, alone and behind one that has them: A3D_MISSING_FIELD, nothing from the call is inserted
    for batch in ([bare[1]], [clouds[1], bare[2]]):
        with pytest.raises(A3dError) as e:
            m.insert_many(batch)
        assert e.value.status == MISSING and m.stats() == stats
    views = DevicePointCloud._views([clouds[1]])
    assert ctx.lib.a3d_voxel_map_insert(m.handle, views, None, 1, None, None) == MISSING and m.stats() == stats
    _assert_map_equals(ctx, m, model, "after the refusals")
    # capacity cells - 1: nothing written, the cell count reported
    cells = m.cells()
    st, n, gp, gn, gc, gi = _extract(ctx, m, cells - 1)
    assert st == INVALID and n == cells
    for buf in (gp, gn, gc, gi):
        untouched(buf, "capacity cells - 1")
    # the old extract on a map with colours: points, normals and indices as ever
    st, n, gp, gn, _, gi = _extract(ctx, m, cells + SPARE_ROWS, colors=False, rgb=False)
    exp_p, exp_n, _, exp_i = model.expected()
    assert st == OK and n == cells
    check_rows(gp, cells, exp_p, 12, "old extract points"), check_rows(gn, cells, exp_n, 12, "old extract normals")
    check_rows(gi, cells, exp_i, 4, "old extract index")
    # colours asked of a map without them; such a map ignores the colours it is offered
    plain = DeviceVoxelMap(ctx, VOXEL)
    n_dropped = (C.c_uint64 * 1)()
    views = DevicePointCloud._views([clouds[0]])
    assert ctx.lib.a3d_voxel_map_insert_rgb(plain.handle, views, DevicePointCloud._colors_array([clouds[0]]),
                                            (_abi.PoseC * 1)(transforms[0].to_c()), 1, n_dropped, None) == OK
    st, n, gp, gn, gc, gi = _extract(ctx, plain, cells + SPARE_ROWS)
    assert st == MISSING and n == 12345
    for buf in (gp, gn, gc, gi):
        untouched(buf, "colours of a map without them")
    st, n, gp, gn, _, gi = _extract(ctx, plain, cells + SPARE_ROWS, colors=False)
    assert st == OK and n == cells
    check_rows(gp, cells, exp_p, 12, "plain map points"), check_rows(gn, cells, exp_n, 12, "plain map normals")
    check_rows(gi, cells, exp_i, 4, "plain map index")
    got = plain.extract()
    assert not got.has_colors()
    got.free(), plain.free(), m.free()


def test_the_spatial_index_is_colour_blind(ctx, world):
    transforms, clouds, bare = world["transforms"], world["clouds"], world["bare"]
    coloured, plain = DeviceVoxelMap(ctx, VOXEL, colors=True), DeviceVoxelMap(ctx, VOXEL)
    coloured.insert_many(clouds, transforms), plain.insert_many(bare, transforms)
    assert coloured.stats() == plain.stats()
    rng = np.random.default_rng(23)
    queries = rng.uniform(0.0, 3.5, size=(2049, 3)).astype(np.float32)
    (seq_a, d2_a), (seq_b, d2_b) = coloured.nearest(queries), plain.nearest(queries)
    assert (seq_a != 0xFFFFFFFF).sum() > 1500
    assert np.array_equal(seq_a, seq_b) and np.array_equal(d2_a.view(np.uint32), d2_b.view(np.uint32))
    params = IcpParams.default()
    nudge = Transform.from_c(O.exp_se3(np.asarray([0.01, -0.02, 0.015, 0.01, 0.02, -0.01], np.float32)))
    a = coloured.accumulate(clouds[1], params, nudge * transforms[1])
    b = plain.accumulate(bare[1], params, nudge * transforms[1])
    assert a["count"] == b["count"] > 0
    for key in ("H", "g"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    assert np.float32(a["ssq"]).view(np.uint32) == np.float32(b["ssq"]).view(np.uint32)
    coloured.free(), plain.free()


def test_end_to_end_fixture_frames_keep_their_colours(ctx):
    frames = 4
    ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
    loaded = [ds.get(i) for i in range(frames)]
    cam, _, _, depth_scale = loaded[0]
    built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(
        cam, [(f[1], f[2]) for f in loaded], depth_scale)
    images = [pyramid[0] for pyramid in built]
    clouds = DevicePointCloud.from_range_images(images, colors=True)
    for im in images:
        im.free()
    trajectory = ds.trajectory()
    transforms = [trajectory[i] for i in range(frames)]
    model = _Model(0.02)
    hosts = []
    for i in range(frames):
        fr = oracle_frame("sample1", i)
        keep = fr.mask.reshape(-1) != 0
        hosts.append((fr.points.reshape(-1, 3)[keep], fr.normals.reshape(-1, 3)[keep], loaded[i][2].reshape(-1, 3)[keep]))
    model.insert(hosts, [t.to_c() for t in transforms])
    m = DeviceVoxelMap(ctx, 0.02, colors=True)
    assert m.insert_many(clouds, transforms) == [0] * frames
    got, index = m.extract(return_index=True)
    exp_p, exp_n, exp_c, exp_i = model.expected()
    # a condition on the input, read off the restatement (13 810 cells; 3 690 / 2 991 / 3 281 / 3 848 winners per frame):
    # every frame's colours reach the map, and most offered points lose their cell
    ends = np.cumsum([len(h[0]) for h in hosts])
    per_frame = [int(((exp_i >= e - len(h[0])) & (exp_i < e)).sum()) for h, e in zip(hosts, ends)]
    print(f"{len(exp_i)} cells of {ends[-1]} points, winners per frame {per_frame}")
    assert min(per_frame) > 100 and len(exp_i) < ends[-1] // 4
    assert np.array_equal(index, exp_i)
    assert np.array_equal(got.download_colors(), exp_c)
    assert np.array_equal(got.download()[0].view(np.uint32), exp_p.view(np.uint32))
    got.free(), m.free()
    for c in clouds:
        c.free()
