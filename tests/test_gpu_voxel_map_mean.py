"""The voxel map of cell means (a3d_voxel_map_new_mean, DeviceVoxelMap(mode="mean")) on the GPU.

The contract under test: after any sequence of inserts, extract(return_index=True, return_counts=True) equals
voxel_mean (voxel_mean_restatement.py) of the merged input, the concatenation of the ORACLE-transformed host clouds in
insertion order: points, normals, colours, representative indices and counts, however the inserts were grouped and
whatever the table's size history was.  Retains are held to voxel_map_mean_restatement.retained_mean / continued_mean,
the readers to MeanMapRestatement.  Every bit-for-bit comparison is on uint32 views; the tolerances of the accumulate and
align comparisons are those of test_gpu_voxel_map_icp.py for the same comparisons (gn_rel_err < 1e-6; 1e-4 rad, 1e-4 m)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import voxel_map_icp_restatement as R
import voxel_mean_cases as cases
import voxel_restatement as V
from align3d_amd import (CameraIntrinsics, Context, DevicePointCloud, DeviceVoxelMap, IcpParams, InvalidParameter, PointCloud,
                         Transform, _abi)
from gpu_util import gn_rel_err, small_pose, transform_diff
from voxel_map_mean_restatement import MeanMapRestatement, continued_mean, retained_mean
from voxel_mean_restatement import voxel_mean

pytestmark = pytest.mark.gpu

VOXEL = 0.05
ORIGIN = (0.013, -0.4, 0.021)
SIZES = (1, 63, 64, 65, 1024, 1025, 4097)
TWISTS = ([0.05, -0.03, 0.02, 0.03, -0.02, 0.01], [-0.04, 0.01, 0.06, -0.01, 0.025, 0.03], [0.01, 0.07, -0.05, 0.02, 0.02, -0.03])
SCENE_VOXEL = 0.03  # of the readers' map: a few thousand cells
FIELDS = ((True, True), (False, False), (True, False), (False, True))  # (normals, colours) of the map


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cloud(seed, n, sort=False):
    """(points, normals, colors) of n points: six tenths uniform in a 0.4 m cube (a few points per cell), three tenths in
    ONE cell (hundreds at the larger sizes), the rest spread over 3 m (mostly alone in their cells).  sort: by cell, so
    that the runs of a wave are long."""
    rng = np.random.default_rng([seed, n])
    a, b = (6 * n) // 10, (3 * n) // 10
    points = np.concatenate([rng.uniform(0.0, 0.4, size=(a, 3)), 0.625 + 0.004 * rng.normal(size=(b, 3)),
                             rng.uniform(-1.5, 1.5, size=(n - a - b, 3))]).astype(np.float32)
    order = rng.permutation(n)
    if sort:
        order = np.lexsort(np.floor(points / np.float32(VOXEL)).T)
    normals = rng.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(np.float32)
    return points[order], normals[order], rng.integers(0, 256, size=(n, 3), dtype=np.uint8)[order]


def _transformed(pose, points, normals):
    if pose is None or len(points) == 0:
        return points, normals
    return O.transform_points(pose, points), None if normals is None else R.transform_normals(pose, normals)


def _merged(hosts, poses):
    """The merged input of [(points, normals, colors)] under [PoseC or None], through the oracle, and each cloud's
    dropped count."""
    parts = [_transformed(None if poses is None else poses[i], p, n) + (c,) for i, (p, n, c) in enumerate(hosts)]
    dropped = [int((~_kept(p)).sum()) for p, _, _ in parts]
    return tuple(np.concatenate([part[k] for part in parts]) for k in range(3)), dropped


def _kept(points):
    return V.voxel_keys(points, VOXEL, ORIGIN)[0]


def _dev(ctx, points, normals, colors, fields=(True, True)):
    return DevicePointCloud(ctx, PointCloud(points, normals if fields[0] else None, colors if fields[1] else None))


def _new_map(ctx, fields=(True, True), voxel=VOXEL, origin=ORIGIN, **kw):
    return DeviceVoxelMap(ctx, voxel, origin=origin, normals=fields[0], colors=fields[1], mode="mean", **kw)


def _insert(ctx, m, hosts, poses=None, how="one", fields=(True, True)):
    """Inserts the host clouds, grouped into calls by `how`; returns the dropped counts per cloud."""
    clouds = [_dev(ctx, *h, fields=fields) for h in hosts]
    transforms = None if poses is None else [Transform.from_c(T) for T in poses]
    step = {"one": len(clouds), "each": 1, "pairs": 2}[how]
    dropped = []
    for at in range(0, len(clouds), step):
        dropped += m.insert_many(clouds[at:at + step], None if transforms is None else transforms[at:at + step])
    for c in clouds:
        c.free()
    return dropped


def _extract(m):
    """(points bits, normals bits or None, colours or None, index, counts) of the map."""
    cloud, index, counts = m.extract(return_index=True, return_counts=True)
    points, normals = cloud.download()
    colors = cloud.download_colors() if cloud.has_colors() else None
    cloud.free()
    assert index.dtype == counts.dtype == np.uint32 and len(points) == len(index) == len(counts) == m.cells()
    return _bits(points), None if normals is None else _bits(normals), colors, index, counts


def _assert_extract(got, want, fields=(True, True), what=""):
    """`got` of _extract against (points, normals, colors, index, counts, ...) of the restatement."""
    assert np.array_equal(got[3], want[3]), (what, "index")
    assert np.array_equal(got[4], want[4]), (what, "counts")
    assert np.array_equal(got[0], _bits(want[0])), (what, "points", np.flatnonzero((got[0] != _bits(want[0])).any(axis=1))[:5])
    assert (got[1] is None) == (not fields[0]) and (got[2] is None) == (not fields[1]), what
    if fields[0]:
        assert np.array_equal(got[1], _bits(want[1])), (what, "normals", np.flatnonzero((got[1] != _bits(want[1])).any(axis=1))[:5])
    if fields[1]:
        assert np.array_equal(got[2], want[2]), (what, "colours")


# ---- 1. the contract --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def frames():
    """The seven clouds, their poses, the merged input and its mean for every kind of map, once."""
    hosts = [_cloud(20 + i, n, sort=i % 2 == 1) for i, n in enumerate(SIZES)]
    hosts[3][0][7] = (np.nan, 0.1, 0.1)  # dropped points that consume sequence numbers
    hosts[5][0][1000] = (0.1, np.inf, 0.1)
    hosts[6][0][[5, 4000]] = (1e9, 0.0, 0.0)
    poses = [O.exp_se3(TWISTS[i % 3]) for i in range(len(hosts))]
    merged, dropped = _merged(hosts, poses)
    assert dropped == [0, 0, 0, 1, 0, 1, 2]
    want = {f: voxel_mean(merged[0], merged[1] if f[0] else None, merged[2] if f[1] else None, VOXEL, ORIGIN) for f in FIELDS}
    counts = want[(True, True)][4]
    assert (counts == 1).sum() > 100 and counts.max() > 300 and ((counts > 1) & (counts < 20)).sum() > 100
    return hosts, poses, want, dropped


@pytest.mark.parametrize("how", ["one", "each", "pairs"])
@pytest.mark.parametrize("fields", FIELDS, ids=lambda f: f"normals={f[0]},colours={f[1]}")
def test_extract_is_the_mean_of_the_merged_input(ctx, frames, fields, how):
    hosts, poses, want, dropped = frames
    runs = []
    for run in range(2):
        m = _new_map(ctx, fields)
        assert _insert(ctx, m, hosts, poses, how, fields) == dropped
        s = m.stats()
        assert s["total"] == sum(SIZES) and s["dropped_total"] == sum(dropped) and s["mode"] == "mean"
        assert s["bytes_per_slot"] == 64 + (36 if fields[0] else 0) + (28 if fields[1] else 0)
        runs.append(_extract(m))
        _assert_extract(runs[-1], want[fields], fields, (how, run))
        m.free()
    for a, b in zip(*runs):  # two runs give the same bits
        assert (a is None and b is None) or np.array_equal(a, b)


def test_a_short_capacity_writes_nothing(ctx, frames):
    hosts, poses, want, _ = frames
    m = _new_map(ctx)
    _insert(ctx, m, hosts[:5], poses[:5])
    cells = m.cells()
    words = ctx.to_device(np.full(4 * cells, 0xC0FFEE11, np.uint32))  # points, then counts
    n = C.c_uint64()
    st = ctx.lib.a3d_voxel_map_extract_mean(m.handle, words, None, None, None, C.c_void_p(words.value + 12 * cells),
                                            cells - 1, C.byref(n))
    assert st == _abi.A3D_INVALID_PARAMETER and n.value == cells > 100
    assert (ctx.to_host(words, np.empty(4 * cells, np.uint32)) == 0xC0FFEE11).all()
    ctx.free(words)
    m.free()


# ---- 2. cells across calls --------------------------------------------------------------------------------------------


def _two_inserts(ctx, first, second, voxel=VOXEL, origin=ORIGIN):
    """A map after `first` and then `second` (points, normals, colors) went in as two calls: (extract after the first,
    extract after the second, dropped of both)."""
    m = _new_map(ctx, voxel=voxel, origin=origin)
    dropped = _insert(ctx, m, [first]) if len(first[0]) else [0]
    after_first = _extract(m)
    dropped += _insert(ctx, m, [second])
    after_second = _extract(m)
    m.free()
    return after_first, after_second, dropped


def test_a_lone_row_is_kept_bit_for_bit_until_a_second_point_comes(ctx):
    rng = np.random.default_rng(3)
    # cells 0 ... 39 along x get one point each in the first call; the even ones a second point in the second call
    cell = np.stack([np.arange(40), np.zeros(40), np.zeros(40)], axis=1)
    first_p = ((cell + rng.uniform(0.1, 0.85, size=(40, 3))) * VOXEL).astype(np.float32) + np.float32(ORIGIN)
    second_p = first_p[::2] + np.float32(0.0011)
    # (normals that the sums would not count or would change: a lone row keeps them as they are)
    first = (first_p, rng.normal(size=(40, 3)).astype(np.float32) * 3, rng.integers(0, 256, (40, 3), dtype=np.uint8))
    first[1][5] = (np.nan, 0.0, 1.0)
    second = (second_p, rng.normal(size=(20, 3)).astype(np.float32), rng.integers(0, 256, (20, 3), dtype=np.uint8))
    a, b, dropped = _two_inserts(ctx, first, second)
    assert dropped == [0, 0]
    assert np.array_equal(a[0], _bits(first[0])) and np.array_equal(a[1], _bits(first[1])) and np.array_equal(a[2], first[2])
    assert np.array_equal(a[3], np.arange(40)) and (a[4] == 1).all()
    want = voxel_mean(*(np.concatenate([x, y]) for x, y in zip(first, second)), VOXEL, ORIGIN)
    assert np.array_equal(want[4], np.tile([2, 1], 20))
    _assert_extract(b, want, what="after the second call")
    assert np.array_equal(b[0][1::2], a[0][1::2]) and not (b[0][::2] == a[0][::2]).all(axis=1).any()


def test_one_cell_takes_a_whole_call(ctx):
    rng = np.random.default_rng(4)
    centre = (np.float32([20, -3, 2]) + np.float32(0.5)) * np.float32(VOXEL) + np.float32(ORIGIN)
    n = 4097  # every run of every wave has 64 lanes: the greatest contention on one slot
    second = ((centre + rng.uniform(-0.45, 0.45, size=(n, 3)) * VOXEL).astype(np.float32),) + _cloud(1, n)[1:]
    first = _cloud(2, 65)
    a, b, _ = _two_inserts(ctx, first, second)
    want = voxel_mean(*(np.concatenate([x, y]) for x, y in zip(first, second)), VOXEL, ORIGIN)
    assert want[4].max() == n and want[3][np.argmax(want[4])] == 65
    _assert_extract(b, want)


def test_two_cells_alternate_lane_by_lane(ctx):
    rng = np.random.default_rng(5)
    n = 1025  # every run has length 1
    cell = np.where((np.arange(n) % 2 == 0)[:, None], np.float32([1, 1, 1]), np.float32([-4, 2, 0]))
    points = ((cell + rng.uniform(0.05, 0.95, size=(n, 3))) * VOXEL).astype(np.float32) + np.float32(ORIGIN)
    cloud = (points,) + _cloud(6, n)[1:]
    a, b, _ = _two_inserts(ctx, tuple(x[:300] for x in cloud), tuple(x[300:] for x in cloud))
    want = voxel_mean(*cloud, VOXEL, ORIGIN)
    assert want[4].tolist() == [513, 512] and want[3].tolist() == [0, 1]
    _assert_extract(a, voxel_mean(*(x[:300] for x in cloud), VOXEL, ORIGIN))
    _assert_extract(b, want)


@pytest.mark.parametrize("case", cases.edge_arithmetic(), ids=lambda c: c["name"])
def test_tie_cases_split_over_two_inserts(ctx, case):
    cloud = (case["points"], case["normals"], case["colors"])
    want = voxel_mean(*cloud, case["voxel"], case["origin"])
    assert (want[4] > 1).any()
    for cut in (len(cloud[0]) // 2, 1):
        a, b, dropped = _two_inserts(ctx, tuple(x[:cut] for x in cloud), tuple(x[cut:] for x in cloud), case["voxel"], case["origin"])
        assert sum(dropped) == want[5]
        _assert_extract(b, want, what=(case["name"], cut))


# ---- 3. growth --------------------------------------------------------------------------------------------------------


def test_growth_moves_the_sums(ctx, frames):
    hosts, poses, want, dropped = frames
    grown, reserved = _new_map(ctx, reserve_cells=0), _new_map(ctx, reserve_cells=1 << 16)
    assert _insert(ctx, grown, hosts, poses, "each") == dropped == _insert(ctx, reserved, hosts, poses, "each")
    assert grown.stats()["growths"] >= 3 and reserved.stats()["growths"] == 0
    assert reserved.stats()["slots"] == 1 << 17 > grown.stats()["slots"]
    a, b = _extract(grown), _extract(reserved)
    _assert_extract(a, want[(True, True)], what="grown")
    _assert_extract(b, want[(True, True)], what="reserved")
    grown.free(), reserved.free()


def test_the_uncombined_pass_a_of_the_diagnostics_build_gives_the_same_bits(frames, monkeypatch):
    """The diagnostics library holds pass A without run combining (A3D_VOXEL_MAP_MEAN_NO_COMBINE=1, read by every insert;
    the probe times it): every lane sends its own atomics.  The sums are integers, so the bits are the same."""
    assert b"A3D_VOXEL_MAP_MEAN_NO_COMBINE" in open(_abi.DIAG_LIB_PATH, "rb").read()
    assert b"A3D_VOXEL_MAP_MEAN_NO_COMBINE" not in open(_abi.LIB_PATH, "rb").read()
    hosts, poses, want, dropped = frames
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    for form in ("0", "1"):
        monkeypatch.setenv("A3D_VOXEL_MAP_MEAN_NO_COMBINE", form)
        m = _new_map(diag)
        assert _insert(diag, m, hosts, poses, "pairs") == dropped
        _assert_extract(_extract(m), want[(True, True)], what=form)
        m.free()
    monkeypatch.delenv("A3D_VOXEL_MAP_MEAN_NO_COMBINE")
    diag.close()


# ---- 4. hostile rows --------------------------------------------------------------------------------------------------


def test_hostile_points_and_normals(ctx):
    rng = np.random.default_rng(8)
    n = 2049
    points, normals, colors = _cloud(9, n)
    raw = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    hostile = rng.permutation(n)[:400]
    points[hostile[:200]] = raw[hostile[:200]]  # NaNs with payloads, infinities, magnitudes far beyond the cell range
    points[hostile[200:206]] = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e9, 0, 0], [0, -1e9, 0], [3e38, 3e38, 3e38]])
    bad = rng.permutation(n)[:600]  # normals that are not counted, many of them in the crowded cell
    normals[bad[:150]] = raw[bad[:150]]
    normals[bad[150:300], 0] = np.nan
    normals[bad[300:400], 1] = np.inf
    normals[bad[400:500], 2] = -np.inf
    normals[bad[500:550]] *= np.float32(2.5)
    normals[bad[550:600], 0] = np.float32(2.0000002)
    normals[bad[590:600], 0] = np.float32(2.0)  # counted: the bound is closed
    want = voxel_mean(points, normals, colors, VOXEL, ORIGIN)
    assert want[5] > 150 and want[4].max() > 300
    for cut in (0, 1000):
        m = _new_map(ctx)
        parts = [tuple(x[:cut] for x in (points, normals, colors)), tuple(x[cut:] for x in (points, normals, colors))]
        parts = [p for p in parts if len(p[0])]
        dropped = _insert(ctx, m, parts, None, "each")
        assert dropped == [int((~_kept(p[0])).sum()) for p in parts] and sum(dropped) == want[5]
        assert m.total() == n and m.stats()["dropped_total"] == want[5]
        _assert_extract(_extract(m), want, what=cut)
        m.free()


# ---- 5. retain and compact --------------------------------------------------------------------------------------------


def test_retain_keeps_rows_sums_and_counts(ctx, frames):
    hosts, poses, _, _ = frames
    hosts, poses = hosts[3:], poses[3:]  # 65, 1024, 1025, 4097 points
    merged, _ = _merged(hosts, poses)
    model = MeanMapRestatement(*merged, VOXEL, ORIGIN)
    extra = _cloud(77, 1500)
    for what in ("box, min_seq, marks", "compact"):
        m = _new_map(ctx, reserve_cells=0)
        marks = [0]
        for h, T in zip(hosts, poses):
            _insert(ctx, m, [h], [T])
            marks.append(m.total())
        assert marks[-1] == len(merged[0])
        if what == "compact":
            keep, removed, new_marks, k, continued = retained_mean(model)
            assert m.compact() == removed == 0
        else:
            lo, hi = np.float32([-0.2, -0.6, -0.2]), np.float32([0.7, 0.5, 0.45])
            keep, removed, new_marks, k, continued = retained_mean(model, marks[2], (lo, hi), marks + [1 << 40])
            got_removed, got_marks = m.retain(box=(lo, hi), min_seq=marks[2], marks=np.asarray(marks + [1 << 40], np.uint64))
            assert got_removed == removed and got_marks.tolist() == new_marks
            assert 100 < k < len(model.rows) - 100 and (model.counts[keep] > 1).sum() > 20
        s = m.stats()
        assert s["cells"] == s["total"] == k and s["dropped_total"] == 0
        want = (model.rows[keep], model.normals[keep], model.colors[keep], np.arange(k, dtype=np.uint32), model.counts[keep])
        _assert_extract(_extract(m), want, what=what)
        # one more cloud: it hits surviving cells, removed cells and new ones, and the sums go on
        assert _insert(ctx, m, [extra]) == [0]
        want = continued_mean(continued, k, *extra, VOXEL, ORIGIN)
        grew = want[4][:k] > model.counts[keep]
        assert grew.any() and not grew.all() and len(want[3]) > k and m.total() == k + len(extra[0])
        _assert_extract(_extract(m), want, what=what + ", then an insert")
        m.clear()
        assert m.stats()["cells"] == 0 and _insert(ctx, m, [extra]) == [0]  # clear zeroes the sums
        _assert_extract(_extract(m), voxel_mean(*extra, VOXEL, ORIGIN), what=what + ", cleared")
        m.free()


# ---- 6. the readers ---------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def scene(ctx):
    """A map of means of a few thousand cells over three surfaces, its restatement, and a source a small pose away."""
    world_p, world_n = R.surfaces(1, 24000)
    colors = np.random.default_rng(2).integers(0, 256, size=(len(world_p), 3), dtype=np.uint8)
    poses = [O.exp_se3(u) for u in TWISTS]
    inverse = []
    for T in poses:
        inv = _abi.PoseC()
        O.load().orc_inverse(C.byref(T), C.byref(inv))
        inverse.append(inv)
    hosts = [_transformed(inv, world_p[k::3], world_n[k::3]) + (colors[k::3],) for k, inv in enumerate(inverse)]
    merged, _ = _merged(hosts, poses)
    model = MeanMapRestatement(*merged, SCENE_VOXEL, ORIGIN)
    m = _new_map(ctx, voxel=SCENE_VOXEL)
    assert _insert(ctx, m, hosts, poses, "each") == [0, 0, 0]
    assert m.cells() == len(model.rows) > 3000 and (model.counts > 1).sum() > 2000
    offset = small_pose(7, rot=0.01, trans=0.01).to_c()
    inv = _abi.PoseC()
    O.load().orc_inverse(C.byref(offset), C.byref(inv))
    src_p, src_n = _transformed(inv, *R.surfaces(5, 3000, noise=0.002))
    src = DevicePointCloud(ctx, PointCloud(src_p, src_n))
    yield m, model, src, src_p, src_n
    src.free(), m.free()


def test_nearest_reads_the_mean_rows(scene):
    m, model, src, src_p, _ = scene
    want = model.nearest(src_p)
    assert (want[2] >= 0).sum() > 0.9 * len(src_p)
    for got in (m.nearest(src), m.nearest(src_p)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_accumulate_and_align_read_the_mean_rows(scene):
    m, model, src, src_p, src_n = scene
    prm = IcpParams(max_iterations=5)
    for T in (Transform.eye(), small_pose(2)):
        ref = model.accumulate(src_p, src_n, T.to_c(), prm.to_c())
        gpu = m.accumulate(src, prm, T)
        eh, eg, es = gn_rel_err(gpu, ref)
        print(f"accumulate: count {gpu['count']} / {ref['count']}, rel err H {eh:.3g} g {eg:.3g} ssq {es:.3g}")
        assert gpu["count"] == ref["count"] > 1000
        assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (eh, eg, es)
    status, want = model.align(src_p, src_n, prm.to_c())
    ang, tr = transform_diff(m.align(src, prm), want)
    print(f"align: d_angle {ang:.3g} rad, d_trans {tr:.3g} m")
    assert status == _abi.A3D_OK and ang <= 1e-4 and tr <= 1e-4, (ang, tr)


def test_render_equals_extract_then_render(scene):
    m = scene[0]
    cam = CameraIntrinsics(140.0, 140.0, 80.0, 60.0, 160, 120)
    pose = Transform((0.7, 0.7, -2.0), (0.0, 0.0, 0.0, 1.0))
    cloud = m.extract()
    for radius in (0.0, 0.025):
        planes = []
        for source in (m, cloud):
            image, index = source.render(cam, pose, radius, return_index=True)
            host = image.download(normals=True, intensity=False, colors=True)
            image.free()
            planes.append((host.mask, index, _bits(host.points), _bits(host.normals), host.colors))
        assert planes[0][0].sum() > 500
        for a, b in zip(*planes):
            assert np.array_equal(a, b)
    cloud.free()


# ---- 7. the interface -------------------------------------------------------------------------------------------------


def test_modes_side_by_side(ctx, frames):
    import voxel_restatement as V

    hosts, poses, want, dropped = frames
    with pytest.raises(InvalidParameter):
        DeviceVoxelMap(ctx, VOXEL, mode="median")
    nearest, mean = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, colors=True), _new_map(ctx)
    clouds = [_dev(ctx, *h) for h in hosts]
    transforms = [Transform.from_c(T) for T in poses]
    assert nearest.insert_many(clouds, transforms) == dropped == mean.insert_many(clouds, transforms)
    with pytest.raises(InvalidParameter):
        nearest.extract(return_counts=True)
    assert set(nearest.stats()) == {"cells", "slots", "total", "dropped_total", "growths"} and nearest.mode == "nearest"
    merged, _ = _merged(hosts, poses)
    exp_p, exp_n, exp_i, _ = V.voxel_downsample_cloud(merged[0], merged[1], VOXEL, ORIGIN)
    cloud, index = nearest.extract(return_index=True)
    got_p, got_n = cloud.download()
    assert np.array_equal(index, exp_i) and np.array_equal(_bits(got_p), _bits(exp_p)) and np.array_equal(_bits(got_n), _bits(exp_n))
    assert np.array_equal(cloud.download_colors(), merged[2][exp_i])
    _assert_extract(_extract(mean), want[(True, True)])
    assert nearest.cells() == mean.cells()
    cloud.free(), nearest.free(), mean.free()
    for c in clouds:
        c.free()
