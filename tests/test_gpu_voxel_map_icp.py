"""Aligning against the voxel map on the GPU: DeviceVoxelMap.nearest / accumulate / align (a3d_voxel_map_nearest_device,
a3d_voxel_map_icp_*).

Every expected value comes from voxel_map_icp_restatement.py: the association in numpy f32 over the dict of cells of
voxel_downsample_cloud(merged input), one iteration from the oracle's bricks, the loop of pcl_icp.rs.  `nearest` is
compared bit for bit (seq, and d2 on uint32 views); an accumulation by count and by gn_rel_err < 1e-6 against sums taken
in f64 (the bound and the form of test_gpu_pcl_icp.py for the same engine); a pose within 1e-4 rad and 1e-4 m of the
restatement's end-to-end run (the project's bound for Icp).  The scene: 3 000 points with normals on a floor, a wall and
a sphere cap, inserted as three clouds under three poses at v = 0.05; the sources are prefixes of 5 000 other points on
the same surfaces, moved by a small pose."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import voxel_map_icp_restatement as R
from align3d_amd import A3dError, DevicePointCloud, DeviceVoxelMap, IcpParams, PointCloud, Transform, _abi
from gpu_util import gn_rel_err, small_pose, transform_diff

pytestmark = pytest.mark.gpu

VOXEL = 0.05
ORIGIN = (0.013, -0.4, 0.021)
SOURCE_LENS = (1, 63, 64, 65, 257, 1025, 5000)
NONE = R.NONE_SEQ


def _inverse(pose):
    out = _abi.PoseC()
    O.load().orc_inverse(C.byref(pose), C.byref(out))
    return out


def _moved(pose, points, normals):
    return O.transform_points(pose, points), R.transform_normals(pose, normals)


def _dev(ctx, points, normals=None):
    return DevicePointCloud(ctx, PointCloud(points, normals))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_nearest(got, want, what=""):
    seq, d2 = got
    assert seq.dtype == np.uint32 and d2.dtype == np.float32
    assert np.array_equal(seq, want[0]), (what, np.flatnonzero(seq != want[0])[:5])
    assert np.array_equal(_bits(d2), _bits(want[1])), what


class _Scene:
    """The clouds of the map (in their own frames), their poses, the merged input and its restatement; the source."""

    def __init__(self):
        world_p, world_n = R.surfaces(1, 3000)
        self.poses = [O.exp_se3(u) for u in ([0.5, -0.3, 0.2, 0.3, -0.2, 0.1], [-0.4, 0.1, 0.6, -0.1, 0.25, 0.3],
                                            [0.1, 0.7, -0.5, 0.2, 0.2, -0.3])]
        self.hosts = [_moved(_inverse(T), world_p[k::3], world_n[k::3]) for k, T in enumerate(self.poses)]
        merged = [_moved(T, p, n) for T, (p, n) in zip(self.poses, self.hosts)]
        self.merged_p, self.merged_n = np.concatenate([m[0] for m in merged]), np.concatenate([m[1] for m in merged])
        self.model = R.MapRestatement(self.merged_p, self.merged_n, VOXEL, ORIGIN)
        # the source: other points of the same surfaces, seen from a frame a small pose away
        self.offset = small_pose(7, rot=0.01, trans=0.01).to_c()
        self.src_p, self.src_n = _moved(_inverse(self.offset), *R.surfaces(5, SOURCE_LENS[-1], noise=0.002))
        self._cache = {}

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def new_map(self, ctx, how="one call", **kw):
        m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, **kw)
        clouds = [_dev(ctx, p, n) for p, n in self.hosts]
        transforms = [Transform.from_c(T) for T in self.poses]
        if how == "one call":
            assert m.insert_many(clouds, transforms) == [0, 0, 0]
        else:
            assert [m.insert(c, t) for c, t in zip(clouds, transforms)] == [0, 0, 0]
        for c in clouds:
            c.free()
        return m


@pytest.fixture(scope="module")
def scene():
    return _Scene()


@pytest.fixture(scope="module")
def vmap(ctx, scene):
    m = scene.new_map(ctx)
    assert m.cells() == len(scene.model.rows) > 1000
    yield m
    m.free()


@pytest.fixture(scope="module")
def source(ctx, scene):
    """The resident sources: a prefix of the 5 000 points per length."""
    clouds = {m: _dev(ctx, scene.src_p[:m], scene.src_n[:m]) for m in SOURCE_LENS}
    yield clouds
    for c in clouds.values():
        c.free()


# ---- nearest ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", SOURCE_LENS)
def test_nearest_is_the_restatement_bit_for_bit(scene, vmap, source, m):
    want = scene.cached(("nearest", m), lambda: scene.model.nearest(scene.src_p[:m]))
    assert (want[2] >= 0).sum() >= min(m, 1) and (m < 1000 or (want[2] >= 0).sum() > 0.9 * m)
    _assert_nearest(vmap.nearest(source[m]), want, "resident queries")
    _assert_nearest(vmap.nearest(scene.src_p[:m]), want, "host queries")
    pose = O.exp_se3([0.02, -0.03, 0.01, 0.01, 0.02, -0.015])
    want = scene.model.nearest(scene.src_p[:m], pose)
    _assert_nearest(vmap.nearest(source[m], Transform.from_c(pose)), want, "under a pose")


def test_nearest_of_queries_that_the_map_would_drop_or_cannot_reach(scene, vmap):
    q = np.asarray([[np.nan, 0.5, 0.0], [0.5, np.inf, 0.0], [0.5, 0.5, -np.inf], [1e9, 0.5, 0.0], [0.5, -1e9, 0.0],
                    [3.0, 3.0, 3.0], [0.5, 0.5, 0.0], [0.0, 0.7, 0.5]], np.float32)
    want = scene.model.nearest(q)
    assert want[0][:6].tolist() == [NONE] * 6 and np.isposinf(want[1][:6]).all() and (want[2][6:] >= 0).all()
    _assert_nearest(vmap.nearest(q), want)
    # a pose that sends every query out of range, and one that brings a far query back
    far = O.pose(t=(4.0e6, 0.0, 0.0))
    got = vmap.nearest(q, Transform.from_c(far))
    assert got[0].tolist() == [NONE] * len(q) and np.isposinf(got[1]).all()
    back = O.pose(t=(-2.5, -2.5, -3.0))
    _assert_nearest(vmap.nearest(q, Transform.from_c(back)), scene.model.nearest(q, back))


def test_nearest_in_a_minimum_table_near_half_full(ctx, scene):
    """31 points in 31 cells go into the 64 slots of the smallest table: probe chains meet, and those that reach the
    last slot wrap around to slot 0.  That they do is checked on the host with the table's own hash: which slots are
    occupied does not depend on who claimed first, so the walk for a key the map does not hold is known exactly."""
    p, n = scene.model.rows[::43][:31], scene.model.normals[::43][:31]  # rows of the map: one per cell
    model = R.MapRestatement(p, n, VOXEL, ORIGIN)
    assert len(model.rows) == 31
    cloud = _dev(ctx, p, n)
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN)
    assert m.insert(cloud) == 0 and m.stats()["slots"] == 64 and m.cells() == 31
    rng = np.random.default_rng(11)
    q = (p[rng.integers(0, 31, size=600)] + rng.uniform(-0.07, 0.07, size=(600, 3))).astype(np.float32)
    want = model.nearest(q)
    assert 100 < (want[2] >= 0).sum() < 600
    # the probes these queries make for absent cells: some run through several occupied slots, some past slot 63
    occupied = R.occupied_slots(model.cells, 64)
    cell = np.floor((q - model.origin) / model.voxel).astype(np.int64) + R.LIM
    asked = {int(k) for d in R.DELTAS for k in ((cell[:, 0] + d[0]) << 42 | (cell[:, 1] + d[1]) << 21 | (cell[:, 2] + d[2])).tolist()}
    walks = [R.absent_probe(k, occupied, 64) for k in asked if k not in model.cells]
    assert len(occupied) == 31 and max(w[0] for w in walks) > 4 and sum(w[1] for w in walks) > 10
    _assert_nearest(m.nearest(q), want)
    m.free(), cloud.free()


def test_nearest_after_forced_growth_after_retain_on_an_empty_and_on_a_cleared_map(ctx, scene):
    q = scene.src_p[:1025]
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, reserve_cells=0)
    got = m.nearest(q)  # no table yet
    assert got[0].tolist() == [NONE] * len(q) and np.isposinf(got[1]).all()
    step = 100
    for a in range(0, len(scene.merged_p), step):  # frame by frame from the smallest table
        c = _dev(ctx, scene.merged_p[a:a + step], scene.merged_n[a:a + step])
        assert m.insert(c) == 0
        c.free()
    assert m.stats()["growths"] >= 4 and m.cells() == len(scene.model.rows)
    _assert_nearest(m.nearest(q), scene.model.nearest(q), "after growth")
    # retain with a box: the survivors in the new numbering
    lo, hi = np.float32([-0.1, 0.2, -0.1]), np.float32([1.0, 1.2, 0.6])
    keep = ((scene.model.rows >= lo) & (scene.model.rows <= hi)).all(axis=1)
    assert 100 < keep.sum() < len(keep) - 100
    assert m.retain(box=(lo, hi)) == (~keep).sum()
    kept = R.MapRestatement(scene.model.rows[keep], scene.model.normals[keep], VOXEL, ORIGIN)
    want = kept.nearest(q)
    assert np.array_equal(kept.seq, np.arange(keep.sum())) and 0 < (want[2] >= 0).sum() < len(q)
    _assert_nearest(m.nearest(q), want, "after retain")
    m.clear()
    got = m.nearest(q)  # a table of empty slots
    assert got[0].tolist() == [NONE] * len(q) and np.isposinf(got[1]).all()
    m.free()


@pytest.mark.parametrize("axis,end,query,trap,fair", R.borrow_cases())
def test_nearest_skips_a_neighbour_per_axis_before_the_key_is_packed(ctx, axis, end, query, trap, fair):
    q = np.asarray([query], np.float32)
    up = np.asarray([[0.0, 0.0, 1.0]], np.float32)
    if trap is not None:  # only the cell that a borrowed / carried key would name is occupied: nothing is found
        m = DeviceVoxelMap(ctx, 1.0)
        c = _dev(ctx, np.asarray([trap], np.float32), up)
        assert m.insert(c) == 0 and m.cells() == 1
        got = m.nearest(q)
        assert got[0].tolist() == [NONE] and np.isposinf(got[1]).all()
        m.free(), c.free()
    rows = np.asarray([fair] if trap is None else [trap, fair], np.float32)
    m = DeviceVoxelMap(ctx, 1.0)
    c = _dev(ctx, rows, np.repeat(up, len(rows), axis=0))
    assert m.insert(c) == 0 and m.cells() == len(rows)
    _assert_nearest(m.nearest(q), R.MapRestatement(rows, np.repeat(up, len(rows), axis=0), 1.0).nearest(q))
    got = m.nearest(q)
    assert got[0].tolist() == [len(rows) - 1] and got[1].tolist() == [1.0]
    m.free(), c.free()


# ---- independence of history --------------------------------------------------------------------------------------------


def test_rows_and_pose_do_not_depend_on_how_the_map_was_filled(ctx, scene, vmap, source):
    prm = IcpParams(max_iterations=5)
    q = source[5000]
    first_rows, first_pose = vmap.nearest(q), vmap.align(q, prm)
    _assert_nearest(first_rows, scene.cached(("nearest", 5000), lambda: scene.model.nearest(scene.src_p)))
    for how, kw in (("frame by frame", {}), ("one call", {"reserve_cells": 1 << 16})):
        m = scene.new_map(ctx, how, **kw)
        assert m.stats()["slots"] != vmap.stats()["slots"] or how == "frame by frame"
        _assert_nearest(m.nearest(q), first_rows, how)
        assert bytes(m.align(q, prm).to_c()) == bytes(first_pose.to_c()), how
        # compaction: the same rows under their ranks, the same pose bits
        assert m.compact() == 0 and m.total() == m.cells()
        renumbered = scene.cached("renumbered", scene.model.renumbered)
        want = scene.cached("nearest renumbered", lambda: renumbered.nearest(scene.src_p))
        assert np.array_equal(renumbered.seq, np.arange(len(scene.model.rows)))
        _assert_nearest(m.nearest(q), want, how + ", after compact")
        assert np.array_equal(want[2], scene.cached(("nearest", 5000), None)[2])  # the same rows as before
        assert bytes(m.align(q, prm).to_c()) == bytes(first_pose.to_c()), how + ", after compact"
        m.free()


# ---- accumulate -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", SOURCE_LENS)
def test_accumulate_is_the_restatements_iteration(scene, vmap, source, m):
    prm = IcpParams(max_iterations=5)
    for name, T in (("eye", Transform.eye()), ("small pose", small_pose(2))):
        ref = scene.model.accumulate(scene.src_p[:m], scene.src_n[:m], T.to_c(), prm.to_c())
        gpu = vmap.accumulate(source[m], prm, T)
        eh, eg, es = gn_rel_err(gpu, ref)
        print(f"accumulate m={m} {name}: count {gpu['count']} / {ref['count']}, rel err H {eh:.3g} g {eg:.3g} ssq {es:.3g}")
        assert gpu["count"] == ref["count"] and (m < 5000 or ref["count"] > 1000), (name, gpu["count"], ref["count"])
        assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (name, eh, eg, es)


# ---- align ----------------------------------------------------------------------------------------------------------------


def _assert_pose(got, want, what):
    ang, tr = transform_diff(got, want)
    print(f"align {what}: d_angle {ang:.3g} rad, d_trans {tr:.3g} m")
    assert ang <= 1e-4 and tr <= 1e-4, (what, ang, tr)


@pytest.mark.parametrize("m", SOURCE_LENS)
@pytest.mark.parametrize("run", ["default x5", "weight 0.7 x3"])
def test_align_is_the_restatements_end_to_end_run(scene, vmap, source, m, run):
    prm = IcpParams(max_iterations=5) if run == "default x5" else IcpParams(max_iterations=3, weight=0.7)
    status, want = scene.model.align(scene.src_p[:m], scene.src_n[:m], prm.to_c())
    try:
        got, got_status = vmap.align(source[m], prm), _abi.A3D_OK
    except A3dError as e:
        got, got_status = None, e.status
    # (m = 1: the one point does not pass the normal gate, so no point passes and the solve fails, here as there)
    assert got_status == status == (_abi.A3D_SOLVE_FAILED if m == 1 else _abi.A3D_OK), (m, got_status, status)
    if got is None:
        return
    _assert_pose(got, want, f"m={m} {run}")
    assert vmap.last_device_ms() > 0.0
    if m == 5000:  # the alignment finds the pose the source was moved by
        ang, tr = transform_diff(got, scene.offset)
        assert ang < 2e-3 and tr < 2e-3, (ang, tr)


def test_align_starts_from_the_initial_pose(ctx, scene, vmap, source):
    big = O.exp_se3([3.0, -2.0, 2.5, 0.3, -0.2, 0.25])
    initial = Transform.from_c(big)
    # no iteration: the initial pose comes back bit for bit (None: eye)
    for m in (1, 5000):
        assert bytes(vmap.align(source[m], IcpParams(max_iterations=0), initial=initial).to_c()) == bytes(big)
        assert bytes(vmap.align(source[m], IcpParams(max_iterations=0)).to_c()) == bytes(Transform.eye().to_c())
    # a source seen from a frame `big` away: aligned from `big`, it comes back as the restatement's run from `big` does
    far_p, far_n = _moved(_inverse(big), scene.src_p[:1025], scene.src_n[:1025])
    prm = IcpParams(max_iterations=5)
    status, want = scene.model.align(far_p, far_n, prm.to_c(), initial=big)
    assert status == _abi.A3D_OK
    cloud = _dev(ctx, far_p, far_n)
    got = vmap.align(cloud, prm, initial=initial)
    _assert_pose(got, want, "from an initial pose")
    ang, tr = transform_diff(got, O.compose(scene.offset, big))
    assert ang < 2e-3 and tr < 2e-3, (ang, tr)
    with pytest.raises(A3dError) as e:  # from eye the source is metres away from the map: no point finds a row
        vmap.align(cloud, prm)
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    cloud.free()


def test_gates_at_the_edge(ctx):
    """One row; a source point whose distance to it is exactly max_distance is kept (the reference rejects d2 >
    max_distance^2 only), one ulp beyond is not, and a neighbourhood whose only row is beyond max_distance gives nothing."""
    row = np.asarray([[0.5, 0.5, 0.5]], np.float32)
    nx = np.asarray([[1.0, 0.0, 0.0]], np.float32)
    m = DeviceVoxelMap(ctx, VOXEL)
    c = _dev(ctx, row, nx)
    assert m.insert(c) == 0
    model = R.MapRestatement(row, nx, VOXEL)
    reach = np.float32(2.0 ** -5)  # 0.03125: its square and the differences below are exact in f32
    prm = IcpParams(max_iterations=1, max_distance=float(reach))
    at = np.asarray([[0.5 + 2.0 ** -5, 0.5, 0.5]], np.float32)
    beyond = at.copy()
    beyond[0, 0] = np.nextafter(at[0, 0], np.float32(1.0))
    apart = np.asarray([[0.5 + 0.04, 0.5, 0.5]], np.float32)  # in the 27 cells of the row, beyond max_distance
    for q, count in ((at, 1), (beyond, 0), (apart, 0)):
        seq, d2 = m.nearest(q)
        assert seq.tolist() == [0], "the row is found: the gate decides"
        assert (d2[0] == reach * reach) == (q is at) and (d2[0] > reach * reach) == (q is not at)
        src = _dev(ctx, q, nx)
        got = m.accumulate(src, prm, Transform.eye())
        want = model.accumulate(q, nx, Transform.eye().to_c(), prm.to_c())
        assert got["count"] == want["count"] == count, (q, got["count"], want["count"])
        if count:
            assert got["ssq"] == want["ssq"] == reach * reach
        src.free()
    m.free(), c.free()


def _snapshot(m):
    cloud, index = m.extract(return_index=True)
    p, n = cloud.download()
    cloud.free()
    return m.stats(), p.tobytes(), None if n is None else n.tobytes(), index.tobytes()


def test_failures_leave_the_map_as_it_was(ctx, scene, vmap, source):
    before = _snapshot(vmap)
    pose_before = vmap.align(source[1025], IcpParams(max_iterations=2))
    with pytest.raises(A3dError) as e:  # every point is gated out
        vmap.align(source[1025], IcpParams(max_iterations=5, max_distance=1e-7))
    assert e.value.status == _abi.A3D_SOLVE_FAILED
    bare = _dev(ctx, scene.src_p[:65])
    for call in (lambda: vmap.align(bare, IcpParams(max_iterations=5)),
                 lambda: vmap.accumulate(bare, IcpParams(max_iterations=5), Transform.eye())):
        with pytest.raises(A3dError) as e:  # a source without normals
            call()
        assert e.value.status == _abi.A3D_MISSING_FIELD
    assert _snapshot(vmap) == before
    flat = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, normals=False)  # a map without normals
    assert flat.insert(bare) == 0
    before_flat = _snapshot(flat)
    for call in (lambda: flat.align(source[65], IcpParams(max_iterations=5)),
                 lambda: flat.accumulate(source[65], IcpParams(max_iterations=5), Transform.eye())):
        with pytest.raises(A3dError) as e:
            call()
        assert e.value.status == _abi.A3D_MISSING_FIELD
    _assert_nearest(flat.nearest(source[65]), R.MapRestatement(scene.src_p[:65], None, VOXEL, ORIGIN).nearest(scene.src_p[:65]))
    assert _snapshot(flat) == before_flat
    flat.free(), bare.free()
    # the map still aligns as before
    assert bytes(vmap.align(source[1025], IcpParams(max_iterations=2)).to_c()) == bytes(pose_before.to_c())
