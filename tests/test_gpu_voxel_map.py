"""The persistent voxel map (a3d_voxel_map_*, DeviceVoxelMap) on the GPU.

The contract under test: after any sequence of inserts the map's contents equal merge(all inserted clouds under their
poses, in insertion order) followed by voxel_downsample — points, normals, order, winner indices — however the inserts
were grouped into calls and whatever the table's size history was.  The expected value is always the numpy restatement
(voxel_restatement.py) applied to the concatenation of the ORACLE-transformed host clouds (orc_transform_points /
orc_transform_normals, as test_gpu_cloud_transform.py), never the code under test.  Every comparison is on uint32 views,
bit for bit; the one tolerance is the 1e-4 / 1e-4 of the ICP check (test_gpu_pcl_icp.py).  Extracts go into buffers that
are filled with a canary word from end to end, with CANARY_WORDS more of it on both sides: rows past `cells` and both
guards must still hold it."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import voxel_restatement as V
from align3d_amd import (A3dError, Context, DevicePointCloud, DeviceVoxelMap, Icp, IcpBatch, IcpParams, InvalidParameter,
                         PointCloud, RangeImageBuilder, SlamTbDataset, Transform, TrajectoryBuilder, _abi)
from align3d_amd._abi import PoseC
from gpu_util import transform_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 63, 64, 65, 2047, 2049)
VOXELS = (0.02, 0.1, 1e3, 1e-5)
ORIGINS = (None, (0.013, -0.4, 7.5))
CANARY_WORDS = 64
CANARY = np.uint32(0xC0FFEE11)
SPARE_ROWS = 3  # rows of capacity beyond `cells`: they must stay canary
MAP_FRAMES = 8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uniform(seed, n, with_normals=True):
    """([n, 3] seeded points in the 3 m cube [0.25, 3.25)^3, [n, 3] unit-free 'normals' or None)."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(0.25, 3.25, size=(n, 3)).astype(np.float32)
    normals = rng.normal(size=(n, 3)).astype(np.float32) if with_normals else None
    return points, normals


def _raw_bits(seed, n):
    """[n, 3] raw random bits (the recipe of test_gpu_cloud_transform.py): NaNs with payloads, infinities, -0.0, denormals
    and magnitudes far beyond the 21-bit cell range all occur."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _device_cloud(ctx, points, normals=None):
    if len(points) == 0:
        return DevicePointCloud._allocate(ctx, 0, normals is not None)
    return DevicePointCloud(ctx, PointCloud(points, normals))


class _Guarded:
    """A device buffer of `count` elements of `width` words, canary-filled from end to end, CANARY_WORDS more on both
    sides."""

    def __init__(self, ctx, count, width):
        self.ctx, self.count, self.width = ctx, count, width
        self.words = 2 * CANARY_WORDS + width * count
        self.base = ctx.to_device(np.full(self.words, CANARY, np.uint32))
        self.ptr = C.c_void_p(self.base.value + 4 * CANARY_WORDS)

    def read(self):
        """(the body as [count, width] uint32, True iff both guards are intact)."""
        w = self.ctx.to_host(self.base, np.empty(self.words, np.uint32))
        body = w[CANARY_WORDS:self.words - CANARY_WORDS].reshape(self.count, self.width)
        return body, bool((w[:CANARY_WORDS] == CANARY).all() and (w[self.words - CANARY_WORDS:] == CANARY).all())

    def free(self):
        self.ctx.free(self.base)


def _extract(ctx, m, capacity=None, want_normals=None, want_index=True):
    """The raw extract into guarded buffers.  Returns (status, out_len, {points, normals, index: [capacity, width] uint32
    bodies or None}); asserts the guards."""
    want_normals = m.normals if want_normals is None else want_normals
    capacity = m.cells() + SPARE_ROWS if capacity is None else capacity
    g = {"points": _Guarded(ctx, capacity, 3), "normals": _Guarded(ctx, capacity, 3) if want_normals else None,
         "index": _Guarded(ctx, capacity, 1) if want_index else None}
    n = C.c_uint64(12345)
    st = ctx.lib.a3d_voxel_map_extract(m.handle, g["points"].ptr, g["normals"].ptr if g["normals"] else None,
                                       g["index"].ptr if g["index"] else None, capacity, C.byref(n))
    out = {}
    for name, buf in g.items():
        out[name] = None
        if buf is not None:
            out[name], intact = buf.read()
            assert intact, f"the extract wrote outside its {name} buffer"
            buf.free()
    return st, int(n.value), out


def _transformed(pose_c, points, normals):
    """The oracle's (transform_vectors, transform_normals or None) of host arrays under a PoseC; None = verbatim."""
    if pose_c is None or len(points) == 0:
        return points, normals
    out_p = O.transform_points(pose_c, points)
    if normals is None:
        return out_p, None
    normals = np.ascontiguousarray(normals, np.float32)
    out_n = np.empty_like(normals)
    O.load().orc_transform_normals(C.byref(pose_c), _abi.ptr(normals), normals.size // 3, _abi.ptr(out_n))
    return out_p, out_n


def _merged(hosts, poses, with_normals=True):
    """The merged cloud of [(points, normals)] under [PoseC] (None: verbatim) on the host, through the oracle."""
    parts = [_transformed(None if poses is None else poses[i], p, nrm if with_normals else None)
             for i, (p, nrm) in enumerate(hosts)]
    points = np.concatenate([p.reshape(-1, 3) for p, _ in parts]).astype(np.float32)
    normals = np.concatenate([nrm.reshape(-1, 3) for _, nrm in parts]).astype(np.float32) if with_normals else None
    return points, normals


def _dropped_per_cloud(merged_points, lens, voxel, origin):
    kept, _, _ = V.voxel_keys(merged_points, voxel, origin)
    ends = np.cumsum(lens)
    return [int((~kept[e - k:e]).sum()) for k, e in zip(lens, ends)]


def _assert_map_equals(ctx, m, expected, label=""):
    """The map's extract (guarded, with SPARE_ROWS rows of room to spare) against (points, normals or None, index, _)."""
    exp_p, exp_n, exp_i, _ = expected
    cells = len(exp_i)
    assert m.cells() == cells, label
    st, n, out = _extract(ctx, m)
    assert st == _abi.A3D_OK and n == cells, label
    assert np.array_equal(out["points"][:cells], _bits(exp_p).reshape(-1, 3)), label
    assert (out["points"][cells:] == CANARY).all(), label
    if m.normals:
        assert np.array_equal(out["normals"][:cells], _bits(exp_n).reshape(-1, 3)), label
        assert (out["normals"][cells:] == CANARY).all(), label
    assert np.array_equal(out["index"][:cells, 0], exp_i), label
    assert (out["index"][cells:] == CANARY).all(), label
    return out


def _poses(seed, n):
    """n distinct non-trivial poses (PoseC) through the oracle's exp_se3: rotations up to ~1 rad, translations ~0.5 m."""
    rng = np.random.default_rng(seed)
    return [O.exp_se3(rng.uniform(-0.6, 0.6, size=6).astype(np.float32)) for _ in range(n)]


def _transforms(poses):
    return None if poses is None else [Transform.from_c(p) for p in poses]


GROUPINGS = {
    "one call": lambda n: [list(range(n))],
    "one cloud per call": lambda n: [[i] for i in range(n)],
    "pairs": lambda n: [list(range(i, min(i + 2, n))) for i in range(0, n, 2)],
}


def _insert_grouped(m, clouds, transforms, groups):
    dropped = []
    for group in groups:
        dropped += m.insert_many([clouds[i] for i in group], None if transforms is None else [transforms[i] for i in group])
    return dropped


def test_contract_on_a_grid_of_sizes_voxels_origins_poses_and_groupings(ctx):
    hosts = [_uniform(200 + k, n) for k, n in enumerate(SIZES)]
    lens = [len(p) for p, _ in hosts]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    one = _poses(31, 1)
    pose_sets = {"identity": None, "one pose": one * len(SIZES), "a pose per cloud": _poses(32, len(SIZES))}
    cloud_of = np.repeat(np.arange(len(SIZES)), lens)
    for pose_name, poses in pose_sets.items():
        merged_p, merged_n = _merged(hosts, poses)
        transforms = _transforms(poses)
        for voxel in VOXELS:
            for origin in ORIGINS:
                expected = V.voxel_downsample_cloud(merged_p, merged_n, voxel, origin)
                exp_dropped = _dropped_per_cloud(merged_p, lens, voxel, origin)
                if voxel == 0.1:
                    # on the host, before the GPU is touched: with one cloud per call, some cell's winner comes from a
                    # later call than its first occupant, and some shared cell's winner is its first occupant's call
                    kept, key, _ = V.voxel_keys(merged_p, voxel, origin)
                    first_of_key = {}
                    for i in np.flatnonzero(kept):
                        first_of_key.setdefault(int(key[i]), int(cloud_of[i]))
                    winner_call = cloud_of[expected[2]]
                    first_call = np.asarray([first_of_key[int(k)] for k in key[expected[2]]])
                    _, inverse, counts = np.unique(key[kept], return_inverse=True, return_counts=True)
                    shared = dict(zip(key[kept].tolist(), (counts[inverse] > 1).tolist()))
                    is_shared = np.asarray([shared[int(k)] for k in key[expected[2]]])
                    assert (winner_call > first_call).sum() > 10 and ((winner_call == first_call) & is_shared).sum() > 10
                for with_normals in (True, False):
                    exp = (expected[0], expected[1] if with_normals else None, expected[2], expected[3])
                    for group_name, groups in GROUPINGS.items():
                        label = (pose_name, voxel, origin, with_normals, group_name)
                        m = DeviceVoxelMap(ctx, voxel, origin=origin, normals=with_normals)
                        dropped = _insert_grouped(m, clouds, transforms, groups(len(clouds)))
                        assert dropped == exp_dropped, label
                        s = m.stats()
                        assert s["total"] == sum(lens) and s["dropped_total"] == sum(exp_dropped), label
                        assert s["slots"] >= 2 * s["cells"] and s["slots"] & (s["slots"] - 1) == 0, label
                        _assert_map_equals(ctx, m, exp, label)
                        m.free()
    for c in clouds:
        c.free()


def test_ties_across_calls_keep_the_earlier_calls_point(ctx):
    v = np.float32(0.25)  # a power of two: cell centres and the offsets below are exact in f32
    rng = np.random.default_rng(62)
    cells = rng.integers(-40, 40, size=(3000, 3)).astype(np.float32)
    centre = (cells + np.float32(0.5)) * v
    delta = (rng.integers(1, 120, size=(3000, 3)) / 1024.0).astype(np.float32)  # < v / 2
    plus, minus = centre + delta, centre - delta  # mirror images about the cell centres: equal distances
    perm = rng.permutation(3000)
    minus = minus[perm]
    for first, second in ((plus, minus), (minus, plus)):
        # on the host: cells whose best distance in the first call equals their best distance in the second
        best = []
        for part in (first, second):
            kept, key, dist = V.voxel_keys(part, v)
            assert kept.all()
            order = np.lexsort((dist, key))
            head = np.ones(len(order), bool)
            head[1:] = key[order][1:] != key[order][:-1]
            best.append(dict(zip(key[order][head].tolist(), dist[order][head].tolist())))
        tied = [k for k, d in best[0].items() if best[1].get(k) == d]
        assert len(tied) >= 1000
        merged = np.concatenate([first, second])
        expected = V.voxel_downsample_cloud(merged, None, float(v))
        _, key, _ = V.voxel_keys(merged, v)
        winner_of = dict(zip(key[expected[2]].tolist(), expected[2].tolist()))
        assert all(winner_of[k] < len(first) for k in tied)  # the earlier call's point stays
        a, b = _device_cloud(ctx, first), _device_cloud(ctx, second)
        m = DeviceVoxelMap(ctx, float(v), normals=False)
        assert m.insert(a) == 0 and m.insert(b) == 0
        _assert_map_equals(ctx, m, expected)
        m.free(), a.free(), b.free()


def test_growth_keeps_the_contents_and_a_reserved_table_gives_the_same_bits(ctx):
    # points of a 3 m cube at v = 0.02 (3.4 M cells): most of the 100 k points are alone in their cell
    hosts = [_uniform(300, 65), _uniform(301, 2049), _uniform(302, 100003)]
    voxel = 0.02
    merged_p, merged_n = _merged(hosts, None)
    expected = V.voxel_downsample_cloud(merged_p, merged_n, voxel)
    assert len(expected[2]) > 90000
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    grown = DeviceVoxelMap(ctx, voxel, reserve_cells=0)
    slots = []
    for c in clouds:
        grown.insert(c)
        slots.append(grown.stats()["slots"])
    # the reservation rule, slots >= 2 * (cells + L) at the next power of two: 2 * 65 -> 256 (the first table, no growth);
    # 2 * (<= 65 + 2049) -> 8192; 2 * (<= 2114 + 100003) -> 262144: exactly two growths
    assert slots == [256, 8192, 262144] and grown.stats()["growths"] == 2
    got_grown = _assert_map_equals(ctx, grown, expected)
    reserved = DeviceVoxelMap(ctx, voxel, reserve_cells=131072)
    for c in clouds:
        reserved.insert(c)
    assert reserved.stats()["growths"] == 0 and reserved.stats()["slots"] == 262144
    got_reserved = _assert_map_equals(ctx, reserved, expected)
    for name in ("points", "normals", "index"):
        assert np.array_equal(got_grown[name], got_reserved[name])
    grown.free(), reserved.free()
    for c in clouds:
        c.free()


def test_hostile_bit_patterns_dropped_points_consume_sequence_numbers(ctx):
    """Under a pose the NORMALS are finite: the payload and sign of a computed NaN differ between x86 and the GPU
    (test_gpu_cloud_transform.py), and a normal plays no part in the drop rule.  The points are raw bits throughout: a
    kept point is never NaN, so its bits must be the oracle's."""
    sizes = (65, 2047, 2049)
    raw = [(_raw_bits(4000 + k, n), _raw_bits(5000 + k, n)) for k, n in enumerate(sizes)]
    tame = [(p, _uniform(5100 + k, len(p))[1]) for k, (p, _) in enumerate(raw)]
    lens = list(sizes)
    for hosts, poses in ((raw, None), (tame, _poses(41, len(sizes)))):
        clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
        merged_p, merged_n = _merged(hosts, poses)
        assert np.isnan(merged_p).any() and np.isinf(merged_p).any()
        for voxel, origin in ((0.02, None), (1e3, (0.5, -2.0, 1e-3)), (1e25, None), (1e-40, None)):
            expected = V.voxel_downsample_cloud(merged_p, merged_n, voxel, origin)
            exp_dropped = _dropped_per_cloud(merged_p, lens, voxel, origin)
            if voxel in (1e3, 1e25):
                # every cloud drops points and keeps points, and a kept point of a later cloud lies behind dropped ones of
                # an earlier cloud: its index counts them
                kept, _, _ = V.voxel_keys(merged_p, voxel, origin)
                assert all(0 < d < n for d, n in zip(exp_dropped, lens))
                later = expected[2][expected[2] >= lens[0]]
                assert len(later) and (~kept[:lens[0]]).any()
                kept_rank = np.cumsum(kept) - 1  # the index such a point would have if dropped points consumed no number
                assert (kept_rank[later] != later).all()
            for group_name, groups in GROUPINGS.items():
                m = DeviceVoxelMap(ctx, voxel, origin=origin)
                assert _insert_grouped(m, clouds, _transforms(poses), groups(len(clouds))) == exp_dropped
                assert m.stats()["dropped_total"] == sum(exp_dropped) and m.total() == sum(lens)
                _assert_map_equals(ctx, m, expected, (voxel, origin, group_name, poses is None))
                m.free()
        for c in clouds:
            c.free()


_world = {}


def _sample1_world(ctx):
    """MAP_FRAMES frames of sample1 as resident clouds, their odometry poses (IcpBatch over the consecutive pairs, as
    examples/pcl_map.py), the host copies of the clouds, and per prefix of the frames the restatement of the merged,
    oracle-transformed cloud at v = 0.02; built once per session."""
    if not _world:
        ds = SlamTbDataset.load(os.path.join(ROOT, "tests", "golden", "rgbd", "sample1"))
        frames = [ds.get(i) for i in range(MAP_FRAMES)]
        cam, _, _, depth_scale = frames[0]
        built = RangeImageBuilder(ctx).pyramid_levels(1).with_intensity(False).build_many(
            cam, [(f[1], f[2]) for f in frames], depth_scale)
        images = [pyramid[0] for pyramid in built]
        clouds = DevicePointCloud.from_range_images(images)
        for im in images:
            im.free()
        batch = IcpBatch(ctx, IcpParams.default(), clouds[:-1])
        poses, status = batch.align(clouds[1:])
        batch.free()
        traj = TrajectoryBuilder.with_start(Transform.eye(), 0.0)
        camera_to_world = [traj.current_camera_to_world()]
        for k, (now_to_previous, st) in enumerate(zip(poses, status)):
            if st == 0:
                traj.accumulate(now_to_previous, float(k + 1))
            camera_to_world.append(traj.current_camera_to_world())
        hosts = [c.download() for c in clouds]
        merged_p, merged_n = _merged(hosts, [t.to_c() for t in camera_to_world])
        ends = np.cumsum([len(p) for p, _ in hosts])
        assert ends[-1] > MAP_FRAMES * 200000
        prefixes = [V.voxel_downsample_cloud(merged_p[:e], merged_n[:e], 0.02) for e in ends]
        _world.update(clouds=clouds, poses=camera_to_world, prefixes=prefixes)
    return _world


def _download_bits(cloud):
    p, nrm = cloud.download()
    return _bits(p), _bits(nrm)


def test_equals_merge_and_downsample_on_fixture_frames_and_runs_are_identical(ctx):
    w = _sample1_world(ctx)
    clouds, poses, expected = w["clouds"], w["poses"], w["prefixes"][-1]
    assert all(e[3] == 0 for e in w["prefixes"]) and len(expected[2]) < sum(c.len() for c in clouds) // 4
    # the existing device path
    merged = DevicePointCloud.merge(clouds, poses)
    thin, thin_index = merged.voxel_downsample(0.02, return_index=True)
    merged.free()
    want_p, want_n = _download_bits(thin)
    thin.free()
    assert np.array_equal(thin_index, expected[2])
    assert np.array_equal(want_p, _bits(expected[0])) and np.array_equal(want_n, _bits(expected[1]))
    # one call, twice: the same bits and indices as the device path, as the restatement, and as each other
    for run in range(2):
        m = DeviceVoxelMap(ctx, 0.02)
        assert m.insert_many(clouds, poses) == [0] * len(clouds)
        got, index = m.extract(return_index=True)
        assert got.len() == m.cells() == len(expected[2]) and index.dtype == np.uint32 and got.d_normals is not None
        got_p, got_n = _download_bits(got)
        assert np.array_equal(index, thin_index) and np.array_equal(got_p, want_p) and np.array_equal(got_n, want_n), run
        got.free(), m.free()
    # frame by frame
    m = DeviceVoxelMap(ctx, 0.02)
    for c, t in zip(clouds, poses):
        assert m.insert(c, t) == 0
    _assert_map_equals(ctx, m, expected)
    m.free()


def test_an_extract_after_every_frame_is_the_prefixs_map_and_leaves_later_inserts_alone(ctx):
    w = _sample1_world(ctx)
    m = DeviceVoxelMap(ctx, 0.02)
    for k, (c, t) in enumerate(zip(w["clouds"], w["poses"])):
        assert m.insert(c, t) == 0
        _assert_map_equals(ctx, m, w["prefixes"][k], k)
    assert m.total() == sum(c.len() for c in w["clouds"])
    m.free()


def test_capacity_one_short_writes_nothing_and_reports_the_cells(ctx):
    points, normals = _uniform(400, 2049)
    cloud = _device_cloud(ctx, points, normals)
    expected = V.voxel_downsample_cloud(points, normals, 0.1)
    cells = len(expected[2])
    assert 1 < cells < len(points)
    m = DeviceVoxelMap(ctx, 0.1)
    m.insert(cloud)
    for capacity in (cells - 1, 0):
        st, n, out = _extract(ctx, m, capacity=capacity)
        assert st == _abi.A3D_INVALID_PARAMETER and n == cells
        for name in ("points", "normals", "index"):
            assert (out[name] == CANARY).all(), name
    st, n, out = _extract(ctx, m, capacity=cells)  # exactly enough is enough
    assert st == _abi.A3D_OK and n == cells
    assert np.array_equal(out["points"], _bits(expected[0]).reshape(-1, 3))
    assert np.array_equal(out["normals"], _bits(expected[1]).reshape(-1, 3))
    assert np.array_equal(out["index"][:, 0], expected[2])
    # points only and no index, from a map with normals
    st, n, out = _extract(ctx, m, capacity=cells, want_normals=False, want_index=False)
    assert st == _abi.A3D_OK and out["normals"] is None and out["index"] is None
    assert np.array_equal(out["points"], _bits(expected[0]).reshape(-1, 3))
    m.free(), cloud.free()


def test_maps_without_normals_take_any_cloud_and_maps_with_normals_refuse_a_bare_one(ctx):
    hosts = [_uniform(500, 2047), _uniform(501, 65, with_normals=False), _uniform(502, 2049)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    merged_p, _ = _merged(hosts, None, with_normals=False)
    bare = DeviceVoxelMap(ctx, 0.1, normals=False)
    assert bare.insert_many(clouds) == [0, 0, 0]
    _assert_map_equals(ctx, bare, V.voxel_downsample_cloud(merged_p, None, 0.1))
    st, _, _ = _extract(ctx, bare, want_normals=True)
    assert st == _abi.A3D_MISSING_FIELD
    cloud, index = bare.extract(return_index=True)
    assert cloud.d_normals is None and cloud.len() == bare.cells() == len(index)
    cloud.free(), bare.free()
    full = DeviceVoxelMap(ctx, 0.1)
    full.insert(clouds[0])
    expected = V.voxel_downsample_cloud(*hosts[0], 0.1)
    before = _assert_map_equals(ctx, full, expected)
    stats = full.stats()
    for batch in ([clouds[1]], [clouds[2], clouds[1]], clouds):
        with pytest.raises(A3dError) as e:
            full.insert_many(batch)
        assert e.value.status == _abi.A3D_MISSING_FIELD
    assert full.stats() == stats  # nothing was inserted from any of the calls, the cloud before the bare one included
    after = _assert_map_equals(ctx, full, expected)
    for name in ("points", "normals", "index"):
        assert np.array_equal(before[name], after[name])
    # host clouds and clouds of another context are refused as _resident_batch refuses them
    with pytest.raises(TypeError):
        full.insert(PointCloud(*hosts[0]))
    other = Context(0)
    foreign = _device_cloud(other, *hosts[0])
    with pytest.raises(InvalidParameter):
        full.insert(foreign)
    foreign.free()
    other.close()
    assert full.stats() == stats
    full.free()
    for c in clouds:
        c.free()


def test_clear_makes_the_map_behave_as_new(ctx):
    hosts = [_uniform(600, 2049), _uniform(601, 2047)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    poses = _poses(51, 2)
    merged_p, merged_n = _merged(hosts[::-1], poses)
    expected = V.voxel_downsample_cloud(merged_p, merged_n, 0.1, ORIGINS[1])
    fresh = DeviceVoxelMap(ctx, 0.1, origin=ORIGINS[1])
    fresh.insert_many(clouds[::-1], _transforms(poses))
    want = _assert_map_equals(ctx, fresh, expected)
    used = DeviceVoxelMap(ctx, 0.1, origin=ORIGINS[1])
    used.insert_many(clouds)  # other contents first: other winners, other sequence numbers
    used.insert(clouds[0], _transforms(poses)[0])
    slots = used.stats()["slots"]
    assert used.cells() > 0 and used.total() == 2 * 2049 + 2047
    used.clear()
    s = used.stats()
    assert (s["cells"], s["total"], s["dropped_total"], s["slots"]) == (0, 0, 0, slots)  # the allocation stays
    empty, index = used.extract(return_index=True)
    assert empty.len() == 0 and len(index) == 0
    empty.free()
    used.insert_many(clouds[::-1], _transforms(poses))
    got = _assert_map_equals(ctx, used, expected)  # indices start at 0 again
    for name in ("points", "normals", "index"):
        assert np.array_equal(got[name], want[name])
    fresh.free(), used.free()
    for c in clouds:
        c.free()


def test_extracted_map_is_an_icp_target_and_agrees_with_the_oracle(ctx):
    w = _sample1_world(ctx)
    m = DeviceVoxelMap(ctx, 0.02)
    m.insert_many(w["clouds"], w["poses"])
    thin = m.extract()
    map_p, map_n = thin.download()
    exp_p, exp_n, _, _ = w["prefixes"][-1]
    assert np.array_equal(_bits(map_p), _bits(exp_p)) and np.array_equal(_bits(map_n), _bits(exp_n))
    assert np.isfinite(map_p).all()
    # frame to map: a fixture frame under its odometry pose against the extracted map
    k = MAP_FRAMES // 2
    source = w["poses"][k] * w["clouds"][k]
    src_p, src_n = source.download()
    prm = IcpParams(max_iterations=5)
    icp = Icp.new(ctx, prm, thin)  # the kd-tree builds over the extracted cloud
    T_gpu = icp.align(source)      # raises unless the status is A3D_OK
    tree = O.KdTree(map_p)
    out = PoseC()
    tv, sv = O.pcl_view(map_p, map_n), O.pcl_view(src_p, src_n)
    p = prm.to_c()
    assert O.load().orc_pcl_icp_align(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(out), None) == 0
    ang, tr = transform_diff(T_gpu, out)
    print(f"[frame {k} against the extracted map of {thin.len()} points (v = 0.02)] d_angle={ang:.3e} d_trans={tr:.3e}")
    assert ang <= 1e-4 and tr <= 1e-4
    batch = IcpBatch(ctx, prm, [thin])
    _, status = batch.align([source])
    assert status[0] == 0
    icp.free(), batch.free(), m.free()
    for x in (thin, source):
        x.free()


def test_stored_slot_pass_b_of_the_diagnostics_build_gives_the_same_bits(monkeypatch):
    """The diagnostics library holds a second form of pass B, which reads the slot pass A left per point instead of
    probing again (A3D_VOXEL_MAP_STORED_SLOT=1, read by every insert).  Both forms, on inputs that drop points, overwrite
    older winners, grow the table between calls and hold several clouds per call, equal the restatement bit for bit."""
    assert b"A3D_VOXEL_MAP_STORED_SLOT" in open(_abi.DIAG_LIB_PATH, "rb").read()
    diag = Context(0, library=_abi.DIAG_LIB_PATH)
    sizes = (65, 0, 2049, 2047, 63)
    hosts = [(_raw_bits(7000 + k, n), _uniform(7100 + k, n)[1]) for k, n in enumerate(sizes)]
    tame = [_uniform(7200 + k, n) for k, n in enumerate(sizes)]
    poses = _poses(71, len(sizes))
    groups = GROUPINGS["pairs"](len(sizes))
    for cloud_hosts, voxel in ((hosts, 1e3), (tame, 0.1)):
        clouds = [_device_cloud(diag, p, nrm) for p, nrm in cloud_hosts]
        lens = [len(p) for p, _ in cloud_hosts]
        merged_p, merged_n = _merged(cloud_hosts, poses)
        exp_dropped = _dropped_per_cloud(merged_p, lens, voxel, None)
        assert (voxel == 0.1) == (sum(exp_dropped) == 0)
        for with_normals in (True, False):
            expected = V.voxel_downsample_cloud(merged_p, merged_n if with_normals else None, voxel)
            assert 1 < len(expected[2]) < sum(lens) - sum(exp_dropped)  # cells are shared
            got = {}
            for form in ("0", "1"):
                monkeypatch.setenv("A3D_VOXEL_MAP_STORED_SLOT", form)
                m = DeviceVoxelMap(diag, voxel, normals=with_normals)
                assert _insert_grouped(m, clouds, _transforms(poses), groups) == exp_dropped
                assert m.stats()["growths"] >= 1
                got[form] = _assert_map_equals(diag, m, expected, (voxel, with_normals, form))
                m.free()
            for name in ("points", "index"):
                assert np.array_equal(got["0"][name], got["1"][name])
        for c in clouds:
            c.free()
    monkeypatch.delenv("A3D_VOXEL_MAP_STORED_SLOT")
    diag.close()
