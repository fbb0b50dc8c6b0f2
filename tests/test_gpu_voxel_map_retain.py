"""a3d_voxel_map_retain (DeviceVoxelMap.retain / compact) on the GPU.

The contract under test: after a retain the map is indistinguishable from a new map into which the surviving rows of
extract() — the rows that pass the rule, in extract order — were inserted as ONE cloud without a pose.  The expected value
is always the numpy restatement (voxel_restatement.py): `_Model` keeps the rows of everything offered since the last
retain (oracle-transformed on the host, as test_gpu_voxel_map.py), the survivors of that retain first; its map is
V.voxel_downsample_cloud of those rows, and its survivors are chosen from that map's rows by the numpy f32 predicate.
Nothing expected comes from the library.  Points and normals are compared on uint32 views, bit for bit, through the
canary-guarded extract of test_gpu_voxel_map.py; indices, stats, removed counts and translated marks exactly."""
import numpy as np
import pytest

import voxel_restatement as V
from align3d_amd import DeviceVoxelMap
from test_gpu_voxel_map import (_assert_map_equals, _device_cloud, _merged, _poses, _raw_bits, _sample1_world, _transforms,
                                _uniform)

pytestmark = pytest.mark.gpu

INF = float("inf")
ORIGIN = (0.013, -0.4, 7.5)
# the clouds of a map; their ends are the sequence numbers at the 64-bit word and 1024-point chunk edges, and 20 000
# points at a small voxel put more than 256 x 64 sequence numbers into the bitmap (two prefix chunks, two tiles)
CONTENTS = ((1, 63, 64, 65), (1024, 1025), (1025, 1, 1024), (20000,), (64, 20011, 63))
LATER = (65, 1025)  # the two clouds inserted after the retain
VOXELS = (0.05, 0.5)  # of the 4 m cube: nearly every point alone in its cell / 512 cells shared by many points
BOX = ((-1.2, -2.5, -0.9), (1.5, 1.1, 3.0))
ONE_SIDED = ((-INF, -INF, -0.3), (INF, 0.8, INF))
RULES = {"box": (BOX, None), "min_seq": (None, 1 / 3), "both": (BOX, 1 / 5), "one-sided": (ONE_SIDED, None)}


def _cube(seed, n):
    """([n, 3] seeded points in [-2, 2]^3, [n, 3] 'normals')."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def _slots_rule(k, reserve=0):
    slots = 64
    while slots < max(2 * k, 2 * reserve):
        slots <<= 1
    return slots


class _Model:
    """The expected map by the restatement alone."""

    def __init__(self, voxel, origin=None, with_normals=True):
        self.voxel, self.origin, self.with_normals = voxel, origin, with_normals
        self.p = np.empty((0, 3), np.float32)
        self.n = np.empty((0, 3), np.float32) if with_normals else None

    def insert(self, hosts, poses=None):
        """Offers [(points, normals)] under [PoseC] (None: verbatim); returns the dropped count of each cloud."""
        p, n = _merged(hosts, poses, self.with_normals)
        kept, _, _ = V.voxel_keys(p, self.voxel, self.origin)
        ends = np.cumsum([len(h[0]) for h in hosts])
        self.p = np.concatenate([self.p, p])
        if self.with_normals:
            self.n = np.concatenate([self.n, n])
        return [int((~kept[e - len(h[0]):e]).sum()) for h, e in zip(hosts, ends)]

    def total(self):
        return len(self.p)

    def expected(self):
        return V.voxel_downsample_cloud(self.p, self.n, self.voxel, self.origin)

    def retain(self, box=None, min_seq=0, marks=()):
        """(removed, translated marks, k): the survivors become the model's only rows."""
        p, n, index, _ = self.expected()
        keep = index.astype(np.uint64) >= np.uint64(min(min_seq, 1 << 63))
        if box is not None:
            lo, hi = np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)
            keep &= ((p >= lo) & (p <= hi)).all(axis=1)
        old = index[keep].astype(np.uint64)
        new_marks = [int((old < np.uint64(min(int(m), 1 << 63))).sum()) for m in marks]
        self.p = p[keep]
        if self.with_normals:
            self.n = n[keep]
        return int(len(index) - keep.sum()), new_marks, int(keep.sum())


def _check(ctx, m, model, label, growths=None, reserve=0, after_retain=False):
    exp = model.expected()
    out = _assert_map_equals(ctx, m, exp, label)
    s = m.stats()
    kept, _, _ = V.voxel_keys(model.p, model.voxel, model.origin)
    assert s["cells"] == len(exp[2]) and s["total"] == model.total() and s["dropped_total"] == int((~kept).sum()), label
    if after_retain:
        k = len(exp[2])
        assert s["cells"] == s["total"] == k and s["dropped_total"] == 0, label
        assert np.array_equal(exp[2], np.arange(k, dtype=np.uint32)), label
        if k:
            assert s["slots"] == _slots_rule(k, reserve), label
    if growths is not None:
        assert s["growths"] == growths, label
    return out


def _cut(model, fraction):
    return None if fraction is None else int(model.total() * fraction)


def test_contract_on_a_grid_of_contents_rules_voxels_origins_poses_and_normals(ctx):
    later_hosts = [_cube(900 + k, n) for k, n in enumerate(LATER)]
    later_clouds = [_device_cloud(ctx, p, nrm) for p, nrm in later_hosts]
    later_poses = _poses(91, len(LATER))
    case = 0
    for ci, sizes in enumerate(CONTENTS):
        hosts = [_cube(100 * ci + k, n) for k, n in enumerate(sizes)]
        clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
        poses = _poses(70 + ci, len(sizes))
        for rule_name, (box, fraction) in RULES.items():
            for voxel in VOXELS:
                origin = ORIGIN if case & 1 else None
                posed = bool(case & 2)
                with_normals = not case & 4
                case += 1
                label = (sizes, rule_name, voxel, origin, posed, with_normals)
                model = _Model(voxel, origin, with_normals)
                m = DeviceVoxelMap(ctx, voxel, origin=origin, normals=with_normals)
                exp_dropped = model.insert(hosts, poses if posed else None)
                assert m.insert_many(clouds, _transforms(poses) if posed else None) == exp_dropped, label
                growths = m.stats()["growths"]
                cells = len(model.expected()[2])
                min_seq = _cut(model, fraction)
                exp_removed, _, k = model.retain(box, min_seq or 0)
                # by the restatement alone: the rule keeps a part and removes a part
                assert 0.1 * cells <= k <= 0.9 * cells and exp_removed == cells - k, (label, cells, k)
                removed = m.retain(box=box, min_seq=min_seq or 0)
                assert removed == exp_removed, label
                _check(ctx, m, model, label, growths=growths, after_retain=True)
                # later points beat or lose to the survivors exactly as in the model, ties included
                model.insert(later_hosts, later_poses if posed else None)
                m.insert_many(later_clouds, _transforms(later_poses) if posed else None)
                _check(ctx, m, model, label)
                m.free()
        for c in clouds:
            c.free()
    assert case == len(CONTENTS) * len(RULES) * len(VOXELS) and case % 8 == 0  # every combination of the three bits occurs
    for c in later_clouds:
        c.free()


def test_bits_of_best_survive_a_tie_keeps_the_survivor_and_a_nearer_point_wins(ctx):
    v = np.float32(0.25)  # a power of two: cell centres and the offsets below are exact in f32
    rng = np.random.default_rng(62)
    cells = np.unique(rng.integers(-40, 40, size=(3000, 3)), axis=0).astype(np.float32)
    rng.shuffle(cells)
    centre = (cells + np.float32(0.5)) * v
    delta = (rng.integers(2, 120, size=centre.shape) / 1024.0).astype(np.float32)  # < v / 2, even halves are exact
    first = centre + delta  # one point per cell
    perm = rng.permutation(len(centre))
    tied = (centre - delta)[perm]  # the mirror images: the same distance to the centre, bit for bit
    nearer = (centre + delta * np.float32(0.5))[perm[::2]]  # every other cell: strictly nearer
    box = ((-INF, -INF, -INF), (0.0, INF, INF))  # about half of the cells
    model = _Model(float(v), None, False)
    model.insert([(first, None)])
    _, key_first, dist_first = V.voxel_keys(first, v)
    _, key_tied, dist_tied = V.voxel_keys(tied, v)
    assert np.array_equal(key_tied, key_first[perm]) and np.array_equal(dist_tied.view(np.uint32), dist_first[perm].view(np.uint32))
    removed, _, k = model.retain(box)
    assert 1000 < k < len(first) - 1000 and removed == len(first) - k
    a, b, c = (_device_cloud(ctx, x) for x in (first, tied, nearer))
    m = DeviceVoxelMap(ctx, float(v), normals=False)
    assert m.insert(a) == 0
    assert m.retain(box=box) == removed
    _check(ctx, m, model, "retained", after_retain=True)
    survivor_keys = set(V.voxel_keys(model.p, v)[1].tolist())
    # the tie: in every surviving cell the survivor (index < k) stays; the removed cells are won by the mirror image
    model.insert([(tied, None)])
    exp = model.expected()
    in_surviving = np.asarray([key in survivor_keys for key in V.voxel_keys(exp[0], v)[1].tolist()])
    assert in_surviving.sum() == k and (exp[2][in_surviving] < k).all() and (exp[2][~in_surviving] >= k).all()
    assert m.insert(b) == 0
    _check(ctx, m, model, "tied")
    # strictly nearer: it wins, in surviving cells too
    model.insert([(nearer, None)])
    exp = model.expected()
    nearer_keys = set(V.voxel_keys(nearer, v)[1].tolist())
    won = np.asarray([key in nearer_keys for key in V.voxel_keys(exp[0], v)[1].tolist()])
    assert (exp[2][won] >= k + len(tied)).all() and (won & (exp[2] >= k + len(tied))).sum() == len(nearer)
    assert len(survivor_keys & nearer_keys) > 200
    assert m.insert(c) == 0
    _check(ctx, m, model, "nearer")
    m.free(), a.free(), b.free(), c.free()


@pytest.mark.parametrize("sizes", [(64, 65, 63, 1024, 1025, 1), (64, 64, 128, 1024, 576, 64)])
def test_marks_are_translated_and_age_the_map_by_frame(ctx, sizes):
    total = sum(sizes)
    assert (total % 64 == 0) == (sizes[1] == 64)  # the second run ends on a word of the bitmap: the mark `total` lies past it
    hosts = [_cube(300 + k, n) for k, n in enumerate(sizes)]
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    for voxel, box in ((0.05, BOX), (0.5, BOX), (0.05, None)):
        model = _Model(voxel)
        m = DeviceVoxelMap(ctx, voxel)
        bounds = []
        for host, cloud in zip(hosts, clouds):
            bounds.append(m.total())  # the caller's record: the first sequence number of the frame
            model.insert([host])
            m.insert(cloud)
        assert m.total() == total and bounds[0] == 0
        marks = np.asarray(bounds + [total, total + 1, 1 << 63], np.uint64)
        cells = len(model.expected()[2])
        exp_removed, exp_marks, k = model.retain(box, 0, marks)
        removed, new_marks = m.retain(box=box, marks=marks)
        assert removed == exp_removed and new_marks.dtype == np.uint64 and new_marks.tolist() == exp_marks
        assert exp_marks[0] == 0 and exp_marks[-3:] == [k, k, k] and sorted(exp_marks) == exp_marks
        if box is not None:
            assert 0.1 * cells <= k <= 0.9 * cells
        _check(ctx, m, model, (voxel, "first"), after_retain=True)
        # ageing: the translated boundary of frame 1 as min_seq removes exactly what is left of frame 0
        frame0 = exp_marks[1]
        assert 0 < frame0 < k
        exp_removed, exp_marks2, k2 = model.retain(None, exp_marks[1], exp_marks)
        removed, new_marks2 = m.retain(min_seq=int(new_marks[1]), marks=new_marks)
        assert removed == exp_removed == frame0 and k2 == k - frame0
        assert new_marks2.tolist() == exp_marks2 == [max(0, x - frame0) for x in exp_marks]
        _check(ctx, m, model, (voxel, "second"), after_retain=True)
        m.free()
    for c in clouds:
        c.free()


def test_edges_no_table_nothing_kept_everything_kept_shrink_and_regrow_and_identical_runs(ctx):
    # no table yet
    m = DeviceVoxelMap(ctx, 0.5)
    assert m.retain(box=BOX, min_seq=3) == 0 and m.compact() == 0
    removed, new = m.retain(marks=np.asarray([0, 5], np.uint64))
    assert removed == 0 and new.tolist() == [0, 0]
    assert m.stats() == dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)
    m.free()
    big, small = _cube(400, 20000), _cube(401, 1025)
    d_big, d_small = _device_cloud(ctx, *big), _device_cloud(ctx, *small)
    # a retain that keeps nothing behaves as clear: the allocation stays, the next insert numbers from 0
    for kwargs in (dict(min_seq=20000), dict(min_seq=1 << 63), dict(box=((1, 1, 1), (-1, -1, -1))),
                   dict(box=((5, 5, 5), (INF, INF, INF)))):
        m = DeviceVoxelMap(ctx, 0.5)
        m.insert(d_big)
        before = m.stats()
        removed, new = m.retain(marks=np.asarray([0, 777, 20000, 20001], np.uint64), **kwargs)
        assert removed == before["cells"] and new.tolist() == [0, 0, 0, 0], kwargs
        assert m.stats() == dict(cells=0, slots=before["slots"], total=0, dropped_total=0, growths=before["growths"]), kwargs
        model = _Model(0.5)
        model.insert([small])
        m.insert(d_small)
        _check(ctx, m, model, kwargs)
        m.free()
    # a retain that keeps everything is a pure compaction; the table shrinks to the rule's slots and grows again
    runs = []
    for run in range(2):
        model = _Model(0.5)
        m = DeviceVoxelMap(ctx, 0.5, reserve_cells=0)
        model.insert([big])
        m.insert(d_big)
        before = _check(ctx, m, model, "before")
        cells = m.cells()
        assert 300 < cells < 700 and m.stats()["slots"] == 65536 and not np.array_equal(before["index"][:cells, 0], np.arange(cells))
        assert model.retain() == (0, [], cells)
        assert m.compact() == 0
        after = _check(ctx, m, model, "compacted", growths=0, after_retain=True)
        assert m.stats()["slots"] == _slots_rule(cells) <= 2048
        for name in ("points", "normals"):
            assert np.array_equal(before[name], after[name])
        model.insert([big, small])
        m.insert_many([d_big, d_small])  # 2 * (cells + 21025) slots are needed: one growth, as on a new map
        grown = _check(ctx, m, model, "grown", growths=1)
        assert m.stats()["slots"] == 65536
        assert m.compact() == 0 and model.retain()[0] == 0
        again = _check(ctx, m, model, "compacted again", growths=1, after_retain=True)
        runs.append((after, grown, again))
        m.free()
    for x, y in zip(*runs):
        for name in ("points", "normals", "index"):
            assert np.array_equal(x[name], y[name])
    # a reservation is part of the rule
    model = _Model(0.5)
    m = DeviceVoxelMap(ctx, 0.5, reserve_cells=3000)
    model.insert([small])
    m.insert(d_small)
    assert m.stats()["slots"] == 8192
    exp_removed, _, k = model.retain(BOX)
    assert m.retain(box=BOX) == exp_removed and 0 < k < 700
    _check(ctx, m, model, "reserved", growths=0, reserve=3000, after_retain=True)
    assert m.stats()["slots"] == 8192
    m.free(), d_big.free(), d_small.free()


def test_hostile_bit_patterns_dropped_points_leave_no_trace_after_a_retain(ctx):
    sizes = (65, 2047, 2049)
    hosts = [(_raw_bits(4000 + k, n), _raw_bits(5000 + k, n)) for k, n in enumerate(sizes)]
    more = (_raw_bits(4100, 1025), _raw_bits(5100, 1025))
    clouds = [_device_cloud(ctx, p, nrm) for p, nrm in hosts]
    d_more = _device_cloud(ctx, *more)
    box = ((0.0, -INF, -INF), (INF, INF, 1e30))  # -0.0 and denormals sit on its face x = 0
    for voxel, origin in ((1e3, (0.5, -2.0, 1e-3)), (1e25, None), (0.02, None)):
        model = _Model(voxel, origin)
        m = DeviceVoxelMap(ctx, voxel, origin=origin)
        exp_dropped = model.insert(hosts)
        assert m.insert_many(clouds) == exp_dropped and all(0 < d < n for d, n in zip(exp_dropped, sizes))
        before = model.expected()
        assert m.stats()["dropped_total"] == sum(exp_dropped) and len(before[2]) < before[2][-1] + 1  # numbers were consumed
        cells = len(before[2])
        exp_removed, exp_marks, k = model.retain(box, 0, [sizes[0], sizes[0] + sizes[1]])
        assert 0.1 * cells <= k <= 0.9 * cells
        removed, new_marks = m.retain(box=box, marks=np.asarray([sizes[0], sizes[0] + sizes[1]], np.uint64))
        assert removed == exp_removed and new_marks.tolist() == exp_marks
        _check(ctx, m, model, (voxel, "retained"), after_retain=True)  # dense indices, no dropped point exists
        exp_dropped = model.insert([more])
        assert [m.insert(d_more)] == exp_dropped and 0 < exp_dropped[0] < 1025
        _check(ctx, m, model, (voxel, "more"))
        m.free()
    for c in clouds + [d_more]:
        c.free()


def test_a_sliding_box_window_over_the_fixture_frames(ctx):
    w = _sample1_world(ctx)
    clouds, poses = w["clouds"][:6], w["poses"][:6]
    first = w["prefixes"][0][0]
    # half-side of the window, from the restatement alone: the median Chebyshev distance of the first frame's map rows
    # to the first pose's translation, so that about half of them survive the first retain
    radius = np.float32(np.median(np.abs(first - poses[0].translation()).max(axis=1)))
    model = _Model(0.02)
    m = DeviceVoxelMap(ctx, 0.02)
    totals, any_removed = [], 0
    for k, (cloud, pose) in enumerate(zip(clouds, poses)):
        assert model.insert([cloud.download()], [pose.to_c()]) == [0]
        assert m.insert(cloud, pose) == 0
        t = pose.translation()
        box = (t - radius, t + radius)
        cells = len(model.expected()[2])
        exp_removed, _, kept = model.retain(box)
        if k == 0:
            assert 0.4 * cells <= kept <= 0.6 * cells
        assert m.retain(box=box) == exp_removed and 0 < kept
        any_removed += exp_removed
        _check(ctx, m, model, k, after_retain=True)
        totals.append(m.total())
    assert any_removed > 0 and totals[-1] < sum(c.len() for c in clouds)  # total follows the window, not the trajectory
    m.free()
