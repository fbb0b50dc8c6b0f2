"""The voxel map at sequence numbers past 2^31 and at the ceiling 2^32 - 2^21 - 1 (a3d_voxel_map_insert / extract / retain,
a3d_voxel_map_nearest_device, a3d_voxel_map_icp_align_device).

Every offered point consumes a 32-bit sequence number, a dropped one too; a 270 k-point frame stream reaches the ceiling
after about 15 900 frames.  Here the numbers are consumed by FILLER: a resident cloud of 2^22 all-NaN points (NaN
normals), inserted one cloud per call (the table is sized for the call's points), about 1 020 calls to the ceiling.  Every
filler call must report all its points dropped and leave cells() alone.  Between the fillers go real pieces: a few
thousand points each on the surfaces of voxel_map_icp_restatement.surfaces at v = 0.05 under a non-zero origin, so
that every piece revisits cells of the earlier ones and newer points both win and lose cells.

The expected value is voxel_map_icp_restatement.SparseMapRestatement: voxel_downsample_cloud of the real points alone,
local indices translated to true sequence numbers (test_voxel_map_sparse_restatement_cpu.py holds it to the plain
restatement with the filler materialised).  Extract (points, normals, order, index as uint32), stats and `nearest` (seq
and d2) are compared bit for bit; the one tolerance is the project's 1e-4 rad / 1e-4 m of a pose against the
restatement's run.  The pieces (their first numbers in brackets):
  P0 [0] | filler | P1 [2^31 - 300, ends above 2^31] | P2 [right behind P1] | filler | P3 [ends at the ceiling]
P1 carries, in cells of their own away from the surfaces, pairs with one member below 2^31 and the other above: mirror
images through the cell centre and exact duplicates (the lower number keeps the tie), a strictly nearer later point
(it takes the cell) and a strictly farther later point (it does not).  The restatement is asserted to contain them.

The module has a context of its own: an extract near the ceiling takes 0.75 GiB of scratch, which the session's shared
context must not keep."""
import ctypes as C
import time

import numpy as np
import pytest

import voxel_map_icp_restatement as R
import voxel_restatement as V
from align3d_amd import A3dError, Context, DevicePointCloud, DeviceVoxelMap, IcpParams, PointCloud, _abi
from gpu_util import small_pose, transform_diff
from test_gpu_voxel_map_icp import _assert_nearest, _assert_pose, _bits, _dev, _inverse, _moved, _snapshot
from test_gpu_voxel_map_retain import _slots_rule

pytestmark = pytest.mark.gpu

VOXEL = 0.05
ORIGIN = (0.013, -0.4, 0.021)
HALF = 1 << 31
CEILING = (1 << 32) - (1 << 21) - 1  # the largest total() the contract admits
FILL = 1 << 22  # filler points per call: the table stays at 2^24 slots
BELOW = 300  # points of P1 below 2^31
PAIRS = 40  # special cells of P1 per kind
KINDS = ("mirror", "duplicate", "nearer later", "farther later")


def _special_pairs(rng):
    """(first [4 PAIRS, 3], second [4 PAIRS, 3]): per kind PAIRS cells of the plane z-cell 40 (z ~ 2 m: the surfaces end
    at 1 m), one pair of points each.  Offsets are multiples of 2^-12 below v / 2 and every coordinate stays inside one
    binade, so centre + d and centre - d are exact and the two distances are the same bits."""
    v, o, half = np.float32(VOXEL), np.asarray(ORIGIN, np.float32), np.float32(0.5)
    cx, cy = np.meshgrid(np.arange(42, 58), np.arange(30, 40), indexing="ij")
    cells = np.stack([cx.ravel(), cy.ravel(), np.full(cx.size, 40)], axis=1).astype(np.float32)
    assert len(cells) == len(KINDS) * PAIRS
    centre = (cells + half) * v + o  # as voxel_key forms it
    assert centre.dtype == np.float32
    d = (rng.integers(8, 90, size=centre.shape) * rng.choice([-1, 1], size=centre.shape) / 4096.0).astype(np.float32)
    first, second = centre + d, centre - d  # kind 0: mirror images
    k = PAIRS
    second[k:2 * k] = first[k:2 * k]  # kind 1: exact duplicates
    second[2 * k:3 * k] = centre[2 * k:3 * k] + d[2 * k:3 * k] * half  # kind 2: the later point is strictly nearer
    first[3 * k:] = centre[3 * k:] + d[3 * k:] * half  # kind 3: the later point is strictly farther
    second[3 * k:] = centre[3 * k:] + d[3 * k:]
    _, key_a, dist_a = V.voxel_keys(first, VOXEL, ORIGIN)
    _, key_b, dist_b = V.voxel_keys(second, VOXEL, ORIGIN)
    assert np.array_equal(key_a, key_b) and len(set(key_a.tolist())) == len(cells)
    bits_a, bits_b = dist_a.view(np.uint32), dist_b.view(np.uint32)
    assert np.array_equal(bits_a[:2 * k], bits_b[:2 * k]) and (bits_b[2 * k:3 * k] < bits_a[2 * k:3 * k]).all()
    assert (bits_b[3 * k:] > bits_a[3 * k:]).all() and not np.array_equal(first[:k], second[:k])
    return first, second


def _across_the_sign_bit(model):
    """(ties, takeovers, holds) among the cells of a SparseMapRestatement, from every real point offered: cells whose
    winner lies below 2^31 with a point at the same distance bits at or above it; cells whose winner lies at or above
    2^31 that hold a point below it (the winner is strictly nearer: a tie would have kept the lower number); cells
    whose winner lies below 2^31 that hold a strictly farther point at or above it."""
    kept, key, dist = V.voxel_keys(model.points_in, model.voxel, model.origin)
    assert kept.all()
    bits, seq = dist.view(np.uint32), model.true_seq
    per_cell = {}
    for i, k in enumerate(key.tolist()):
        per_cell.setdefault(k, []).append(i)
    ties = takeovers = holds = 0
    for k, (win_seq, _) in model.cells.items():
        members = per_cell[k]
        win = next(i for i in members if int(seq[i]) == win_seq)
        high = [i for i in members if int(seq[i]) >= HALF]
        low = [i for i in members if int(seq[i]) < HALF]
        if win_seq < HALF:
            ties += any(bits[i] == bits[win] for i in high)
            holds += any(bits[i] > bits[win] for i in high)
        else:
            assert all(bits[i] > bits[win] for i in low)
            takeovers += bool(low)
    return ties, takeovers, holds


class _World:
    """The pieces on the host, their first sequence numbers, the restatement at every station, queries and an ICP source."""

    def __init__(self):
        rng = np.random.default_rng(2031)
        surf = [R.surfaces(60 + k, 3000) for k in range(5)]
        first, second = _special_pairs(rng)
        order = rng.permutation(len(second))
        normal = lambda n: rng.normal(size=(n, 3)).astype(np.float32)  # noqa: E731 (a normal names its point: duplicates differ in it)
        p1, n1 = surf[1]
        self.specials = len(first)
        cut = BELOW - self.specials
        assert 0 < cut
        piece1 = (np.concatenate([first, p1[:cut], second[order], p1[cut:]]),
                  np.concatenate([normal(len(first)), n1[:cut], normal(len(second)), n1[cut:]]))
        self.pieces = [surf[0], piece1, surf[2], surf[3]]
        self.later = surf[4]  # goes in after the retain by age
        lens = [len(p) for p, _ in self.pieces]
        self.starts = [0, HALF - BELOW, HALF - BELOW + lens[1], CEILING - lens[3]]
        self.ends = [s + n for s, n in zip(self.starts, lens)]
        assert self.starts[1] < HALF < self.ends[1] == self.starts[2] and self.ends[2] < self.starts[3] and self.ends[3] == CEILING
        self.models = [R.SparseMapRestatement([(s, p, n) for s, (p, n) in zip(self.starts[:k + 1], self.pieces[:k + 1])],
                                              VOXEL, ORIGIN) for k in range(4)]
        # by the restatement alone: the pieces share cells and each wins some, and the pairs across 2^31 are there
        final = self.models[3]
        owner = np.searchsorted(np.asarray(self.starts, np.uint64), final.seq.astype(np.uint64), side="right") - 1
        assert all((owner == k).sum() > 200 for k in range(4)) and len(final.rows) < 0.5 * sum(lens)
        ties, takeovers, holds = _across_the_sign_bit(self.models[1])
        assert ties >= 2 * PAIRS and takeovers >= PAIRS and holds >= PAIRS, (ties, takeovers, holds)
        high = self.models[1].seq >= HALF
        assert 100 < high.sum() < len(high) - 100
        qi = rng.integers(0, len(final.rows), size=1000)
        qi[:100] = np.flatnonzero(final.rows[:, 2] > 1.5)[:100]  # the special cells are asked about as well
        self.queries = (final.rows[qi] + rng.uniform(-0.07, 0.07, size=(1000, 3))).astype(np.float32)
        self.offset = small_pose(7, rot=0.01, trans=0.01).to_c()
        self.src_p, self.src_n = _moved(_inverse(self.offset), *R.surfaces(5, 1025, noise=0.002))
        self._cache = {}

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]


@pytest.fixture(scope="module")
def world():
    return _World()


@pytest.fixture(scope="module")
def own_ctx():
    c = Context(0)
    try:
        yield c
    finally:
        c.close()


@pytest.fixture(scope="module")
def filler(own_ctx):
    nan = np.full((FILL, 3), np.nan, np.float32)
    cloud = DevicePointCloud(own_ctx, PointCloud(nan, nan.copy()))
    yield cloud
    cloud.free()


@pytest.fixture(scope="module")
def seen():
    """What one route leaves for the next to compare with."""
    return {}


def _part(cloud, a, b):
    """Points a ... b-1 of a resident cloud as a cloud of their own (a view: it owns nothing and is never freed)."""
    assert 0 <= a <= b <= cloud.n
    v = DevicePointCloud.__new__(DevicePointCloud)
    v.ctx, v.n = cloud.ctx, b - a
    v.d_points = C.c_void_p(cloud.d_points.value + 12 * a)
    v.d_normals = C.c_void_p(cloud.d_normals.value + 12 * a)
    return v


def _fill_to(m, filler, target, timing):
    """Consumes sequence numbers up to total() == target with NaN points, one cloud of at most FILL per call."""
    total, cells = m.total(), m.cells()
    assert total <= target
    t0, calls = time.perf_counter(), 0
    while total < target:
        n = min(FILL, target - total)
        assert m.insert(filler if n == FILL else _part(filler, 0, n)) == n  # every point is dropped
        total += n
        calls += 1
        assert m.cells() == cells
    assert m.total() == target
    timing[0] += time.perf_counter() - t0
    timing[1] += calls


def _check(ctx, m, model, total, queries, label, want_nearest=None):
    """Extract with its index, stats and `nearest` against a restated map at `total` offered points, bit for bit.
    Returns (index, nearest seq) as the device gave them."""
    cloud, index = m.extract(return_index=True)
    p, n = cloud.download()
    cloud.free()
    assert index.dtype == np.uint32 and np.array_equal(index, model.seq), (label, "index")
    assert np.array_equal(_bits(p), _bits(model.rows)) and np.array_equal(_bits(n), _bits(model.normals)), (label, "rows")
    s = m.stats()
    offered = len(model.true_seq) if hasattr(model, "true_seq") else total
    assert (s["cells"], s["total"], s["dropped_total"]) == (len(model.rows), total, total - offered + model.dropped), (label, s)
    want = model.nearest(queries) if want_nearest is None else want_nearest
    assert 0.5 * len(queries) < (want[2] >= 0).sum()
    got = m.nearest(queries)
    _assert_nearest(got, want, label)
    return index, got[0]


def _to_the_top(ctx, world, filler, grouped):
    """A new map taken through stations 1 (P0), 2 (P1, P2: across 2^31) and 3 (P3: the ceiling), checked at each.
    grouped=False: a real piece per insert call.  grouped=True: the same points as other clouds and calls: P0 as two
    clouds of one call; P1 cut exactly at 2^31 and P2 in one call of three clouds; P3 as clouds of 1, 2 048 and the rest."""
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN)
    clouds = [_dev(ctx, p, n) for p, n in world.pieces]
    timing = [0.0, 0]
    try:
        bounds = []
        # station 1: low numbers
        bounds.append(m.total())
        if grouped:
            assert m.insert_many([_part(clouds[0], 0, 1500), _part(clouds[0], 1500, clouds[0].n)]) == [0, 0]
        else:
            assert m.insert(clouds[0]) == 0
        _check(ctx, m, world.models[0], world.ends[0], world.queries, "station 1")
        # station 2: a piece that starts below 2^31 and ends above it, and the next frame right behind it
        _fill_to(m, filler, world.starts[1], timing)
        bounds.append(m.total())
        if grouped:
            bounds.append(world.starts[2])
            assert m.insert_many([_part(clouds[1], 0, BELOW), _part(clouds[1], BELOW, clouds[1].n), clouds[2]]) == [0, 0, 0]
        else:
            assert m.insert(clouds[1]) == 0
            assert m.stats()["total"] == world.ends[1] >= HALF
            index, near = _check(ctx, m, world.models[1], world.ends[1], world.queries, "station 2, the straddling piece")
            assert (index >= HALF).any() and (index < HALF).any()
            assert ((near >= HALF) & (near != R.NONE_SEQ)).sum() > 50 and (near < HALF).sum() > 50
            bounds.append(m.total())
            assert m.insert(clouds[2]) == 0
        assert m.stats()["total"] == world.ends[2] >= HALF  # the regime is entered
        index, near = _check(ctx, m, world.models[2], world.ends[2], world.queries, "station 2")
        assert (index >= HALF).any() and ((near >= HALF) & (near != R.NONE_SEQ)).any()
        # station 3: the last piece ends at the largest total the contract admits
        _fill_to(m, filler, world.starts[3], timing)
        bounds.append(m.total())
        if grouped:
            assert m.insert_many([_part(clouds[3], 0, 1), _part(clouds[3], 1, 2049), _part(clouds[3], 2049, clouds[3].n)]) == [0, 0, 0]
        else:
            assert m.insert(clouds[3]) == 0
        assert m.stats()["total"] == CEILING == 2**32 - 2**21 - 1
        index, near = _check(ctx, m, world.models[3], CEILING, world.queries, "station 3")
        assert (index >= HALF).any() and (index >= world.starts[3]).any() and ((near >= world.starts[3]) & (near != R.NONE_SEQ)).any()
        assert bounds == world.starts
        print(f"filler: {timing[1]} calls of up to 2^22 points, {1e3 * timing[0] / timing[1]:.3f} ms per call, {timing[0]:.2f} s in all")
    except BaseException:
        m.free()
        raise
    finally:
        for c in clouds:
            c.free()
    return m


def _refused_at_the_top(ctx, m, one):
    """At the ceiling a one-point cloud is refused, an empty one is accepted, and neither changes the map."""
    before = _snapshot(m)
    with pytest.raises(A3dError) as e:
        m.insert(one)
    assert e.value.status == _abi.A3D_INVALID_PARAMETER
    empty = DevicePointCloud._allocate(ctx, 0, True)
    assert m.insert(empty) == 0
    empty.free()
    assert _snapshot(m) == before and m.total() == CEILING


def _align_at_the_top(ctx, world, m):
    src = _dev(ctx, world.src_p, world.src_n)
    prm = IcpParams(max_iterations=5)
    status, want = world.cached("align", lambda: world.models[3].align(world.src_p, world.src_n, prm.to_c()))
    assert status == _abi.A3D_OK
    got = m.align(src, prm)
    src.free()
    _assert_pose(got, want, "at the ceiling")
    ang, tr = transform_diff(got, world.offset)
    assert ang < 2e-3 and tr < 2e-3, (ang, tr)
    return bytes(got.to_c())


def test_stations_low_across_the_sign_bit_at_the_ceiling_and_a_retain_by_age(own_ctx, world, filler, seen):
    ctx = own_ctx
    m = _to_the_top(ctx, world, filler, grouped=False)
    one = _dev(ctx, world.later[0][:1], world.later[1][:1])
    later = _dev(ctx, *world.later)
    try:
        _refused_at_the_top(ctx, m, one)
        seen["pose at the ceiling"] = _align_at_the_top(ctx, world, m)
        # station 4: retain by age across the sign bit, from the first frame boundary above 2^31
        min_seq = world.starts[2]
        assert HALF < min_seq < HALF + (1 << 20)
        marks = np.asarray(world.starts + [0, CEILING, CEILING + 1, 1 << 63], np.uint64)
        survivors, exp_removed, exp_marks, k = R.retained(world.models[3], min_seq=min_seq, marks=marks, total=CEILING)
        assert 500 < k < len(world.models[3].rows) - 500 and exp_marks[:4] == [0, 0, 0, exp_marks[3]] and 0 < exp_marks[3] < k
        assert exp_marks[4:] == [0, k, k, k]
        removed, new_marks = m.retain(min_seq=min_seq, marks=marks)
        assert removed == exp_removed and new_marks.dtype == np.uint64 and new_marks.tolist() == exp_marks
        assert m.total() == m.cells() == k and m.stats()["slots"] == _slots_rule(k)
        _check(ctx, m, survivors, k, world.queries, "station 4")
        # the contract of a retain: a new map into which the survivors went as one cloud, then the next piece
        after = R.SparseMapRestatement([(0, survivors.rows, survivors.normals), (k, *world.later)], VOXEL, ORIGIN)
        assert m.insert(later) == 0
        index, _ = _check(ctx, m, after, k + len(world.later[0]), world.queries, "station 4, a later piece")
        assert 100 < (index >= k).sum() and 100 < (index < k).sum()  # the later piece wins cells and loses cells
    finally:
        m.free(), one.free(), later.free()


def test_other_grouping_to_the_ceiling_then_a_compaction(own_ctx, world, filler, seen):
    ctx = own_ctx
    m = _to_the_top(ctx, world, filler, grouped=True)  # the same expected arrays as the first route: whatever the grouping
    one = _dev(ctx, world.later[0][:1], world.later[1][:1])
    try:
        _refused_at_the_top(ctx, m, one)
        pose = _align_at_the_top(ctx, world, m)
        assert seen.get("pose at the ceiling", pose) == pose  # the grouping leaves no trace in the pose bits either
        # station 5: compact from the top
        model = world.models[3]
        renumbered = model.renumbered()
        k = len(model.rows)
        assert m.compact() == 0
        assert m.total() == m.cells() == k and m.stats()["slots"] == _slots_rule(k) and m.stats()["dropped_total"] == 0
        want = renumbered.nearest(world.queries)
        assert np.array_equal(want[2], model.nearest(world.queries)[2])  # the same rows under their ranks
        _check(ctx, m, renumbered, k, world.queries, "station 5", want)
        assert _align_at_the_top(ctx, world, m) == pose  # a winner's number feeds the tie-break only, never the sums
        # the insert that the ceiling refused succeeds now
        after = R.SparseMapRestatement([(0, renumbered.rows, renumbered.normals), (k, world.later[0][:1], world.later[1][:1])],
                                       VOXEL, ORIGIN)
        assert m.insert(one) == 0
        _check(ctx, m, after, k + 1, world.queries, "station 5, one more point")
    finally:
        m.free(), one.free()


def test_retain_by_box_and_age_together_above_the_sign_bit(own_ctx, world, filler):
    """Station 6: a map taken to P2 (total just above 2^31); the rule cuts P1 above 2^31 by age and the scene by a box."""
    ctx = own_ctx
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN)
    clouds = [_dev(ctx, p, n) for p, n in world.pieces[:3]]
    timing = [0.0, 0]
    try:
        assert m.insert(clouds[0]) == 0
        _fill_to(m, filler, world.starts[1], timing)
        assert m.insert_many(clouds[1:]) == [0, 0]
        print(f"filler: {timing[1]} calls of up to 2^22 points, {1e3 * timing[0] / timing[1]:.3f} ms per call, {timing[0]:.2f} s in all")
        model, total = world.models[2], world.ends[2]
        assert m.stats()["total"] == total >= HALF
        min_seq = HALF + 1000
        box = ((-0.1, 0.2, -0.1), (1.0, 1.2, 3.0))
        marks = np.asarray([0, HALF - 1, HALF, min_seq, world.starts[2], total, total + 7], np.uint64)
        survivors, exp_removed, exp_marks, k = R.retained(model, min_seq=min_seq, box=box, marks=marks, total=total)
        by_box, by_age = R.retained(model, box=box, total=total)[3], R.retained(model, min_seq=min_seq, total=total)[3]
        assert 200 < k < min(by_box, by_age) - 200  # both conditions bite
        inside = ((model.rows >= np.float32(box[0])) & (model.rows <= np.float32(box[1]))).all(axis=1)
        seq = model.seq.astype(np.uint64)
        assert ((seq >= HALF) & (seq < min_seq) & inside).sum() > 50  # removed by age alone, at numbers above 2^31
        assert ((seq >= min_seq) & ~inside).sum() > 50  # removed by the box alone, at numbers above 2^31
        assert exp_marks[:4] == [0, 0, 0, 0] and 0 < exp_marks[4] < k and exp_marks[5:] == [k, k]
        removed, new_marks = m.retain(box=box, min_seq=min_seq, marks=marks)
        assert removed == exp_removed and new_marks.tolist() == exp_marks
        assert m.total() == m.cells() == k and m.stats()["slots"] == _slots_rule(k)
        rng = np.random.default_rng(6)  # queries around the survivors: the box has removed most of what world.queries ask for
        queries = (survivors.rows[rng.integers(0, k, size=1000)] + rng.uniform(-0.07, 0.07, size=(1000, 3))).astype(np.float32)
        _check(ctx, m, survivors, k, queries, "station 6")
    finally:
        m.free()
        for c in clouds:
            c.free()
