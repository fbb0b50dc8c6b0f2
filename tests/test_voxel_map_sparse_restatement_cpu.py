"""The helpers that restate a voxel map at sparse sequence numbers, a retain of it, and a periodic source
(voxel_map_icp_restatement.py: SparseMapRestatement, retained, PeriodicSource) against the plain restatement they
abbreviate, at sizes where the plain one can still be formed.  No GPU: both sides are numpy and the oracle."""
import numpy as np

import voxel_map_icp_restatement as R
from align3d_amd import IcpParams
from gpu_util import small_pose
from test_gpu_voxel_map_retain import BOX, CONTENTS, ORIGIN as RETAIN_ORIGIN, _Model, _cube

VOXEL = 0.1
ORIGIN = (0.013, -0.4, 0.021)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_sparse_restatement_is_the_plain_one_with_the_filler_materialised():
    reals = [R.surfaces(40 + k, n) for k, n in enumerate((300, 257, 411))]
    fillers = (3000, 4097, 2500)  # NaN points behind each real cloud: dropped, they only consume numbers
    merged_p, merged_n, pieces, at = [], [], [], 0
    for (p, n), gap in zip(reals, fillers):
        pieces.append((at, p, n))
        merged_p += [p, np.full((gap, 3), np.nan, np.float32)]
        merged_n += [n, np.full((gap, 3), np.nan, np.float32)]
        at += len(p) + gap
    plain = R.MapRestatement(np.concatenate(merged_p), np.concatenate(merged_n), VOXEL, ORIGIN)
    sparse = R.SparseMapRestatement(pieces, VOXEL, ORIGIN)
    assert plain.dropped == sum(fillers) and sparse.dropped == 0
    assert 300 < len(plain.rows) < 900  # cells are shared: later clouds win some and lose some
    owner = np.searchsorted([s for s, _, _ in pieces], plain.seq, side="right") - 1
    assert all(50 < (owner == k).sum() for k in range(3))
    assert sparse.seq.dtype == np.uint32 and np.array_equal(sparse.seq, plain.seq)
    assert np.array_equal(_bits(sparse.rows), _bits(plain.rows)) and np.array_equal(_bits(sparse.normals), _bits(plain.normals))
    assert sparse.cells == plain.cells
    assert np.array_equal(sparse.true_seq[sparse.local], plain.seq) and sparse.local.max() < sum(len(p) for p, _ in reals)
    rng = np.random.default_rng(3)
    q = (plain.rows[rng.integers(0, len(plain.rows), size=400)] + rng.uniform(-0.15, 0.15, size=(400, 3))).astype(np.float32)
    want, got = plain.nearest(q), sparse.nearest(q)
    assert 100 < (want[2] >= 0).sum() < 400
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    pose = small_pose(4, rot=0.05, trans=0.05).to_c()
    for a, b in zip(sparse.nearest(q, pose), plain.nearest(q, pose)):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_periodic_source_is_the_plain_computation_on_the_repeated_source():
    model = R.MapRestatement(*R.surfaces(1, 1500), 0.05, ORIGIN)
    period_p, period_n = R.surfaces(5, 50, noise=0.002)
    m = 3 * 50 + 17  # three periods and a ragged remainder
    reps = -(-m // 50)
    long_p, long_n = np.tile(period_p, (reps, 1))[:m], np.tile(period_n, (reps, 1))[:m]
    view = R.PeriodicSource(model, m)
    pose = small_pose(2).to_c()
    for T in (None, pose):
        for a, b in zip(view.nearest(period_p, T), model.nearest(long_p, T)):
            assert len(a) == m and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                  b.view(np.uint32) if b.dtype == np.float32 else b)
    prm = IcpParams(max_iterations=4).to_c()
    r, J, kept = view.point_terms_kept(period_p, period_n, pose, prm)
    r2, J2, kept2 = model.point_terms_kept(long_p, long_n, pose, prm)
    assert 50 < len(r) < m and np.array_equal(kept, kept2) and kept.max() >= 150  # some points fail a gate, the tail is served
    assert np.array_equal(_bits(r), _bits(r2)) and np.array_equal(_bits(J), _bits(J2))
    a, b = view.accumulate(period_p, period_n, pose, prm), model.accumulate(long_p, long_n, pose, prm)
    assert a["count"] == b["count"] == len(r) and a["ssq"] == b["ssq"]
    assert np.array_equal(_bits(a["H"]), _bits(b["H"])) and np.array_equal(_bits(a["g"]), _bits(b["g"]))
    assert bytes(view.gn_state(period_p, period_n, pose, prm)) == bytes(model.gn_state(long_p, long_n, pose, prm))
    (sa, Ta), (sb, Tb) = view.align(period_p, period_n, prm), model.align(long_p, long_n, prm)
    assert sa == sb == 0 and bytes(Ta) == bytes(Tb) and bytes(Ta) != bytes(R.O.pose())


def test_retained_agrees_with_the_model_of_the_retain_tests():
    """The case (1024, 1025) x "both" (box and min_seq) x v = 0.5 x origin of test_gpu_voxel_map_retain.py, with marks."""
    sizes, voxel = CONTENTS[1], 0.5
    hosts = [_cube(100 + k, n) for k, n in enumerate(sizes)]
    theirs = _Model(voxel, RETAIN_ORIGIN)
    theirs.insert(hosts)
    total = theirs.total()
    min_seq = int(total / 5)
    marks = [0, sizes[0], 777, total, total + 1, 1 << 63]
    ours = R.MapRestatement(theirs.p, theirs.n, voxel, RETAIN_ORIGIN)
    survivors, removed, new_marks, k = R.retained(ours, min_seq=min_seq, box=BOX, marks=marks, total=total)
    by_box = R.retained(ours, box=BOX, total=total)[3]
    by_age = R.retained(ours, min_seq=min_seq, total=total)[3]
    assert 0 < k < min(by_box, by_age) and max(by_box, by_age) < len(ours.rows)  # both conditions bite
    assert theirs.retain(BOX, min_seq, marks) == (removed, new_marks, k)
    assert new_marks[0] == 0 and new_marks[-3:] == [k, k, k] and 0 < new_marks[2] < k
    assert np.array_equal(_bits(survivors.rows), _bits(theirs.p)) and np.array_equal(_bits(survivors.normals), _bits(theirs.n))
    # the survivors as one cloud, then a later cloud: the retain tests' model of what follows
    later = _cube(900, 1025)
    theirs.insert([later])
    after = R.SparseMapRestatement([(0, survivors.rows, survivors.normals), (k, *later)], voxel, RETAIN_ORIGIN)
    exp = theirs.expected()
    assert np.array_equal(_bits(after.rows), _bits(exp[0])) and np.array_equal(after.seq, exp[2])
