"""GPU parity for the paths of IcpBatch (a3d_pcl_icp_batch_*) and the one-pair Icp that tests/test_gpu_pcl_icp_batch.py,
test_gpu_pcl_icp.py and test_gpu_pcl_icp_deep.py never reach: the "return the best transform" rule
(src/icp/pcl_icp.rs:94-106), even and tiny iteration counts (the state / partials ping-pong on seq & 1), the three
tile-count paths of head_sum_and_advance and its loop running more than once, more pairs than CUs, one handle over
passes of different geometry, the per-pair LDS depth of a batch, non-default gates, unaligned views, the empty batch.

The reference everywhere is the sequential CPU oracle (orc_kdtree_new + orc_pcl_icp_align, with its trace where the
test needs it), pair by pair; the bound is the project's parity bound, 1e-4 rad / 1e-4 m, with equal status words.

Best is not last (BEST_CASES).  On the pairs of the existing suite the oracle's best pose is within the bound of its
last pose (2.4e-6 .. 1.4e-4 rad), so a kernel that returned the last pose would pass there.  Searched on the CPU with
the oracle's trace: sample1 target frame 0 against source frames 1, 5, 10, 13, 16, 19, both cut [0::64], [7::64],
[0::128], [7::128]; 6 and 15 iterations; weight 0.45, 0.7, 1, 2, 3; max_distance 0.05, 0.1, 0.5; max_normal_angle
default and 0.2.  What they gave:
 * weight 1 (default): 2 of 288 combinations meet the conditions (0<-13 [7::128]); none of the near frames does.
 * weight 0.45 (a step of 2.2 Newton steps: the iteration diverges): the best pose is the one after the first update
   and 0.03 .. 0.5 rad from the last, but the oracle's own answer moves by up to 3.6e-4 rad / 3.0e-4 m when every
   source coordinate is shifted by at most one ulp: above the bound, not used.
 * weight 0.7 (overshoots, the sign of the error alternates): best = iteration 4 of 6, 1e-3 from the last pose, but the
   oracle moves by up to 1.2e-4 / 1.0e-4 under the one-ulp shift: at the bound, not used.
 * weight 2 and 3 (a half and a third of a Newton step: the pose is still moving when the mean residual, which rises
   again as more correspondences pass the gates, has had its minimum): the three cases used.  Under the one-ulp shift
   (three seeds) the argmin stays where it is and the oracle moves by at most 8.9e-6 rad / 8.9e-6 m.
Their traces (mean squared residual per iteration, ^ = the minimum; margin = (second lowest - lowest) / lowest; the
last column is best pose against last pose):
 "w2 0<-19": frames 0 <- 19 [7::128] (2111 <- 2108 points), 15 iterations, weight 2, max_distance 0.5, angle 0.2
    5.9846e-4 2.0416e-4 9.0690e-5 5.5297e-5 4.8077e-5 ^4.5311e-5 4.6189e-5 4.6120e-5 4.6029e-5 4.6597e-5 4.6631e-5
    4.6542e-5 4.6585e-5 4.6585e-5 4.6453e-5            best = 5, margin 1.58e-2, 1.35e-3 rad / 7.80e-4 m
 "w2 0<-16": frames 0 <- 16 [7::128] (2111 <- 2110 points), 15 iterations, weight 2, max_distance 0.5
    5.5417e-4 1.8747e-4 7.6421e-5 5.0110e-5 3.7687e-5 3.5691e-5 ^3.3909e-5 3.5097e-5 3.5192e-5 3.4986e-5 3.4723e-5
    3.4727e-5 3.4727e-5 3.4748e-5 3.4748e-5            best = 6, margin 2.40e-2, 8.85e-4 rad / 3.67e-4 m
 "w3 0<-19": frames 0 <- 19 [7::128], 15 iterations, weight 3, max_distance 0.5
    5.6475e-4 3.1835e-4 1.8498e-4 1.1555e-4 8.2824e-5 6.4390e-5 5.6013e-5 5.2584e-5 5.1552e-5 ^5.1101e-5 5.1714e-5
    5.1684e-5 5.1588e-5 5.1681e-5 5.1691e-5            best = 9, margin 8.83e-3, 9.93e-4 rad / 3.50e-4 m
No case has its minimum at iteration 0, so each of them also fails a `best` that is stored once and never updated.
Real data reaches 5e-4: the synthetic height field was not needed.

Gates (GATED): weight 0.7, max_distance 0.05, max_normal_angle 0.2, 4 iterations.  orc_pcl_icp_accumulate at the
identity counts 2271 / 2262 / 4459 correspondences on the three pairs of gated_pairs() against 3332 / 3328 / 6674
with the default parameters (the angle gate does most of it: 2276 with the angle alone, 3325 with the distance alone),
and the oracle moves by at most 1.5e-5 rad / 1.8e-5 m under the one-ulp shift.

Under a reordering of the source (reversed, three random orders: what the GPU changes is the order of the sums) the
oracle's answer moves by at most 1.1e-7 for the best cases, the pairs of counted_pairs() at every iteration count and
gated_pairs().

More pairs than CUs (many_pairs): every one of the first 293 pairs was run through the oracle on the CPU, in four
source orders, before the first GPU run: see many_pairs()."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import A3dError, DevicePointCloud, Icp, IcpBatch, IcpParams, PointCloud, _abi
from align3d_amd._abi import GnStateC, PoseC
from gpu_util import transform_diff
from test_gpu_pcl_icp_batch import BOUND, RAGGED_FAILS, _bits, _cloud, _Resident, _spread, _sub, ragged_pairs

gpu = pytest.mark.gpu  # (the two tests of the oracle-side conditions alone run without a GPU)

IDENTITY_BITS = np.array([0, 0, 0, 0, 0, 0, 1], np.float32).view(np.uint32)
_KNOBS = ("A3D_PCLB_BLOCK", "A3D_PCLB_LDS_LEVELS", "A3D_PCLB_BLOCKS_PER_CU")


# ---- inputs: every host cloud exists once per session, so that the oracle's answers can be shared ------------------

@functools.lru_cache(maxsize=None)
def _frame(k):
    return _cloud(k)


@functools.lru_cache(maxsize=None)
def _cut(k, first, step):
    """Points first, first + step, ... of sample1 frame k."""
    return _sub(_frame(k), slice(first, None, step))


@functools.lru_cache(maxsize=None)
def _far(k, first, step):
    """_cut(k, first, step) 100 m away: no correspondence, count == 0, the oracle's solve() fails in iteration 0."""
    c = _cut(k, first, step)
    return PointCloud(c.points + np.float32(100.0) * np.asarray([1, 0, 0], np.float32), c.normals)


@functools.lru_cache(maxsize=None)
def _ragged():
    return ragged_pairs()


def _key(prm):
    return dataclasses.astuple(prm)


_trees, _answers = {}, {}


def _tree(tgt):
    if id(tgt) not in _trees:
        _trees[id(tgt)] = (O.KdTree(tgt.points), tgt)  # (keeps the cloud alive: its id stays its own)
    return _trees[id(tgt)][0]


def oracle_trace(prm, tgt, src):
    """(status, pose, trace [max_iterations][8] = residual, t, q after the update) of the oracle; computed once per
    (params, target, source) and per session.  After a failed solve() the oracle's pose is set to the identity here
    (the reference panics; the product freezes the pair, and a pair that fails in iteration 0 is still at eye())."""
    key = (_key(prm), id(tgt), id(src))
    if key not in _answers:
        out = PoseC()
        trace = np.zeros((max(1, int(prm.max_iterations)), 8), np.float32)
        tv, sv = O.pcl_view(tgt.points, tgt.normals), O.pcl_view(src.points, src.normals)
        p = prm.to_c()
        st = O.load().orc_pcl_icp_align(C.byref(p), _tree(tgt).h, C.byref(tv), C.byref(sv), C.byref(out), O.ptr(trace))
        if st != 0:
            out = O.pose()
        _answers[key] = (st, out, trace[:int(prm.max_iterations)], src)
    return _answers[key][:3]


def oracle_count(prm, tgt, src):
    """Correspondences that pass the gates at the identity."""
    g = GnStateC()
    tv, sv = O.pcl_view(tgt.points, tgt.normals), O.pcl_view(src.points, src.normals)
    p, eye = prm.to_c(), O.pose()
    assert O.load().orc_pcl_icp_accumulate(C.byref(p), _tree(tgt).h, C.byref(tv), C.byref(sv), C.byref(eye), 1,
                                           C.byref(g)) == 0
    return g.as_dict()["count"]


def _with_knobs(monkeypatch, knobs, make):
    """make() with the diagnostics build's launch knobs set: they are read where the handle is created, only there."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    try:
        return make()
    finally:
        for k in knobs:
            monkeypatch.delenv(k, raising=False)


def _compare(prm, pairs, poses, status, label, fails=(), each=True):
    """Pair by pair against the oracle: equal status words, the pose within the bound (a failed pair: the identity,
    bit for bit).  Prints the worst differences; returns them."""
    bits, _ = _bits(poses, status)
    expected = np.zeros(len(pairs), np.int32)
    worst_a = worst_t = 0.0
    for k, ((tgt, src), T) in enumerate(zip(pairs, poses)):
        st, ref, _ = oracle_trace(prm, tgt, src)
        assert st == (_abi.A3D_SOLVE_FAILED if k in fails else 0), f"{label} pair {k}: oracle status {st}"
        expected[k] = st
        if st != 0:
            assert np.array_equal(bits[k], IDENTITY_BITS), f"{label} pair {k}: a failed pair must stay at the identity"
        ang, tr = transform_diff(T, ref)
        if each:
            print(f"[{label} it={prm.max_iterations} pair {k}: n={tgt.len()} m={src.len()}] d_angle={ang:.3e} "
                  f"d_trans={tr:.3e} status={status[k]}")
        worst_a, worst_t = max(worst_a, ang), max(worst_t, tr)
    print(f"[{label} it={prm.max_iterations} worst of {len(pairs)} pairs] d_angle={worst_a:.3e} d_trans={worst_t:.3e}")
    assert np.array_equal(status, expected), (label, status, expected)
    assert worst_a <= BOUND and worst_t <= BOUND, (label, worst_a, worst_t)
    return worst_a, worst_t


def _batch_parity(ctx, prm, pairs, label, fails=(), make_batch=IcpBatch, each=True):
    up = _Resident(ctx)
    batch = make_batch(ctx, prm, [up(t) for t, _ in pairs])
    poses, status = batch.align([up(s) for _, s in pairs])
    batch.free()
    up.free()
    return _compare(prm, pairs, poses, status, label, fails, each)


def _num_cus(ctx):
    """The device's compute units as the library counts them (hipDeviceProp_t::multiProcessorCount, what
    torch.cuda.get_device_properties(0).multi_processor_count reads; torch does not see the GPU on every box that has
    one, see test_gpu_multirank.py)."""
    cus = ctx.num_cus()
    assert cus > 0
    return cus


def _tiles(num_cus, n_pairs, max_m, block=1024, per_cu=1):
    """Blocks per pair of a pass = the tile count its head sums (batch_geometry + a3d_pcl_icp_batch_align_device)."""
    return min(max(1, num_cus * per_cu // n_pairs), -(-max_m // block))


# ---- A. best is not last ----------------------------------------------------------------------------------------------

BEST_CASES = {
    "w2 0<-19": (0, 19, dict(max_iterations=15, weight=2.0, max_distance=0.5, max_normal_angle=0.2)),
    "w2 0<-16": (0, 16, dict(max_iterations=15, weight=2.0, max_distance=0.5)),
    "w3 0<-19": (0, 19, dict(max_iterations=15, weight=3.0, max_distance=0.5)),
}


def best_case(name):
    tf, sf, kw = BEST_CASES[name]
    return IcpParams(**kw), _cut(tf, 7, 128), _cut(sf, 7, 128)


def best_case_facts(prm, tgt, src):
    """(index of the lowest residual, its relative margin to the second lowest, angle and translation between the
    oracle's best pose and its last pose) from the oracle's trace."""
    st, best, trace = oracle_trace(prm, tgt, src)
    assert st == 0
    res = trace[:, 0].astype(np.float64)
    assert np.all(np.isfinite(res)) and np.all(res > 0)
    k = int(np.argmin(res))
    margin = float((np.delete(res, k).min() - res[k]) / res[k])
    assert list(O.pose_tuple(best)[0]) == list(trace[k, 1:4]) and list(O.pose_tuple(best)[1]) == list(trace[k, 4:8])
    ang, tr = O.transform_metrics(best, O.pose(trace[-1, 1:4], trace[-1, 4:8]))
    return k, margin, ang, tr


def assert_best_is_not_last(prm, tgt, src, name):
    k, margin, ang, tr = best_case_facts(prm, tgt, src)
    print(f"[best case {name}] lowest residual at iteration {k} of {prm.max_iterations}, margin {margin:.2e}, best against "
          f"last pose {ang:.2e} rad / {tr:.2e} m")
    assert k != prm.max_iterations - 1, "the lowest residual must not be the last iteration's"
    assert margin >= 1e-3, "the argmin must be decided by the data, not by the summation order"
    assert max(ang, tr) >= 5e-4, "returning the last pose must miss the bound five times over"
    return k


def test_best_cases_cover_a_late_minimum():
    """A `best` that is stored once and never updated passes a case whose minimum is at iteration 0."""
    assert any(best_case_facts(*best_case(name))[0] != 0 for name in BEST_CASES)



@gpu
@pytest.mark.parametrize("name", list(BEST_CASES))
def test_best_is_not_last(ctx, name):
    prm, tgt, src = best_case(name)
    assert_best_is_not_last(prm, tgt, src, name)
    _, ref, trace = oracle_trace(prm, tgt, src)
    last = O.pose(trace[-1, 1:4], trace[-1, 4:8])

    def check(T, what):
        ang, tr = transform_diff(T, ref)
        la, lt = transform_diff(T, last)
        print(f"[best {name} {what}] d_angle={ang:.3e} d_trans={tr:.3e} (against the oracle's last pose {la:.3e} / {lt:.3e})")
        assert ang <= BOUND and tr <= BOUND, (what, ang, tr)

    icp = Icp.new(ctx, prm, tgt)
    check(icp.align(src), "Icp, host clouds")
    icp.free()
    up = _Resident(ctx)
    icp = Icp.new(ctx, prm, up(tgt))
    check(icp.align(up(src)), "Icp, resident clouds")
    icp.free()
    up.free()
    # in a batch, behind an ordinary pair that runs under the same parameters
    pairs = [(_cut(0, 0, 64), _cut(1, 0, 64)), (tgt, src)]
    _batch_parity(ctx, prm, pairs, f"best {name} batch")


# ---- B. iteration counts ----------------------------------------------------------------------------------------------

def counted_pairs():
    """Three small pairs; the middle one fails (its source is 100 m away)."""
    return [(_cut(0, 0, 64), _cut(1, 0, 64)), (_cut(1, 3, 64), _far(2, 3, 64)), (_cut(2, 5, 64), _cut(3, 5, 96))]


@gpu
@pytest.mark.parametrize("iterations", [0, 1, 2, 4, 6])
def test_iteration_counts(ctx, iterations):
    prm = IcpParams(max_iterations=iterations)
    pairs = counted_pairs()
    fails = {1} if iterations else set()  # with no iteration the reference never calls solve()
    up = _Resident(ctx)
    batch = IcpBatch(ctx, prm, [up(t) for t, _ in pairs])
    poses, status = batch.align([up(s) for _, s in pairs])
    batch.free()
    _compare(prm, pairs, poses, status, "iterations batch", fails)
    if iterations == 0:
        assert list(status) == [0, 0, 0]
        assert all(np.array_equal(b, IDENTITY_BITS) for b in _bits(poses, status)[0])
    # the one-pair form, host and resident clouds
    for k, (tgt, src) in enumerate(pairs):
        st, ref, _ = oracle_trace(prm, tgt, src)
        for what, t, s in (("host", tgt, src), ("resident", up(tgt), up(src))):
            icp = Icp.new(ctx, prm, t)
            if k in fails:
                with pytest.raises(A3dError) as e:
                    icp.align(s)
                assert e.value.status == _abi.A3D_SOLVE_FAILED == st
            else:
                T = icp.align(s)
                ang, tr = transform_diff(T, ref)
                print(f"[iterations Icp {what} it={iterations} pair {k}] d_angle={ang:.3e} d_trans={tr:.3e}")
                assert st == 0 and ang <= BOUND and tr <= BOUND, (what, k, ang, tr)
                if iterations == 0:
                    assert np.array_equal(_bits([T], [0])[0][0], IDENTITY_BITS)
            icp.free()
    up.free()


# ---- C. the three paths of the head's partial sum, product library ---------------------------------------------------

def full_pairs(n):
    """n full-cloud pairs over two targets (the oracle builds two trees)."""
    return [(_frame(0), _frame(1)), (_frame(1), _frame(2)), (_frame(0), _frame(2)), (_frame(1), _frame(0)),
            (_frame(0), _frame(3))][:n]


@gpu
def test_head_sum_paths(ctx):
    """head_sum_and_advance: the 32-deep loop (a slice t with t + 248 < tiles), the 32-wide masked round (t + 56 < tiles)
    and the 8-wide masked round, chosen by the tile count, which 1 .. 5 full-cloud pairs move through all three."""
    cus = _num_cus(ctx)
    prm = IcpParams(max_iterations=5)
    tiles = {}
    for n in range(1, 6):
        tiles[n] = _tiles(cus, n, max(s.len() for _, s in full_pairs(n)))
    print(f"[head sum paths] {cus} CUs, tiles per pair by batch size: {tiles}")
    covered = (any(t > 256 - 8 for t in tiles.values()), any(57 <= t <= 256 for t in tiles.values()),
               any(t <= 56 for t in tiles.values()))
    if not all(covered):
        pytest.skip(f"{cus} CUs: batches of 1 .. 5 full pairs give {tiles} tiles per pair, which does not reach all of "
                    f"> 248, 57 .. 256 and <= 56 (reached: {covered})")
    for n in range(1, 6):
        _batch_parity(ctx, prm, full_pairs(n), f"head sum P={n} tiles={tiles[n]}")


# ---- D. the head's loop and the geometry knobs, diagnostics library ------------------------------------------------------

@gpu
def test_head_sum_loop_rounds_and_ragged_tail(diag_ctx, monkeypatch):
    """256-thread blocks, eight per CU: one full pair is cut into more than 1 000 tiles, so the 32-deep loop runs several
    times and leaves a tail that is no multiple of 8; with two pairs of different length one pair's trailing blocks
    store zero partials."""
    cus = _num_cus(diag_ctx)
    prm = IcpParams(max_iterations=5)
    knobs = {"A3D_PCLB_BLOCK": 256, "A3D_PCLB_BLOCKS_PER_CU": 8}

    def make(ctx, prm, targets):
        return _with_knobs(monkeypatch, knobs, lambda: IcpBatch(ctx, prm, targets))

    full1 = _frame(1)
    cut = _head_loop_source()
    for pairs in ([(_frame(0), cut)], [(_frame(0), full1), (_frame(1), _cut(2, 0, 3))]):
        t = _tiles(cus, len(pairs), max(s.len() for _, s in pairs), 256, 8)
        print(f"[head sum loop] P={len(pairs)}: {t} tiles per pair")
        if len(pairs) == 1 and not (t > 2 * 256 + 248 and t % 8 != 0):
            pytest.skip(f"{cus} CUs: {t} tiles do not run the loop more than twice with a tail that is no multiple of 8")
        _batch_parity(diag_ctx, prm, pairs, f"head sum loop P={len(pairs)} tiles={t}", make_batch=make)


@functools.lru_cache(maxsize=None)
def _head_loop_source():
    """Frame 1 cut to 1053 blocks of 256 points (1053 = 131 * 8 + 5): the full frame has 1056."""
    full1 = _frame(1)
    assert full1.len() > 256 * 1053
    return _sub(full1, slice(0, 256 * 1053 - 100))


@gpu
@pytest.mark.parametrize("levels", [0, 1, 7, 13])
@pytest.mark.parametrize("block", [256, 512])
def test_ragged_batch_lds_cap_and_block(diag_ctx, monkeypatch, levels, block):
    """Trees of depth 15, 12 and 0 in one launch: the cap on the heap levels held in LDS lies below, between and above
    the pairs' depths (lds_levels = min(depth, cap) per pair, kd_stage_splits with the pair's own table size)."""
    knobs = {"A3D_PCLB_BLOCK": block, "A3D_PCLB_LDS_LEVELS": levels}

    def make(ctx, prm, targets):
        return _with_knobs(monkeypatch, knobs, lambda: IcpBatch(ctx, prm, targets))

    depths = {_tree(t).stats()[2] for t, _ in _ragged()}
    assert depths == {0, 12, 15} and any(d < levels for d in depths) == (levels > 0) and any(d > levels for d in depths), depths
    _batch_parity(diag_ctx, IcpParams(max_iterations=5), _ragged(), f"ragged block={block} lds_levels={levels}",
                  RAGGED_FAILS, make_batch=make)


# ---- E. more pairs than CUs ----------------------------------------------------------------------------------------------

def many_pairs(n):
    """n small, distinct pairs: target = frame f cut [first::64] (about 4 200 points), source = frame f + 1 cut
    [first::step], step 64, 96, 176 or 400 (4 200 .. 675 points: the longest needs five rounds of a 1024-thread block,
    the shortest less than one); the first and the last pair fail (source 100 m away).  (f, first, step) repeats after
    448 pairs.  The first 293 pairs on the CPU, 5 iterations: the oracle fails on the first and the last pair only.  What
    the GPU changes is the order of the sums, so each source was also given to the oracle in reversed and in three
    random orders: its answer moves by at most 8.2e-6 (rad or m), but for pair 117 (1.9e-5: its two lowest residuals are
    1.6e-6 apart, an argmin tie between two poses that far from each other).  (Shifting every source coordinate by one
    ulp says little here: it moves correspondences across the gates at the identity, where the GPU's are the oracle's
    bit for bit, and then the best iteration changes.)"""
    pairs = []
    for k in range(n):
        f, first, step = k % 7, (5 * k) % 64, (64, 96, 176, 400)[k % 4]
        src = _far if k in (0, n - 1) else _cut
        pairs.append((_cut(f, first, 64), src(f + 1, first, step)))
    return pairs


@gpu
@pytest.mark.parametrize("extra", [None, 37], ids=["P=129", "P=CUs+37"])
def test_more_pairs_than_cus(ctx, extra):
    """From 129 pairs on 256 CUs a pair has ONE block, which strides over its whole source, and the head sums one tile;
    with more pairs than CUs the grid does not fit the device at once."""
    cus = _num_cus(ctx)
    n = 129 if extra is None else cus + extra
    prm = IcpParams(max_iterations=5)
    pairs = many_pairs(n)
    lens = [s.len() for _, s in pairs]
    assert max(lens) > 1024 and len(set(lens)) > 4
    print(f"[many pairs P={n} on {cus} CUs] {_tiles(cus, n, max(lens))} tile(s) per pair, sources of {min(lens)} .. {max(lens)} points")
    up = _Resident(ctx)
    dev = [(up(t), up(s)) for t, s in pairs]

    def run(dev_pairs):
        batch = IcpBatch(ctx, prm, [t for t, _ in dev_pairs])
        out = batch.align([s for _, s in dev_pairs])
        batch.free()
        return out

    poses, status = run(dev)
    _compare(prm, pairs, poses, status, f"many pairs P={n} on {cus} CUs", {0, n - 1}, each=False)
    p0, s0 = _bits(poses, status)
    pr, sr = _bits(*run(dev[::-1]))
    assert np.array_equal(pr, p0[::-1]) and np.array_equal(sr, s0[::-1])
    up.free()


# ---- F. one handle, many passes --------------------------------------------------------------------------------------------

@gpu
def test_one_handle_passes_of_different_geometry(ctx):
    prm = IcpParams(max_iterations=5)
    up = _Resident(ctx)
    targets = [up(_frame(k)) for k in range(3)]
    full = [up(_frame(k + 1)) for k in range(3)]
    small = [up(_spread(_frame(k + 1), 17)) for k in range(3)]

    def fresh(sources):
        batch = IcpBatch(ctx, prm, targets)
        out = _bits(*batch.align(sources))
        batch.free()
        return out

    want_full, want_small = fresh(full), fresh(small)
    assert list(want_full[1]) == [0, 0, 0]
    assert not np.array_equal(want_full[0], want_small[0])
    batch = IcpBatch(ctx, prm, targets)
    for what, sources, want in (("full", full, want_full), ("17 points", small, want_small), ("full again", full, want_full)):
        got = _bits(*batch.align(sources))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
        assert batch.last_device_ms() > 0.0
    batch.enqueue(full)
    batch.enqueue(small)  # must wait for the first pass before it rewrites the page-locked descriptor table
    got = _bits(*batch.results())
    assert np.array_equal(got[0], want_small[0]) and np.array_equal(got[1], want_small[1])
    assert batch.last_device_ms() > 0.0
    batch.free()
    up.free()


# ---- G. gates, unaligned views, the empty batch ------------------------------------------------------------------------

GATED = dict(max_iterations=4, weight=0.7, max_distance=0.05, max_normal_angle=0.2)


def gated_pairs():
    return [(_cut(0, 0, 64), _cut(1, 0, 64)), (_cut(2, 5, 64), _cut(3, 5, 64)), (_cut(0, 3, 32), _cut(5, 3, 32))]


def assert_gates_bite(pairs):
    for k, (tgt, src) in enumerate(pairs):
        default, gated = oracle_count(IcpParams.default(), tgt, src), oracle_count(IcpParams(**GATED), tgt, src)
        print(f"[gates pair {k}] {gated} of {src.len()} correspondences pass at the identity, {default} with the default gates")
        assert 0 < gated < default, (k, gated, default)


def test_gates_reject_some_not_all():
    assert_gates_bite(gated_pairs())



@gpu
def test_non_default_gates_and_weight(ctx):
    pairs = gated_pairs()
    assert_gates_bite(pairs)
    _batch_parity(ctx, IcpParams(**GATED), pairs, "gates")


def _view(ctx, base, first, n):
    """Points first .. first + n of a resident cloud: a view over its buffers (never freed on its own)."""
    v = DevicePointCloud.__new__(DevicePointCloud)
    v.ctx, v.n = ctx, n
    v.d_points = C.c_void_p(base.d_points.value + 12 * first)
    v.d_normals = C.c_void_p(base.d_normals.value + 12 * first)
    return v


@gpu
def test_views_at_a_twelve_byte_offset(ctx):
    """Targets (kdtree_build_device) and sources (the 12-byte loads of pcl_point_loop) that start one point into a
    buffer: 4-byte aligned, not 16."""
    prm = IcpParams(max_iterations=5)
    host = [(_frame(0), _frame(1)), (_cut(2, 0, 64), _cut(3, 0, 96)), (_spread(_frame(0), 18), _cut(1, 0, 50))]
    up = _Resident(ctx)
    views = [(_view(ctx, up(t), 1, t.len() - 1), _view(ctx, up(s), 1, s.len() - 1)) for t, s in host]
    assert all(v.d_points.value % 16 == 12 for pair in views for v in pair)
    copies = [(up(_sub(t, slice(1, None))), up(_sub(s, slice(1, None)))) for t, s in host]

    def run(dev_pairs):
        batch = IcpBatch(ctx, prm, [t for t, _ in dev_pairs])
        out = _bits(*batch.align([s for _, s in dev_pairs]))
        batch.free()
        return out

    got, want = run(views), run(copies)
    assert list(want[1]) == [0, 0, 0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    up.free()


@gpu
def test_empty_batch(ctx):
    batch = IcpBatch(ctx, IcpParams.default(), [])
    poses, status = batch.align([])
    assert poses == [] and status.shape == (0,)
    assert batch.last_device_ms() == 0.0
    batch.enqueue([])
    poses, status = batch.results()
    assert poses == [] and status.shape == (0,)
    batch.free()
    batch.free()  # a second free is a no-op
