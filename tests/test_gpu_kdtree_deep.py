"""GPU parity of R3dTree::nearest below the LDS split table.

kdtree_descend (csrc/kdtree.hpp) walks the top lds_levels heap levels out of LDS (at most 15: kd_launch_config), then
goes on in global memory three levels per round trip with a rest of 0, 1 or 2 levels.  Every tree with max_depth >= 16
(more than 524 288 points) takes that branch in the product.  Here: trees of depth 16-19 through the product library,
and every LDS depth 0..14 through the diagnostics build's launch knobs on smaller trees, which gives every combination
of LDS depth mod 3, number of triple rounds and rest.  Indices and squared distances bit for bit the oracle's."""
import time

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import R3dTree
from data_util import uniform01

pytestmark = pytest.mark.gpu

M_QUERIES = 300_007  # >= 2 grid-stride rounds at 256 CUs x 1024 threads; not a multiple of 1024


def _lattice(seed, n, r):
    """Integer lattice points in [-r, r]^3, n / (2r + 1)^3 per site on average: heavy ties, +-0.0 mixed in (as
    _kd_cases()["dup"], at depth >= 16)."""
    rng = np.random.default_rng(seed)
    db = rng.integers(-r, r + 1, size=(n, 3)).astype(np.float32)
    db[::7, 0] = -0.0
    db[::5, 1] = 0.0
    return db


def _wall(seed, w, h):
    """A depth image's cloud: a fronto-parallel wall (60 % of the pixels at one z) beside z quantised to 1 / 5000 m."""
    rng = np.random.default_rng(seed)
    vv, uu = np.mgrid[0:h, 0:w]
    zz = np.where(uu < (w * 3) // 5, 3.0, np.round(rng.uniform(1.0, 4.0, size=uu.shape) * 5000) / 5000).astype(np.float32)
    return np.stack([(uu - w / 2) * zz / 500, (vv - h / 2) * zz / 500, zz], axis=-1).reshape(-1, 3).astype(np.float32)


def _queries(db, seed, m=M_QUERIES, lattice=False):
    """m queries over the bounding box and a quarter of its span beyond it; a few NaN and +-inf ones."""
    lo, hi = db.min(axis=0), db.max(axis=0)
    span = np.maximum(hi - lo, np.float32(1e-3))
    q = (lo - 0.25 * span + uniform01(seed, 3 * m).reshape(-1, 3) * 1.5 * span).astype(np.float32)
    if lattice:  # half of them on the lattice: ties of distance between equal points and on split planes
        q[::2] = np.round(q[::2])
    q[11] = np.nan
    q[12, 0] = np.nan
    q[13, 1] = np.inf
    q[14, 2] = -np.inf
    q[15] = np.inf
    return q


def _assert_nearest(tree, ref, q, what):
    ri, rd = ref.nearest(q)
    gi, gd = tree.nearest(q)
    bad = np.flatnonzero((gi != ri) | (gd.view(np.uint32) != rd.view(np.uint32)))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), gi[bad[:5]].tolist(), ri[bad[:5]].tolist())
    return ri, rd


def _inner_share_at_last(stats):
    """Share of the nodes at depth max_depth - 1 that are inner (their children are leaves at max_depth)."""
    leaves, _, depth = stats
    return (leaves - (1 << (depth - 1))) / (1 << (depth - 1))


# (n, depth): n/2^(depth-1) ~ 16.5, so about half of the nodes at depth - 1 are inner; depth 19 just above 4 194 304
_DEEP = [(540_000, 16), (1_080_000, 17), (2_160_000, 18)]


@pytest.mark.parametrize("n,depth", _DEEP + [(4_200_000, 19)], ids=lambda v: str(v))
def test_kdtree_deep_uniform_bit_exact(ctx, n, depth):
    t0 = time.perf_counter()
    db = uniform01(100 + depth, 3 * n).reshape(n, 3)
    ref = O.KdTree(db)
    tree = R3dTree.new(ctx, db)
    assert tree.stats() == ref.stats() and ref.stats()[2] == depth
    if depth < 19:
        assert _inner_share_at_last(ref.stats()) >= 0.25, ref.stats()
    _assert_nearest(tree, ref, _queries(db, 200 + depth), ("uniform", n))
    if depth == 16:
        # every database point: it finds itself at distance 0 unless a coordinate it shares with another point sent the
        # one-leaf search (kdtree.rs) the other way at a split; the oracle's search does the same (3 of these points)
        si, _ = _assert_nearest(tree, ref, db, ("self", n))
        assert np.count_nonzero(si != np.arange(n, dtype=np.uint64)) <= 10
    print(f"[kd deep uniform n={n} depth={depth}] {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("n,depth", _DEEP, ids=lambda v: str(v))
def test_kdtree_deep_lattice_ties_bit_exact(ctx, n, depth):
    t0 = time.perf_counter()
    db = _lattice(300 + depth, n, 20)
    ref = O.KdTree(db)
    tree = R3dTree.new(ctx, db)
    assert tree.stats() == ref.stats() and ref.stats()[2] == depth
    assert _inner_share_at_last(ref.stats()) >= 0.25, ref.stats()
    q = _queries(db, 400 + depth, lattice=True)
    if depth == 16:  # and every database point: distance 0, first of its equal points in the oracle's order
        q = np.concatenate([q, db])
    _assert_nearest(tree, ref, q, ("lattice", n))
    print(f"[kd deep lattice n={n} depth={depth}] {time.perf_counter() - t0:.1f} s")


def test_kdtree_deep_depth_image_cloud_and_resident_queries(ctx):
    t0 = time.perf_counter()
    db = _wall(5, 760, 720)  # 547 200 points: depth 16
    ref = O.KdTree(db)
    tree = R3dTree.new(ctx, db)
    assert tree.stats() == ref.stats() and ref.stats()[2] == 16
    assert _inner_share_at_last(ref.stats()) >= 0.25, ref.stats()
    q = np.concatenate([_queries(db, 501), db[::3]])
    ri, rd = _assert_nearest(tree, ref, q, "depth image")
    # the same queries resident in HBM (a3d_kdtree_nearest_device: u32 indices)
    m = len(q)
    d_q = ctx.to_device(q)
    d_i, d_d = ctx.malloc(4 * m), ctx.malloc(4 * m)
    try:
        tree.nearest_device(d_q, m, d_i, d_d)
        gi = ctx.to_host(d_i, np.empty(m, np.uint32))
        gd = ctx.to_host(d_d, np.empty(m, np.float32))
    finally:
        for p in (d_q, d_i, d_d):
            ctx.free(p)
    assert np.array_equal(gi.astype(np.uint64), ri) and np.array_equal(gd.view(np.uint32), rd.view(np.uint32))
    print(f"[kd deep depth image n={len(db)}] {time.perf_counter() - t0:.1f} s")


_KD_LAUNCH_KNOBS = ("A3D_KD_LDS_LEVELS", "A3D_KD_BLOCK", "A3D_KD_BLOCKS_PER_CU")


@pytest.fixture(scope="module")
def shallow_clouds():
    """A depth-15 uniform cloud and a depth-12 tie-heavy one, each with its queries and the oracle's answers."""
    out = {}
    u = uniform01(6, 3 * 270213).reshape(-1, 3)
    t = _lattice(7, 33_800, 8)
    for name, db, depth, lattice in (("uniform15", u, 15, False), ("ties12", t, 12, True)):
        ref = O.KdTree(db)
        assert ref.stats()[2] == depth and _inner_share_at_last(ref.stats()) >= 0.25, ref.stats()
        q = _queries(db, 600 + depth, m=100_003, lattice=lattice)
        ri, rd = ref.nearest(q)
        out[name] = (db, q, ri, rd, ref.stats())
    return out


def _nearest_with(diag_ctx, monkeypatch, tree, q, env):
    for k in _KD_LAUNCH_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return tree.nearest(q)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", ["uniform15", "ties12"])
def test_kdtree_every_lds_depth(diag_ctx, monkeypatch, shallow_clouds, case):
    """A3D_KD_LDS_LEVELS 0..14: the global descent from every entry level (every level % 3, 0-4 triple rounds, every
    rest), and on the depth-12 tree also with the whole descent in LDS (levels capped at the depth)."""
    db, q, ri, rd, stats = shallow_clouds[case]
    tree = R3dTree.new(diag_ctx, db)
    assert tree.stats() == stats
    for levels in range(15):
        gi, gd = _nearest_with(diag_ctx, monkeypatch, tree, q, {"A3D_KD_LDS_LEVELS": str(levels)})
        bad = np.flatnonzero((gi != ri) | (gd.view(np.uint32) != rd.view(np.uint32)))
        assert bad.size == 0, (case, levels, bad.size, bad[:5].tolist())


@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("per_cu", [1, 3])
def test_kdtree_launch_geometry(diag_ctx, monkeypatch, shallow_clouds, block, per_cu):
    """The 256-, 512- and 1024-thread kernels, one or three blocks per CU, at LDS depth 0 and 7 on the depth-15 tree."""
    db, q, ri, rd, stats = shallow_clouds["uniform15"]
    tree = R3dTree.new(diag_ctx, db)
    for levels in (0, 7):
        env = {"A3D_KD_LDS_LEVELS": str(levels), "A3D_KD_BLOCK": str(block), "A3D_KD_BLOCKS_PER_CU": str(per_cu)}
        gi, gd = _nearest_with(diag_ctx, monkeypatch, tree, q, env)
        assert np.array_equal(gi, ri) and np.array_equal(gd.view(np.uint32), rd.view(np.uint32)), env
