"""The definition of the voxel map's association (include/align3d_hip.h, "Aligning against the map") and of the
frame-to-map ICP on top of it, restated on the host.  It is the expected value of the voxel map ICP tests and of
__graft_entry__.smoke(), and never the code under test.

The association is plain numpy float32 on top of voxel_restatement.voxel_keys (each f32 operation on its own, IEEE
divide): the map is a dict from cell key to (seq, row) built from voxel_downsample_cloud of the merged input, a query is
looked up in its 27 cells, and the winner minimises bits(d2) << 32 | seq.  Poses are applied by the oracle
(orc_transform_points / orc_transform_normals).  One ICP iteration is put together from the oracle's bricks
(orc_acos_gate_rejects, orc_gn_steps, orc_gn_weight, orc_gn_mean_squared_residual, orc_gn_solve, orc_exp_se3,
orc_compose); the loop and the best-pose rule are those of src/icp/pcl_icp.rs:59-106, started from `initial`."""
import ctypes as C
import itertools

import numpy as np

import oracle_lib as O
import voxel_restatement as V
from align3d_amd._abi import A3D_OK, A3D_SOLVE_FAILED, GnStateC, PoseC, ptr

NONE_SEQ = 0xFFFFFFFF
LIM = V.CELL_LIMIT
DELTAS = np.asarray(list(itertools.product((-1, 0, 1), repeat=3)), np.int64)  # [27, 3]


def transform_normals(pose, normals):
    n = np.ascontiguousarray(normals, np.float32)
    out = np.empty_like(n)
    O.load().orc_transform_normals(C.byref(pose), ptr(n), n.size // 3, ptr(out))
    return out


def word_of(d2, seq):
    """bits(d2) << 32 | seq as uint64 (d2 >= 0: its bit pattern is monotone)."""
    return np.asarray(d2, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32) | np.asarray(seq, np.uint64)


def dist2(q, r):
    """d = q - r, d2 = (dx dx + dy dy) + dz dz in f32."""
    with np.errstate(all="ignore"):
        d = np.asarray(q, np.float32) - np.asarray(r, np.float32)
        out = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


class MapRestatement:
    """The map after `points` / `normals` (the merged input: every offered cloud under its pose, in insertion order) went
    in: rows, normals and sequence numbers by voxel_downsample_cloud, and the dict from cell key to (seq, row)."""

    def __init__(self, points, normals, voxel_size, origin=None):
        self.voxel = np.float32(voxel_size)
        self.origin = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        self.rows, self.normals, self.seq, self.dropped = V.voxel_downsample_cloud(points, normals, voxel_size, origin)
        kept, keys, _ = V.voxel_keys(self.rows, voxel_size, origin)
        assert kept.all()
        self.cells = {int(k): (int(s), i) for i, (k, s) in enumerate(zip(keys.tolist(), self.seq.tolist()))}
        assert len(self.cells) == len(self.rows)  # one row per cell

    def renumbered(self):
        """The map after a retain that keeps everything: the rows numbered 0 ... k-1 in their old order."""
        return MapRestatement(self.rows, self.normals, self.voxel, self.origin)

    def nearest(self, queries, pose=None):
        """(seq [m] uint32, d2 [m] f32, row [m] int64, -1 = none) of the association; `pose`: a PoseC applied first."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        if pose is not None:
            q = O.transform_points(pose, q)
        m = len(q)
        lim = np.float32(LIM)
        with np.errstate(all="ignore"):
            c = np.floor((q - self.origin) / self.voxel)
        assert c.dtype == np.float32
        ok = (np.isfinite(c) & (c >= -lim) & (c < lim)).all(axis=1)  # the drop rule
        ci = np.where(ok[:, None], c, np.float32(0)).astype(np.int64)
        best = np.full(m, word_of(np.float32(np.inf), NONE_SEQ), np.uint64)
        best_row = np.full(m, -1, np.int64)
        for delta in DELTAS:
            n = ci + delta
            valid = ok & ((n >= -LIM) & (n < LIM)).all(axis=1)  # per axis, before the key is packed
            k = n + LIM
            keys = np.where(valid, k[:, 0] << 42 | k[:, 1] << 21 | k[:, 2], -1)
            hits = [self.cells.get(key) for key in keys.tolist()]
            found = np.asarray([h is not None for h in hits], bool) & valid
            row = np.asarray([h[1] if h is not None else 0 for h in hits], np.int64)
            if not found.any():
                continue
            word = word_of(dist2(q, self.rows[row]), self.seq[row])
            better = found & (word < best)
            best = np.where(better, word, best)
            best_row = np.where(better, row, best_row)
        return (best & np.uint64(0xFFFFFFFF)).astype(np.uint32), (best >> np.uint64(32)).astype(np.uint32).view(np.float32), best_row

    def point_terms(self, src_points, src_normals, pose, params):
        """(residuals [k] f32, jacobians [k, 6] f32) of the source points that pass both gates under `pose` (a PoseC), in
        source order: the body of src/icp/pcl_icp.rs:68-91."""
        return self.point_terms_kept(src_points, src_normals, pose, params)[:2]

    def point_terms_kept(self, src_points, src_normals, pose, params):
        """point_terms and, third, the source indices [k] (ascending) of the points that passed."""
        p = O.transform_points(pose, src_points)
        sn = transform_normals(pose, src_normals)
        _, d2, row = self.nearest(p)
        max_d2 = np.float32(params.max_distance) * np.float32(params.max_distance)
        keep = (row >= 0) & ~(d2 > max_d2)
        kept = np.flatnonzero(keep)
        p, sn, row = p[keep], sn[keep], row[keep]
        tp, tn = self.rows[row], self.normals[row]
        dot = (sn[:, 0] * tn[:, 0] + sn[:, 1] * tn[:, 1]) + sn[:, 2] * tn[:, 2]
        keep = ~O.acos_gate_rejects(dot, params.max_normal_angle, strict=True) if len(dot) else np.zeros(0, bool)
        kept = kept[keep]
        p, tp, tn = p[keep], tp[keep], tn[keep]
        d = tp - p
        r = (d[:, 0] * tn[:, 0] + d[:, 1] * tn[:, 1]) + d[:, 2] * tn[:, 2]
        tw = np.stack([p[:, 1] * tn[:, 2] - p[:, 2] * tn[:, 1], p[:, 2] * tn[:, 0] - p[:, 0] * tn[:, 2],
                       p[:, 0] * tn[:, 1] - p[:, 1] * tn[:, 0]], axis=1)
        J = np.ascontiguousarray(np.concatenate([tn, tw], axis=1), np.float32)
        assert r.dtype == np.float32 and J.shape == (len(r), 6)
        return np.ascontiguousarray(r), J, kept

    def gn_state(self, src_points, src_normals, pose, params):
        """The GaussNewton<6> state after the point loop, by orc_gn_steps (f32 running sums, as the reference)."""
        r, J = self.point_terms(src_points, src_normals, pose, params)
        g = GnStateC()
        O.load().orc_gn_steps(C.c_void_p(ptr(r)), C.c_void_p(ptr(J)), len(r), C.byref(g))
        return g

    def accumulate(self, src_points, src_normals, pose, params):
        """{H, g, ssq, count} of one pass with the sums taken in f64 and rounded to f32 once, the form of the oracle's
        orc_pcl_icp_accumulate(accum_f64 = 1) that a3d_pcl_icp_accumulate is tested against: the per-point terms are the
        f32 values above, and the expected sums carry no summation error of their own."""
        r, J = self.point_terms(src_points, src_normals, pose, params)
        r64, J64 = r.astype(np.float64), J.astype(np.float64)
        return {"H": (J64.T @ J64).astype(np.float32), "g": (J64.T @ r64).astype(np.float32),
                "ssq": np.float32((r64 * r64).sum()), "count": len(r)}

    def align(self, src_points, src_normals, params, initial=None):
        """(status, PoseC): Icp::align's loop (pcl_icp.rs:59-106) from `initial` (None: eye) with this association."""
        lib = O.load()
        optim = O.pose() if initial is None else initial
        best, best_residual = optim, np.float32(np.inf)
        for _ in range(int(params.max_iterations)):
            g = self.gn_state(src_points, src_normals, optim, params)
            residual = np.float32(lib.orc_gn_mean_squared_residual(C.byref(g)))
            lib.orc_gn_weight(C.byref(g), params.weight)
            update = (C.c_float * 6)()
            if lib.orc_gn_solve(C.byref(g), update) != 1:
                return A3D_SOLVE_FAILED, optim
            optim = O.compose(O.exp_se3(list(update)), optim)
            if residual < best_residual:
                best_residual, best = residual, optim
        return A3D_OK, best


class SparseMapRestatement(MapRestatement):
    """The map after `pieces` = [(seq0, points, normals)] went in, piece k's point i under sequence number seq0 + i, and
    every number between the pieces was consumed by a point that the map drops (all NaN: it changes no cell).  The
    merged input of such a map has up to 2^32 rows and is never formed: the map is voxel_downsample_cloud of the real
    points alone, each local index translated to its true sequence number.  The translation is strictly increasing, so
    every "the lower number wins" decision is the one the merged input would give.  `seq` is uint32 as everywhere;
    `local` keeps the indices into the concatenated real points.  nearest / accumulate / align work unchanged."""

    def __init__(self, pieces, voxel_size, origin=None):
        pieces = [(int(s), np.ascontiguousarray(p, np.float32).reshape(-1, 3), n) for s, p, n in pieces]
        true = np.concatenate([np.uint64(s) + np.arange(len(p), dtype=np.uint64) for s, p, _ in pieces])
        assert (true[1:] > true[:-1]).all() and (len(true) == 0 or int(true[-1]) < 1 << 32)  # the pieces do not overlap
        self.points_in = np.concatenate([p for _, p, _ in pieces])
        with_normals = all(n is not None for _, _, n in pieces)
        self.normals_in = np.concatenate([np.ascontiguousarray(n, np.float32).reshape(-1, 3) for _, _, n in pieces]) if with_normals else None
        self.true_seq = true  # of every real point offered, kept or not
        super().__init__(self.points_in, self.normals_in, voxel_size, origin)
        self.local = self.seq
        self.seq = true[self.local].astype(np.uint32)
        self.cells = {key: (int(self.seq[row]), row) for key, (_, row) in self.cells.items()}


def retained(model, min_seq=0, box=None, marks=(), total=None):
    """a3d_voxel_map_retain on a restated map (MapRestatement or SparseMapRestatement) whose `total` points were offered
    (None: one past its last row's number).  Returns (survivors, removed, new_marks, k): `survivors` is the
    MapRestatement of the rows with seq >= min_seq that lie inside the closed box = (min3, max3), numbered 0 ... k-1 in
    their old order; new_marks[i] = the survivors whose old number is below marks[i], marks above `total` counting as
    `total`."""
    seq = model.seq.astype(np.uint64)
    total = (int(seq[-1]) + 1 if len(seq) else 0) if total is None else int(total)
    assert len(seq) == 0 or int(seq.max()) < total
    keep = seq >= np.uint64(min(int(min_seq), total))
    if box is not None:
        lo, hi = np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)
        keep &= ((model.rows >= lo) & (model.rows <= hi)).all(axis=1)
    old = seq[keep]
    new_marks = [int((old < np.uint64(min(int(m), total))).sum()) for m in marks]
    k = int(keep.sum())
    survivors = MapRestatement(model.rows[keep], None if model.normals is None else model.normals[keep], model.voxel, model.origin)
    assert len(survivors.rows) == k and np.array_equal(survivors.seq, np.arange(k))  # one row per cell: all of them stay
    return survivors, int(len(seq) - k), new_marks, k


class PeriodicSource:
    """`model` as a long source of `m` points sees it, where the long source is a short one repeated: the methods are
    handed ONE period of P points, and point i of the long source is point i % P of that period.  Association and
    per-point terms are computed for the one period and indexed; the sums, the iteration and the loop are
    MapRestatement's own, taken over all m points."""

    def __init__(self, model, m):
        self.model, self.m = model, int(m)

    def _index(self, period):
        assert 0 < period
        return np.arange(self.m, dtype=np.int64) % period

    def nearest(self, queries, pose=None):
        seq, d2, row = self.model.nearest(queries, pose)
        i = self._index(len(seq))
        return seq[i], d2[i], row[i]

    def point_terms_kept(self, src_points, src_normals, pose, params):
        r, J, kept = self.model.point_terms_kept(src_points, src_normals, pose, params)
        period = len(np.ascontiguousarray(src_points, np.float32).reshape(-1, 3))
        place = np.full(period, -1, np.int64)  # of a period's point among the period's terms
        place[kept] = np.arange(len(kept))
        at = place[self._index(period)]
        long_kept = np.flatnonzero(at >= 0)
        at = at[long_kept]
        return np.ascontiguousarray(r[at]), np.ascontiguousarray(J[at]), long_kept

    point_terms = MapRestatement.point_terms
    gn_state = MapRestatement.gn_state
    accumulate = MapRestatement.accumulate
    align = MapRestatement.align


def brute_force(rows, seq, queries):
    """(seq, d2, row) of the nearest of ALL rows by the same word, for every query: what the association is measured
    against where a row lies within reach."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    word = word_of(dist2(q[:, None, :], rows[None, :, :]), np.asarray(seq, np.uint64)[None, :])
    row = word.argmin(axis=1)
    best = word[np.arange(len(q)), row]
    return (best & np.uint64(0xFFFFFFFF)).astype(np.uint32), (best >> np.uint64(32)).astype(np.uint32).view(np.float32), row


def surfaces(seed, n, noise=0.001):
    """Test data: ([n, 3] points, [n, 3] unit normals) on a floor (z = 0), a wall (x = 0) and the upper cap of a sphere,
    a third each, within two metres of the origin: three families of normals, so that a point-to-plane alignment is
    well conditioned.  `noise`: standard deviation of the displacement along the normal."""
    rng = np.random.default_rng(seed)
    a = n // 3
    b = n - 2 * a
    u = rng.uniform(0.0, 1.0, size=(n, 2))
    floor = np.stack([1.5 * u[:a, 0], 1.5 * u[:a, 1], np.zeros(a)], axis=1)
    wall = np.stack([np.zeros(a), 1.5 * u[a:2 * a, 0], u[a:2 * a, 1]], axis=1)
    polar, azimuth = np.arccos(1.0 - 0.5 * u[2 * a:, 0]), 2.0 * np.pi * u[2 * a:, 1]  # up to 60 degrees from the pole
    radial = np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
    cap = np.asarray([0.8, 0.8, 0.2]) + 0.5 * radial
    normals = np.concatenate([np.tile([0.0, 0.0, 1.0], (a, 1)), np.tile([1.0, 0.0, 0.0], (a, 1)), radial])
    points = np.concatenate([floor, wall, cap]) + normals * rng.normal(size=(n, 1)) * noise
    order = rng.permutation(n)
    assert len(points) == n and b >= a
    return points[order].astype(np.float32), normals[order].astype(np.float32)


def borrow_cases():
    """[(axis, end, query, trap row, fair row)] at v = 1, origin 0: the query sits in the first (end 0) or last (end 1) cell
    of `axis`, cell 0 on the other two.  `trap`: the centre of the cell that the key of the out-of-range neighbour would
    name if its field borrowed from (carried into) the next axis's field, or None where that key has bit 63 set (axis x:
    no cell has it).  `fair`: the centre of the in-range neighbour on the other side."""
    lim = float(LIM)
    cases = []
    for axis in range(3):
        for end in (0, 1):
            cell = [0.0, 0.0, 0.0]
            cell[axis] = -lim if end == 0 else lim - 1.0
            query = [c + 0.5 for c in cell]
            fair = list(query)
            fair[axis] += 1.0 if end == 0 else -1.0
            trap = None
            if axis > 0:  # the borrow / carry lands in the field of axis - 1 and wraps this one
                t = list(cell)
                t[axis] = lim - 1.0 if end == 0 else -lim
                t[axis - 1] += -1.0 if end == 0 else 1.0
                trap = [c + 0.5 for c in t]
            cases.append((axis, end, query, trap, fair))
    return cases


def slot_hash(key):
    """The table's hash of a cell key (the 64-bit finaliser of MurmurHash3), as voxel_grid.hpp states it."""
    m64 = (1 << 64) - 1
    k = int(key)
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & m64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & m64
    return k ^ k >> 33


def occupied_slots(keys, slots):
    """The slots that `keys` occupy in an open-addressing table of `slots` slots with linear probing: the SET does not
    depend on the order in which the keys claimed their slots (which key sits where does)."""
    occupied = set()
    for key in keys:
        s = slot_hash(key) & (slots - 1)
        while s in occupied:
            s = (s + 1) & (slots - 1)
        occupied.add(s)
    return occupied


def absent_probe(key, occupied, slots):
    """(slots looked at, whether the walk passed from the last slot to slot 0) of the probe for a key the table does not
    hold: from its home slot on to the first empty one."""
    s, looked, wrapped = slot_hash(key) & (slots - 1), 1, False
    while s in occupied and looked <= slots:
        wrapped |= s == slots - 1
        s, looked = (s + 1) & (slots - 1), looked + 1
    return looked, wrapped
