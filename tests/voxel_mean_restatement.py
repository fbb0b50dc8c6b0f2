"""The definition of the voxel-grid downsample by cell mean (include/align3d_hip.h, a3d_point_clouds_voxel_mean_device)
restated in plain numpy, step by step as the header numbers them, on top of voxel_restatement.voxel_keys.  It is the
expected value of every voxel-mean test and never the code under test.  numpy evaluates each f32 and f64 operation on its
own (no fused multiply-add, IEEE divide and square root), which is the arithmetic the library is compiled for; the sums
are int64 and uint64, so no order of summation can matter."""
import numpy as np

from voxel_restatement import voxel_keys

LATTICE = np.float32(32768.0)
NORMAL_SCALE = np.float32(1048576.0)


def _segment_sum(values, starts):
    """Sums of the runs of `values` ([n] or [n, k], an integer type) that begin at `starts`."""
    if len(starts) == 0:
        return values[:0].copy()
    return np.add.reduceat(values, starts, axis=0)


def voxel_mean(points, normals, colors, voxel_size, origin=None):
    """(points [m,3] f32, normals [m,3] f32 or None, colors [m,3] u8 or None, index [m] u32, counts [m] u32, dropped)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    v = np.float32(voxel_size)
    o = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
    s, u = LATTICE / v, v / LATTICE
    assert s.dtype == np.float32 and u.dtype == np.float32
    kept, key, _ = voxel_keys(p, voxel_size, origin)  # step 1
    idx = np.flatnonzero(kept)
    dropped = int(len(p) - len(idx))
    order = idx[np.argsort(key[idx], kind="stable")]  # by cell, ascending input index inside a cell
    k = key[order]
    first = np.ones(len(order), bool)
    first[1:] = k[1:] != k[:-1]
    starts = np.flatnonzero(first)
    rep = order[starts]  # step 6: the lowest input index of every cell
    counts = np.diff(np.append(starts, len(order))).astype(np.int64)
    with np.errstate(all="ignore"):
        # step 2
        pk = p[order]
        c = np.floor((pk - o) / v)
        ctr = (c + np.float32(0.5)) * v + o
        d = pk - ctr
        assert d.dtype == np.float32
        q = np.rint(d * s).astype(np.int32).astype(np.int64)
        S = _segment_sum(q, starts)
        # step 3
        m = (S.astype(np.float64) / counts[:, None].astype(np.float64)).astype(np.float32)
        out_p = ctr[starts] + m * u
        assert out_p.dtype == np.float32
        single = counts == 1
        out_p[single] = p[rep[single]]
        out_n = out_c = None
        if nrm is not None:  # step 4
            nk = nrm[order]
            counted = (np.isfinite(nk) & (np.abs(nk) <= np.float32(2.0))).all(axis=1)
            r = np.rint(np.where(counted[:, None], nk, np.float32(0)) * NORMAL_SCALE).astype(np.int32).astype(np.int64)
            T = _segment_sum(r, starts).astype(np.float64)
            L = np.sqrt((T[:, 0] * T[:, 0] + T[:, 1] * T[:, 1]) + T[:, 2] * T[:, 2])
            out_n = np.where(L[:, None] > 0, T / np.where(L > 0, L, 1.0)[:, None], 0.0).astype(np.float32)
            out_n[single] = nrm[rep[single]]
        if col is not None:  # step 5
            C = _segment_sum(col[order].astype(np.uint64), starts)
            n64 = counts.astype(np.uint64)[:, None]
            out_c = ((np.uint64(2) * C + n64) // (np.uint64(2) * n64)).astype(np.uint8)
            out_c[single] = col[rep[single]]
    rows = np.argsort(rep, kind="stable")  # step 6: ascending representative
    return (out_p[rows], None if out_n is None else out_n[rows], None if out_c is None else out_c[rows],
            rep[rows].astype(np.uint32), counts[rows].astype(np.uint32), dropped)


def exact_mean(points, voxel_size, origin=None):
    """([m,3] f64: the f64 mean of every cell's f32 points, in the row order of voxel_mean): what the rule approximates."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    kept, key, _ = voxel_keys(p, voxel_size, origin)
    idx = np.flatnonzero(kept)
    order = idx[np.argsort(key[idx], kind="stable")]
    k = key[order]
    first = np.ones(len(order), bool)
    first[1:] = k[1:] != k[:-1]
    starts = np.flatnonzero(first)
    counts = np.diff(np.append(starts, len(order))).astype(np.float64)
    sums = np.add.reduceat(p[order].astype(np.float64), starts, axis=0) if len(starts) else np.zeros((0, 3))
    return (sums / counts[:, None])[np.argsort(order[starts], kind="stable")]


def error_bound(points, voxel_size, origin=None):
    """v * 2^-15 + 2 ulp32(M), M the largest absolute finite input or origin coordinate: half a lattice step, the rounding
    of d_k, and the final add."""
    p = np.ascontiguousarray(points, np.float32)
    finite = np.abs(p[np.isfinite(p)])
    big = float(finite.max()) if finite.size else 0.0
    if origin is not None:
        big = max(big, float(np.abs(np.asarray(origin, np.float32)).max()))
    return float(np.float32(voxel_size)) * 2.0 ** -15 + 2.0 * float(np.spacing(np.float32(big)))
