"""The definition of the voxel-grid downsample (include/align3d_hip.h, a3d_point_clouds_voxel_downsample_device) restated
in plain numpy float32, step by step as the header numbers them.  It is the expected value of every voxel test and of
__graft_entry__.smoke(), and never the code under test.  numpy evaluates each f32 operation on its own (no fused
multiply-add, IEEE divide), which is the arithmetic the library is compiled for."""
import numpy as np

CELL_LIMIT = 1 << 20


def voxel_keys(points, voxel_size, origin=None):
    """(kept [n] bool, key [n] uint64 (0 where dropped), dist [n] f32) of a cloud: steps 1 and 2."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    v = np.float32(voxel_size)
    o = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
    half, lim = np.float32(0.5), np.float32(CELL_LIMIT)
    with np.errstate(all="ignore"):
        c = np.floor((p - o) / v)  # step 1: the cell, f32
        assert c.dtype == np.float32
        kept = (np.isfinite(c) & (c >= -lim) & (c < lim)).all(axis=1)
        ci = np.where(kept[:, None], c, np.float32(0)).astype(np.int64) + CELL_LIMIT
        key = (ci[:, 0] << 42 | ci[:, 1] << 21 | ci[:, 2]).astype(np.uint64)
        key[~kept] = 0
        ctr = (c + half) * v + o  # step 2: the distance to the cell centre, f32, the kd-tree's association
        d = p - ctr
        dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert dist.dtype == np.float32
    assert not np.isnan(dist[kept]).any()
    return kept, key, dist


def voxel_downsample(points, voxel_size, origin=None):
    """(index [m] uint32 ascending: the input index of every kept point, dropped count): steps 3 and 4."""
    kept, key, dist = voxel_keys(points, voxel_size, origin)
    idx = np.flatnonzero(kept).astype(np.uint64)
    # step 3: per key the minimum of bits(dist) << 32 | i (dist >= 0: its bit pattern is monotone)
    word = dist[kept].view(np.uint32).astype(np.uint64) << np.uint64(32) | idx
    k = key[kept]
    order = np.lexsort((word, k))  # by key, then by word
    first = np.ones(order.size, bool)
    first[1:] = k[order][1:] != k[order][:-1]
    winners = idx[order][first]
    # step 4: ascending input index
    return np.sort(winners).astype(np.uint32), int(kept.size - idx.size)


def voxel_downsample_cloud(points, normals, voxel_size, origin=None):
    """(points [m,3], normals [m,3] or None, index [m] uint32, dropped): the rows copied bit for bit."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    index, dropped = voxel_downsample(p, voxel_size, origin)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)[index]
    return p[index], n, index, dropped
