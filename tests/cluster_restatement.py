"""The rule of a3d_point_clouds_cluster_device (align3d_amd/csrc/cloud_outliers.hip) restated in numpy: the neighbour pairs
by brute force over pairs, chunked, as outlier_restatement.knn_distance finds them (or by a sort by cell, for clouds whose
full pair count is out of reach; the two are checked against each other), the grid from normals_restatement.cells, a plain
sequential union-find (quick-find: one component number per row, a union renumbers the higher component) over the
core-core pairs in row order (or, for clouds of tens of thousands of rows, min-label hooking with pointer jumping: the
two are checked against each other), the border key and the ranking.  It is the expected value of every cluster test and
never the code under test.  numpy evaluates each f32 operation on its own, which is the arithmetic the library is compiled
for.

The rule of the cluster call.  All f32 operations are rounded on their own (-ffp-contract=off).  Per call: radius r,
finite and > 0, r2 = r * r computed on the host in f32; min_points m >= 1.
 1. Grid and neighbours.  Steps 1 and 2 of a3d_point_clouds_knn_distance_device, word for word: pitch r, origin 0,
    voxel_key; refused rows are DROPPED and are nobody's neighbour; the neighbours of row i are the kept rows j of the
    same cloud, i included, whose cell coordinates differ by at most 1 each and with
    d2 = (d_x*d_x + d_y*d_y) + d_z*d_z <= r2.  d2 has the same bits seen from i and from j, so the relation is
    symmetric.
 2. Core.  N_i is the number of neighbours, the row itself counted: the same bits as that entry's counts.  Row i is a
    CORE row iff it is kept and N_i >= m.  (Open3D counts the point itself too.)
 3. Clusters.  Two core rows are linked iff they are neighbours.  A cluster is a connected component of the core rows
    under that link.  Its ROOT is its lowest row index.
 4. Border.  A kept row that is not core and has at least one core neighbour joins the cluster of one of them: the
    core neighbour j that minimises bits(d2) << 32 | j, which is the nearest core row, the lower row on a tie (the
    idiom of DeviceVoxelMap.nearest).  A border row never links two clusters.
 5. Noise.  Every other row is noise: dropped rows, and non-core rows without a core neighbour.  Its label is
    0xFFFFFFFF.
 6. Labels.  Clusters are numbered 0 ... C-1 by ascending root.  labels[i] is the number of row i's cluster;
    sizes[c] is the number of rows labelled c, border rows included; roots[c] is strictly increasing;
    row_sizes[i] = sizes[labels[i]], and 0 for noise.
Every output is integers decided on integers or on d2 bits: the same on every run.
"""
from collections import namedtuple

import numpy as np

import normals_restatement as NR

F = np.float32
NONE = 0xFFFFFFFF

Pairs = namedtuple("Pairs", "n kept i j d2")  # every ordered neighbour pair (i, j), i == j included; d2 as uint32 bits
Clusters = namedtuple("Clusters", "labels sizes roots row_sizes counts core border noise dropped")


def _radius(radius):
    r = F(radius)
    r2 = r * r
    assert r2.dtype == F
    return r, r2


def pairs_brute(points, radius, chunk=256):
    """Rule 1 over every pair of kept rows, a chunk of rows against all of them at a time."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    r, r2 = _radius(radius)
    kept, cell = NR.cells(p, r)
    idx = np.flatnonzero(kept)
    pc, cc = p[idx], cell[idx].astype(np.int32)
    out_i, out_j, out_d = [], [], []
    for a in range(0, len(idx), chunk):
        these = idx[a:a + chunk]
        pr, cr = p[these], cell[these].astype(np.int32)
        with np.errstate(all="ignore"):
            d = [pc[None, :, k] - pr[:, None, k] for k in range(3)]  # d_k = p_jk - p_ik
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert d2.dtype == F
            nb = d2 <= r2
        for k in range(3):
            nb &= np.abs(cc[None, :, k] - cr[:, None, k]) <= 1
        ri, cj = np.nonzero(nb)
        out_i.append(these[ri]), out_j.append(idx[cj]), out_d.append(d2[ri, cj].view(np.uint32))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return Pairs(len(p), kept, cat(out_i, np.int64), cat(out_j, np.int64), cat(out_d, np.uint32))


def pairs_by_cell(points, radius):
    """Rule 1 by a sort by cell: for each of the 27 offsets, every kept row against the run of the cell at that offset."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    r, r2 = _radius(radius)
    kept, cell = NR.cells(p, r)
    idx = np.flatnonzero(kept)
    c = cell[idx] + (1 << 20)  # [0, 2^21) each
    key = c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2]
    order = np.argsort(key, kind="stable")
    idx, c, key = idx[order], c[order], key[order]
    out_i, out_j, out_d = [], [], []
    for o in range(27):
        off = np.array([o // 9 - 1, o // 3 % 3 - 1, o % 3 - 1], np.int64)
        nc = c + off
        ok = ((nc >= 0) & (nc < (1 << 21))).all(axis=1)
        nkey = nc[:, 0] << 42 | nc[:, 1] << 21 | nc[:, 2]
        begin, end = np.searchsorted(key, nkey, "left"), np.searchsorted(key, nkey, "right")
        run = np.where(ok, end - begin, 0)
        rows = np.repeat(np.arange(len(idx)), run)  # positions in cell order
        cols = np.arange(len(rows)) - np.repeat(np.cumsum(run) - run, run) + np.repeat(begin, run)
        pi, pj = p[idx[rows]], p[idx[cols]]
        with np.errstate(all="ignore"):
            d = [pj[:, k] - pi[:, k] for k in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nb = d2 <= r2
        out_i.append(idx[rows[nb]]), out_j.append(idx[cols[nb]]), out_d.append(d2[nb].view(np.uint32))
    i, j, d = np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)
    order = np.lexsort((j, i))
    return Pairs(len(p), kept, i[order].astype(np.int64), j[order].astype(np.int64), d[order].astype(np.uint32))


def sorted_pairs(pairs):
    """The pairs in (i, j) order, for comparing two enumerations."""
    order = np.lexsort((pairs.j, pairs.i))
    return pairs.i[order], pairs.j[order], pairs.d2[order]


def components_quick_find(n, li, lj):
    """comp [n]: the lowest row of every row's set under the links (li[k], lj[k]), lj < li.  A sequential union-find
    over the links in row order, one component number per row; a union renumbers the higher component, an O(n) pass."""
    comp = np.arange(n, dtype=np.int64)
    order = np.argsort(li, kind="stable")
    li, lj = li[order], lj[order]
    starts = np.searchsorted(li, np.arange(n + 1))
    for row in np.flatnonzero(np.diff(starts)):
        sets = np.unique(comp[lj[starts[row]:starts[row + 1]]])
        low = min(int(sets[0]), int(comp[row]))
        for s in np.r_[sets, comp[row]]:
            if s != low:
                comp[comp == s] = low
    return comp


def components_hooking(n, li, lj):
    """The same comp without a pass over the rows per union, for clouds of tens of thousands of rows: every row starts as
    its own root; a round hooks the root of each end of a link under the lower of the two roots (the minimum wins where
    several links hook one root), then every row jumps to its parent's parent until nothing moves, so that comp[x] is
    x's root again; rounds repeat until a round hooks nothing.  A root is only ever hooked under a lower row, so a
    set's root is its lowest row, and a link whose ends have different roots hooks one of them, so the last round has
    seen every link inside one set.  The sets that are left at least halve per round: O(log n) rounds."""
    comp = np.arange(n, dtype=np.int64)
    while len(li):
        a, b = comp[li], comp[lj]
        apart = a != b
        if not apart.any():
            break
        a, b = a[apart], b[apart]
        low = np.minimum(a, b)
        np.minimum.at(comp, a, low)  # a and b are roots: comp[root] == root before this
        np.minimum.at(comp, b, low)
        while True:
            up = comp[comp]
            if np.array_equal(up, comp):
                break
            comp = up
    return comp


COMPONENTS = {"quick_find": components_quick_find, "hooking": components_hooking}


def cluster_pairs(pairs, min_points, components="quick_find"):
    """Rules 2 to 6 from the neighbour pairs.  components: the routine of rule 3, a key of COMPONENTS."""
    n, m = pairs.n, int(min_points)
    assert m >= 1
    counts = np.bincount(pairs.i, minlength=n).astype(np.int64)  # rule 2 (the row itself is a pair)
    core = pairs.kept & (counts >= m)
    # rule 3: the components of the core-core pairs with j < i; comp[x] = lowest row of x's set
    link = core[pairs.i] & core[pairs.j] & (pairs.j < pairs.i)
    comp = COMPONENTS[components](n, pairs.i[link], pairs.j[link])
    # rule 4: the minimum key over the core neighbours of a kept row that is not core
    cand = ~core[pairs.i] & core[pairs.j]
    bi, bj = pairs.i[cand], pairs.j[cand]
    key = pairs.d2[cand].astype(np.uint64) << np.uint64(32) | bj.astype(np.uint64)
    order = np.lexsort((key, bi))
    bi, bj = bi[order], bj[order]
    first = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, bool)
    border = np.zeros(n, bool)
    border[bi[first]] = True
    root_of = np.full(n, -1, np.int64)
    root_of[core] = comp[core]
    root_of[bi[first]] = comp[bj[first]]
    # rules 5 and 6
    roots = np.unique(root_of[root_of >= 0])
    labels = np.full(n, NONE, np.int64)
    member = root_of >= 0
    labels[member] = np.searchsorted(roots, root_of[member])
    sizes = np.bincount(labels[member], minlength=len(roots)).astype(np.uint32)
    row_sizes = np.zeros(n, np.uint32)
    row_sizes[member] = sizes[labels[member]]
    return Clusters(labels.astype(np.uint32), sizes, roots.astype(np.uint32), row_sizes, counts.astype(np.uint32), core, border,
                    ~member, int((~pairs.kept).sum()))


def cluster(points, radius, min_points, by_cell=False, components="quick_find"):
    """Clusters(labels [n] u32, sizes [C] u32, roots [C] u32, row_sizes [n] u32, counts [n] u32, core / border / noise [n]
    bool, dropped) of one cloud."""
    return cluster_pairs((pairs_by_cell if by_cell else pairs_brute)(points, radius), min_points, components)


def remove_small_clusters(points, radius, min_points, min_size, max_size=NONE):
    """The rows DevicePointCloud.remove_small_clusters keeps."""
    sizes = cluster(points, radius, min_points).row_sizes.astype(np.int64)
    return np.flatnonzero((sizes >= int(min_size)) & (sizes <= int(max_size))).astype(np.uint32)


def largest_cluster(points, radius, min_points):
    """The rows DevicePointCloud.largest_cluster keeps."""
    c = cluster(points, radius, min_points)
    if len(c.sizes) == 0:
        return np.zeros(0, np.uint32)
    return np.flatnonzero(c.labels == np.argmax(c.sizes)).astype(np.uint32)
