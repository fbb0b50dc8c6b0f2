"""The voxel map of cell means (include/align3d_hip.h, a3d_voxel_map_new_mean) restated on the host, on top of
voxel_mean_restatement.voxel_mean (the rule) and voxel_map_icp_restatement.MapRestatement (the readers).  It is the expected
value of the mean-map tests and never the code under test.  The merged input is what the callers hand in: every offered
cloud under its pose (through the oracle), in insertion order."""
import numpy as np

import voxel_restatement as V
from voxel_map_icp_restatement import MapRestatement
from voxel_mean_restatement import voxel_mean


def input_keys(points, voxel_size, origin=None):
    """(kept [n] bool, key [n] int64) of the input points."""
    kept, keys, _ = V.voxel_keys(np.ascontiguousarray(points, np.float32).reshape(-1, 3), voxel_size, origin)
    return kept, keys.astype(np.int64)


class MeanMapRestatement(MapRestatement):
    """A map of means after `points` / `normals` / `colors` (the merged input) went in: rows, normals, colours, seq (the
    representatives) and counts by voxel_mean.  The dict from cell key to (seq, row) is built from the keys of the INPUT
    points: a mean may round onto a face of its cell, and its own key would then name the neighbour.  nearest,
    accumulate and align are MapRestatement's, on these rows."""

    def __init__(self, points, normals, colors, voxel_size, origin=None):
        self.voxel = np.float32(voxel_size)
        self.origin = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        self.points_in = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals_in = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.colors_in = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        self.rows, self.normals, self.colors, self.seq, self.counts, self.dropped = voxel_mean(
            self.points_in, self.normals_in, self.colors_in, voxel_size, origin)
        self.kept_in, self.keys_in = input_keys(self.points_in, voxel_size, origin)
        assert self.kept_in[self.seq].all()
        self.row_keys = self.keys_in[self.seq]
        self.cells = {int(k): (int(s), i) for i, (k, s) in enumerate(zip(self.row_keys.tolist(), self.seq.tolist()))}
        assert len(self.cells) == len(self.rows)  # one row per cell


def retained_mean(model, min_seq=0, box=None, marks=(), total=None):
    """a3d_voxel_map_retain on a MeanMapRestatement whose `total` points were offered (None: all of its input).  A cell
    survives iff its representative's seq >= min_seq and its mean row lies in the closed box = (min3, max3).  Returns
    (keep [rows] bool, removed, new_marks, k, continued): `continued` = (points, normals, colors) of the input points
    that fell into surviving cells, in their original order: the input a later insert continues from."""
    seq = model.seq.astype(np.uint64)
    total = len(model.points_in) if total is None else int(total)
    keep = seq >= np.uint64(min(int(min_seq), total))
    if box is not None:
        lo, hi = np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)
        keep &= ((model.rows >= lo) & (model.rows <= hi)).all(axis=1)
    old = seq[keep]
    new_marks = [int((old < np.uint64(min(int(m), total))).sum()) for m in marks]
    k = int(keep.sum())
    stays = model.kept_in & np.isin(model.keys_in, model.row_keys[keep])
    continued = (model.points_in[stays], None if model.normals_in is None else model.normals_in[stays],
                 None if model.colors_in is None else model.colors_in[stays])
    return keep, int(len(seq) - k), new_marks, k, continued


def continued_mean(continued, k, points, normals, colors, voxel_size, origin=None):
    """The extract of a retained map of k survivors (`continued` of retained_mean) after `points` / `normals` / `colors`
    (merged, possibly empty) were inserted: voxel_mean of the continued input with the indices in the map's numbering
    (survivor j has seq j, point i of the new input has seq k + i).  (points, normals, colors, index, counts, dropped)."""
    cp, cn, cc = continued
    new_p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    p = np.concatenate([cp, new_p])
    n = None if cn is None else np.concatenate([cn, np.ascontiguousarray(normals, np.float32).reshape(-1, 3)])
    c = None if cc is None else np.concatenate([cc, np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)])
    out_p, out_n, out_c, index, counts, dropped = voxel_mean(p, n, c, voxel_size, origin)
    old = index < len(cp)
    assert int(old.sum()) == k and old[:k].all()  # the survivors come first, in their old order
    index = np.where(old, np.arange(len(index)), index.astype(np.int64) - len(cp) + k).astype(np.uint32)
    return out_p, out_n, out_c, index, counts, dropped
