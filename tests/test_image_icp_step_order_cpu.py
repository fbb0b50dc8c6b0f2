"""Stage B of the image ICP pixel loop requests the 2 x 2 intensity-map cell at (u, v) for every lane that is live after its
bounds test, before stage C's gates (image_icp.hip).  The bound it relies on, restated in numpy f32 and checked for every
representable u around each cut: a lane with u + 0.5 in (-1, tw) has ui = (u as u32, saturating, NaN -> 0) <= tw - 1, so
columns ui, ui + 1 <= tw lie inside the (tw + 2)-wide map; with the same for v, both 8-byte loads of the cell end inside
the (th + 2) x (tw + 2) map."""
import numpy as np
import pytest

F32 = np.float32
STEPS = 4096  # floats on either side of each cut


def _next(x, k):
    """The floats k steps above x (k < 0: below) in the total order of the floats (-0 and +0 count as one)."""
    u = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(u < 0, -(u & 0x7FFFFFFF), u) + k
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _candidates(dim):
    cuts = [-1.5, -0.5, 0.0, dim - 1.5, dim - 0.5, float(dim)]
    grid = np.concatenate([_next(np.full(2 * STEPS + 1, c, F32), np.arange(-STEPS, STEPS + 1)) for c in cuts])
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 3e9, -3e9, 4294967296.0, 1e30, -1e30, dim - 1.0, dim - 2.0], F32)
    return np.concatenate([grid, special])


def _live(x, dim):
    """Stage B's test on one axis: !(x + 0.5 <= -1 | x + 0.5 >= dim), the sum rounded to f32 (a NaN passes)."""
    with np.errstate(invalid="ignore"):
        xr = (x + F32(0.5)).astype(F32)
        return ~((xr <= F32(-1.0)) | (xr >= F32(dim)))


def _as_usize(x):
    """v_cvt_u32_f32: truncation, saturating at 0 and 2^32 - 1, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=2.0 ** 32, neginf=0.0))
    return np.clip(t, 0.0, 2.0 ** 32 - 1).astype(np.uint64)


@pytest.mark.parametrize("tw,th", [(16, 12), (24, 16), (640, 480)])
def test_a_lane_live_after_stage_b_reads_a_cell_inside_the_map(tw, th):
    u, v = _candidates(tw), _candidates(th)
    lu, lv = _live(u, tw), _live(v, th)
    ui, vi = _as_usize(u), _as_usize(v)
    assert lu.any() and (~lu).any() and lv.any() and (~lv).any()
    # one axis at a time: live => ui + 1 <= tw + 1 (the last column of the (tw + 2)-wide map), in fact ui <= tw - 1
    assert (ui[lu] + 1 <= tw + 1).all() and (ui[lu] <= tw - 1).all() and (ui[lu] == tw - 1).any()
    assert (vi[lv] + 1 <= th + 1).all() and (vi[lv] <= th - 1).all() and (vi[lv] == th - 1).any()
    # both axes: the byte offsets of the two f32x2 loads of a live lane (texel_offset, image_icp.hip) end inside the map
    mw, map_bytes = tw + 2, (th + 2) * (tw + 2) * 4
    cu, cv = np.unique(ui[lu]), np.unique(vi[lv])
    off = (cv[:, None] * mw + cu[None, :]) * 4
    assert off.min() == 0 and (off + mw * 4 + 8 <= map_bytes).all()
    # a lane that is dead after stage B reads texel 0 and the texel below it
    assert mw * 4 + 8 <= map_bytes
