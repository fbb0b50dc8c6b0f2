"""The claim behind the early request of the shifted intensity samples (image_icp.hip, Shifted / request_shifted), by
exhaustion in f32 on the CPU.

IntensityMap::bilinear_grad samples at (u + 0.005, v) and (u, v + 0.005).  The pixel loop holds the 2 x 2 cell at
(usize(u), usize(v)); when a shifted sample falls into the next texel it evaluates bilinear_at there.  The kernel now
loads only the column (row) that the held cell lacks, which is right iff

    usize(fl(u + 0.005)) != usize(u)   implies   usize(fl(u + 0.005)) == usize(u) + 1

for every u a live lane can have (u + 0.5 in (-1, tw): negative values, which cast to 0, and the last column included).
Checked here for every float within 64 of each integer 0 ... 4096 (a texel cut) and of the value 0.005 below it (where
leaving begins), around -1.5, -1, -0.5, -0.005 and both zeros, on a sweep through (-1.5, 0), and for NaN; for each value:
the shifted index, the bound of the load (column ui + 2 inside a map of tw + 2 columns for the narrowest image in which
the lane is live), and that the texels and the fraction handed to bilerp are those bilinear_at reads and computes.
The same function serves v with rows for columns."""
import numpy as np

F32 = np.float32
H = F32(0.005)


def _next(x, k):
    """The float k steps above x (k < 0: below) in the total order of the floats (-0 and +0 count as one)."""
    u = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(u < 0, -(u & 0x7FFFFFFF), u) + k
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _around(x, k=64):
    x = np.atleast_1d(np.asarray(x, F32))
    return _next(np.repeat(x, 2 * k + 1), np.tile(np.arange(-k, k + 1), len(x)))


def _usize(x):
    """`x as usize` = v_cvt_u32_f32: truncates, a negative or a NaN gives 0."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.trunc(x), 0).astype(np.int64)


def _values():
    cuts = np.arange(0, 4097, dtype=np.int64)
    parts = [_around(cuts.astype(F32)), _around((cuts.astype(np.float64) - 0.005).astype(F32)),
             _around(F32([-1.5, -1.0, -0.5, -0.005, -0.0, 0.0, 0.005, 0.995])),
             np.array([0x80000001, 0x807FFFFF, 0x00000001, 0x007FFFFF], np.uint32).view(F32)]  # denormals
    lo, hi = int(F32(-1.5).view(np.int32)) & 0x7FFFFFFF, 0
    parts.append((np.arange(hi, lo, 2039, dtype=np.int64) | 0x80000000).astype(np.uint32).view(F32))  # (-1.5, -0]
    parts.append(F32([np.nan]))
    return np.unique(np.concatenate(parts).view(np.uint32)).view(F32)


def _live_width(u):
    """The narrowest image in which a lane at u passes stage B's bounds test, -1 < fl(u + 0.5) < tw (NaN passes as
    column 0); -1 where no image admits it."""
    ur = (u + F32(0.5)).astype(F32)
    with np.errstate(invalid="ignore"):
        tw = np.where(np.isnan(ur), 1, np.floor(ur.astype(np.float64)) + 1).astype(np.int64)
        return np.where(ur <= -1.0, -1, np.maximum(tw, 1))


def _bilinear_at_operands(u):
    """bilinear_at along one axis: the two texel columns it loads and the fraction it hands to bilerp."""
    ui = _usize(u)
    return ui, ui + 1, (u - ui.astype(F32)).astype(F32)


def _shifted_operands(u):
    """stage_d with Shifted along one axis: (leaves, first column = the held cell's second, second column = the one
    requested, fraction)."""
    ui = _usize(u)
    u2 = (u + H).astype(F32)
    leaves = _usize(u2) != ui
    return leaves, ui + 1, ui + 2, (u2 - (ui + 1).astype(F32)).astype(F32)


def test_values_cover_the_cuts():
    u = _values()
    ui, u2i = _usize(u), _usize((u + H).astype(F32))
    leaves = u2i != ui
    assert len(u) > 2 * 4097 * 100
    for c in (1, 2, 640, 4095, 4096):  # leaving and staying lanes on either side of a cut's pre-image
        near = (u > c - 0.01) & (u < c + 0.01)
        assert leaves[near].any() and (~leaves[near]).any(), c
        assert (u[near & leaves] < c).all() and ((u[near & ~leaves] >= c) | (u[near & ~leaves] < c - 0.0049)).all(), c
    neg = u < 0
    assert neg.sum() > 100000 and ((u > -0.005) & neg).sum() > 64 and (u[neg].min() < -1.0)
    assert np.isnan(u).any()


def test_a_shifted_sample_leaves_by_exactly_one_texel():
    u = _values()
    ui, u2i = _usize(u), _usize((u + H).astype(F32))
    assert ((u2i == ui) | (u2i == ui + 1)).all()
    with np.errstate(invalid="ignore"):
        assert (u2i[~(u >= F32(0.5))] == 0).all()  # a negative u (and a NaN) casts to 0 and stays there
        assert (ui[~(u > 0)] == 0).all()


def test_the_requested_texels_lie_inside_the_map():
    u = _values()
    tw = _live_width(u)
    live = tw > 0
    assert live.sum() > 0.9 * len(u) and (~live).any()
    ui = _usize(u)
    leaves, _, second, _ = _shifted_operands(u)
    assert (ui[live] <= tw[live] - 1).all()               # stage B's bound, which the request relies on
    assert (second[live] <= tw[live] + 1).all()           # column ui + 2 of a map tw + 2 wide (item 2's bound)
    assert (second[live & leaves] <= tw[live & leaves]).all()  # (in fact never the last column: u + 0.005 < tw - 0.495)
    # the last column of the image is reached by live lanes that do not leave, the one before it by lanes that do
    for w in (1, 2, 37, 640, 4096):
        at = live & (tw == w)
        assert at.any() and (ui[at] == w - 1).any(), w
        if w > 1:
            assert (leaves & live & (ui == w - 2)).any(), w


def test_bilerp_gets_the_operands_of_bilinear_at():
    u = _values()
    leaves, c0, c1, frac = _shifted_operands(u)
    assert leaves.sum() > 4096 * 30
    u2 = (u + H).astype(F32)
    a0, a1, afrac = _bilinear_at_operands(u2[leaves])     # the sample that leaves: bilinear_at(u + 0.005, .)
    assert np.array_equal(a0, c0[leaves]) and np.array_equal(a1, c1[leaves])
    assert np.array_equal(afrac.view(np.uint32), frac[leaves].view(np.uint32))
    # the other axis of that sample is the unshifted coordinate: the held cell's rows and the fraction stage D has already
    b0, b1, bfrac = _bilinear_at_operands(u)
    ui = _usize(u)
    assert np.array_equal(b0, ui) and np.array_equal(b1, ui + 1)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bfrac.view(np.uint32), (u - ui.astype(F32)).astype(F32).view(np.uint32))


def test_on_a_map_the_two_forms_read_the_same_texels():
    """bilerp's four texel arguments and two fractions for uh and vh, through a small map of distinct values: the form
    that reuses the held cell against bilinear_at, on a lattice of (u, v) that leave in u, in v, in both and in neither."""
    tw, th = 9, 7
    imap = np.random.default_rng(7).random((th + 2, tw + 2)).astype(F32)
    edge = F32([0.0, 0.3, 0.9949, 0.995, 0.9951, 0.99999])
    us = (np.arange(tw)[:, None].astype(F32) + edge[None, :]).astype(F32).ravel()
    vs = (np.arange(th)[:, None].astype(F32) + edge[None, :]).astype(F32).ravel()
    us, vs = us[us + F32(0.5) < tw], vs[vs + F32(0.5) < th]
    u, v = [a.ravel() for a in np.meshgrid(us, vs)]
    ui, vi = _usize(u), _usize(v)
    ul, uc0, uc1, ufr = _shifted_operands(u)
    vl, vr0, vr1, vfr = _shifted_operands(v)
    assert (ul & ~vl).any() and (~ul & vl).any() and (ul & vl).any() and (~ul & ~vl).any()
    uf, vf = (u - ui.astype(F32)).astype(F32), (v - vi.astype(F32)).astype(F32)

    def at(um, vm):  # bilinear_at's six operands
        a, b = _usize(um), _usize(vm)
        return (imap[b, a], imap[b, a + 1], imap[b + 1, a], imap[b + 1, a + 1], (um - a.astype(F32)).astype(F32),
                (vm - b.astype(F32)).astype(F32))

    t10, t01, t11 = imap[vi, ui + 1], imap[vi + 1, ui], imap[vi + 1, ui + 1]  # the held cell
    new_u = (t10, imap[vi, uc1], t11, imap[vi + 1, uc1], ufr, vf)
    new_v = (t01, t11, imap[vr1, ui], imap[vr1, ui + 1], uf, vfr)
    for sel, new, old in ((ul, new_u, at((u + H).astype(F32), v)), (vl, new_v, at(u, (v + H).astype(F32)))):
        for k, (a, b) in enumerate(zip(new, old)):
            assert np.array_equal(a[sel].view(np.uint32), b[sel].view(np.uint32)), k
