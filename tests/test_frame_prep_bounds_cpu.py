"""The two arguments the packed bilateral grid rests on, and the inputs of tests/test_gpu_frame_prep_edges.py (CPU: numpy
and the oracle).

(a) "at most floor(sigma) + 1 image rows round to one grid row" (bilateral.hip, bilateral_grids_enqueue): the narrow u32
    cells (value sum << 8 | count) hold a count below 2^8 and a sum below 2^24 because of it.
(b) "pixels splat into grid rows 2 .. gh - 2" (splat_packed_kernel): one splat thread per such row, `(gh - 3) * (gw - 3)`
    extents, and `splat_starts` tables of gh - 2 entries.
gh is sized by a division, (h - 1) / sigma; a pixel's row is placed by a multiplication, x * (1 / sigma) + 0.5
(src/bilateral/grid.rs:37-78).  The two round differently, so both bounds are evaluated in the splat's own float64
arithmetic, over random sigmas, the integers and their float64 neighbours, and for (b) the sigmas at which (size - 1) / sigma
is an integer."""
import numpy as np

import frame_prep_edge_cases as E
import oracle_lib as O

SIZES = (1, 2, 7, 50, 257, 640)


def _sweep():
    rng = np.random.default_rng(20240)
    ints = np.arange(1, 41, dtype=np.float64)
    s = np.concatenate([rng.uniform(0.05, 40.0, size=3000), ints, np.nextafter(ints, 0.0), np.nextafter(ints, 100.0)])
    assert s.size >= 3120 and s.min() > 0.05 - 1e-9
    return s


def _adversarial(size):
    """(size - 1) / k for k = 1 .. size - 1 and both float64 neighbours: where division and multiplication can disagree."""
    if size < 2:
        return np.empty(0)
    q = np.float64(size - 1) / np.arange(1, size, dtype=np.float64)
    return np.concatenate([q, np.nextafter(q, 0.0), np.nextafter(q, 1e9)])


def test_the_switch_rule_is_floor_sigma_space_at_most_13():
    # the rule, stated once (E.is_narrow): (floor(sigma_space) + 2)^2 <= 255  <=>  floor(sigma_space) <= 13
    for s in np.concatenate([_sweep(), [13.0, 13.999, 14.0, 14.999, 15.0, 1e3, 1e6, 1e12, E.WRAPPED_SWITCH_SIGMA, np.inf]]):
        assert E.is_narrow(s) == ((int(np.floor(min(s, 1e300))) + 2) ** 2 <= 255), s
    assert E.is_narrow(13.999) and E.is_narrow(np.nextafter(14.0, 0.0)) and not E.is_narrow(14.0)
    assert all(E.is_narrow(s) for s in E.SMALL_SIGMAS) and not any(E.is_narrow(s) for s in E.LARGE_SIGMAS)
    # the square formed in 32 bits is 0 at floor(sigma_space) + 2 == 65536: the sigma the device tests run as a wide case
    reach = int(np.floor(E.WRAPPED_SWITCH_SIGMA)) + 2
    assert (reach * reach) % 2 ** 32 == 0 and not E.is_narrow(E.WRAPPED_SWITCH_SIGMA)


def test_bound_a_rows_per_grid_row_and_the_narrow_cell():
    checked = 0
    for sigma in _sweep():
        fl = int(np.floor(sigma))
        for size in SIZES:
            per_row = int(np.bincount(E.splat_rows(size, sigma)).max())
            assert per_row <= fl + 1, (sigma, size, per_row)
            if E.is_narrow(sigma):
                # a cell counts at most per_row^2 pixels of at most 65535 each
                assert per_row * per_row <= E.NARROW_COUNT_MAX, (sigma, size)
                assert per_row * per_row * 65535 <= E.NARROW_SUM_MAX < 2 ** 24, (sigma, size)
            checked += 1
    assert checked >= 3120 * len(SIZES)
    assert E.NARROW_SUM_MAX * 4 ** 4 < 2 ** 32  # four unnormalised integer blur passes stay in u32


def test_bound_b_splat_rows_and_slice_reads_stay_inside_the_grid():
    checked = 0
    for size in SIZES:
        for sigma in np.concatenate([_sweep(), _adversarial(size)]):
            inv = np.float64(1.0) / np.float64(sigma)
            gh = E.grid_side(size, sigma)
            last = np.float64(size - 1) * inv
            assert int(np.floor(last + 0.5)) + 2 <= gh - 2, (size, sigma)  # the splat's highest row
            assert int(np.floor(last + 2.0)) + 1 <= gh - 1, (size, sigma)  # the slice's highest read (grid.rs:132-146)
            checked += 1
    assert checked >= len(SIZES) * 3120 + 3 * sum(s - 1 for s in SIZES)


# ---- the inputs of the device tests do their job ------------------------------------------------------------------------

def test_cell_switch_images_fill_a_cell_to_13x13_and_14x14():
    imgs = E.images_40x50()
    for ss, side in ((13.0, 13), (13.999, 14)):
        for img in imgs.values():
            assert E.fullest_column(img, ss) == side * side
    # image A puts exactly that many pixels of 65535 into one cell: 196 x 65535 of the 2^24 the narrow sum holds
    a = imgs["A"]
    r, c = E.splat_rows(40, 13.999), E.splat_rows(50, 13.999)
    counts = np.zeros((r.max() + 1, c.max() + 1), np.int64)
    np.add.at(counts, (r[:, None], c[None, :]), 1)
    assert counts.max() == 196 and 196 * int(a.max()) == 12844860 < 2 ** 24
    assert {cs.sigma_space for cs in E.cell_switch_cases()} == set(E.CELL_SWITCH_SIGMAS)
    assert len(E.cell_switch_cases()) == 20


def test_small_sigma_cases_leave_grid_rows_empty():
    cases = E.small_sigma_cases()
    assert len(cases) == len(E.SMALL_SIGMAS) * len(E.SMALL_SHAPES)
    for cs in cases:
        empty = 0
        for size in cs.image.shape:
            g = E.grid_side(size, cs.sigma_space)
            got = set(E.splat_rows(size, cs.sigma_space).tolist())
            assert max(got) <= g - 4
            empty += sum(1 for t in range(g - 3) if t not in got)  # the splat's threads whose [starts[t], starts[t + 1]) is empty
        assert empty >= 1, cs.name
        if cs.sigma_space <= 0.5 and max(cs.image.shape) > 1:
            assert empty >= max(cs.image.shape) - 1  # grids with more rows than the image: most rows hold nothing


def test_large_sigma_cases_have_a_5x5_grid():
    for cs in E.large_sigma_cases():
        if cs.sigma_space > max(cs.image.shape):
            st, _, dims = O.bilateral(cs.image, cs.sigma_space, cs.sigma_color)
            assert st == 0 and dims[0] == dims[1] == 5, cs.name
            assert E.grid_side(cs.image.shape[0], cs.sigma_space) == E.grid_side(cs.image.shape[1], cs.sigma_space) == 5
    assert sum(cs.host_only for cs in E.large_sigma_cases()) == 2
    assert {cs.sigma_space for cs in E.large_sigma_cases()} >= set(E.LARGE_SIGMAS)


def test_tiny_and_builder_case_lists():
    tiny = E.tiny_cases()
    assert len(tiny) == 2 * (len(E.TINY) + 1)
    assert {cs.image.shape for cs in tiny} == set(E.TINY)
    assert any(cs.image.shape == (1, 1) and cs.image[0, 0] == 0 for cs in tiny)
    assert any(cs.image.shape == (1, 1) and cs.image[0, 0] > 0 for cs in tiny)
    assert all(min(cs.image.shape) < 32 or cs.image.shape in ((32, 32), (33, 33)) for cs in tiny)
    one = E.one_pixel()
    assert one.shape == (13, 13) and one[6, 6] == 777 and np.count_nonzero(one) == 1
    for batch, n in zip(E.sequence_batches(), (33, 65)):
        assert batch.shape == (n, 5, 6) and len({b.tobytes() for b in batch}) == n
    assert len(E.BUILDER_SIZES) == 14
    for h, w, levels in E.BUILDER_SIZES:
        assert 1 <= levels <= 4
        build, refused = E.builder_level_sets(h, w, levels)
        accepted = (h >> (levels - 1)) >= 2 and (w >> (levels - 1)) >= 2  # the entry points' own condition
        assert refused == (not accepted) == ((h, w, levels) in E.BUILDER_REFUSED)
        assert all((min(h, w) >> (n - 1)) >= 2 for n in build) and (build or (h, w) == (1, 1))
        assert (levels in build) == accepted and E.accepted_levels(h, w) in build + [0]
        frames = E.builder_frames_3(h, w)
        assert not frames[1][0].any() and frames[0][0].any()
        assert (h * w == 1) or not np.array_equal(frames[0][0], frames[2][0])
        assert E.builder_sigma_sets(h, w)[:2] == (None, (4.5, 30.0))
        assert (len(E.builder_sigma_sets(h, w)) == 4) == (min(h, w) >= 8)


def test_the_oracle_accepts_every_filter_case():
    """Status 0 and at most 2^20 cells for every case (a condition the cases meet: it keeps the device tests at seconds
    each); the all-65535 image comes back as 65534 / 65535 — a truncating cast of a convex combination of equal values."""
    biggest = 0
    for cs in E.filter_cases():
        st, out, dims = O.bilateral(cs.image, cs.sigma_space, cs.sigma_color)
        assert st == 0, cs
        cells = int(np.prod([int(d) for d in dims]))
        assert cells <= 2 ** 20, (cs.group, cs.name, dims)
        biggest = max(biggest, cells)
        if cs.image.min() == 65535:
            assert out.min() >= 65534 and out.max() <= 65535, (cs.name, int(out.min()))
        if not cs.image.any():
            assert not out.any()
    # the largest grids: the checkerboard's 8 x 8 x 2189 (0 .. 65535 at sigma_color 30), and by rows x columns the
    # 81 x 68 x 6 of sigma_space 0.3 on 24 x 20
    assert biggest == 8 * 8 * 2189
    small = [cs for cs in E.small_sigma_cases() if cs.name == "24x20@0.3"][0]
    assert O.bilateral(small.image, small.sigma_space, small.sigma_color)[2] == (81, 68, 6)
    tiny = [cs for cs in E.tiny_cases() if cs.image.shape == (1, 1)][0]
    assert O.bilateral(tiny.image, tiny.sigma_space, tiny.sigma_color)[2] == (5, 5, 5)  # one blur tile
    for batch in E.sequence_batches():
        assert all(O.bilateral(img, 4.5, 30.0)[0] == 0 for img in batch[:3])


def test_the_oracle_builds_every_builder_case():
    for h, w, listed in E.BUILDER_SIZES:
        depth, rgb = E.builder_frame(h, w)
        for levels in E.builder_level_sets(h, w, listed)[0]:
            for sig in E.builder_sigma_sets(h, w):
                d = depth
                if sig is not None:
                    st, d, _ = O.bilateral(depth, *sig)
                    assert st == 0
                pyr = O.build_pyramid(d, rgb, *E.builder_camera(h, w), E.DEPTH_SCALE, levels=levels, use_bilateral=False)
                assert [p.mask.shape for p in pyr] == [(h >> k, w >> k) for k in range(levels)]
            assert len(O.build_pyramid(depth, rgb, *E.builder_camera(h, w), E.DEPTH_SCALE, levels=levels, use_bilateral=True)) == levels
