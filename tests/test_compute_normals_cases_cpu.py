"""The inputs of tests/test_gpu_compute_normals_forms.py, checked without a GPU: the host oracle and the numpy restatement
— two independent references — agree on every one of them (so a device mismatch later is the device's), the inputs do
what they are meant to do (so the device tests cannot pass vacuously), and the pixel arithmetic that decides which tile
form a launch takes (launch_compute_normals_batch, align3d_amd/csrc/image.hip) puts every case where it is meant to go."""
import numpy as np
import pytest

import normals_image_cases as N
import numpy_restatement as R
import oracle_lib as O

SEEDS = (0, 1, 2, 3)
NAMED_SIZES = N.BATCH_SIZES + (N.SINGLE_SIZE,)
EXTRA_SIZES = tuple(s for s in (N.REMAINDER_SIZE,) + N.DIAG_SIZES if s not in NAMED_SIZES)


def _valid_next_to(normals, mask, value):
    """Pixels with a non-zero, NaN-free normal and a 4-neighbour whose mask is `value`."""
    valid = normals.any(axis=-1) & ~np.isnan(normals).any(axis=-1)
    hit = np.zeros_like(valid)
    m = mask == value
    hit[:, 1:] |= m[:, :-1]
    hit[:, :-1] |= m[:, 1:]
    hit[1:, :] |= m[:-1, :]
    hit[:-1, :] |= m[1:, :]
    return int((valid & hit).sum())


@pytest.mark.parametrize("w,h", NAMED_SIZES + EXTRA_SIZES)
def test_references_agree_and_inputs_bite(w, h):
    for seed in SEEDS:
        points, mask = N.image(seed, w, h)
        again = N.image(seed, w, h)
        assert np.array_equal(points.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(mask, again[1])
        assert points.shape == (h, w, 3) and points.dtype == np.float32 and mask.shape == (h, w) and mask.dtype == np.uint8
        want = O.compute_normals(points, mask)
        with np.errstate(all="ignore"):  # (overflow and inf - inf are what the inputs are for)
            restated = R.compute_normals(points, mask)
        N.assert_normals_equal(restated, want, f"numpy restatement vs oracle, {w} x {h}, seed {seed}")
        assert set(np.unique(mask)) <= {0, 1, 2, 255}
        if (w, h) not in NAMED_SIZES:
            continue
        nan_words = int(np.isnan(want).sum())
        nonzero = float((want != 0).any(axis=-1).mean())  # (NaN != 0 too: a NaN normal was computed, not skipped)
        print(f"{w} x {h} seed {seed}: {100 * nonzero:.1f} % non-zero normals, {nan_words} NaN words of {want.size}")
        assert nan_words < 0.001 * want.size, (seed, nan_words, want.size)
        if w > 1 and h > 1:
            assert nonzero >= 0.30, (seed, nonzero)


def test_masks_other_than_one_meet_valid_normals():
    """Across the cases at least one valid normal lies next to a mask-2 neighbour and one next to a mask-255 neighbour
    (computed here on the first ragged size, so that the test stands on its own)."""
    w, h = N.BATCH_SIZES[0]
    seen = {2: 0, 255: 0}
    for seed in SEEDS:
        points, mask = N.image(seed, w, h)
        want = O.compute_normals(points, mask)
        for value in seen:
            seen[value] += _valid_next_to(want, mask, value)
    assert seen[2] > 0 and seen[255] > 0, seen


def test_seeds_differ():
    a, b = N.image(0, 161, 121), N.image(64, 161, 121)
    assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and not np.array_equal(a[1], b[1])
    # the band starts at seed % 7: columns 0 .. 4 of seed 3 are at scale 1, of seed 6 at 1e12
    big, unit = np.abs(N.image(6, 40, 200)[0][:, :5]), np.abs(N.image(3, 40, 200)[0][:, :5])
    assert np.nanmedian(big) > 1e11 and 0.1 < np.nanmedian(unit) < 10


def test_assert_normals_equal_refuses_what_it_should():
    want = np.array([[[0.0, np.nan, 1.0]]], np.float32)
    other_nan = want.copy()
    other_nan.view(np.uint32)[0, 0, 1] ^= 0x80000000  # the other sign of NaN: accepted
    N.assert_normals_equal(other_nan, want, "NaN sign")
    for bad in (np.array([[[-0.0, np.nan, 1.0]]], np.float32),      # a signed zero is a different word
                np.array([[[0.0, 0.0, 1.0]]], np.float32),          # a number where the reference has NaN
                np.array([[[np.nan, np.nan, 1.0]]], np.float32),    # NaN where the reference has a number
                np.array([[[0.0, np.nan, np.nextafter(np.float32(1), np.float32(2))]]], np.float32)):
        with pytest.raises(AssertionError):
            N.assert_normals_equal(bad, want, "must differ")
    canary = N.canary_plane(3, 2)
    assert canary.dtype == np.float32 and canary.shape == (2, 3, 3) and not np.isnan(canary).any()
    assert -8.0 < canary[0, 0, 0] < -7.9  # no component of a unit normal


def test_the_pixel_arithmetic_that_picks_the_form():
    """launch_compute_normals_batch: shape 1 (64 x 16 tiles, four pixels per thread) when frames * w * h >= 4 * 640 * 480,
    shape 0 (32 x 8, one pixel per thread) below; a launch holds at most 64 images."""
    assert N.FORM_THRESHOLD == 4 * 640 * 480 == 1228800 and N.MAX_LAUNCH == 64
    for (w, h) in N.BATCH_SIZES:
        assert 64 * w * h >= 4 * 640 * 480, (w, h)
    assert 5 * 131 * 37 < 4 * 640 * 480          # the ragged part of test_compute_normals_batch_bit_exact runs shape 0
    assert 63 * 129 * 152 >= 4 * 640 * 480
    assert N.SINGLE_SIZE[0] * N.SINGLE_SIZE[1] == 1230397 >= 4 * 640 * 480
    assert N.four_pixel_form(64, 640, 480) and not N.four_pixel_form(2, 640, 480)
    # the launch border: 65 = 64 | 1 and 130 = 64 | 64 | 2 images, and the tail launches fall below the threshold
    w, h = N.BORDER_SIZE
    assert N.four_pixel_form(64, w, h) and not N.four_pixel_form(1, w, h) and not N.four_pixel_form(2, w, h)
    assert [n % 64 for n in N.BORDER_COUNTS] == [1, 2]
    # the remainder branch of xcd_contiguous_index: a tile count that is no multiple of 8 (64 frames always give one)
    tx, ty = N.tiles(*N.REMAINDER_SIZE)
    assert (tx, ty) == (3, 10) and tx * ty * N.REMAINDER_COUNT == 1890 and 1890 % 8 == 2
    assert N.four_pixel_form(N.REMAINDER_COUNT, *N.REMAINDER_SIZE)
    # what each ragged size is there for, in 64 x 16 tiles
    assert 161 - 2 * 64 == 33 and 121 - 7 * 16 == 9       # rows ty, ty + 4, ty + 8 of the last tile row: 3, 2, 2, 2 inside
    assert N.tiles(65, 296) == (2, 19) and 65 - 64 == 1
    assert N.tiles(63, 305) == (1, 20)
    assert N.tiles(129, 149)[0] * N.tiles(129, 149)[1] == 30
    assert [N.tiles(w, h)[1] for (w, h) in ((1281, 15), (1201, 16), (1130, 17))] == [1, 1, 2]
    assert N.tiles(1, 19201) == (1, 1201) and N.tiles(19201, 1) == (301, 1)


def test_xcd_contiguous_index_is_a_bijection_with_a_remainder():
    """common.hpp's remap, restated: group g = b % 8 takes the g-th contiguous share of the n tiles; the first n % 8
    groups hold one tile more.  Every tile is visited once for the tile counts of the cases above."""
    for n in (1890, 30 * 64, 1, 2, 7, 9, 1201 * 64, 3 * 8 * 5):
        b = np.arange(n)
        g, k, q, r = b & 7, b >> 3, n >> 3, n & 7
        v = np.where(g < r, g * (q + 1), r * (q + 1) + (g - r) * q) + k
        assert np.array_equal(np.sort(v), b), n
