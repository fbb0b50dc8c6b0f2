"""Frame preparation at the edges of its parameter space: the shared case list of tests/test_frame_prep_bounds_cpu.py (which
checks that every input does what it is meant to do, and the two bounds the narrow cells and the splat's launch rest on)
and tests/test_gpu_frame_prep_edges.py (which runs every case on the device, bit for bit against the oracle).  Plain data
and numpy: images below one 32 x 32 patch / one 5 x 6 load patch / one 12^3 blur tile, single rows and columns, sigma_space
on both sides of the narrow / wide cell switch, below 1 and above the image side."""
from collections import namedtuple

import numpy as np

# ---- the grid's own arithmetic (src/bilateral/grid.rs:37-78), restated in float64 ---------------------------------------

NARROW_FLOOR_MAX = 13  # THE RULE of the cell switch: 4-byte cells while floor(sigma_space) <= 13 (13.999 narrow, 14.0 wide)
NARROW_COUNT_MAX = 255
NARROW_SUM_MAX = 255 * 65535  # < 2^24


def is_narrow(sigma_space):
    """The rule, stated once: (floor(sigma_space) + 2)^2 <= 255, i.e. floor(sigma_space) <= 13."""
    return bool(np.floor(min(sigma_space, 1e300)) <= NARROW_FLOOR_MAX)


def grid_side(size, sigma):
    """gh / gw (grid.rs:37-56): sized by a DIVISION."""
    return int(np.float64(size - 1) / np.float64(sigma)) + 5


def splat_rows(size, sigma):
    """floor(x * (1 / sigma) + 0.5) for x = 0 .. size - 1 (grid.rs:60-78): placed by a MULTIPLICATION; the grid row is this
    plus 2."""
    inv = np.float64(1.0) / np.float64(sigma)
    return np.floor(np.arange(size, dtype=np.float64) * inv + 0.5).astype(np.int64)


def fullest_column(img, sigma_space):
    """The most pixels (zeros included: an upper bound on what a cell can count) that one grid (row, column) receives."""
    h, w = img.shape
    return int(np.bincount(splat_rows(h, sigma_space)).max()) * int(np.bincount(splat_rows(w, sigma_space)).max())


# ---- shared sets and images ------------------------------------------------------------------------------------------

SIGMAS = ((4.5, 30.0), (13.0, 30.0), (13.999, 30.0), (14.0, 30.0))

FilterCase = namedtuple("FilterCase", "group name image sigma_space sigma_color host_only")


def _rng(*key):
    return np.random.default_rng([17, *key])


def images_40x50():
    """A: all 65535.  B: 65535 minus 0 .. 2.  C: a 0 / 65535 checkerboard.  D: full-range noise."""
    yy, xx = np.mgrid[0:40, 0:50]
    return {
        "A": np.full((40, 50), 65535, np.uint16),
        "B": (65535 - _rng(1).integers(0, 3, size=(40, 50))).astype(np.uint16),
        "C": (((yy + xx) & 1) * 65535).astype(np.uint16),
        "D": _rng(2).integers(0, 65536, size=(40, 50)).astype(np.uint16),
    }


CELL_SWITCH_SIGMAS = (13.0, 13.999, 14.0, 14.999, 15.0)
CELL_SWITCH_COLORS = {"A": 30.0, "B": 1.0, "C": 30.0, "D": 900.0}  # (1.0 puts image B into adjacent channels)

TINY = ((1, 1), (1, 2), (2, 1), (3, 2), (5, 6), (6, 7), (1, 257), (257, 1), (31, 31), (32, 32), (33, 33), (31, 65))


def shallow_depth(h, w, *key, zeros=True):
    """1000 + 0 .. 59 with about 10 % zeros."""
    rng = _rng(3, h, w, *key)
    d = (1000 + rng.integers(0, 60, size=(h, w))).astype(np.uint16)
    if zeros and h * w > 1:
        d[rng.random((h, w)) < 0.1] = 0
    return d


def one_pixel():
    d = np.zeros((13, 13), np.uint16)
    d[6, 6] = 777
    return d


SMALL_SIGMAS = (0.3, 0.5, 0.75, 0.999)
SMALL_SHAPES = ((24, 20), (1, 37), (37, 1))
LARGE_SIGMAS = (33.0, 1e3, 1e6, 1e12)
# floor(sigma_space) + 2 == 65536: where the switch's square, formed in 32 bits, wrapped to 0 and chose narrow cells
WRAPPED_SWITCH_SIGMA = 65534.5


def cell_switch_cases():
    imgs = images_40x50()
    return [FilterCase("cell switch", f"{k}@{ss}", imgs[k], ss, CELL_SWITCH_COLORS[k], False)
            for ss in CELL_SWITCH_SIGMAS for k in "ABCD"]


def small_sigma_cases():
    return [FilterCase("small sigma_space", f"{h}x{w}@{ss}", shallow_depth(h, w, 1, zeros=False), ss, 30.0, False)
            for ss in SMALL_SIGMAS for (h, w) in SMALL_SHAPES]


def large_sigma_cases():
    img = shallow_depth(24, 20, 1, zeros=False)
    cases = [FilterCase("large sigma_space", f"24x20@{ss:g}", img, ss, 30.0, False) for ss in LARGE_SIGMAS]
    # every pixel of an all-65535 image in ONE cell: 2000 pixels, a count and a sum far beyond the narrow cells
    cases.append(FilterCase("large sigma_space", f"A@{WRAPPED_SWITCH_SIGMA}", images_40x50()["A"], WRAPPED_SWITCH_SIGMA, 30.0, False))
    cases.append(FilterCase("large sigma_space", f"24x20@{WRAPPED_SWITCH_SIGMA}", img, WRAPPED_SWITCH_SIGMA, 30.0, False))
    cases.append(FilterCase("large sigma_space", "24x20@inf,30", img, float("inf"), 30.0, True))
    cases.append(FilterCase("large sigma_space", "24x20@4.5,inf", img, 4.5, float("inf"), True))
    return cases


def tiny_cases():
    cases = []
    for ss, sc in (SIGMAS[0], SIGMAS[2]):
        for (h, w) in TINY:
            cases.append(FilterCase("tiny images", f"{h}x{w}@{ss}", shallow_depth(h, w, 2), ss, sc, False))
        cases.append(FilterCase("tiny images", f"1x1 of 0@{ss}", np.zeros((1, 1), np.uint16), ss, sc, False))
    return cases


def colour_minimum_cases():
    return [
        FilterCase("colour minimum", "one pixel", one_pixel(), 4.5, 30.0, False),
        FilterCase("colour minimum", "0/1", _rng(4).integers(0, 2, size=(30, 30)).astype(np.uint16), 4.5, 0.25, False),
        FilterCase("colour minimum", "1/65535", np.where(_rng(5).random((20, 20)) < 0.5, 1, 65535).astype(np.uint16), 4.5, 900.0, False),
    ]


def filter_cases():
    """Every filter case, the mildest group first."""
    return tiny_cases() + colour_minimum_cases() + cell_switch_cases() + small_sigma_cases() + large_sigma_cases()


def sequence_batches():
    """33 and 65 distinct 5 x 6 images: the device entry's 32-image launch sequence is crossed once and twice."""
    return [np.stack([shallow_depth(5, 6, 6, n, k) for k in range(n)]) for n in (33, 65)]


# ---- builder sizes: (h, w, levels) -----------------------------------------------------------------------------------
# The builder and a3d_range_image_pyramids accept `levels` while side >> (levels - 1) >= 2 on both sides (at most 4 here).
# Six of the sizes ask for more than that — (1, 1, 1), (2, 2, 2), (4, 4, 3), (3, 5, 2), (2, 33, 2), (33, 2, 2): their
# coarsest level would have a side of 1 — and are refused as asked: the device test pins the refusal (status 1, no handle)
# and builds the size with the most levels the entry accepts (none for 1 x 1).  Where the entry accepts more levels than
# listed (four for 17 x 31, 48 x 16 and the 31 .. 33 squares) the size is built both ways.

BUILDER_SIZES = ((1, 1, 1), (2, 2, 2), (4, 4, 3), (5, 3, 1), (3, 5, 2), (8, 8, 3), (17, 31, 3), (48, 16, 3), (2, 33, 2),
                 (33, 2, 2), (31, 31, 3), (32, 32, 3), (33, 33, 3), (65, 31, 4))
BUILDER_REFUSED = ((1, 1, 1), (2, 2, 2), (4, 4, 3), (3, 5, 2), (2, 33, 2), (33, 2, 2))


def accepted_levels(h, w):
    """The most pyramid levels the entry points accept for the size, capped at 4 (0: none)."""
    n = 0
    while n < 4 and (min(h, w) >> n) >= 2:
        n += 1
    return n


def builder_level_sets(h, w, levels):
    """(the level counts to build and compare, whether `levels` as listed is refused)."""
    top = accepted_levels(h, w)
    refused = levels > top
    return sorted({n for n in (levels, top) if 1 <= n <= top}), refused
BUILDER_SIGMAS_ALL = (SIGMAS[0],)                       # every size (and every size without the filter)
BUILDER_SIGMAS_FROM_8 = (SIGMAS[2], (0.75, 30.0))       # sizes with both sides >= 8
DEPTH_SCALE = 0.001


def builder_frame(h, w, k=0):
    """Frame k of a size: depth 900 + 0 .. 199 with about 10 % zeros, random rgb."""
    rng = _rng(7, h, w, k)
    d = (900 + rng.integers(0, 200, size=(h, w))).astype(np.uint16)
    if h * w > 1:
        d[rng.random((h, w)) < 0.1] = 0
    return d, rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def builder_frames_3(h, w):
    """build_many's three frames of a size: two different ones and one whose depth is all zeros."""
    a, b = builder_frame(h, w, 0), builder_frame(h, w, 1)
    return [a, (np.zeros((h, w), np.uint16), b[1]), b]


def builder_camera(h, w):
    return (0.9 * w, 0.9 * w, w / 2.0, h / 2.0)


def builder_sigma_sets(h, w):
    """None = without the filter."""
    return (None,) + BUILDER_SIGMAS_ALL + (BUILDER_SIGMAS_FROM_8 if min(h, w) >= 8 else ())
