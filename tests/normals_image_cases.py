"""Pixel-grid normals (RangeImage::compute_normals, align3d_amd/csrc/image.hip) at ragged sizes: the shared inputs of
tests/test_compute_normals_cases_cpu.py (the two host references agree on every input, the inputs do what they are meant
to do, and the pixel arithmetic that picks the kernel's tile form) and tests/test_gpu_compute_normals_forms.py (every tile
form on the device, bit for bit against the oracle).  Plain data and numpy; the oracle is loaded on first use only."""
import functools

import numpy as np

# ---- which tile form a launch takes (launch_compute_normals_batch, restated) ------------------------------------------------

MAX_LAUNCH = 64                      # images per launch (NORMALS_MAX_BATCH)
FORM_THRESHOLD = 4 * 640 * 480       # pixels in the launch: at or above it 64 x 16 tiles, four pixels per thread
TILE = {0: (32, 8), 1: (64, 16), 2: (64, 32), 3: (128, 8), 4: (64, 8)}  # shape -> (tile width, tile height)
SHAPES = tuple(TILE)                 # 0 and 1 are in the product library; 2, 3, 4 exist in the diagnostics build only


def four_pixel_form(frames, w, h):
    """Whether a launch of `frames` images of w x h runs shape 1 (otherwise shape 0)."""
    return frames * w * h >= FORM_THRESHOLD


def tiles(w, h, shape=1):
    tw, th = TILE[shape]
    return -(-w // tw), -(-h // th)


# ---- sizes, as (w, h) ---------------------------------------------------------------------------------------------------------

# 64 images of each are at or above the threshold, so a full launch of them runs shape 1
BATCH_SIZES = (
    (161, 121),   # last tile column 33 wide; last tile row 9 high: a thread has two or three of its four rows inside
    (65, 296),    # ONE column in the second tile column
    (63, 305),    # one tile column, not full
    (129, 149),   # 30 tiles per image
    (1281, 15),   # one row below a tile's height
    (1201, 16),   # exactly a tile's height
    (1130, 17),   # one row above it
    (1, 19201),   # degenerate strips: they are here for the loads and stores, not for the values
    (19201, 1),
)
SINGLE_SIZE = (1283, 959)            # 1 230 397 pixels: ONE frame at the threshold (a3d_compute_normals runs shape 1)
BORDER_SIZE, BORDER_COUNTS = (161, 121), (65, 130)   # launches of 64 | 1 and 64 | 64 | 2 images: the tails run shape 0
REMAINDER_SIZE, REMAINDER_COUNT = (129, 152), 63     # 30 * 63 = 1890 tiles = 2 mod 8: the remap's remainder branch
# the diagnostics build forces the shape, so no pixel count is needed
DIAG_SIZES = ((131, 37), (161, 121), (1, 300), (300, 1), (127, 33), (129, 31), (64, 16), (65, 17))
DIAG_BATCH = 5

# ---- images -------------------------------------------------------------------------------------------------------------------

BANDS = (1e-12, 1e-6, 1e-3, 1.0, 1e4, 1e9, 1e12)
BAND_COLUMNS = 5
MASK_VALUES = (0, 1, 1, 1, 1, 1, 2, 255)   # only == 1 counts as valid for a NEIGHBOUR; the centre's mask is not checked
HOSTILE = (np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 3e38)
HOSTILE_WORDS = 40
CANARY_WORD = 0xC0FFEE11             # as an f32 about -7.99: no component of a unit normal, and not NaN


def image(seed, w, h):
    """(points [h, w, 3] f32, mask [h, w] u8).  The scale is constant over runs of 5 columns and cycles through BANDS from
    seed % 7, so one wave holds several scales: some pixels fail mag > 1e-6, some overflow |n|^2, some take the shared
    reciprocal and some the plain division.  40 words are NaN, +-inf, signed zeros, denormals and 3e38."""
    rng = np.random.default_rng([23, seed, w, h])
    band = np.array(BANDS)[(seed + np.arange(w) // BAND_COLUMNS) % len(BANDS)]
    points = (rng.normal(size=(h, w, 3)) * band[None, :, None]).astype(np.float32)
    mask = np.array(MASK_VALUES, np.uint8)[rng.integers(0, len(MASK_VALUES), size=(h, w))]
    at = rng.integers(0, points.size, size=HOSTILE_WORDS)
    points.reshape(-1)[at] = np.array(HOSTILE, np.float32)[np.arange(HOSTILE_WORDS) % len(HOSTILE)]
    return points, mask


@functools.lru_cache(maxsize=320)
def case(seed, w, h):
    """(points, mask, the oracle's normals) of image(seed, w, h), computed once and shared: read-only arrays."""
    import oracle_lib as O

    points, mask = image(seed, w, h)
    want = O.compute_normals(points, mask)
    for a in (points, mask, want):
        a.setflags(write=False)
    return points, mask, want


def canary_plane(w, h):
    return np.full((h, w, 3), CANARY_WORD, np.uint32).view(np.float32)


@functools.lru_cache(maxsize=1)
def wide_range_cases():
    """The twelve 48 x 80 cases of test_compute_normals_wide_dynamic_range_and_signed_zeros as [(points, mask)]: point
    clouds at seven scales from 1e-12 to 1e12, four axis-aligned planes (cross products with -0.0 components), and a grid whose
    neighbour distances stand in the exact ratios 4, 1/4, 1 and 0 / 0."""
    rng = np.random.default_rng(99)
    h, w = 48, 80
    cases = []
    for scale in (1e-12, 1e-6, 1e-3, 1.0, 1e4, 1e9, 1e12):
        cases.append((rng.normal(size=(h, w, 3)) * scale).astype(np.float32))
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    for plane in ((xx, yy, np.zeros_like(xx)), (-xx, yy, np.full_like(xx, 2.0)), (xx, -yy, xx * 0), (yy * 0, xx, -yy)):
        cases.append(np.stack(plane, axis=-1).astype(np.float32))
    # neighbour distances in exact ratios 4, 1/4, 1 and with repeated points (0 / 0)
    steps = np.array([1.0, 2.0, 1.0, 0.5, 0.0, 4.0, 1.0, 1.0], np.float32)
    xs = np.concatenate([[0.0], np.cumsum(np.tile(steps, w // 8 + 1))])[:w].astype(np.float32)
    cases.append(np.stack([np.broadcast_to(xs, (h, w)), np.broadcast_to(xs[:h, None], (h, w)) if h <= w else yy, np.ones((h, w), np.float32)], axis=-1).astype(np.float32))
    out = []
    for pts in cases:
        pts = np.ascontiguousarray(pts)
        mask = (rng.random((h, w)) > 0.1).astype(np.uint8)
        out.append((pts, mask))
    return out


@functools.lru_cache(maxsize=1)
def wide_range_reference():
    """The oracle's normals of wide_range_cases(), computed once."""
    import oracle_lib as O

    return [O.compute_normals(p, m) for (p, m) in wide_range_cases()]


# ---- comparison ---------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_normals_equal(got, want, label):
    """A word that is NaN in the reference is NaN in the result and the reverse; every other word is equal by bits.  (The
    host oracle and the numpy restatement both emit 0xffc00000 for a NaN produced by inf - inf or inf / inf, the GPU's
    default NaN has the other sign: the NaN POSITIONS agree, their signs are nobody's contract.)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (label, got.shape, want.shape, got.dtype)
    nan_got, nan_want = np.isnan(got), np.isnan(want)
    bad = (nan_got != nan_want) | (~nan_want & (_bits(got) != _bits(want)))
    if bad.any():
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(
            f"{label}: {int(bad.sum())} of {bad.size} words differ ({int((nan_got != nan_want).sum())} in NaN-ness); first at "
            f"(row, col, component) {first}: got {got[first]!r} (0x{int(_bits(got)[first]):08x}), "
            f"want {want[first]!r} (0x{int(_bits(want)[first]):08x})")
