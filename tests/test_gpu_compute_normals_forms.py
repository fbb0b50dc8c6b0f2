"""Pixel-grid normals (compute_normals_kernel, align3d_amd/csrc/image.hip) in every tile form at ragged sizes, bit for bit
the oracle's.

The product library picks the form per launch (launch_compute_normals_batch): 64 x 16 tiles with four pixels per thread
when the launch holds at least 4 * 640 * 480 pixels — the form the benchmark measures — and 32 x 8 tiles with one pixel per
thread below.  The sizes here (tests/normals_image_cases.py) put the four-pixel form where an image border cuts a tile:
threads whose four rows straddle the last row, halo rows and columns beyond the image, the dummy loads of lanes outside
it, a tile count that is no multiple of 8 in the XCD-contiguous remap; tests/test_compute_normals_cases_cpu.py asserts the
pixel arithmetic that sends each case to its form.  The diagnostics build forces each of the five shapes
(A3D_NORMALS_SHAPE).  normal_from_neighbours_dev chooses its division by a wave-wide ballot, so which path a pixel takes
depends on the tile shape: every shape meets inputs whose waves mix scales from 1e-12 to 1e12.

Every image goes up WITH a normals plane filled with the word 0xC0FFEE11 (about -7.99: no component of a unit normal
equals it, and it is not NaN), so equality with the oracle proves every pixel was written where it belongs; the image's
points and mask — the normals' neighbours in one arena — come back bit for bit as they went up."""
import numpy as np
import pytest

import normals_image_cases as N
from align3d_amd import CameraIntrinsics, RangeImage, compute_normals_batch

pytestmark = pytest.mark.gpu


def _upload(ctx, points, mask, canary=True):
    h, w = mask.shape
    ri = RangeImage(points, mask, CameraIntrinsics(100, 100, w / 2, h / 2, w, h), normals=N.canary_plane(w, h) if canary else None)
    return ri.device(ctx)


def _check(dev, points, mask, want, label):
    got = dev.download(normals=True, intensity=False, colors=False)
    assert np.array_equal(got.points.view(np.uint32), points.view(np.uint32)), f"{label}: the points changed"
    assert np.array_equal(got.mask, mask), f"{label}: the mask changed"
    N.assert_normals_equal(got.normals, want, label)


def _batch(ctx, w, h, seeds, own=(), label="product"):
    """Uploads image(seed, w, h) for every seed (the seeds in `own` without a normals plane), ONE compute_normals_batch call,
    every image against the oracle."""
    cases = [N.case(seed, w, h) for seed in seeds]
    devs = [_upload(ctx, p, m, canary=seed not in own) for seed, (p, m, _) in zip(seeds, cases)]
    for seed, d in zip(seeds, devs):
        assert d.has_normals() == (seed not in own)
    compute_normals_batch(devs)
    for seed, d, (p, m, want) in zip(seeds, devs, cases):
        assert d.has_normals()
        _check(d, p, m, want, f"{label}, {w} x {h}, image {seed} of {len(devs)}")
    for d in devs:
        d.free()


# ---- product library ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", N.BATCH_SIZES)
def test_batch_of_64_in_the_four_pixel_form(ctx, w, h):
    """64 distinct images in one launch of at least 4 * 640 * 480 pixels: shape 1 at a size that cuts its tiles."""
    assert N.four_pixel_form(64, w, h)
    _batch(ctx, w, h, range(64))


@pytest.mark.parametrize("count", N.BORDER_COUNTS)
def test_launch_border_changes_the_form(ctx, count):
    """65 and 130 images in one call: launches of 64 | 1 and 64 | 64 | 2 images.  The tails fall below the threshold and run
    the one-pixel form; the seeds differ across the border, so an image taken from the wrong launch slot shows."""
    w, h = N.BORDER_SIZE
    assert N.four_pixel_form(64, w, h) and not N.four_pixel_form(count % 64, w, h)
    _batch(ctx, w, h, range(count))


def test_tile_count_with_a_remainder(ctx):
    """63 images of 129 x 152: 1890 tiles of 64 x 16, 2 mod 8 — the remainder branch of xcd_contiguous_index in the batch
    form (64 frames always give a multiple of 8)."""
    w, h = N.REMAINDER_SIZE
    assert N.four_pixel_form(N.REMAINDER_COUNT, w, h)
    _batch(ctx, w, h, range(N.REMAINDER_COUNT))


def test_single_frame_at_the_threshold(ctx):
    """One image of 1283 x 959 = 1 230 397 pixels runs shape 1 on its own: host in / host out, and resident."""
    w, h = N.SINGLE_SIZE
    assert N.four_pixel_form(1, w, h)
    points, mask, want = N.case(0, w, h)
    host = RangeImage(points, mask, CameraIntrinsics(100, 100, w / 2, h / 2, w, h)).compute_normals(ctx)
    N.assert_normals_equal(host.normals, want, "RangeImage.compute_normals, 1283 x 959")
    dev = _upload(ctx, points, mask)
    dev.compute_normals()
    _check(dev, points, mask, want, "DeviceRangeImage.compute_normals, 1283 x 959")
    dev.free()


def test_mixed_ownership_of_the_normals_plane(ctx):
    """One call holds images uploaded without normals (the call allocates them) next to images that carry the canary."""
    w, h = N.BATCH_SIZES[0]
    _batch(ctx, w, h, range(64), own=set(range(0, 64, 3)) | {63})


# ---- diagnostics build: every shape, forced -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", N.SHAPES)
def test_every_tile_shape_forced(diag_ctx, monkeypatch, shape):
    """A3D_NORMALS_SHAPE (read on every launch, diagnostics build only): the resident single-image call and a batch of 5 at
    sizes around every shape's tile, and the twelve wide-dynamic-range cases of
    test_compute_normals_wide_dynamic_range_and_signed_zeros — every shape equals the oracle."""
    monkeypatch.setenv("A3D_NORMALS_SHAPE", str(shape))
    try:
        for (w, h) in N.DIAG_SIZES:
            points, mask, want = N.case(0, w, h)
            dev = _upload(diag_ctx, points, mask)
            dev.compute_normals()
            _check(dev, points, mask, want, f"shape {shape}, single, {w} x {h}")
            dev.free()
            _batch(diag_ctx, w, h, range(N.DIAG_BATCH), label=f"shape {shape}")
        wide = N.wide_range_cases()
        assert len(wide) == 12  # seven scales, four planes, the exact-ratio grid
        wants = N.wide_range_reference()
        for k, ((p, m), want) in enumerate(zip(wide, wants)):
            dev = _upload(diag_ctx, p, m)
            dev.compute_normals()
            _check(dev, p, m, want, f"shape {shape}, single, wide-range case {k}")
            dev.free()
        devs = [_upload(diag_ctx, p, m) for (p, m) in wide]
        compute_normals_batch(devs)
        for k, (d, (p, m), want) in enumerate(zip(devs, wide, wants)):
            _check(d, p, m, want, f"shape {shape}, batch of 12, wide-range case {k}")
            d.free()
    finally:
        monkeypatch.delenv("A3D_NORMALS_SHAPE", raising=False)
