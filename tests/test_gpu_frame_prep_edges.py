"""Frame preparation (bilateral.hip, bilateral.hpp, frame.hip) at the edges of its parameter space, bit for bit against the
oracle over every pixel of every case of tests/frame_prep_edge_cases.py: images smaller than one 32 x 32 patch / one 5 x 6
load patch / one 12^3 blur tile, single rows and columns, sigma_space on both sides of the narrow / wide cell switch
(floor(sigma_space) <= 13), below 1 (grids with more rows than the image) and above the image side (one (row, column) takes
every pixel).  tests/test_frame_prep_bounds_cpu.py checks that each input does what it is meant to do.  One test per group,
the mildest first; each prints how many cases and images it compared."""
import ctypes as C

import numpy as np
import pytest

import frame_prep_edge_cases as E
import oracle_lib as O
from align3d_amd import A3dError, BilateralFilter, CameraIntrinsics, Context, RangeImageBuilder, _abi

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(cs):
    """The oracle's filter of a case, computed once: (output, grid dimensions)."""
    key = (cs.group, cs.name)
    if key not in _refs:
        st, out, dims = O.bilateral(cs.image, cs.sigma_space, cs.sigma_color)
        assert st == 0, key
        out.setflags(write=False)
        _refs[key] = (out, dims)
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_image(got, ref, what):
    assert got.shape == ref.shape and np.array_equal(got, ref), (what, int(np.sum(got != ref)))


def _host_filter(c, cs):
    f = BilateralFilter.new(cs.sigma_space, cs.sigma_color)
    out = f.filter(c, cs.image)
    ref, dims = _ref(cs)
    assert f.last_grid_dims == dims, (cs.group, cs.name, f.last_grid_dims, dims)
    _same_image(out, ref, (cs.group, cs.name))


def _device_filter(c, imgs, ss, sc):
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, h, w = imgs.shape
    d_in, d_out = c.to_device(imgs), c.malloc(imgs.nbytes)
    try:
        BilateralFilter.new(ss, sc).filter_device(c, d_in, n, w, h, d_out)
        return c.to_host(d_out, np.empty_like(imgs))
    finally:
        c.free(d_in), c.free(d_out)


# ---- 1. the filter, three ways ---------------------------------------------------------------------------------------

def test_filter_host_entry(ctx):
    cases = E.filter_cases()
    for cs in cases:
        _host_filter(ctx, cs)
    print(f"host entry: {len(cases)} cases, {len(cases)} images")


def test_filter_device_entry(ctx):
    batches = {}
    for cs in E.filter_cases():
        if not cs.host_only:
            batches.setdefault((cs.image.shape, cs.sigma_space, cs.sigma_color), []).append(cs)
    images = 0
    for (shape, ss, sc), group in batches.items():  # all images of one size and sigma: one batch
        got = _device_filter(ctx, np.stack([cs.image for cs in group]), ss, sc)
        for g, cs in zip(got, group):
            _same_image(g, _ref(cs)[0], (cs.group, cs.name))
        images += len(group)
    for batch in E.sequence_batches():  # 33 and 65 images: the 32-image launch sequence is crossed once and twice
        got = _device_filter(ctx, batch, 4.5, 30.0)
        for k, (g, img) in enumerate(zip(got, batch)):
            st, ref, _ = O.bilateral(img, 4.5, 30.0)
            assert st == 0
            _same_image(g, ref, ("sequence", len(batch), k))
        images += len(batch)
    refused = [cs for cs in E.filter_cases() if cs.host_only]
    assert len(refused) == 2
    for cs in refused:  # the infinities are the host entry's alone
        with pytest.raises(A3dError) as e:
            _device_filter(ctx, cs.image[None], cs.sigma_space, cs.sigma_color)
        assert e.value.status == 1
    print(f"device entry: {len(batches) + 2} batches, {images} images; 2 refused")


# ---- 2. the cell switch, cross-checked -------------------------------------------------------------------------------

def test_narrow_cells_equal_wide_cells_below_the_switch(diag_ctx, monkeypatch):
    """For sigma_space < 14 the default run (u32 cells) equals the run with A3D_BILATERAL_CELLS=wide (u64 cells, f64 blur),
    and both the oracle; every blurred cell starts as NaN (A3D_BILATERAL_POISON), so a slice that read a cell no marked
    tile wrote fails the cast check."""
    cases = [cs for cs in E.filter_cases() if cs.sigma_space < 14.0]
    assert all(E.is_narrow(cs.sigma_space) for cs in cases) and len(cases) > 40
    monkeypatch.setenv("A3D_BILATERAL_POISON", "1")
    for cs in cases:
        outs = []
        for mode in (None, "wide"):
            if mode:
                monkeypatch.setenv("A3D_BILATERAL_CELLS", mode)
            else:
                monkeypatch.delenv("A3D_BILATERAL_CELLS", raising=False)
            f = BilateralFilter.new(cs.sigma_space, cs.sigma_color)
            outs.append(f.filter(diag_ctx, cs.image))
            assert f.last_grid_dims == _ref(cs)[1]
        _same_image(outs[0], outs[1], (cs.group, cs.name, "narrow against wide"))
        _same_image(outs[0], _ref(cs)[0], (cs.group, cs.name))
    print(f"cell switch cross-check: {len(cases)} cases, {2 * len(cases)} images")


# ---- 3. the builder --------------------------------------------------------------------------------------------------

def _assert_same_level(dev_level, ref, what):
    got = dev_level.download()
    assert got.mask.shape == ref.mask.shape, what
    assert np.array_equal(got.mask, ref.mask), what
    assert np.array_equal(_bits(got.points), _bits(ref.points)), what
    assert np.array_equal(_bits(got.normals), _bits(ref.normals)), what
    assert np.array_equal(got.colors, ref.colors), what
    assert np.array_equal(got.intensities, ref.intensities), what
    assert np.array_equal(_bits(got.intensity_map), _bits(ref.intensity_map)), what
    k = got.intrinsics
    assert (k.fx, k.fy, k.cx, k.cy) == (ref.fx, ref.fy, ref.cx, ref.cy), what


def _oracle_pyramid(depth, rgb, h, w, levels, sig):
    """`sig`: None (no filter), "default" (the oracle's own builder with the default filter) or (sigma_space, sigma_color):
    the oracle's filter, then its builder without one."""
    cam = E.builder_camera(h, w)
    if sig == "default":
        return O.build_pyramid(depth, rgb, *cam, E.DEPTH_SCALE, levels=levels, use_bilateral=True)
    if sig is not None:
        st, depth, _ = O.bilateral(depth, *sig)
        assert st == 0
    return O.build_pyramid(depth, rgb, *cam, E.DEPTH_SCALE, levels=levels, use_bilateral=False)


def _builder(c, levels, sig):
    b = RangeImageBuilder(c).pyramid_levels(levels)
    if sig == "default":
        b = b.with_bilateral_filter(BilateralFilter.default())
    elif sig is not None:
        b = b.with_bilateral_filter(BilateralFilter.new(*sig))
    return b


def _free(pyramids):
    for pyr in pyramids:
        for lv in pyr:
            lv.free()


def _builder_runs():
    for h, w, listed in E.BUILDER_SIZES:
        for levels in E.builder_level_sets(h, w, listed)[0]:
            for sig in E.builder_sigma_sets(h, w):
                yield h, w, levels, sig


def _raw_build(c, levels, h, w, depth, rgb):
    """a3d_range_image_build_pyramids as RangeImageBuilder.build_many calls it: (status, the handle array)."""
    p = RangeImageBuilder(c).pyramid_levels(levels)._params()
    fx, fy, cx, cy = E.builder_camera(h, w)
    dptr, cptr = (C.c_void_p * 1)(_abi.ptr(depth)), (C.c_void_p * 1)(_abi.ptr(rgb))
    out = (C.c_void_p * levels)()
    st = c.lib.a3d_range_image_build_pyramids(c.handle, C.byref(p), 1, dptr, cptr, w, h, fx, fy, cx, cy, float(E.DEPTH_SCALE), out)
    return st, out


def test_builder_single_frames(ctx):
    runs = 0
    for h, w, levels, sig in _builder_runs():
        depth, rgb = E.builder_frame(h, w)
        cam = CameraIntrinsics(*E.builder_camera(h, w), w, h)
        pyr = _builder(ctx, levels, sig).build(cam, depth, rgb, E.DEPTH_SCALE)
        assert [lv.shape for lv in pyr] == [(h >> k, w >> k) for k in range(levels)]
        for k, (lv, r) in enumerate(zip(pyr, _oracle_pyramid(depth, rgb, h, w, levels, sig))):
            _assert_same_level(lv, r, (h, w, levels, sig, k))
        _free([pyr])
        runs += 1
    # a level count whose coarsest side would be 1 is refused, and nothing is handed out
    refused = 0
    for h, w, listed in E.BUILDER_SIZES:
        if E.builder_level_sets(h, w, listed)[1]:
            st, out = _raw_build(ctx, listed, h, w, *E.builder_frame(h, w))
            assert st == _abi.A3D_INVALID_PARAMETER and all(o is None for o in out), (h, w, listed)
            refused += 1
    assert refused == len(E.BUILDER_REFUSED)
    print(f"builder, build: {runs} pyramids of {len(E.BUILDER_SIZES) - 1} sizes; {refused} level counts refused")


def test_builder_batches_of_three(ctx):
    runs = 0
    for h, w, levels, sig in _builder_runs():
        frames = E.builder_frames_3(h, w)  # (the second frame's depth is all zeros)
        cam = CameraIntrinsics(*E.builder_camera(h, w), w, h)
        many = _builder(ctx, levels, sig).build_many(cam, frames, E.DEPTH_SCALE)
        assert len(many) == 3
        for f, ((depth, rgb), pyr) in enumerate(zip(frames, many)):
            for k, (lv, r) in enumerate(zip(pyr, _oracle_pyramid(depth, rgb, h, w, levels, sig))):
                _assert_same_level(lv, r, (h, w, levels, sig, f, k))
        _free(many)
        runs += 1
    print(f"builder, build_many: {runs} batches, {3 * runs} pyramids")


def test_builder_patch_kernel_from_a_poisoned_grid(diag_ctx, monkeypatch):
    """The default sigmas (and no filter) again on the diagnostics build with the earlier level-0 kernel
    (A3D_BUILDER_L0=patch) and every blurred cell starting as NaN: the same bits."""
    for k in ("A3D_BUILDER_FUSE_L1", "A3D_BUILDER_FUSE_L2", "A3D_BUILDER_UNSPLAT", "A3D_BILATERAL_MINMAX", "A3D_BILATERAL_CELLS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("A3D_BUILDER_L0", "patch")
    monkeypatch.setenv("A3D_BILATERAL_POISON", "1")
    runs = 0
    for h, w, listed in E.BUILDER_SIZES:
        for levels in E.builder_level_sets(h, w, listed)[0]:
            for sig in (None, "default", E.SIGMAS[0]):
                depth, rgb = E.builder_frame(h, w)
                cam = CameraIntrinsics(*E.builder_camera(h, w), w, h)
                pyr = _builder(diag_ctx, levels, sig).build(cam, depth, rgb, E.DEPTH_SCALE)
                for k, (lv, r) in enumerate(zip(pyr, _oracle_pyramid(depth, rgb, h, w, levels, sig))):
                    _assert_same_level(lv, r, (h, w, levels, sig, k))
                _free([pyr])
                runs += 1
    print(f"builder, patch kernel + poison: {runs} pyramids")


def test_pyramid_of_a_built_level0_equals_the_builders_levels(ctx):
    """RangeImage::pyramid (a3d_range_image_pyramids) on a level 0 the builder made, at sizes below the 34 x 66 where
    test_builder_equivalence stops: the builder's own levels, every field."""
    runs = 0
    for h, w, listed in E.BUILDER_SIZES:
        for levels in E.builder_level_sets(h, w, listed)[0]:
            for sig in (None, E.SIGMAS[0]):
                depth, rgb = E.builder_frame(h, w)
                cam = CameraIntrinsics(*E.builder_camera(h, w), w, h)
                ref = _builder(ctx, levels, sig).build(cam, depth, rgb, E.DEPTH_SCALE)
                lv0 = _builder(ctx, 1, sig).build(cam, depth, rgb, E.DEPTH_SCALE)[0]
                got = lv0.pyramid(levels, 1.0)
                assert got[0] is lv0 and len(got) == levels
                for k, (g, r, o) in enumerate(zip(got, ref, _oracle_pyramid(depth, rgb, h, w, levels, sig))):
                    _assert_same_level(g, o, (h, w, levels, sig, k, "pyramid"))
                    _assert_same_level(r, o, (h, w, levels, sig, k, "builder"))
                _free([got, ref])
                runs += 1
        if E.builder_level_sets(h, w, listed)[1] and E.accepted_levels(h, w) >= 1:  # refused here as by the builder
            lv0 = _builder(ctx, 1, None).build(CameraIntrinsics(*E.builder_camera(h, w), w, h), *E.builder_frame(h, w), E.DEPTH_SCALE)[0]
            with pytest.raises(A3dError) as e:
                lv0.pyramid(listed, 1.0)
            assert e.value.status == 1
            lv0.free()
    print(f"pyramid of a built level 0: {runs} pyramids")


# ---- 4. the scratch region across layouts ----------------------------------------------------------------------------

def test_scratch_region_stays_clean_across_layouts():
    """One context of its own; the host filter, the device filter and the builder in turn, every step with another layout
    of the grid scratch region (a3d_context::grid_clean / grid_layout_frames): narrow then wide cells, the 5^3 grid of a
    1 x 1 image then 81 x 68 rows x columns, 1 x 1 then 40 x 50 pixels, one frame then 33.  Then the first three steps
    again.  Every result is the oracle's."""
    imgs = E.images_40x50()
    one = [cs for cs in E.tiny_cases() if cs.image.shape == (1, 1) and cs.image.any()][0]
    small = [cs for cs in E.small_sigma_cases() if cs.name == "24x20@0.3"][0]
    narrow = E.FilterCase("layouts", "B narrow", imgs["B"], 13.999, 1.0, False)
    wide = E.FilterCase("layouts", "D wide", imgs["D"], 14.0, 900.0, False)
    own = Context(0)
    steps = 0

    def build(frames, h, w, levels, sig):
        many = _builder(own, levels, sig).build_many(CameraIntrinsics(*E.builder_camera(h, w), w, h), frames, E.DEPTH_SCALE)
        for f, ((depth, rgb), pyr) in enumerate(zip(frames, many)):
            for k, (lv, r) in enumerate(zip(pyr, _oracle_pyramid(depth, rgb, h, w, levels, sig))):
                _assert_same_level(lv, r, (h, w, levels, sig, f, k))
        _free(many)

    first_three = (lambda: _host_filter(own, narrow),                                 # 40 x 50, narrow cells
                   lambda: build([E.builder_frame(2, 2)], 2, 2, 1, E.SIGMAS[0]),      # the builder's smallest: one blur tile
                   lambda: _host_filter(own, wide))                                   # wide cells
    try:
        for step in first_three:
            step()
        _host_filter(own, one)                                                        # 1 x 1: a 5 x 5 x 5 grid
        build([E.builder_frame(8, 8, k) for k in range(33)], 8, 8, 3, E.SIGMAS[2])    # 33 frames, narrow
        _host_filter(own, small)                                                      # 81 x 68 x 6
        build([E.builder_frame(65, 31)], 65, 31, 4, E.SIGMAS[3])                      # one frame, wide
        batch = E.sequence_batches()[0]                                               # 33 images through the device entry
        got = _device_filter(own, batch, 4.5, 30.0)
        for g, img in zip(got, batch):
            _same_image(g, O.bilateral(img, 4.5, 30.0)[1], "layouts, device entry")
        _host_filter(own, one)
        build(E.builder_frames_3(40, 50), 40, 50, 3, E.SIGMAS[1])                     # 40 x 50 after 1 x 1
        steps = 3 + 7
        for step in first_three:
            step()
        steps += 3
    finally:
        own.close()
    print(f"scratch layouts: {steps} steps on one context")


# ---- 5. errors ---------------------------------------------------------------------------------------------------------

def test_a_refused_build_leaves_the_context_usable():
    """3 x 3 with pyramid_levels == 2: the coarsest side would be 1.  Status 1, no handle written, and the next build on
    the same context equals the oracle."""
    own = Context(0)
    try:
        depth, rgb = E.builder_frame(3, 3)
        for sig in (None, E.SIGMAS[0]):
            st, out = _raw_build(own, 2, 3, 3, depth, rgb)
            assert st == _abi.A3D_INVALID_PARAMETER == 1 and all(o is None for o in out)
            with pytest.raises(A3dError) as e:
                _builder(own, 2, sig).build(CameraIntrinsics(*E.builder_camera(3, 3), 3, 3), depth, rgb, E.DEPTH_SCALE)
            assert e.value.status == 1
            pyr = _builder(own, 1, sig).build(CameraIntrinsics(*E.builder_camera(3, 3), 3, 3), depth, rgb, E.DEPTH_SCALE)
            for lv, r in zip(pyr, _oracle_pyramid(depth, rgb, 3, 3, 1, sig)):
                _assert_same_level(lv, r, (3, 3, sig))
            _free([pyr])
    finally:
        own.close()
