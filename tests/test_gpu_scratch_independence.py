"""No result depends on what the context's scratch regions, pooled image arenas or spare blocks held before the call.

Every batched operation works in a grow-only scratch region that other operations, and larger inputs of its own, have
used before it, and clears only what it believes it must ("Who clears what").  A read of a word the
call never wrote goes unnoticed as long as fresh device memory is zero and the suite runs in one order.  Here every case
of scratch_cases.py runs on a context of its own (both builds of the library) whose idle memory
a3d_selftest_fill_scratch has filled:

 (a) over zeros, S must be the numpy restatement bit for bit: the anchor, so that "equally wrong every time" cannot pass;
 (b) over 0xFF (VX_EMPTY, RD_EMPTY, CO_NONE, NaN: "empty" for half the tables, poison for the rest) and over 0x5A (a finite
     positive float, a 63-bit key with the top bit clear: a cell that looks alive), S must be (a) bit for bit;
 (c) L, S, L, S with nothing in between: both S are (a), the second L is the first;
 (d) for every other case that shares a scratch region: its L, then this S, is (a);
 (e) cases that take pooled arenas or spare blocks: run, free, fill, run again is (a).

A case whose declared region was never allocated has tested nothing and fails."""
import pytest

import scratch_cases as SC

pytestmark = pytest.mark.gpu

POISON = (0xFF, 0x5A)
NAMES = list(SC.CASES)
PAIRS = [(name, other) for name in NAMES for other in SC.sharing(name)]


@pytest.fixture(scope="module", params=["product", "diagnostics"])
def own(request):
    """A context of this module's own (never the session's: its gigabytes of scratch are not ours to fill), and the (a)
    results it has produced so far."""
    from align3d_amd import Context, _abi

    c = Context(0, library=_abi.DIAG_LIB_PATH if request.param == "diagnostics" else None)
    yield c, {}
    c.close()


def _anchor(own, name):
    """(a): S over zeros, equal to the independent reference; computed once per context and case."""
    ctx, done = own
    if name not in done:
        SC.CASES[name].run(ctx, "S")  # (the regions exist from here on)
        ctx.selftest_fill_scratch(0x00)
        got = SC.CASES[name].run(ctx, "S")
        bad = SC.mismatches(got, SC.reference(name), computed_nans=name in SC.COMPUTED_NANS,
                            poses=SC.POSES.get(name, ()))
        assert not bad, (name, SC.CASES[name].reference_name, bad)
        done[name] = got
    return done[name]


def _fill(ctx, name, byte):
    filled = ctx.selftest_fill_scratch(byte)
    for region in SC.CASES[name].regions:
        assert filled[region] > 0, f"{name} declares region {region} but nothing of it was there to fill: {filled}"
    return filled


@pytest.mark.parametrize("name", NAMES)
def test_reference_parity_over_zeros(own, name):
    _anchor(own, name)


@pytest.mark.parametrize("byte", POISON)
@pytest.mark.parametrize("name", NAMES)
def test_poisoned_memory(own, name, byte):
    ctx, _ = own
    want = _anchor(own, name)
    print(name, hex(byte), "filled:", _fill(ctx, name, byte))
    got = SC.CASES[name].run(ctx, "S")
    assert not SC.mismatches(got, want), (name, hex(byte), SC.mismatches(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_own_leftovers(own, name):
    ctx, _ = own
    want = _anchor(own, name)
    run = SC.CASES[name].run
    large = run(ctx, "L")
    assert not SC.mismatches(run(ctx, "S"), want), (name, "S after L")
    assert not SC.mismatches(run(ctx, "L"), large), (name, "L after S")
    assert not SC.mismatches(run(ctx, "S"), want), (name, "S after L, S, L")


@pytest.mark.parametrize("name,other", PAIRS)
def test_other_layouts_leftovers(own, name, other):
    ctx, _ = own
    want = _anchor(own, name)
    SC.CASES[other].run(ctx, "L")
    got = SC.CASES[name].run(ctx, "S")
    assert not SC.mismatches(got, want), (name, "after", other, SC.mismatches(got, want))


@pytest.mark.parametrize("byte", POISON)
@pytest.mark.parametrize("name", list(SC.POOLED))
def test_pooled_arenas_and_spare_blocks(own, name, byte):
    """The run frees every image and map it made; what they held is then idle in the pool, is filled, and is handed out
    again to the next run."""
    ctx, _ = own
    want = _anchor(own, name)
    SC.CASES[name].run(ctx, "S")
    filled = _fill(ctx, name, byte)
    for kind in SC.POOLED[name]:
        assert filled[kind] > 0, (name, kind, filled)
    got = SC.CASES[name].run(ctx, "S")
    assert not SC.mismatches(got, want), (name, hex(byte), SC.mismatches(got, want))


@pytest.mark.parametrize("mode", ["sync", "unfused"])
def test_lone_filter_path_grows_its_region_inside_the_call(monkeypatch, mode):
    """bilateral_filter_device (images of 2^24 pixels or more; here through the diagnostics build's A3D_BILATERAL knob) asks
    for its three scalar words first and for the grids once their size is known: the region grows INSIDE the call, after
    the overflow flag was uploaded into the old one.  On a context of its own the first call grows a region that does not
    exist yet, the larger image grows it again over poison, and the small one then runs inside the poisoned larger region:
    each result is the oracle's, and no call reports a cast overflow from a flag word it never wrote."""
    from align3d_amd import BilateralFilter, Context, _abi

    monkeypatch.setenv("A3D_BILATERAL", mode)
    ctx = Context(0, library=_abi.DIAG_LIB_PATH)
    try:
        f = BilateralFilter.default()
        small, large = SC.depth_images("S")[0][0], SC.depth_images("L")[0][0]
        want_small, want_large = SC.reference("bilateral_host")["host0"], SC.CASES["bilateral_host"].reference("L")["host0"]
        assert (f.filter(ctx, small) == want_small).all()
        for byte in POISON:
            assert ctx.selftest_fill_scratch(byte)[1] > 0
            assert (f.filter(ctx, large) == want_large).all(), (mode, hex(byte), "large")
            assert ctx.selftest_fill_scratch(byte)[1] > 0
            assert (f.filter(ctx, small) == want_small).all(), (mode, hex(byte), "small")
    finally:
        ctx.close()
