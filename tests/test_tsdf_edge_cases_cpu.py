"""tsdf_edge_cases.py without a GPU: every case is what it claims to be, a scalar walk written here from the header's rule
agrees with the vectorised restatement on the layered fields, and every case changes under the slip it targets (a case
whose expectation survives its own variant would prove nothing on the device)."""
import numpy as np
import pytest

import tsdf_edge_cases as E
import tsdf_restatement as T
from align3d_amd import Transform

F = np.float32
ZERO, ONE = F(0), F(1)
FLUSH_BELOW = F(2.0 ** -126)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _volume(case, colors=True, max_weight=64, tau=None):
    vol = T.Volume(case["dims"], case["v"], case["origin"], case.get("tau", 1.0) if tau is None else tau, max_weight, colors)
    if "D" in case:
        vol.D, vol.W = case["D"].copy(), case["W"].copy()
        if colors:
            vol.C = case["C"].copy()
    return vol


def _inverse(pose):
    inv = Transform(*pose).inverse()
    return inv.t, inv.q


def _fuse(vol, frame, pose):
    return vol.integrate(frame["points"], frame["mask"], frame["colors"], frame["intrinsics"], _inverse(pose))


def _cast(vol, case, **over):
    a = dict(case, **over)
    return vol.raycast(a["intrinsics"], a["width"], a["height"], a.get("pose", E.EYE), a["z_near"], a["z_far"], a["step"])


def _same_volume(a, b):
    same = np.array_equal(_bits(a.D), _bits(b.D)) and np.array_equal(_bits(a.W), _bits(b.W))
    return same and (a.C is None or np.array_equal(a.C, b.C))


def _same_image(a, b):
    return (np.array_equal(a["mask"], b["mask"]) and np.array_equal(_bits(a["points"]), _bits(b["points"]))
            and np.array_equal(_bits(a["normals"]), _bits(b["normals"]))
            and (a["colors"] is None or np.array_equal(a["colors"], b["colors"])))


def half_even(x):
    """rintf: the rounding the rule does NOT use."""
    return np.round(np.asarray(x, F)).astype(F)


def flushed(D):
    """What a load that flushes denormals would see."""
    D = np.asarray(D, F)
    return np.where(np.abs(D) < FLUSH_BELOW, np.copysign(ZERO, D), D).astype(F)


# ---- the scalar walk: steps 1-5 and 7 of the raycast rule for one ray, no pose, np.float32 scalars -------------------------

def _lerp(a, b, t, other_form):
    if other_form:
        return F(F(a * F(ONE - t)) + F(b * t))
    return F(a + F(t * F(b - a)))


def _tri(case, D, g, strict_upper=False, ignore_weights=False, other_lerp=False):
    """Step 3: (valid, value)."""
    W = case["W"]
    lo, t = [], []
    for axis, n in enumerate(case["dims"]):
        f0 = F(np.floor(g[axis]))
        upper = F(f0 + ONE) < F(n - 1) if strict_upper else F(f0 + ONE) <= F(n - 1)
        if not (f0 >= ZERO and upper):  # (a NaN fails)
            return False, None
        lo.append(int(f0))
        t.append(F(g[axis] - f0))
    i, j, k = lo
    if not ignore_weights:
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    if not W[k + dk, j + dj, i + di] > ZERO:
                        return False, None
    c = [[_lerp(D[k + dk, j + dj, i], D[k + dk, j + dj, i + 1], t[0], other_lerp) for dj in (0, 1)] for dk in (0, 1)]
    return True, _lerp(_lerp(c[0][0], c[0][1], t[1], other_lerp), _lerp(c[1][0], c[1][1], t[1], other_lerp), t[2], other_lerp)


def scalar_walk(case, row, col, hit_strict=False, leave_strict=False, strict_upper=False, flush=False, nan_skipped=False,
                ignore_weights=False, other_lerp=False, rounding=T.round_half_away):
    """One ray of a case whose pose is the identity: {reason, started_behind, values, and on a hit s, z, point, g, color}."""
    fx, fy, cx, cy = (F(x) for x in case["intrinsics"])
    z_near, step, v = F(case["z_near"]), F(case["step"]), F(case["v"])
    origin = np.asarray(case["origin"], F)
    D = flushed(case["D"]) if flush else case["D"]
    xn, yn = F(F(F(col) - cx) / fx), F(F(F(row) - cy) / fy)  # step 1

    def g_of(z):
        p = (F(xn * z), F(yn * z), z)
        return [F(F(p[a] - origin[a]) / v) for a in range(3)]

    out = {"reason": T.RAN_OUT, "started_behind": False, "values": []}
    have_prev, D_prev, z_prev = False, ZERO, ZERO
    with np.errstate(all="ignore"):
        for k in range(E.samples(case["z_near"], case["z_far"], case["step"])):  # step 2
            z_k = F(z_near + F(F(k) * step))
            valid, value = _tri(case, D, g_of(z_k), strict_upper, ignore_weights, other_lerp)
            out["values"].append(value)
            if valid and nan_skipped and np.isnan(value):
                continue
            if not valid:  # step 4
                have_prev = False
                continue
            if not have_prev and value <= ZERO:
                out["started_behind"] = True
            if have_prev:
                behind_now = value < ZERO if hit_strict else value <= ZERO
                behind_then = D_prev < ZERO if leave_strict else D_prev <= ZERO
                if D_prev > ZERO and behind_now:
                    s = F(D_prev / F(D_prev - value))  # step 5
                    z = F(z_prev + F(F(z_k - z_prev) * s))
                    g = g_of(z)
                    at = [int(np.clip(rounding(g[a]), ZERO, F(n - 1))) for a, n in enumerate(case["dims"])]  # step 7
                    out.update(reason=T.HIT, s=s, z=z, point=np.asarray([F(xn * z), F(yn * z), z], F), g=g,
                               color=case["C"][at[2], at[1], at[0]])
                    return out
                if behind_then and value > ZERO:
                    out["reason"] = T.LEFT_FROM_BEHIND
                    return out
            have_prev, D_prev, z_prev = True, value, z_k
    return out


LAYERED = {case["name"]: case for case in E.layered_cases()}
CENTRE = E.LAYERED["centre"]


@pytest.fixture(scope="module")
def layered_images():
    return {name: _cast(_volume(case), case) for name, case in LAYERED.items()}


@pytest.mark.parametrize("name", sorted(LAYERED))
def test_the_scalar_walk_agrees_with_the_restatement(layered_images, name):
    case, image = LAYERED[name], layered_images[name]
    assert image["samples"] == (15 if case["step"] == 0.125 else 8)
    for row in range(5):
        for col in range(5):
            walk = scalar_walk(case, row, col)
            label = (name, row, col)
            assert walk["reason"] == image["reason"][row, col], label
            assert walk["started_behind"] == image["started_behind"][row, col], label
            assert (walk["reason"] == T.HIT) == (image["mask"][row, col] == 1), label
            if walk["reason"] == T.HIT:
                assert np.array_equal(_bits(walk["point"]), _bits(image["points"][row, col])), label
                assert np.array_equal(walk["color"], image["colors"][row, col]), label
            else:
                assert not _bits(image["points"][row, col]).any() and not image["colors"][row, col].any(), label


def test_layered_cases_are_what_they_claim(layered_images):
    walks = {name: scalar_walk(case, *CENTRE) for name, case in LAYERED.items()}
    # sample k of the centre ray sits on layer k with t == 0; sample 7 is at nz - 1 and invalid
    assert [float(x) for x in walks["exact zero"]["values"]] == [1.0, 0.5, 0.0]
    ran = scalar_walk(dict(LAYERED["exact zero"], D=np.ones((8, 5, 6), F)), *CENTRE)
    assert len(ran["values"]) == 8 and ran["values"][7] is None and ran["values"][6] is not None and ran["reason"] == T.RAN_OUT
    # the outer columns meet g.x == 0 (valid) and g.x == nx - 1 (invalid)
    flat = dict(LAYERED["exact zero"], D=np.ones((8, 5, 6), F))
    assert scalar_walk(flat, 2, 0)["values"][2] is not None and scalar_walk(flat, 2, 4)["values"][4] is None
    for name in ("exact zero", "minus zero"):
        w = walks[name]
        assert w["reason"] == T.HIT and w["s"] == 1.0 and w["z"] == 1.0 and not w["started_behind"], name
    assert np.signbit(LAYERED["minus zero"]["D"][2]).all() and not np.signbit(LAYERED["exact zero"]["D"][2]).any()
    assert _same_image(layered_images["exact zero"], layered_images["minus zero"])
    w = walks["zero first"]
    assert w["started_behind"] and w["reason"] == T.LEFT_FROM_BEHIND and len(w["values"]) == 2
    w = walks["nan swallows"]
    assert w["reason"] == T.LEFT_FROM_BEHIND and np.isnan(w["values"][1]) and len(w["values"]) == 5 and not w["started_behind"]
    assert layered_images["nan swallows"]["mask"].sum() == 0
    image = layered_images["hole"]
    seen = np.asarray([[any(v is not None for v in scalar_walk(LAYERED["hole"], r, c)["values"]) for c in range(5)] for r in range(5)])
    assert seen.sum() >= 9 and np.array_equal(image["started_behind"], seen) and image["mask"].sum() == 0
    assert all(v is None for v in walks["hole"]["values"][:4]) and walks["hole"]["values"][4] == -1.0
    w = walks["denormal pair"]
    assert w["reason"] == T.HIT and w["s"] == 0.5 and w["z"] == 0.875 and w["g"][2] == 1.5
    w = walks["huge"]
    values = np.asarray(w["values"][:8], F)
    assert np.isnan(values[[0, 2, 4]]).all() and np.isinf(values[[1, 3, 5]]).all() and w["reason"] != T.HIT
    assert layered_images["huge"]["mask"].sum() == 0
    for name in ("infinite", "infinite, half steps"):  # parity only: but no NaN may reach an output, bits could not be compared
        assert not np.isnan(layered_images[name]["points"]).any() and not np.isnan(layered_images[name]["normals"]).any()
    for name in ("denormal tie", "plain tie"):
        w = walks[name]
        assert w["reason"] == T.HIT and w["s"] == 0.5 and [float(x) for x in w["g"]] == [2.5, 2.5, 2.5], name
        assert w["color"].tolist() == LAYERED[name]["C"][3, 3, 3].tolist()
        n = layered_images[name]["normals"][CENTRE]
        assert n.tolist() == [0.0, 0.0, -1.0], name  # (all six samples valid, D falls with z alone)
    colours = E.field_colors((6, 5, 8)).reshape(-1, 3)
    assert len(np.unique(colours, axis=0)) == len(colours)
    for name, image in layered_images.items():  # without colours: the same image
        plain = _cast(_volume(LAYERED[name], colors=False), LAYERED[name])
        assert plain["colors"] is None and _same_image(dict(image, colors=None), plain), name


# the slip each layered case is there to catch: (case, the walk's flag)
SLIPS = (("exact zero", "hit_strict"), ("minus zero", "hit_strict"), ("zero first", "leave_strict"),
         ("nan swallows", "nan_skipped"), ("hole", "ignore_weights"), ("denormal pair", "flush"), ("denormal tie", "flush"),
         ("huge", "other_lerp"), ("exact zero", "strict_upper"))


def _outcome(walk):
    return (walk["reason"], walk["started_behind"], None if walk["reason"] != T.HIT else (_bits(walk["point"]).tolist(), walk["color"].tolist()))


@pytest.mark.parametrize("name,flag", SLIPS)
def test_layered_cases_change_under_their_slip(name, flag):
    case = LAYERED[name]
    pixels = [(r, c) for r in range(5) for c in range(5)] if flag == "strict_upper" else [CENTRE]
    assert any(_outcome(scalar_walk(case, r, c)) != _outcome(scalar_walk(case, r, c, **{flag: True})) for r, c in pixels)


def test_tie_cases_change_under_half_to_even(monkeypatch, layered_images):
    for name in ("denormal tie", "plain tie"):
        case = LAYERED[name]
        even = scalar_walk(case, *CENTRE, rounding=half_even)
        assert even["color"].tolist() == case["C"][2, 2, 2].tolist() != scalar_walk(case, *CENTRE)["color"].tolist()
    monkeypatch.setattr(T, "round_half_away", half_even)
    for name in ("denormal tie", "plain tie"):
        varied = _cast(_volume(LAYERED[name]), LAYERED[name])
        assert not np.array_equal(varied["colors"], layered_images[name]["colors"])
        assert _same_image(dict(varied, colors=None), dict(layered_images[name], colors=None))
    # the case as first written ties at 1.5: both roundings say 2
    first = scalar_walk(LAYERED["denormal pair"], *CENTRE, rounding=half_even)
    assert first["color"].tolist() == scalar_walk(LAYERED["denormal pair"], *CENTRE)["color"].tolist()


# ---- B ---------------------------------------------------------------------------------------------------------------------

def test_the_one_cell_volume():
    case = E.one_cell_case()
    vol = _volume(case)
    name, z_near, z_far, step = case["rays"][0]
    image = _cast(vol, case, z_near=z_near, z_far=z_far, step=step)
    assert image["mask"].sum() >= 6 and image["samples"] == 6
    assert not _bits(image["normals"]).any()  # +0 everywhere, hits included
    hit = image["mask"] == 1
    g = vol.voxel_coordinate(image["points"][hit], E.EYE)
    assert ((g >= 0) & (g < 1)).all()
    picks = T.round_half_away(g).astype(int)
    assert np.array_equal(image["colors"][hit], case["C"][picks[:, 2], picks[:, 1], picks[:, 0]]) and picks.min() == 0 and picks.max() == 1
    # a coordinate of exactly 1.0 is invalid: in x at z == 2 on the last column, in z on every ray
    for row in range(3):
        walk = scalar_walk(dict(case, z_near=z_near, z_far=z_far, step=step, D=np.ones((2, 2, 2), F)), row, 2)
        assert walk["values"][3] is not None and walk["values"][4] is None
    name, z_near, z_far, step = case["rays"][1]
    late = _cast(vol, case, z_near=z_near, z_far=z_far, step=step)
    assert late["mask"].sum() == 0 and (late["reason"] == T.RAN_OUT).all() and not late["started_behind"].any()
    walk = scalar_walk(dict(case, z_near=z_near, z_far=z_far, step=step), 0, 0)
    assert walk["values"][0] > 0 and walk["values"][1:] == [None, None]
    # i0 + 1 < n - 1 would leave no valid sample at all
    strict = scalar_walk(dict(case, z_near=1.0, z_far=2.25, step=0.25), 0, 0, strict_upper=True)
    assert all(v is None for v in strict["values"]) and scalar_walk(dict(case, z_near=1.0, z_far=2.25, step=0.25), 0, 0)["reason"] == T.HIT


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_the_sticks(axis):
    case = E.stick_case(axis)
    assert sorted(case["dims"]) == [2, 2, 1024] and case["dims"][axis] == 1024 and case["D"].size == 4096
    vol = _volume(case)
    for name, cam, pose, z_near, z_far, step in case["rays"]:
        image = vol.raycast(cam[:4], cam[4], cam[5], pose, z_near, z_far, step)
        hit = image["mask"] == 1
        assert hit.any(), name
        along = vol.voxel_coordinate(image["points"][hit], pose)[:, axis]
        if name == "along, upwards":
            assert hit.all() and along.max() < 100
        else:
            assert along.min() > 900, name  # the records at the volume's far end are the ones read
        if name == "across":
            assert hit.sum() >= 10 and along.max() > 1015
        assert not _bits(image["normals"]).any()  # two voxels across: g* +- e leaves the volume on some axis
    fused = _volume(dict(case, D=np.zeros_like(case["D"]), W=np.zeros_like(case["W"]), C=np.zeros_like(case["C"])), tau=case["tau"])
    for f, (frame, pose) in enumerate(zip(case["frames"], case["poses"])):
        assert _fuse(fused, frame, pose) > 150
        index = np.unravel_index(fused.last_pixels[0], fused.D.shape)[2 - axis]
        if f == 0:  # the stick's middle, then its far end
            assert 400 < index.min() and index.max() < 600 and index.max() - index.min() > 64, (axis, index.min(), index.max())
        else:
            assert index.min() > 900 and index.max() >= 1022, (axis, index.min(), index.max())


# ---- C ---------------------------------------------------------------------------------------------------------------------

def _weights_run(case, cap, D=None, colors=True):
    vol = _volume(case, colors=colors, max_weight=cap)
    if D is not None:
        vol.D = D.copy()
    after = []
    for frame, pose in zip(case["frames"], case["poses"]):
        assert _fuse(vol, frame, pose) == vol.D.size  # every voxel, both frames
        after.append(vol.copy())
    return after


def test_weights_at_the_cap_and_colours_in_range(monkeypatch):
    case = E.weight_case()
    assert set(case["W"].reshape(-1).tolist()) == set(float(w) for w in E.WEIGHTS)
    assert set(_bits(case["D"]).reshape(-1).tolist()) == set(_bits(F(E.DISTANCES)).tolist()) and len(set(E.DISTANCES)) == 11
    assert set(case["C"].reshape(-1).tolist()) == set(E.CHANNELS) == set(case["frames"][0]["colors"].reshape(-1).tolist())
    runs = {cap: _weights_run(case, cap) for cap in case["caps"]}
    for cap, (first, second) in runs.items():
        for vol in (first, second):
            assert 0.0 <= vol.color_range[0] and vol.color_range[1] <= 255.0  # the kernel's & 0xFF and numpy's cast agree
            assert not np.isnan(vol.D).any() and np.isinf(vol.D).any()       # D * W overflowed, and no NaN came of it
            assert (vol.W <= cap).all() and (vol.W == np.floor(vol.W)).all()
    first = runs[E.TOP][0]
    for j, w in enumerate(E.WEIGHTS):
        assert (first.W[:, j, :] == min(w + 1, E.TOP)).all(), w  # (2^24 + 1 is not an f32: W + 1 rounds back to 2^24)
    assert (first.W[:, 2, :] == E.TOP - 1).all() and (first.W[:, 3, :] == E.TOP).all() and (first.W[:, 4, :] == E.TOP).all()
    assert (runs[E.TOP][1].W[:, 2:5, :] == E.TOP).all()  # after the second frame: all three at 2^24, W + 1 no longer exact
    small = runs[E.SMALL_CAP][0]
    for j, w in enumerate(E.WEIGHTS):
        assert (small.W[:, j, :] == min(w + 1, E.SMALL_CAP)).all(), w  # an uploaded W above the cap drops to it
    # a kept denormal: layer 0 where the first frame's depth is exactly the voxel's
    tiny = np.abs(first.D[0]) < FLUSH_BELOW
    assert (tiny & (first.D[0] != 0)).any()
    # sensitivity: no cap; denormals flushed on load; half-to-even in the projection
    for got, want in zip(_weights_run(case, np.inf), runs[E.SMALL_CAP]):
        assert not _same_volume(got, want)
    for cap in case["caps"]:
        assert not np.array_equal(_bits(_weights_run(case, cap, D=flushed(case["D"]))[0].D), _bits(runs[cap][0].D))
    monkeypatch.setattr(T, "round_half_away", half_even)
    assert not _same_volume(_weights_run(case, E.TOP)[0], runs[E.TOP][0])


# ---- D ---------------------------------------------------------------------------------------------------------------------

def _as_if(frame, width=None, height=None, intrinsics=None):
    """What a kernel would read that took another frame's width, height or intrinsics with this frame's planes: pixel
    (row, col) is element row * width + col of each plane; past the planes' end it reads whatever lies there, here a kept
    pixel half a metre away."""
    w, h = width or frame["width"], height or frame["height"]

    def plane(a, channels):
        flat = a.reshape(-1, channels) if channels else a.reshape(-1)
        out = np.full((w * h,) + flat.shape[1:], 1 if a.dtype == np.uint8 and not channels else 0.5, a.dtype)
        n = min(len(flat), w * h)
        out[:n] = flat[:n]
        return out.reshape((h, w) + flat.shape[1:])

    return {"points": plane(frame["points"], 3), "mask": plane(frame["mask"], 0), "colors": plane(frame["colors"], 3),
            "intrinsics": intrinsics or frame["intrinsics"], "width": w, "height": h}


def _table_volume(colors=True, max_weight=64):
    dims, v, origin = E.TABLE_VOLUME
    return T.Volume(dims, v, origin, F(4) * F(v), max_weight, colors)


def test_the_mixed_call_depends_on_every_frames_own_fields():
    frames, poses = E.mixed_frames()
    assert {(f["width"], f["height"]) for f in frames} == {(24, 20), (65, 3), (1, 1), (300, 1)}
    want = _table_volume()
    touched = [_fuse(want, frame, pose) for frame, pose in zip(frames, poses)]
    assert all(t > 0 for t in touched), touched
    kinds = set()
    first = frames[0]
    for f in range(1, len(frames)):
        for kind in ("width", "height", "intrinsics"):
            if frames[f][kind] == first[kind]:
                continue
            kinds.add(kind)
            varied = _table_volume()
            for g, (frame, pose) in enumerate(zip(frames, poses)):
                _fuse(varied, _as_if(frame, **{kind: first[kind]}) if g == f else frame, pose)
            assert not _same_volume(varied, want), (f, kind)
    assert kinds == {"width", "height", "intrinsics"}


def test_the_chunk_calls():
    pool = E.chunk_pool()
    assert len(pool) == E.CHUNK_POOL
    for n in E.CHUNK_SIZES:
        picks, poses = E.chunk_call(n)
        assert len(picks) == len(poses) == n and set(picks) == set(range(E.CHUNK_POOL))
        assert n == 64 or picks[63] == picks[64]  # the same image on both sides of the cut

        def fused(skip=None):
            vol = _table_volume(max_weight=3)
            for f in range(n):
                if f != skip:
                    _fuse(vol, pool[picks[f]], poses[f])
            return vol

        want = fused()
        for f in sorted({63, 64, 127, 128, n - 1}):  # a call that lost a frame beside a cut, or its last one
            if f < n:
                assert not _same_volume(fused(skip=f), want), (n, f)


# ---- E ---------------------------------------------------------------------------------------------------------------------

def _model_image():
    dims, v, origin, tau = E.SCENE
    scene = T.Volume(dims, v, origin, tau, 64, True)
    for frame, pose in zip(E.scene_frames(), E.SCENE_POSES):
        _fuse(scene, frame, pose)
    fx, fy, cx, cy, w, h = E.MODEL_CAMERA
    pose, z_near, z_far, step = E.MODEL_RAY
    image = scene.raycast((fx, fy, cx, cy), w, h, pose, z_near, z_far, step)
    return {"points": image["points"], "mask": image["mask"], "colors": image["colors"], "intrinsics": (fx, fy, cx, cy),
            "width": w, "height": h}


def test_the_model_image_is_read_at_its_last_pixel(monkeypatch):
    image = _model_image()
    h, w = image["mask"].shape
    assert image["mask"][h - 1, w - 1] == 1 and image["mask"].sum() > 60 and image["colors"][h - 1, w - 1].any()
    dims, v, origin, tau = E.SECOND_VOLUME
    second = T.Volume(dims, v, origin, tau, 64, True)
    for pose in E.SECOND_POSES:
        assert _fuse(second, image, pose) > 100
        idx, row, col = second.last_pixels
        assert ((row == h - 1) & (col == w - 1)).any() and ((row == h - 1) & (col < w - 1)).any() and (col == w - 1).sum() > 3
    assert second.W.max() == 2.0
    monkeypatch.setattr(T, "round_half_away", half_even)  # the projection's rounding decides which pixel a voxel reads
    varied = T.Volume(dims, v, origin, tau, 64, True)
    for pose in E.SECOND_POSES:
        _fuse(varied, image, pose)
    assert not _same_volume(varied, second)


# ---- F ---------------------------------------------------------------------------------------------------------------------

def test_the_sample_counts():
    cases = {name: (z_near, z_far, step, K) for name, z_near, z_far, step, K in E.k_cases()}
    for name, (z_near, z_far, step, K) in cases.items():
        assert all(float(F(x)) == x or name == "a tenth" for x in (z_near, z_far, step)), name
        assert E.samples(z_near, z_far, step) == (4097 if K is None else K), name
    z_near, z_far, step, _ = cases["4096, the last sample is z_far"]
    assert (z_far - z_near) / step == 4095.0 and F(F(z_near) + F(F(4095) * F(step))) == F(z_far)
    z_near, z_far, step, _ = cases["4096, a quotient just below 4096"]
    assert 4095.999 < (z_far - z_near) / step < 4096.0 and float(np.nextafter(F(z_far), F(3))) == cases["4097"][1]
    z_near, z_far, step, _ = cases["7, a quotient just below 7"]
    assert 6.999999 < (z_far - z_near) / step < 7.0
    # the restatement's K is the f64 one, on the small cases and (run once, 4096 samples on six pixels) on the largest
    case = dict(E.LAYERED, intrinsics=E.K_CAMERA[:4], width=3, height=2)
    case["D"], case["W"], case["C"] = E.layered_field(E.K_PROFILE)
    vol = _volume(case)
    for name, (z_near, z_far, step, K) in cases.items():
        if K is None or (K == 4096 and "last" not in name):
            continue
        image = _cast(vol, case, z_near=z_near, z_far=z_far, step=step)
        assert image["samples"] == K, name
        if K == 4096:
            assert image["mask"].all() and (image["points"][..., 2] > 1.75).all()  # more than 3072 samples walked
        if K == 8:
            assert image["mask"].all()
        if K == 7:
            assert not image["mask"].any()  # (it ends on layer 5, one sample short of the crossing)
    for name, cam in E.SHAPE_CAMERAS.items():
        image = _volume(LAYERED["exact zero"]).raycast(cam[:4], cam[4], cam[5], E.EYE, 0.5, 2.25, 0.25)
        assert image["mask"].shape == (cam[5], cam[4]) and image["mask"].any(), name
