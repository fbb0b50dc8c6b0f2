"""Seeded inputs for the voxel-mean tests whose layout in the kernels is known on the host (no GPU needed to import).

voxel_mean.hip works on 64-lane waves, trips of 256 records and tiles of 1024 (VM_CHUNK) or 2048 records.  Random clouds
reach its branches by accident; these recipes reach them by construction, and tests/test_voxel_mean_cases_cpu.py states, in
numpy, which branch each recipe reaches.  The expected value of every GPU test on them is voxel_mean_restatement.voxel_mean.

uniform_runs    every cell holds exactly L points, so the records sorted by cell are K runs of L IN SOME ORDER and run j
                starts at j * L whatever order the hash table and the atomic cursor of pass 3 produce.
scanline        a tilted plane sampled row-major: the frame-cloud shape, runs of equal keys in INPUT order (passes 1, 4).
sorted_runs     an input fully sorted by cell with run lengths cycling through RUN_CYCLE.
edge_arithmetic small clouds at the edges of the rule's arithmetic."""
import numpy as np

VOXEL = 0.05
WAVE, TRIP, TILE = 64, 256, 1024
# (L, K): K cells of L points each.  K = 67 is odd and coprime to 64, so an odd L starts a run on every lane.
RUN_TABLE = tuple((L, 67) for L in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129)) + tuple((L, 5) for L in (1023, 1024, 1025))
DROP_EVERY = 7
RUN_CYCLE = (1, 2, 3, 5, 7, 62, 63, 64, 65, 130)
SCANLINE_SHAPES = ((83, 61), (29, 67))  # (W, H): wider than a wave, and a width that puts a row and the next in one wave
SCANLINE_PITCH = (0.011, 0.013)


def _unit_normals(rng, n):
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    return (normals / np.maximum(np.linalg.norm(normals, axis=1), np.float32(1e-6))[:, None]).astype(np.float32)


def _distinct_cells(rng, k, half=6):
    """[k, 3] distinct integer cells of [-half, half)^3, with both signs on every axis."""
    side = 2 * half
    while True:  # (drawn again until the signs are there: a few draws at the most for k >= 3)
        flat = rng.choice(side ** 3, size=k, replace=False)
        cells = np.stack([flat // (side * side), (flat // side) % side, flat % side], axis=1).astype(np.int64) - half
        if k < 3 or ((cells < 0).any(axis=0) & (cells >= 0).any(axis=0)).all():
            return cells


def uniform_runs(L, K, seed, drop_every=0):
    """(points [n, 3] f32, normals [n, 3] f32, colors [n, 3] u8): K distinct cells of the VOXEL grid with exactly L points
    each, 0.05 to 0.95 of the pitch inside the cell on every axis, the rows shuffled.  drop_every: a NaN row follows every
    drop_every rows (it is dropped: kept = K * L < len)."""
    rng = np.random.default_rng([seed, L, K])
    cells = np.repeat(_distinct_cells(rng, K), L, axis=0)
    points = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * VOXEL).astype(np.float32)
    points = points[rng.permutation(len(points))]
    if drop_every:
        at = np.arange(drop_every, len(points) + 1, drop_every)
        points = np.insert(points, at, np.float32(np.nan), axis=0)
    n = len(points)
    return points, _unit_normals(rng, n), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def scanline(W, H, seed=0, pitch=SCANLINE_PITCH, nan_every=0):
    """A tilted plane sampled row-major at `pitch` (about a fifth to a quarter of VOXEL), centred on the origin so that
    cells of both signs occur.  nan_every: every nan_every-th point (from index 5) is NaN, inside the runs of its row."""
    rng = np.random.default_rng([seed, W, H])
    i, j = np.meshgrid(np.arange(W), np.arange(H))  # [H, W]: row-major
    x = (i - W / 2.0) * pitch[0] + 0.003
    y = (j - H / 2.0) * pitch[1] + 0.002
    z = 0.11 * x - 0.07 * y + 0.012
    points = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    if nan_every:
        points[5::nan_every] = np.float32(np.nan)
    n = len(points)
    return points, _unit_normals(rng, n), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def sorted_runs(cycles=22, seed=0):
    """An input fully sorted by cell: distinct cells one after another, their sizes cycling through RUN_CYCLE (402 points
    a cycle; after 22 cycles a run has started and a run has ended on every lane)."""
    rng = np.random.default_rng([seed, cycles])
    sizes = np.tile(np.asarray(RUN_CYCLE), cycles)
    cells = np.repeat(_distinct_cells(rng, len(sizes)), sizes, axis=0)
    points = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * VOXEL).astype(np.float32)
    n = len(points)
    return points, _unit_normals(rng, n), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def few_cells(n, k, seed=0):
    """n points spread over k cells of the VOXEL grid in a shuffled order (pass 3: most slot shares are empty)."""
    rng = np.random.default_rng([seed, n, k])
    pick = rng.integers(0, k, size=n)
    pick[:k] = np.arange(k)  # every cell occurs
    cells = _distinct_cells(rng, k)[pick]
    points = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * VOXEL).astype(np.float32)
    return points, _unit_normals(rng, n), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def all_alone(n, seed=0):
    """n points, each alone in a cell of the VOXEL grid."""
    rng = np.random.default_rng([seed, n])
    cells = _distinct_cells(rng, n, half=8)
    points = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * VOXEL).astype(np.float32)
    return points, _unit_normals(rng, n), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def batch_recipe(n_jobs):
    """[(points, normals or None, colors or None)] for clouds 0 .. n_jobs - 1: recipe(n_jobs) of
    test_cloud_batch_recipe_cpu.py (every third non-empty cloud has no normals) with seeded colours on every second
    non-empty cloud.  Cloud i does not depend on n_jobs."""
    from test_cloud_batch_recipe_cpu import SEED, recipe

    out, ordinal = [], 0
    for i, (points, normals, _) in enumerate(recipe(n_jobs)):
        colors = np.random.default_rng([SEED + 2, i]).integers(0, 256, size=(len(points), 3), dtype=np.uint8)
        if len(points):
            ordinal += 1
        out.append((points, normals, colors if len(points) and ordinal % 2 == 0 else None))
    return out


# ---- what the kernels make of an input, restated on the host ------------------------------------------------------------

EMPTY_KEY = np.uint64(2**64 - 1)  # VX_EMPTY: a dropped point or a lane past the end


def wave_keys(points, voxel, origin=None):
    """([waves, 64] uint64: the key every lane of passes 1 and 4 holds, in input order; representative [n] bool)."""
    from voxel_restatement import voxel_keys

    kept, key, _ = voxel_keys(points, voxel, origin)
    k = np.concatenate([np.where(kept, key, EMPTY_KEY), np.full((-len(kept)) % WAVE, EMPTY_KEY)])
    rep = np.zeros(len(kept), bool)
    _, first = np.unique(key[kept], return_index=True)
    rep[np.flatnonzero(kept)[first]] = True
    return k.reshape(-1, WAVE), rep


def wave_runs(keys):
    """run_heads of voxel_mean.hip for one wave's [64] keys: [(first lane, one past the last lane, key)]."""
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return [(int(a), int(b), keys[a]) for a, b in zip(heads, np.append(heads[1:], WAVE))]


def slot_hash(k):
    """slot_hash of voxel_grid.hpp (the 64-bit finaliser of MurmurHash3) on a Python int."""
    m = (1 << 64) - 1
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & m
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & m
    return k ^ k >> 33


def occupied_slots(points, voxel, origin=None):
    """(sorted home slots of the cloud's cells, slots of the table, tiles of the cloud).  Asserts that no two cells hash
    to one slot, so that the linear probe, whose outcome depends on the order of arrival, plays no part and the home
    slots are the slots that pass 1 occupies."""
    from voxel_restatement import voxel_keys

    kept, key, _ = voxel_keys(points, voxel, origin)
    slots = 2
    while slots < 2 * len(kept):
        slots <<= 1
    chunks = (len(kept) + TILE - 1) // TILE
    per_tile = (chunks + 4095) // 4096
    used = sorted(slot_hash(int(k)) & (slots - 1) for k in np.unique(key[kept]))
    assert len(set(used)) == len(used)
    return used, slots, (chunks + per_tile - 1) // per_tile


# ---- the edges of the arithmetic ---------------------------------------------------------------------------------------

TIE_VOXEL = 0.25  # a power of two: centres, offsets and d * s are exact
TIE_KS = (0, 1, 2, 3, 6, 7, 100, 101, 16000, 16001, -1, -2, -3, -4, -7, -8, -101, -102, -16001, -16002)
TIE_CELLS = ((3, -2, 0), (-7, 5, 1), (0, 0, -1), (-1, -1, -1))


def _case(name, points, voxel, normals=None, colors=None, origin=None):
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(len(points))
    if normals is None:
        normals = _unit_normals(rng, len(points))
    if colors is None:
        colors = rng.integers(0, 256, size=(len(points), 3), dtype=np.uint8)
    return {"name": name, "points": points, "normals": np.ascontiguousarray(normals, np.float32).reshape(-1, 3),
            "colors": np.ascontiguousarray(colors, np.uint8).reshape(-1, 3), "voxel": float(voxel), "origin": origin}


def rint_ties():
    """Cells of N = 2 and N = 3 whose offsets are (k + 0.5) lattice steps: q = rintf(d * s) rounds every one of them to
    even.  Per cell the k of the three axes are neighbours in TIE_KS, so the sums differ from round-half-up."""
    v = np.float32(TIE_VOXEL)
    step = v / np.float32(32768.0)
    points, at = [], 0
    for cell_no in range(24):
        n = 2 + cell_no % 2
        cell = np.float32(TIE_CELLS[cell_no % len(TIE_CELLS)]) + np.float32([8 * (cell_no // len(TIE_CELLS)), 0, 0])
        ctr = (cell + np.float32(0.5)) * v
        for _ in range(n):
            k = np.float32([TIE_KS[(at + a) % len(TIE_KS)] for a in range(3)])
            points.append(ctr + (k + np.float32(0.5)) * step)
            at += 1
    return _case("rintf ties", np.asarray(points, np.float32), TIE_VOXEL)


def colour_halves_and_thirds():
    """The cells of test_colour_rounding_at_exact_halves, as one cloud of three cells (2, 4 and 3 rows)."""
    p = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]] + [[0.6, 0.1, 0.1]] * 4 + [[-0.1, 0.1, 0.1]] * 3)
    c = np.uint8([[0, 254, 10], [1, 255, 13], [0, 0, 255], [0, 1, 255], [1, 1, 255], [1, 0, 255], [0, 0, 0], [0, 0, 1], [1, 0, 1]])
    return _case("colour halves and thirds", p, 0.5, colors=c)


def cancelling_normals():
    """Cells of 2, 65 and 66 rows whose counted normals cancel (L == 0: a zero normal), a cell of 4 with two cancelling
    pairs, and cells where one counted normal shares the cell with uncounted ones (NaN, infinite, |n_k| > 2)."""
    rng = np.random.default_rng(11)
    a, b = np.float32([0.6, 0.0, 0.8]), np.float32([0.25, -0.5, 0.125])
    cells, normals = [], []

    def add(cell, rows):
        cells.extend([cell] * len(rows))
        normals.extend(rows)

    add((0, 0, 0), [a, -a])
    add((1, 0, 0), [a] * 32 + [-a] * 32 + [np.float32([0, 0, 0])])                 # 65 rows: crosses a wave
    add((-1, 0, 0), [b] * 33 + [-b] * 33)                                          # 66 rows
    add((0, -1, 0), [a, -a, b, -b])
    bad = [np.float32([np.nan, 0, 1]), np.float32([0, np.inf, 0]), np.float32([3.0, 0, 0]), np.float32([0, -2.5, 0])]
    add((0, 1, 0), [bad[0], np.float32([0, 0, 1]), bad[1], bad[2]])                # one counted: (0, 0, 1)
    add((0, 0, 1), bad + [np.float32([0, -2.0, 0])] + bad * 16)                    # 69 rows, one counted, |n_k| == 2 counts
    add((0, 0, -1), bad[:2])                                                       # none counted: zero
    cells = np.asarray(cells, np.float64)
    order = rng.permutation(len(cells))
    points = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * 0.5).astype(np.float32)
    return _case("cancelling normals", points[order], 0.5, normals=np.asarray(normals, np.float32)[order])


RANGE_LOW, RANGE_HIGH = -float(1 << 20), float((1 << 20) - 1)  # the first and the last cell of the key range at v = 1


def key_range_ends():
    """v = 1, origin 0: three points in each of the cells -2^20 and 2^20 - 1 on each axis in turn, and one point just
    outside each end (dropped and counted).  Near 2^20 an f32 has a spacing of 1/16 below and 1/8 above."""
    points = []
    for axis in range(3):
        for base, outside in ((RANGE_LOW, RANGE_LOW - 0.125), (RANGE_HIGH, RANGE_HIGH + 1.0)):
            for frac, other in ((0.25, 0.25), (0.5, 0.5), (0.8125, 0.75)):
                p = [other, other + 0.125, other - 0.0625]
                p[axis] = base + frac
                points.append(p)
            p = [0.5, 0.5, 0.5]
            p[axis] = outside
            points.append(p)
    return _case("key-range ends", np.asarray(points, np.float64), 1.0)


KEY_RANGE_OUTSIDE = 6


def cell_faces():
    """Points exactly on a cell face (p = c * v in f32) with points one ulp below it, on every axis, at a voxel that is
    a power of two (the face belongs to the upper cell) and at one that is not (the restatement decides)."""
    cases = []
    for v in (0.25, VOXEL):
        v32 = np.float32(v)
        points = []
        for c in (-5, -1, 0, 1, 3, 7):
            face = np.float32(c) * v32
            below = np.nextafter(face, np.float32(-np.inf))
            for axis in range(3):
                for value in (face, face, below, below, np.nextafter(below, np.float32(-np.inf))):
                    p = [np.float32(0.37) * v32 + np.float32(20 + c) * v32] * 3  # the other axes: inside a cell of their own
                    p[axis] = value
                    points.append(p)
        cases.append(_case(f"cell faces, v = {v}", np.asarray(points, np.float32), v))
    return cases


def edge_arithmetic():
    """[{name, points, normals, colors, voxel, origin}]: a few hundred points each at the most."""
    return [rint_ties(), colour_halves_and_thirds(), cancelling_normals(), key_range_ends(), *cell_faces()]
