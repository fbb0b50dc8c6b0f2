"""Seeded clouds whose cells collide in the hash tables BY CONSTRUCTION (numpy only; no GPU needed to import).

Every open-addressing table of the library (voxel_downsample.hip, voxel_mean.hip, cell_sort.hpp, voxel_map.hip,
voxel_map_icp.hip) takes the slot of a cell from slot_hash of voxel_grid.hpp and walks on by one slot, wrapping at the
table's end, until it meets the key or an empty slot.  Random clouds at a load of one half at the most build such walks
by accident and short; the recipes here search a box of cells for keys with a chosen home slot and build long chains, chains
that run through the last slot, chains that merge, and a chain that stays a chain through every growth of the map.
tests/test_hash_collision_cases_cpu.py proves on the host that each case is what it claims.  The expected value of every
GPU test on them is one of the numpy restatements, which know nothing of slots.

The hash is voxel_map_icp_restatement.slot_hash (the one restatement of it that the probe helpers use); slot_hash_u64 is
its vectorised form and is held to it on import.

Geometry: the pitch is 2^-4 and every coordinate is (c + 0.5 + k / 1024) * 2^-4 with |k| <= 307, an exact f32 whose
quotient by the pitch is exact too, so floorf((p - 0) / v) is the intended cell; _case asserts it through
voxel_restatement.voxel_keys.  One pitch serves every entry: the voxel size of the downsamples and of the map, the radius
of normals, knn, the filters and the clustering (their grid has the radius as its pitch and the origin at 0)."""
import functools

import numpy as np

import voxel_restatement as V
from voxel_map_icp_restatement import DELTAS, LIM, absent_probe, occupied_slots, slot_hash

PITCH = 0.0625
OFFSET_STEPS = 1024   # offsets are multiples of 1 / 1024 of the pitch
OFFSET_MAX = 307      # below 0.3 pitches
HALF_FAST, HALF_WIDE = 64, 128  # the boxes of cells [-half, half)^3 that are searched: 0.05 s and 0.45 s, once each
RESIDUE_BITS = 12     # the low hash bits kept per cell of a box
CHAIN_BITS = (6, 9, 11)
CONTENT_BITS = (9, 10)
GROWTH_CELLS, GROWTH_BITS, GROWTH_HOME = 31, 11, (1 << 11) - 6   # low bits ...11111111010: near the end of every table
GROWTH_FILLERS = (30, 60, 120, 240, 480)                         # the table doubles with every one of them
GROWTH_SLOTS = (64, 128, 256, 512, 1024, 2048, 2048)             # after each of the seven frames
EYE = (0.5, -1.0, 4.0)  # the viewpoint of the normals


# ---- the hash, vectorised ------------------------------------------------------------------------------------------------
def cell_keys(cells):
    """[n] uint64 keys of [n, 3] integer cells: (c + 2^20) packed 21 bits per axis, as voxel_grid.hpp."""
    k = (np.asarray(cells, np.int64).reshape(-1, 3) + LIM).astype(np.uint64)
    return k[:, 0] << np.uint64(42) | k[:, 1] << np.uint64(21) | k[:, 2]


def slot_hash_u64(keys):
    """slot_hash on a uint64 array (products wrap modulo 2^64)."""
    k = np.array(keys, np.uint64)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def _hold_vectorised_hash_to_the_scalar_one():
    rng = np.random.default_rng(1)
    sample = np.concatenate([rng.integers(0, 1 << 63, size=61, dtype=np.uint64), np.uint64([0, 1, (1 << 63) - 1])])
    assert slot_hash_u64(sample).tolist() == [slot_hash(int(k)) for k in sample.tolist()]


_hold_vectorised_hash_to_the_scalar_one()


@functools.lru_cache(maxsize=None)
def _box_residues(half):
    """[(2 half)^3] uint16: the low RESIDUE_BITS hash bits of every cell of [-half, half)^3, x slowest, z fastest."""
    side = np.arange(-half, half, dtype=np.int64)
    yz = np.stack(np.meshgrid(side, side, indexing="ij"), axis=-1).reshape(-1, 2)
    out = np.empty((2 * half, len(yz)), np.uint16)
    cells = np.empty((len(yz), 3), np.int64)
    cells[:, 1:] = yz
    for i, x in enumerate(side):
        cells[:, 0] = x
        out[i] = (slot_hash_u64(cell_keys(cells)) & np.uint64((1 << RESIDUE_BITS) - 1)).astype(np.uint16)
    return out.reshape(-1)


def residue_cells(bits, home, half):
    """[m, 3] int64: every cell of [-half, half)^3 whose key has slot_hash(key) & (2^bits - 1) == home, in box order."""
    assert 0 < bits <= RESIDUE_BITS and 0 <= home < 1 << bits
    flat = np.flatnonzero((_box_residues(half) & np.uint16((1 << bits) - 1)) == home).astype(np.int64)
    side = 2 * half
    return np.stack([flat // (side * side), flat // side % side, flat % side], axis=1) - half


def colliding_cells(bits, home, count, half):
    """[count, 3] int64 distinct cells of [-half, half)^3 with home slot `home` in a table of 2^bits slots, spread evenly
    over the box's matches (both signs on every axis)."""
    found = residue_cells(bits, home, half)
    assert len(found) >= count, (bits, home, half, len(found), count)
    return found[np.linspace(0, len(found) - 1, count).astype(np.int64)]


def table_slots(length):
    """The slots of a batch entry's table for a cloud of `length` rows: the power of two at or above 2 * length."""
    slots = 2
    while slots < 2 * length:
        slots <<= 1
    return slots


def map_slots(slots, cells, incoming):
    """The slots of a map (reserve_cells = 0) that had `slots` (0: none yet) and `cells` when `incoming` points arrive."""
    need = 2 * (cells + incoming)
    if slots and slots >= need:
        return slots
    slots = 64
    while slots < need:
        slots <<= 1
    return slots


# ---- points -----------------------------------------------------------------------------------------------------------------
def _offsets(rng, n, lo=0, hi=OFFSET_MAX):
    """[n, 3] int64 offsets in steps, every |component| in [lo, hi], signs seeded."""
    return rng.integers(lo, hi + 1, size=(n, 3)) * rng.choice(np.asarray([-1, 1]), size=(n, 3))


def points_at(cells, steps):
    """[n, 3] f32: the points at `steps` / OFFSET_STEPS pitches from the centres of `cells` (exact)."""
    assert (np.abs(steps) <= OFFSET_MAX).all()
    exact = (np.asarray(cells, np.float64) + 0.5 + np.asarray(steps, np.float64) / OFFSET_STEPS) * PITCH
    out = exact.astype(np.float32)
    assert (out.astype(np.float64) == exact).all()
    return out


def _unit_normals(rng, n):
    normals = rng.normal(size=(n, 3))
    return (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)


def _case(name, cells, steps, rng, **known):
    """The case dict.  `cells` [n, 3]: the intended cell of every row; asserted."""
    points = points_at(cells, steps)
    kept, keys, _ = V.voxel_keys(points, PITCH)
    assert kept.all() and np.array_equal(keys.astype(np.uint64), cell_keys(cells)), name
    n = len(points)
    case = {"name": name, "points": points, "normals": _unit_normals(rng, n),
            "colors": rng.integers(0, 256, size=(n, 3), dtype=np.uint8), "pitch": PITCH, "row_cells": np.asarray(cells, np.int64),
            "slots": table_slots(n)}
    case.update(known)
    return case


def parts(case):
    return case["points"], case["normals"], case["colors"]


def permuted(case, seed=5):
    """(perm, (points, normals, colors) of the rows in the order perm): row j of the result is row perm[j] of the case."""
    perm = np.random.default_rng([seed, len(case["points"])]).permutation(len(case["points"]))
    return perm, tuple(np.ascontiguousarray(a[perm]) for a in parts(case))


def case_keys(case):
    """The distinct cell keys of the case, as Python ints in first-arrival order."""
    keys = cell_keys(case["row_cells"]).tolist()
    return list(dict.fromkeys(keys))


# ---- the cases --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_chain_half_full(bits, last=False):
    """2^(bits - 1) cells of one point each, all with home slot 2^bits - 3 (last: 2^bits - 1) of the 2^bits slots that a
    cloud of that length gets: whatever the arrival order they occupy home ... 2^bits - 1, 0 ... : one chain of half the
    table that wraps."""
    slots, count = 1 << bits, 1 << (bits - 1)
    home = slots - 1 if last else slots - 3
    rng = np.random.default_rng([11, bits, int(last)])
    cells = colliding_cells(bits, home, count, HALF_FAST if bits < 11 else HALF_WIDE)
    cells = cells[rng.permutation(count)]
    name = f"one_chain_half_full[{bits}{', last slot' if last else ''}]"
    case = _case(name, cells, _offsets(rng, count), rng, bits=bits, homes=(home,), chain_cells=cells,
                 occupied={(home + i) & (slots - 1) for i in range(count)})
    assert case["slots"] == slots
    return case


CONTENT_SIZES = (3, 4, 5, 4)         # rows of a colliding cell, in turn
SATELLITE_SIZES = (1, 2, 6, 1, 3, 2)  # rows of its satellite cell, in turn
FACES = [d for d in DELTAS.tolist() if sum(abs(x) for x in d) == 1]
OTHERS = [d for d in DELTAS.tolist() if sum(abs(x) for x in d) > 1]


@functools.lru_cache(maxsize=None)
def chain_with_content(bits):
    """C = 2^bits / 8 colliding cells with content.  Cell i holds CONTENT_SIZES[i % 4] rows: row 0 near the centre, row 1
    its exact duplicate, row 2 its mirror image through the centre (the same distance to the centre, another point), the
    others farther out; and it has one adjacent satellite cell (across a face for three in four, across an edge or a
    corner for the rest) of SATELLITE_SIZES[i % 6] rows pushed towards it, so that some lie within one pitch of the
    cell's rows and some do not.  The length, and with it the table, is fixed BEFORE the cells are chosen: 3 C + C rows
    would fill 2^bits slots to exactly one half with no room for a fourth row anywhere, so the sizes above give between
    2^(bits - 1) and 2^bits rows, a table of 2^(bits + 1) slots, and the home of the colliding cells is computed for
    THAT table: C / 2 slots before its end, so that the chain wraps in its middle.  The rows are shuffled."""
    C = (1 << bits) // 8
    sizes = [CONTENT_SIZES[i % len(CONTENT_SIZES)] for i in range(C)]
    sat_sizes = [SATELLITE_SIZES[i % len(SATELLITE_SIZES)] for i in range(C)]
    length = sum(sizes) + sum(sat_sizes)
    slots = table_slots(length)
    table_bits = slots.bit_length() - 1
    home = slots - C // 2
    rng = np.random.default_rng([13, bits])
    chain = colliding_cells(table_bits, home, C, HALF_FAST)
    taken = {tuple(c) for c in chain.tolist()}
    cells, steps, satellites = [], [], []
    for i, cell in enumerate(chain.tolist()):
        near = _offsets(rng, 1, 20, 100)[0]
        rows = [near, near, -near] + list(_offsets(rng, sizes[i] - 3, 150, OFFSET_MAX))
        cells += [cell] * sizes[i]
        steps += rows
        pool = FACES if i % 4 else OTHERS
        for turn in range(len(pool)):
            delta = pool[(i + turn) % len(pool)]
            sat = tuple(a + b for a, b in zip(cell, delta))
            if sat not in taken:
                break
        else:
            raise AssertionError("no free neighbour cell")
        taken.add(sat)
        satellites.append(sat)
        cells += [list(sat)] * sat_sizes[i]
        steps += list(-np.asarray(delta) * rng.integers(0, 300, size=(sat_sizes[i], 1)) + _offsets(rng, sat_sizes[i], 0, 7))
    order = rng.permutation(length)
    case = _case(f"chain_with_content[{bits}]", np.asarray(cells, np.int64)[order], np.asarray(steps, np.int64)[order], rng,
                 bits=table_bits, homes=(home,), chain_cells=chain, satellites=np.asarray(satellites, np.int64))
    assert case["slots"] == slots and len(case["points"]) == length
    return case


@functools.lru_cache(maxsize=None)
def two_merging_chains(per_chain=24):
    """per_chain cells with home h and per_chain with home h + 1, one row each, interleaved in row order, h ten slots
    before the end of the table: which key sits in which slot depends on the order of arrival."""
    n = 2 * per_chain
    slots = table_slots(n)
    bits, h = slots.bit_length() - 1, slots - 10
    a, b = colliding_cells(bits, h, per_chain, HALF_FAST), colliding_cells(bits, h + 1, per_chain, HALF_FAST)
    cells = np.empty((n, 3), np.int64)
    cells[0::2], cells[1::2] = a, b
    rng = np.random.default_rng([17, per_chain])
    return _case("two_merging_chains", cells, _offsets(rng, n), rng, bits=bits, homes=(h, h + 1), chain_cells=cells,
                 occupied={(h + i) & (slots - 1) for i in range(n)})


@functools.lru_cache(maxsize=None)
def survives_growth():
    """Seven frames for a map.  Frame 0: GROWTH_CELLS cells, one row each, whose hashes agree in the low GROWTH_BITS bits
    (GROWTH_HOME): one chain through the last slot in EVERY table from 64 to 2048 slots.  Even rows lie at x >= 0, odd rows
    at x < 0, so the half space x >= 0 keeps every other one.  Frames 1 to 5: filler clouds of distinct other cells, sized
    so that the table doubles with each.  Frame 6: a point nearer to the centre for every colliding cell at an even row
    (no growth).  Returns {"frames": [case dicts], "slots": GROWTH_SLOTS, "box": the retain box, "chain_cells"}."""
    found = residue_cells(GROWTH_BITS, GROWTH_HOME, HALF_FAST)
    right, left = found[found[:, 0] >= 0], found[found[:, 0] < 0]
    n_right = (GROWTH_CELLS + 1) // 2
    chain = np.empty((GROWTH_CELLS, 3), np.int64)
    chain[0::2] = right[np.linspace(0, len(right) - 1, n_right).astype(np.int64)]
    chain[1::2] = left[np.linspace(0, len(left) - 1, GROWTH_CELLS - n_right).astype(np.int64)]
    rng = np.random.default_rng([19])
    frames = [_case("survives_growth, frame 0", chain, _offsets(rng, GROWTH_CELLS, 150, OFFSET_MAX), rng)]
    side = 2 * HALF_FAST
    taken = {tuple(c) for c in chain.tolist()}
    flat = rng.choice(side ** 3, size=sum(GROWTH_FILLERS) + GROWTH_CELLS, replace=False)
    pool = np.stack([flat // (side * side), flat // side % side, flat % side], axis=1).astype(np.int64) - HALF_FAST
    pool = np.asarray([c for c in pool.tolist() if tuple(c) not in taken], np.int64)
    at = 0
    for k, n in enumerate(GROWTH_FILLERS):
        frames.append(_case(f"survives_growth, frame {k + 1}", pool[at:at + n], _offsets(rng, n), rng))
        at += n
    frames.append(_case("survives_growth, frame 6", chain[0::2], _offsets(rng, n_right, 0, 60), rng))
    big = np.float32(100.0)
    return {"name": "survives_growth", "frames": frames, "slots": GROWTH_SLOTS, "chain_cells": chain, "pitch": PITCH,
            "box": (np.float32([0.0, -big, -big]), np.float32([big, big, big]))}


def merged_frames(growth, upto):
    """(points, normals, colors) of frames 0 ... upto - 1 back to back: what the map holds after they went in."""
    return tuple(np.concatenate([f[k] for f in growth["frames"][:upto]]) for k in ("points", "normals", "colors"))


@functools.lru_cache(maxsize=None)
def growth_as_one_cloud():
    """The seven frames of survives_growth as one cloud for the batch entries: 977 rows in a table of 2048 slots, the
    31-cell chain through its last slot, 16 of those cells with two rows."""
    g = survives_growth()
    p, n, c = merged_frames(g, len(g["frames"]))
    case = {"name": "survives_growth, one cloud", "points": p, "normals": n, "colors": c, "pitch": PITCH,
            "row_cells": np.concatenate([f["row_cells"] for f in g["frames"]]), "slots": table_slots(len(p)),
            "bits": GROWTH_BITS, "homes": (GROWTH_HOME,), "chain_cells": g["chain_cells"]}
    assert case["slots"] == 1 << GROWTH_BITS
    return case


# ---- what is known of the walks -----------------------------------------------------------------------------------------------
def absent_walks(case):
    """[(key, slots looked at, wrapped)] for every neighbour cell (the 27 offsets around every cell of the case) that
    the table of the case does not hold: the walks of the lookups that must cross occupied slots to the first empty one."""
    keys = case_keys(case)
    held, slots = set(keys), case["slots"]
    occupied = occupied_slots(keys, slots)
    cells = np.unique(case["row_cells"], axis=0)
    asked = set()
    for delta in DELTAS:
        asked.update(cell_keys(cells + delta).tolist())
    return [(k,) + absent_probe(k, occupied, slots) for k in sorted(asked - held)]


def chain_length(keys, slots):
    """The longest run of occupied slots (cyclic) of a table of `slots` slots that holds `keys`, and whether a run passes
    from the last slot to slot 0."""
    occupied = occupied_slots(keys, slots)
    assert len(occupied) < slots
    longest = run = 0
    start = next(s for s in range(slots) if s not in occupied)
    for step in range(1, slots + 1):
        s = (start + step) & (slots - 1)
        run = run + 1 if s in occupied else 0
        longest = max(longest, run)
    return longest, (slots - 1 in occupied and 0 in occupied)


def batch_cases():
    """The clouds that every batch entry runs on."""
    out = [one_chain_half_full(b) for b in CHAIN_BITS] + [one_chain_half_full(b, True) for b in CHAIN_BITS]
    return out + [chain_with_content(b) for b in CONTENT_BITS] + [two_merging_chains(), growth_as_one_cloud()]
