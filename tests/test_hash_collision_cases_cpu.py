"""The cases of hash_collision_cases.py are what they claim, and a table that walked wrongly would show on them.

First half: home slots, table size, occupied set, chain length and wrap of every case, restated with the scalar hash and
the probe helpers of voxel_map_icp_restatement.py; the growth case collides in every table it passes through; the
lookups for absent neighbour cells cross long occupied blocks; and the restatements' outputs on the cases are not
degenerate.

Second half: a slot-level model of the table in plain Python (claim by linear probe in a given arrival order, lookup,
growth).  Under the stated rule the slot assignment depends on the arrival order and nothing visible does.  Each of four
wrong tables (no wrap past the last slot, a probe cap of 32 tries, a lookup that stops at the first foreign key, a growth
that copies slot for slot) loses a cell or finds one twice on at least one case: the GPU tests on these cases would
notice each of them."""
import numpy as np
import pytest

import cluster_restatement as CR
import hash_collision_cases as H
import normals_restatement as NR
import outlier_restatement as OR
import voxel_mean_restatement as VM
import voxel_restatement as V
from voxel_map_icp_restatement import occupied_slots, slot_hash


# ---- the construction claims ------------------------------------------------------------------------------------------------
def test_vectorised_hash_is_the_scalar_hash_on_cells_of_the_box():
    cells = np.random.default_rng(3).integers(-128, 128, size=(500, 3))
    keys = H.cell_keys(cells)
    assert H.slot_hash_u64(keys).tolist() == [slot_hash(k) for k in keys.tolist()]
    c = np.asarray([[-3, 7, 100]])
    assert int(H.cell_keys(c)[0]) == (-3 + (1 << 20)) << 42 | (7 + (1 << 20)) << 21 | (100 + (1 << 20))


@pytest.mark.parametrize("case", H.batch_cases(), ids=lambda c: c["name"])
def test_homes_table_size_and_chain(case):
    n, slots = len(case["points"]), case["slots"]
    assert slots == H.table_slots(n) == 1 << case["bits"] and 2 * n <= slots < 4 * n and n <= 4096
    homes = {slot_hash(int(k)) & (slots - 1) for k in H.cell_keys(case["chain_cells"]).tolist()}
    assert homes == set(case["homes"])
    chain = len(np.unique(case["chain_cells"], axis=0))
    assert chain == len(case["chain_cells"]) <= 1024
    keys = H.case_keys(case)
    longest, wraps = H.chain_length(keys, slots)
    assert longest >= chain and wraps
    print(f"{case['name']}: {n} rows, {len(keys)} cells, {slots} slots, {chain} colliding cells, longest run {longest}")
    if "occupied" in case:  # the whole table is the chain: the occupied set is known in closed form
        assert occupied_slots(keys, slots) == case["occupied"] and longest == chain == len(keys)
        assert occupied_slots(reversed(keys), slots) == case["occupied"]


@pytest.mark.parametrize("bits", H.CHAIN_BITS)
def test_one_chain_fills_half_the_table_from_its_home(bits):
    for last in (False, True):
        case = H.one_chain_half_full(bits, last)
        slots, count = 1 << bits, 1 << (bits - 1)
        home = slots - 1 if last else slots - 3
        assert len(case["points"]) == count and case["homes"] == (home,)
        tail = count - (slots - home)
        assert case["occupied"] == set(range(home, slots)) | set(range(tail)) and tail > 0


@pytest.mark.parametrize("bits", H.CONTENT_BITS)
def test_chain_with_content_layout(bits):
    case = H.chain_with_content(bits)
    C = (1 << bits) // 8
    assert len(case["chain_cells"]) == len(case["satellites"]) == C and case["homes"] == (case["slots"] - C // 2,)
    assert (np.abs(case["satellites"] - case["chain_cells"]).max(axis=1) == 1).all()
    cells, counts = np.unique(case["row_cells"], axis=0, return_counts=True)
    assert len(cells) == 2 * C
    by_cell = {tuple(c): k for c, k in zip(cells.tolist(), counts.tolist())}
    assert {by_cell[tuple(c)] for c in case["chain_cells"].tolist()} == {3, 4, 5}
    # an exact duplicate pair and a tie in the distance to the centre among the nearest rows of every colliding cell
    _, keys, dist = V.voxel_keys(case["points"], case["pitch"])
    for key in H.cell_keys(case["chain_cells"]).tolist():
        rows = np.flatnonzero(keys == key)
        nearest = rows[dist[rows] == dist[rows].min()]
        assert len(nearest) == 3 and len(np.unique(case["points"][nearest], axis=0)) == 2


def test_two_merging_chains_interleave():
    case = H.two_merging_chains()
    h = case["homes"][0]
    homes = [slot_hash(int(k)) & (case["slots"] - 1) for k in H.cell_keys(case["row_cells"]).tolist()]
    assert homes == [h, h + 1] * (len(homes) // 2) and h + len(homes) > case["slots"]


def test_growth_case_collides_in_every_table_and_doubles_with_every_filler():
    g = H.survives_growth()
    keys = H.cell_keys(g["chain_cells"]).tolist()
    assert len(set(keys)) == H.GROWTH_CELLS == 31
    for bits in range(6, 12):
        slots = 1 << bits
        homes = {slot_hash(k) & (slots - 1) for k in keys}
        assert homes == {H.GROWTH_HOME & (slots - 1)} and min(homes) + len(keys) > slots, bits  # one chain, and it wraps
        assert H.chain_length(keys, slots) == (31, True)
    slots = cells = 0
    seen = set()
    for frame, want in zip(g["frames"], g["slots"]):
        slots = H.map_slots(slots, cells, len(frame["points"]))
        seen.update(H.case_keys(frame))
        cells = len(seen)
        assert slots == want
    assert [len(f["points"]) for f in g["frames"]] == [31, 30, 60, 120, 240, 480, 16] and cells == 31 + 930
    # the colliding cells still form one run in the final table, the fillers around them
    assert H.chain_length(sorted(seen), 2048)[0] >= 31
    # the last frame is nearer to the centre in every other colliding cell; the box keeps exactly those cells
    first, last = g["frames"][0], g["frames"][6]
    assert np.array_equal(last["row_cells"], first["row_cells"][0::2])
    assert (V.voxel_keys(last["points"], H.PITCH)[2] < V.voxel_keys(first["points"], H.PITCH)[2][0::2]).all()
    lo, hi = g["box"]
    inside = ((first["points"] >= lo) & (first["points"] <= hi)).all(axis=1)
    assert inside.tolist() == [i % 2 == 0 for i in range(31)]
    p = H.merged_frames(g, 7)[0]
    inside = ((p >= lo) & (p <= hi)).all(axis=1)
    assert 300 < inside.sum() < len(p) - 300


def test_absent_neighbour_walks_are_long_and_wrap():
    long_walks = wrapping = 0
    for bits in H.CONTENT_BITS:
        case = H.chain_with_content(bits)
        C = (1 << bits) // 8
        walks = H.absent_walks(case)
        far = [w for w in walks if w[1] > C // 2]
        print(f"{case['name']}: {len(walks)} absent neighbour cells, {len(far)} walks over {C // 2} slots, "
              f"{sum(w[2] for w in far)} of them wrap, the longest {max(w[1] for w in walks)}")
        assert len(far) >= 50 and sum(w[2] for w in far) >= 10
        long_walks += len(far)
        wrapping += sum(w[2] for w in far)
    assert long_walks >= 200 and wrapping >= 20


@pytest.mark.parametrize("bits", H.CONTENT_BITS)
def test_restatements_are_not_degenerate_on_the_content_cases(bits):
    case = H.chain_with_content(bits)
    p, n, c = H.parts(case)
    r = case["pitch"]
    _, _, counts, valid = NR.estimate_normals(p, r, viewpoint=H.EYE)
    assert 50 < valid.sum() < len(p) and counts.max() > 8
    k_counts, qsum, stats = OR.knn_distance(p, r, 8)
    full = qsum != OR.NONE
    assert 10 < full.sum() < len(p) - 10 and stats[0] == full.sum()
    assert (OR.knn_distance(p, r, 1)[1] == OR.NONE).sum() > 0 and (OR.knn_distance(p, r, 17)[1] != OR.NONE).sum() == 0
    cl = CR.cluster(p, r, 3)
    assert len(cl.sizes) >= 2 and cl.noise.sum() > 0 and len(set(cl.sizes.tolist())) > 2
    assert len(CR.cluster(p, r, 1).sizes) > len(cl.sizes)
    mean = VM.voxel_mean(p, n, c, r)
    assert (mean[4] > 1).sum() >= len(case["chain_cells"]) and len(mean[3]) == 2 * len(case["chain_cells"])
    # the nearest-point winner of a colliding cell is decided among tied rows: by the index
    index, _ = V.voxel_downsample(p, r)
    _, keys, dist = V.voxel_keys(p, r)
    tied = sum(int((dist[keys == keys[i]] == dist[i]).sum() > 1) for i in index.tolist())
    assert tied >= len(case["chain_cells"])


# ---- a slot-level model of the table ------------------------------------------------------------------------------------------
class SlotTable:
    """An open-addressing table of `slots` slots as the kernels walk it: s = hash & mask; for (tries = 0; tries <= mask;
    ++tries, s = (s + 1) & mask).  wrap=False: the walk ends past the last slot.  cap: tries at the most.
    foreign_stop: a LOOKUP gives up at the first slot that holds another key."""

    def __init__(self, slots, wrap=True, cap=None, foreign_stop=False):
        self.slots, self.wrap, self.cap, self.foreign_stop = slots, wrap, cap, foreign_stop
        self.key = [None] * slots

    def _walk(self, key):
        s = slot_hash(key) & (self.slots - 1)
        for tries in range(self.slots if self.cap is None else min(self.cap, self.slots)):
            yield s
            if s == self.slots - 1 and not self.wrap:
                return
            s = (s + 1) & (self.slots - 1)

    def claim(self, key):
        """The slot the key has or takes; None: the walk ended without one (the kernels raise their fault word)."""
        for s in self._walk(key):
            if self.key[s] is None:
                self.key[s] = key
            if self.key[s] == key:
                return s
        return None

    def find(self, key):
        for s in self._walk(key):
            if self.key[s] == key:
                return s
            if self.key[s] is None or self.foreign_stop:
                return None
        return None

    def held(self):
        """The keys a pass over the slots sees (extract, rehash, rebuild), with repeats."""
        return sorted(k for k in self.key if k is not None)

    def grown(self, slots, copy=False):
        """The table of `slots` slots after a growth: every held key claims anew; copy=True: slot s goes to slot s."""
        new = SlotTable(slots, self.wrap, self.cap, self.foreign_stop)
        for s, k in enumerate(self.key):
            if k is not None:
                if copy:
                    new.key[s] = k
                else:
                    new.claim(k)
        return new


def visible(table, offered):
    """What a caller can see of a table that `offered` keys went into: (cells a pass over the slots finds, with repeats;
    the offered keys that a lookup finds)."""
    return table.held(), sorted(k for k in set(offered) if table.find(k) is not None)


def filled(keys, slots, **variant):
    table = SlotTable(slots, **variant)
    lost = [k for k in keys if table.claim(k) is None]
    return table, lost


def arrival_orders(keys):
    return {"ascending": sorted(keys), "descending": sorted(keys, reverse=True),
            "shuffled": [keys[i] for i in np.random.default_rng(23).permutation(len(keys))]}


def test_model_slot_assignment_depends_on_arrival_and_nothing_visible_does():
    case = H.two_merging_chains()
    keys = H.case_keys(case)
    layouts = []
    for name, order in arrival_orders(keys).items():
        table, lost = filled(order, case["slots"])
        assert not lost and visible(table, keys) == (sorted(keys), sorted(keys)), name
        assert {s for s, k in enumerate(table.key) if k is not None} == case["occupied"] == occupied_slots(order, case["slots"])
        layouts.append(tuple(table.key))
    assert len(set(layouts)) == 3
    for case in H.batch_cases():
        keys = H.case_keys(case)
        for name, order in arrival_orders(keys).items():
            table, lost = filled(order, case["slots"])
            assert not lost and visible(table, keys) == (sorted(keys), sorted(keys)), (case["name"], name)


def test_model_growth_keeps_every_cell_under_the_stated_rule():
    g = H.survives_growth()
    table, offered = None, []
    for frame, slots in zip(g["frames"], g["slots"]):
        keys = H.case_keys(frame)
        table = SlotTable(slots) if table is None else table if table.slots == slots else table.grown(slots)
        assert all(table.claim(k) is not None for k in keys)
        offered += keys
        assert visible(table, offered) == (sorted(set(offered)), sorted(set(offered)))


VARIANTS = {"no wrap past the last slot": {"wrap": False}, "a probe cap of 32 tries": {"cap": 32},
            "a lookup that stops at the first foreign key": {"foreign_stop": True}}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_wrong_walks_lose_cells(variant):
    caught = []
    for case in H.batch_cases():
        keys = H.case_keys(case)
        table, lost = filled(keys, case["slots"], **VARIANTS[variant])
        held, found = visible(table, keys)
        if lost or held != sorted(keys) or found != sorted(keys):
            caught.append(case["name"])
            assert len(held) < len(keys) or len(found) < len(keys)  # a cell is lost: to the passes over the slots or to lookups
    print(f"{variant}: caught by {caught}")
    assert caught
    if variant != "a probe cap of 32 tries":  # (a chain of 32 cells needs 32 tries at the most)
        assert len(caught) == len(H.batch_cases())
    assert "chain_with_content[10]" in caught and "one_chain_half_full[11]" in caught


def test_model_growth_by_slot_copy_loses_cells_and_finds_cells_twice():
    g = H.survives_growth()
    table, offered = None, []
    for frame, slots in zip(g["frames"], g["slots"]):
        keys = H.case_keys(frame)
        table = SlotTable(slots) if table is None else table if table.slots == slots else table.grown(slots, copy=True)
        for k in keys:
            table.claim(k)
        offered += keys
    held, found = visible(table, offered)
    cells = sorted(set(offered))
    chain = set(H.cell_keys(g["chain_cells"]).tolist())
    twice = {k for k in held if held.count(k) > 1}
    print(f"slot copy: {len(cells)} cells, a pass over the slots sees {len(held)}, {len(twice)} twice; lookups find {len(found)}")
    assert twice and twice <= chain                # the last frame's rows claimed a second slot for their cells
    assert len(found) < len(cells)                 # and lookups no longer reach cells that sit where the smaller table had them
