"""The recipes of voxel_mean_cases.py and the conditions they have to meet, checked without a GPU.

test_gpu_voxel_mean_layout.py and test_gpu_voxel_mean_many_jobs.py send these inputs through voxel_mean.hip and compare
with the restatement.  The tests below say which branch of the kernels each input reaches: a recipe changed so that it no
longer reaches one fails here.  Positions are counted as the kernels count them: a wave is 64 consecutive positions from a
multiple of 64, a block trip 256, a tile 1024 (VM_CHUNK) times the chunks per tile.

  passes 1 and 4 work on the INPUT order: wave_keys / wave_runs restate run_heads, run_first_lane and run_end_lane;
  passes 5 and 6 work on the records SORTED by cell: with L points in every cell, run j is [j * L, (j + 1) * L) whatever
  order pass 3 gives the cells;
  pass 3 works on the slots of the hash table: slot_hash is restated in voxel_mean_cases.py."""
import numpy as np

import voxel_mean_cases as K
import voxel_mean_restatement as M
import voxel_restatement as V
from test_cloud_batch_recipe_cpu import BATCHES, MAX_TILES, TILE_VOXEL, VOXEL, batch_lengths, is_raw, plan

WAVE, TRIP, TILE = K.WAVE, K.TRIP, K.TILE
SINGLED_OUT = (0, 63, 64, 65, 70)  # and n - 1


def _run_kinds(L, k):
    """The kinds of run among the k runs [j * L, (j + 1) * L) of the sorted records, as pass 5 tells them apart."""
    kinds = set()
    for j in range(k):
        a, b = j * L, (j + 1) * L - 1  # first and last position
        if a // WAVE == b // WAVE:
            kinds.add("inside one wave")
        if b % WAVE == WAVE - 1:
            kinds.add("ends on lane 63")
        if a % WAVE == 0 and a > 0:
            kinds.add("starts on lane 0 right after another")
        if a % WAVE == WAVE - 1 and L > 1:
            kinds.add("starts on lane 63")
        first_whole = (a + WAVE - 1) // WAVE + (1 if a % WAVE == 0 else 0)  # the first wave the run enters at lane 0
        if first_whole * WAVE + WAVE - 1 < b:
            kinds.add("covers a whole wave in its middle")  # from_before && open_right
        if a // TRIP != b // TRIP:
            kinds.add("crosses a block trip")
        if a // TILE != b // TILE:
            kinds.add("crosses a tile")  # two blocks add to one accumulator
    return kinds


def test_run_table_is_the_one_that_was_tried():
    assert {L for L, k in K.RUN_TABLE if k == 67} >= {2, 31, 32, 33, 63, 64, 65, 127, 128, 129}
    assert {L for L, k in K.RUN_TABLE if k == 5} >= {1023, 1024, 1025}
    assert max(L * k for L, k in K.RUN_TABLE) <= 10000


def test_uniform_runs_every_cell_holds_exactly_l_points_on_both_sides_of_zero():
    for L, k in K.RUN_TABLE:
        for drop_every in (0, K.DROP_EVERY):
            points, normals, colors = K.uniform_runs(L, k, 1, drop_every)
            kept, key, _ = V.voxel_keys(points, K.VOXEL)
            cells, counts = np.unique(key[kept], return_counts=True)
            assert len(cells) == k and (counts == L).all(), (L, k)
            assert kept.sum() == L * k and len(points) == L * k + (L * k // drop_every if drop_every else 0)
            c = np.floor(points[kept] / np.float32(K.VOXEL))
            assert ((c < 0).any(axis=0) & (c >= 0).any(axis=0)).all(), (L, k)  # negative and positive cell indices on every axis
            frac = points[kept].astype(np.float64) / K.VOXEL - c
            assert frac.min() > 0.04 and frac.max() < 0.96  # strictly inside: no point near a face
            assert normals.shape == points.shape and colors.shape == points.shape and colors.dtype == np.uint8
            again = K.uniform_runs(L, k, 1, drop_every)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((points, normals, colors), again))
            if L > 1:  # shuffled: the rows of a cell are not neighbours
                assert (key[kept][1:] != key[kept][:-1]).mean() > 0.5 or k == 5


def test_uniform_runs_start_lanes_and_kinds_of_run_in_the_sorted_records():
    seen = set()
    for L, k in K.RUN_TABLE:
        lanes = {(j * L) % WAVE for j in range(k)}
        kinds = _run_kinds(L, k)
        seen |= kinds
        if L % 2 == 1 and k == 67:
            assert lanes == set(range(WAVE)), L  # a run starts on every lane
        if L in (64, 128, 1024):  # always aligned: a run starts on lane 0 and ends on lane 63
            assert lanes == {0} and {((j + 1) * L - 1) % WAVE for j in range(k)} == {WAVE - 1}
        if L == 64:
            assert kinds == {"inside one wave", "ends on lane 63", "starts on lane 0 right after another"}
        if L == 32:  # never crosses a wave
            assert lanes == {0, 32} and "covers a whole wave in its middle" not in kinds and "crosses a block trip" not in kinds
        if L >= 129:
            assert "covers a whole wave in its middle" in kinds, L
        if L in (1023, 1025):
            assert "crosses a tile" in kinds and "crosses a block trip" in kinds, L
        print(f"L = {L}, K = {k}: {len(lanes)} start lanes; {sorted(kinds)}")
    assert seen == {"inside one wave", "ends on lane 63", "starts on lane 0 right after another", "starts on lane 63",
                    "covers a whole wave in its middle", "crosses a block trip", "crosses a tile"}


def test_uniform_runs_with_dropped_rows_end_inside_a_wave_and_leave_tiles_behind_kept():
    ragged, behind = 0, 0
    for L, k in K.RUN_TABLE:
        points, _, _ = K.uniform_runs(L, k, 1, K.DROP_EVERY)
        kept = int(V.voxel_keys(points, K.VOXEL)[0].sum())
        assert kept == L * k < len(points)  # kept < len
        if L not in (64, 128, 1024):
            assert kept % WAVE != 0, L  # the last wave of pass 5 has dead lanes, and len gives no hint of where
            ragged += 1
        tiles = (len(points) + TILE - 1) // TILE
        behind += (tiles - 1) * TILE >= kept  # the last tile lies wholly behind kept
        # a dropped row splits the input: it sits between two kept rows of one wave
        waves, _ = K.wave_keys(points, K.VOXEL)
        assert any(a > 0 and b < WAVE and key == K.EMPTY_KEY for w in waves[:4] for a, b, key in K.wave_runs(w))
    assert ragged >= 10 and behind >= 3


def _input_order_facts(points, voxel):
    """What passes 1 and 4 meet in a cloud, from the restated run_heads."""
    waves, rep = K.wave_keys(points, voxel)
    rep = np.concatenate([rep, np.zeros(waves.size - len(rep), bool)]).reshape(-1, WAVE)
    facts = {"lengths": set(), "one key in two runs": 0, "run without its representative": 0, "dropped inside a run": 0,
             "representative leads others": 0, "waves that begin inside a run": 0,
             "dead lanes": int((-len(points)) % WAVE), "start lanes": set(), "end lanes": set()}
    for w, (keys, reps) in enumerate(zip(waves, rep)):
        runs = K.wave_runs(keys)
        live = [(a, b, key) for a, b, key in runs if key != K.EMPTY_KEY]
        for a, b, key in live:
            facts["lengths"].add(b - a)
            facts["start lanes"].add(a)
            facts["end lanes"].add(b - 1)
            if not reps[a:b].any():
                facts["run without its representative"] += 1  # others == run_mask
            else:  # the lowest index of a cell leads every run it is in: `others` is the run without its first lane
                assert reps[a] and reps[a:b].sum() == 1
                facts["representative leads others"] += b - a > 1
        keys_of = [key for _, _, key in live]
        facts["one key in two runs"] += len(keys_of) != len(set(keys_of))
        for (a0, b0, k0), (a1, b1, k1), (a2, b2, k2) in zip(runs, runs[1:], runs[2:]):
            facts["dropped inside a run"] += k1 == K.EMPTY_KEY and k0 == k2 != K.EMPTY_KEY
        if w and keys[0] != K.EMPTY_KEY and keys[0] == waves[w - 1][WAVE - 1]:
            facts["waves that begin inside a run"] += 1
    return facts


def test_scanline_and_sorted_inputs_reach_the_run_arithmetic_of_passes_1_and_4():
    wide = _input_order_facts(K.scanline(*K.SCANLINE_SHAPES[0])[0], K.VOXEL)
    narrow = _input_order_facts(K.scanline(*K.SCANLINE_SHAPES[1])[0], K.VOXEL)
    split = [_input_order_facts(K.scanline(w, h, nan_every=11)[0], K.VOXEL) for w, h in K.SCANLINE_SHAPES]
    ordered = _input_order_facts(K.sorted_runs()[0], K.VOXEL)
    for name, f in (("wide", wide), ("narrow", narrow), ("split", split[0]), ("split, narrow", split[1]), ("sorted", ordered)):
        print(name, {k: (sorted(v) if isinstance(v, set) and len(v) < 12 else len(v) if isinstance(v, set) else v)
                     for k, v in f.items()})
    # the frame-cloud shape: short runs, most waves begin inside one
    assert {2, 3, 4, 5} <= wide["lengths"] and {2, 3, 4, 5} <= narrow["lengths"]
    assert wide["waves that begin inside a run"] > 40
    # W = 83 > 64: no wave holds a key twice; W = 29 puts a row and the next row into one wave
    assert wide["one key in two runs"] == 0 and narrow["one key in two runs"] > 10
    for f in (wide, narrow, ordered):
        assert f["run without its representative"] > 0 and f["representative leads others"] > 0
        assert f["dead lanes"] > 0  # the trailing run of dead lanes
    assert all(f["dropped inside a run"] > 10 and f["dead lanes"] > 0 for f in split)
    # sorted by cell: runs of 63 and 64 and the pieces of 65 and 130, starting and ending on every lane
    assert {1, 2, 3, 5, 7, 62, 63, 64} <= ordered["lengths"]
    assert ordered["start lanes"] == set(range(WAVE)) and ordered["end lanes"] == set(range(WAVE))
    points = K.sorted_runs()[0]
    counts = M.voxel_mean(points, None, None, K.VOXEL)[4]
    assert counts.tolist() == list(K.RUN_CYCLE) * (len(counts) // len(K.RUN_CYCLE))  # first-occurrence order IS the input order
    starts = np.cumsum(np.concatenate([[0], counts[:-1]]))
    assert ((starts // TRIP != (starts + counts - 1) // TRIP) & (counts > 1)).any()
    assert ((starts // TILE != (starts + counts - 1) // TILE) & (counts > 1)).any()


def test_pass_3_shares_empty_ragged_and_more_tiles_than_cells():
    points = K.few_cells(4097, 3)[0]
    counts = M.voxel_mean(points, None, None, K.VOXEL)[4]
    assert len(counts) == 3 and counts.sum() == 4097 and counts.min() > 1000
    used, slots, tiles = K.occupied_slots(points, K.VOXEL)
    per = (slots + tiles - 1) // tiles
    assert (slots, tiles, len(used)) == (16384, 5, 3) and per % K.TRIP != 0  # per = 3277: the last trip of a share is ragged
    owners = {s // per for s in used}
    assert len(owners) < tiles  # a block whose share is empty takes nothing from the cursor
    # inside a block that owns a cell, the waves that own none leave before the second walk (mine == 0)
    waves_with = {(s // per, ((s % per) % K.TRIP) // WAVE) for s in used}
    assert len(waves_with) < 4 * len(owners)
    # every point alone: as many cells as points, two tiles
    points = K.all_alone(1025)[0]
    counts = M.voxel_mean(points, None, None, K.VOXEL)[4]
    assert len(counts) == 1025 and (counts == 1).all()
    # the smallest cloud with two chunks per tile: 2049 tiles, the slot shares of pass 3 are 2^23 / 2049, not a multiple of 256
    assert plan([4096 * 1024 + 1], TILE_VOXEL, MAX_TILES) == [(0, 0, 2049, 2)]
    assert plan([4096 * 1024], TILE_VOXEL, MAX_TILES) == [(0, 0, 4096, 1)]
    assert ((1 << 23) + 2048) // 2049 % K.TRIP != 0


def test_edge_arithmetic_premises_hold_in_numpy():
    cases = {c["name"]: c for c in K.edge_arithmetic()}
    assert all(len(c["points"]) <= 400 for c in cases.values())
    # rintf ties: d * s is a half-integer at every coordinate, and ties-to-even differs from round-half-up in the SUMS
    c = cases["rintf ties"]
    v = np.float32(c["voxel"])
    s = np.float32(32768.0) / v
    p = c["points"]
    ctr = (np.floor(p / v) + np.float32(0.5)) * v
    x = (p - ctr) * s
    assert x.dtype == np.float32 and (x - np.floor(x) == 0.5).all()
    k = np.floor(x)
    assert (k % 2 == 0).any() and (k % 2 == 1).any() and (k < 0).any() and (k >= 0).any() and np.abs(k).max() > 16000
    even, half_up = np.rint(x), np.floor(x + np.float32(0.5))
    assert (even != half_up).sum() > len(x)  # of 3 len coordinates
    out_p, _, _, index, counts, dropped = M.voxel_mean(p, None, None, c["voxel"])
    assert dropped == 0 and set(counts.tolist()) == {2, 3}
    _, key, _ = V.voxel_keys(p, c["voxel"])
    u = v / np.float32(32768.0)
    for row, rep in enumerate(index):  # in every cell, on some axis, the two roundings give different sums and different bits
        rows = key == key[rep]
        assert (even[rows].sum(axis=0) != half_up[rows].sum(axis=0)).any(), row
        m_up = (half_up[rows].astype(np.float64).sum(axis=0) / rows.sum()).astype(np.float32)
        assert ((ctr[rep] + m_up * u).view(np.uint32) != out_p[row].view(np.uint32)).any(), row
    # colours: exact halves (2 C == N mod 2 N) round up, thirds never tie
    c = cases["colour halves and thirds"]
    out = M.voxel_mean(c["points"], None, c["colors"], c["voxel"])
    assert out[4].tolist() == [2, 4, 3] and out[2].tolist() == [[1, 255, 12], [1, 1, 255], [0, 0, 1]]
    sums = [c["colors"][a:b].astype(np.int64).sum(axis=0) for a, b in ((0, 2), (2, 6), (6, 9))]
    assert ((2 * sums[0]) % 4 == 2).all() and ((2 * sums[1][:2]) % 8 == 4).all()
    assert sums[2].tolist() == [1, 0, 2] and ((2 * sums[2]) % 6 != 3).all()  # one third and two thirds
    # normals: the counted rows of a cell cancel (T == 0, so L == 0), or one row counts
    c = cases["cancelling normals"]
    out_p, out_n, _, index, counts, _ = M.voxel_mean(c["points"], c["normals"], None, c["voxel"])
    assert sorted(counts.tolist()) == [2, 2, 4, 4, 65, 66, 69]
    nrm = c["normals"]
    counted = (np.isfinite(nrm) & (np.abs(nrm) <= 2)).all(axis=1)
    _, key, _ = V.voxel_keys(c["points"], c["voxel"])
    zero_cells, one_counted = 0, 0
    for row, rep in enumerate(index):
        rows = (key == key[rep]) & counted
        T = np.rint(nrm[rows].astype(np.float32) * np.float32(1048576.0)).astype(np.int64).sum(axis=0)
        if (T == 0).all():
            zero_cells += 1
            assert (out_n[row].view(np.uint32) == 0).all()  # +0.0
        else:
            one_counted += rows.sum() == 1 and (key == key[rep]).sum() > 1
            assert abs(np.linalg.norm(out_n[row].astype(np.float64)) - 1) < 1e-6
    assert zero_cells == 5 and one_counted == 2
    assert {65, 66} <= {int(n) for n, o in zip(counts, out_n) if (o == 0).all()}  # cancelling across a wave boundary
    # the ends of the key range: cells -2^20 and 2^20 - 1 hold N > 1, the points outside are dropped and counted
    c = cases["key-range ends"]
    kept, key, _ = V.voxel_keys(c["points"], c["voxel"])
    out = M.voxel_mean(c["points"], c["normals"], c["colors"], c["voxel"])
    assert out[5] == K.KEY_RANGE_OUTSIDE == int((~kept).sum()) and (out[4] == 3).all() and len(out[4]) == 6
    fields = {(int(k) >> 42, (int(k) >> 21) & 0x1FFFFF, int(k) & 0x1FFFFF) for k in key[kept]}
    for axis in range(3):
        assert {f[axis] for f in fields} >= {0, (1 << 21) - 1}
    assert np.isfinite(out[0]).all() and (np.floor(out[0]) == np.floor(c["points"][out[3]])).all()  # the mean stays in its cell
    # cell faces: p == c * v exactly, next to points one and two ulp below; both cells of a face hold N > 1
    for v in (0.25, K.VOXEL):
        c = cases[f"cell faces, v = {v}"]
        p, v32 = c["points"], np.float32(v)
        on_face = np.zeros(p.shape, bool)
        for cell in (-5, -1, 0, 1, 3, 7):
            on_face |= p == np.float32(cell) * v32
        assert on_face.any(axis=1).sum() >= 36
        out = M.voxel_mean(p, c["normals"], c["colors"], v)
        assert out[5] == 0 and (out[4] > 1).all() and len(out[4]) == 36
        if v == 0.25:  # exact arithmetic: a point on the face is in the upper cell, the one below it in the lower one
            cells = np.floor(p / v32)
            assert (cells[on_face] * v32 == p[on_face]).all()


def test_many_job_batches_mix_the_fields_and_reach_past_64_jobs():
    n = max(BATCHES)
    clouds = K.batch_recipe(n)
    lengths = batch_lengths(n)
    assert [len(p) for p, _, _ in clouds] == lengths
    combos = {(nrm is not None, col is not None) for p, nrm, col in clouds if len(p)}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    assert all(col is None for p, _, col in clouds if len(p) == 0)
    coloured = [col is not None for p, _, col in clouds if len(p)]
    assert coloured == [k % 2 == 1 for k in range(len(coloured))]  # every second non-empty cloud
    for small in BATCHES:  # a cloud is the same in every batch size
        for (p, nrm, col), (p2, nrm2, col2) in zip(K.batch_recipe(small)[-3:], clouds[small - 3:small]):
            assert np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and (col is None) == (col2 is None)
            assert col is None or np.array_equal(col, col2)
    # vmean_any_over scans the jobs 64 at a time and find_job searches log2(jobs) levels: more than two trips, ten levels
    jobs = plan(lengths, TILE_VOXEL, MAX_TILES)
    assert len(jobs) > 2 * 64 and len(jobs) > 512
    for small in BATCHES:
        assert small == 65 or sum(1 for x in batch_lengths(small) if x) > 64  # (65 clouds are 60 jobs: one trip)
        for i in (*SINGLED_OUT, small - 1):  # the clouds whose capacity is cut: jobs on both sides of the stride of 64
            if i < small:
                p, nrm, col = clouds[i]
                rows = len(M.voxel_mean(p, nrm, col, VOXEL)[3])
                assert rows >= 2, i  # (a capacity one short still leaves room for a row)
    by_cloud = {i: k for k, (i, _, _, _) in enumerate(jobs)}
    assert by_cloud[63] < 64 <= by_cloud[70] and by_cloud[n - 1] == len(jobs) - 1 and by_cloud[64] != 64
    # cells are shared (N > 1) in the tame clouds, and raw-bits clouds past job 64 both drop and keep
    both = 0
    for i in range(64, n):
        if is_raw(i) and lengths[i]:
            out = M.voxel_mean(*clouds[i], VOXEL)
            both += out[5] > 0 and len(out[3]) > 0
    assert both >= 3
    for i in (0, 5, 13, 70):
        counts = M.voxel_mean(*clouds[i], VOXEL)[4]
        assert (counts > 1).any() and counts.max() < 64
