"""Summarises the directory that scripts/solve_split_ab.sh filled: the eight headline figures, the gate (every run of
this tree above every run of the parent, median gain at least twice the parent's spread), the dumped outputs compared on
bits, and the diagnostics build's mask sweep.  Prints the JSON of profiles/solveonce_bench.json.
    python3 scripts/solve_split_summary.py OUTDIR"""
import glob
import json
import os
import sys

import numpy as np

out = sys.argv[1]


def line(name):
    for text in reversed(open(os.path.join(out, name + ".json")).read().splitlines()):
        if text.startswith("{"):
            return json.loads(text)
    raise SystemExit(f"{name}: no result line")


def dump(name):
    return {os.path.basename(f): np.load(f) for f in sorted(glob.glob(os.path.join(out, "dump_" + name, "*.npy")))}


def same(a, b):
    return bool(a) and a.keys() == b.keys() and all(
        a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


runs, values = [], {"parent": [], "this": []}
for i in (1, 2, 3, 4):
    for tree in ("parent", "this"):
        r = line(f"{tree}_{i}")
        runs.append({"tree": tree, "run": i, "frame_pairs_per_s": round(r["value"], 1), "ms_per_step": round(r["ms_per_step"], 5)})
        values[tree].append(r["value"])
mp, mt = float(np.median(values["parent"])), float(np.median(values["this"]))
spread = (max(values["parent"]) - min(values["parent"])) / mp
ref = dump("parent_1")
names = [f"{t}_{i}" for i in (1, 2, 3, 4) for t in ("parent", "this")] + [f"diag_mask{m}" for m in (0, 1, 3, 7)]
result = {
    "command": "python3 bench.py --gpus 1 --steps 600 --warmup 20 --dump-outputs DIR (scripts/solve_split_ab.sh: one MI355X "
               "job, the parent commit's library and this tree's alternating: parent / this, four times; then the "
               "diagnostics build under A3D_ICP_SOLVE_SPLIT)",
    "runs": runs,
    "median_parent": round(mp, 1), "median_this": round(mt, 1), "median_gain": round(mt / mp - 1, 4),
    "parent_min_max": [round(min(values["parent"]), 1), round(max(values["parent"]), 1)],
    "parent_spread_of_median": round(spread, 4), "twice_parent_spread": round(2 * spread, 4),
    "this_min_max": [round(min(values["this"]), 1), round(max(values["this"]), 1)],
    "lowest_this_over_highest_parent": round(min(values["this"]) / max(values["parent"]) - 1, 4),
    "every_run_of_this_tree_above_every_parent_run": min(values["this"]) > max(values["parent"]),
    "median_gain_above_twice_parent_spread": mt / mp - 1 >= 2 * spread,
    "dumped_outputs_bit_identical_to_parent_run_1": {n: same(dump(n), ref) for n in names},
    "diagnostics_build_mask_sweep_64_pairs": {
        f"A3D_ICP_SOLVE_SPLIT={m}": {"frame_pairs_per_s": round(line(f"diag_mask{m}")["value"], 1),
                                     "ms_per_step": round(line(f"diag_mask{m}")["ms_per_step"], 5)} for m in (0, 1, 3, 7)},
}
print(json.dumps(result, indent=1))
