"""Summarises a counter-only rocprofv3 pass (--pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY
SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_WAVES SQ_BUSY_CYCLES, no tracing beside it) of bench.py per alignment kernel and grid:
the pixel launches of image_icp_head_kernel (the grid tells the level and the stream group) and the solve launches of
a split level (job_solve_head_kernel).
    python3 scripts/solve_split_pmc.py DIR"""
import collections
import csv
import glob
import sys

rows = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        short = "head" if "image_icp_head_kernel" in name else "solve" if "job_solve_head_kernel" in name else \
            "finish" if "job_finish_head_kernel" in name else None
        if short:
            rows[(short, int(r["Grid_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
print("kernel | grid | launches | wait_any % | wait_inst % | active % | VALU insts/wave | VMEM-read insts/wave | waves")
for (short, grid), c in sorted(rows.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
    wc = sum(c.get("SQ_WAVE_CYCLES", [0])) or 1.0
    waves = sum(c.get("SQ_WAVES", [0])) or 1.0
    share = lambda k: 100 * sum(c.get(k, [0])) / wc
    print(f"{short} | {grid} | {len(c.get('SQ_WAVE_CYCLES', []))} | {share('SQ_WAIT_ANY'):.1f} | {share('SQ_WAIT_INST_ANY'):.1f} | "
          f"{share('SQ_ACTIVE_INST_ANY'):.1f} | {sum(c.get('SQ_INSTS_VALU', [0])) / waves:.0f} | "
          f"{sum(c.get('SQ_INSTS_VMEM_RD', [0])) / waves:.1f} | {waves:.0f}")
