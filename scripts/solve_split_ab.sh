# The headline A/B of the split solve (one solve launch per pair and iteration at level 0) in ONE GPU job:
# the parent commit's product library and this tree's alternating four times, then the diagnostics build under
# A3D_ICP_SOLVE_SPLIT = 0 / 1 / 3 / 7.  Every run under its own time limit; the first failure ends the job.
#   PARENT_LIB=<the parent commit's libalign3d_hip.so> bash scripts/solve_split_ab.sh OUTDIR
#   python3 scripts/solve_split_summary.py OUTDIR > profiles/solveonce_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:?output directory}
[ -f "${PARENT_LIB:?PARENT_LIB}" ] || { echo "no $PARENT_LIB"; exit 2; }
mkdir -p "$OUT"
THIS_LIB=$PWD/align3d_amd/csrc/libalign3d_hip.so
DIAG_LIB=$PWD/align3d_amd/csrc/libalign3d_hip_diag.so
BENCH="python3 bench.py --gpus 1 --steps 600 --warmup 20"
run() {  # name, library, extra environment
  local name=$1 lib=$2; shift 2
  env A3D_LIBRARY="$lib" "$@" timeout -k 10 240 $BENCH --dump-outputs "$OUT/dump_$name" > "$OUT/$name.json" 2> "$OUT/$name.err"
  local rc=$?
  echo "$name exit $rc: $(tail -c 300 "$OUT/$name.json" | tr -d '\n' | grep -o '"value": *[0-9.]*')"
  return $rc
}
for i in 1 2 3 4; do
  run parent_$i "$PARENT_LIB" && run this_$i "$THIS_LIB" || exit 1
done
for mask in 0 1 3 7; do
  run diag_mask$mask "$DIAG_LIB" A3D_ICP_SOLVE_SPLIT=$mask || exit 1
done
