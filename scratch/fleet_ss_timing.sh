#!/bin/bash
# Fleet safe-set timing in one GPU command: the event-timed run, then a kernel trace of its own for the kernel times.
# Every GPU step has its own time limit and the steps are chained: a failed step ends the script.
#   bash scratch/fleet_ss_timing.sh OUT_DIR
set -u
OUT=${1:-fleet_ss_timing_out}
mkdir -p "$OUT"
cd "$(dirname "$0")/.."
timeout -k 10 300 python scratch/fleet_ss_timing.py --reps 200 --out "$OUT/fleet_ss_query_table.md" > "$OUT/timing.txt" 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/rocprof" -o fleet -- python scratch/fleet_ss_timing.py --reps 50 > "$OUT/rocprof.txt" 2>&1 &&
{ find "$OUT/rocprof" -name "*kernel_stats.csv" | head -1 | xargs -r grep -E "Name|ss_query|fleet_ss" > "$OUT/kernel_stats.txt"; }
rc=$?
tail -8 "$OUT/timing.txt"
cat "$OUT/kernel_stats.txt" 2>/dev/null
exit $rc
