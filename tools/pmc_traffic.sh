#!/bin/bash
# HBM traffic counters for the pjb kernels: separate --pmc passes (FETCH_SIZE takes 3 TCC slots,
# WRITE_SIZE 2), kernel trace only.  Results are summarised by tools/summarize_pmc.py, which averages the dispatches of the two
# timed steps only (keep_last=2/7: three warm-up passes and the two instrumented passes of bench.py --full come first).
# Each pass has its own time limit; a pass that fails ends the script (the next one is not started on a card that has just failed).
set -e -o pipefail
OUT=$GRAFT_REPO_ROOT/gpurun_out/pmc_$1
mkdir -p $OUT
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $OUT/$ctr -o pmc -- python3 "$ROOT/bench.py" --full --steps 2 --warmup 3 --no-cpu-baseline --no-e2e --no-back-to-back > $OUT/bench_$ctr.log 2>&1
  ls $OUT/$ctr | head
done
