#!/bin/bash
# the end-to-end leg's files, then the program under rocprofv3 (kernel + memory-copy trace) and with the host timers
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$(mktemp -d)}  # (where the outputs go)
mkdir -p "$OUT"; echo "outputs in $OUT"
export TMPDIR=/tmp
PJB_BENCH_KEEP_WORKDIR=1 PJB_BENCH_E2E_REPS=${REPS:-1} timeout 900 python bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > "$OUT"/e2e_tr_bench.json 2> "$OUT"/e2e_tr_bench.err
python -c "import json, sys; print(json.load(open(sys.argv[1]))['e2e'])" "$OUT"/e2e_tr_bench.json
W=/tmp/pjb_bench_e2e
PJB_PROFILE_HOST=2 portcullis_amd/host/portcullis_amd junc -t 16 --orientation FR -o $W/out/pc2 $W/prep > /dev/null 2> "$OUT"/e2e_tr_host.txt
grep -E "device thread|workers|main:|context ready" "$OUT"/e2e_tr_host.txt
grep -c "host event" "$OUT"/e2e_tr_host.txt
rm -rf /tmp/e2e_prof
export PJB_NORMAL_EXIT=1
( time rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d /tmp/e2e_prof -- portcullis_amd/host/portcullis_amd junc -t 16 --orientation FR -o $W/out/pc3 $W/prep > /dev/null 2> "$OUT"/e2e_tr_rocprof.err ) 2>&1 | tail -3
python tools/debug/e2e_timeline.py /tmp/e2e_prof > "$OUT"/e2e_timeline.txt 2>&1
head -70 "$OUT"/e2e_timeline.txt
python tools/debug/inflate_gantt.py /tmp/e2e_prof > "$OUT"/e2e_inflate_gantt.txt 2>&1
tail -45 "$OUT"/e2e_inflate_gantt.txt
