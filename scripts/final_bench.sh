#!/bin/bash
# the full bench line (bench.py --full) on the current build -> OUT/bench_final.json
# (OUT: first argument, default bench_out)
cd "$(dirname "$0")/.." || exit 1
out=${1:-bench_out}
mkdir -p "$out"
timeout -k 10 1000 python3 bench.py --full > "$out/bench_final.json" 2> "$out/bench_final.err"; rc=$?
tail -3 "$out/bench_final.err"
exit $rc
