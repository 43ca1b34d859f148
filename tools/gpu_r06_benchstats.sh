#!/usr/bin/env bash
# rocprofv3 --kernel-trace --stats of the driver's bench command itself (all legs mixed; the per-regime windows are the ones to price)
# Usage: tools/gpu_r06_benchstats.sh <log dir>
LOG="${1:?usage: tools/gpu_r06_benchstats.sh <log dir>}"; mkdir -p "$LOG"; LOG="$(cd "$LOG" && pwd)"; cd "$(dirname "$0")/.."; ROOT="$PWD"; PROF="$(mktemp -d)"
(cd "$PROF" && timeout 900 rocprofv3 --kernel-trace --stats -d "$PROF/prof_bench" -o b -- python "$ROOT/bench.py" --gpus 1 --steps 20 --warmup 5 --full --no-sustained > "$LOG/bench_under_rocprof.json" 2> "$LOG/bench_under_rocprof.err")
db=$(find "$PROF/prof_bench" -name "*.db" | head -1); python tools/rocpd_stats.py "$db" "$LOG/r06_bench_kernel_stats.md" > /dev/null 2>&1; head -12 "$LOG/r06_bench_kernel_stats.md" | cut -c1-150
