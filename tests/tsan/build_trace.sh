#!/usr/bin/env bash
# Launch trace of the host side: every source of libmon_core.so compiled --offload-host-only (no sanitizer), linked against hip_stub.cpp and trace_driver.cpp,
# run; the trace goes to <build-dir>/launch_trace.txt.  No GPU needed.  Usage: tests/tsan/build_trace.sh [build-dir].  MON_TRACE_SRC=<checkout> takes the
# product's sources (ro-map_amd/, include/) from another checkout of this repository -- the parent commit's, to show that a refactor kept every schedule.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"; REPO="$HERE/../.."; SRC="${MON_TRACE_SRC:-$REPO}"
OUT="${1:-/tmp/mon_trace}"; mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-host-only -O1 -std=c++17 -fPIC -x hip -ffp-contract=off -fno-math-errno -w)
source "$SRC/ro-map_amd/sources.sh"
pids=()
for s in "${SRCS[@]}"; do "$HIPCC" "${FLAGS[@]}" -c "$SRC/ro-map_amd/csrc/$s" -o "$OUT/${s%.*}.o" & pids+=($!); done
"$HIPCC" "${FLAGS[@]}" -c "$HERE/hip_stub.cpp" -o "$OUT/hip_stub.o" & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
# the host objects reference their (absent) device images: define those symbols
objs=(); for s in "${SRCS[@]}"; do objs+=("$OUT/${s%.*}.o"); done
{ for o in "${objs[@]}"; do nm -u "$o"; done; } | grep -o "__hip_fatbin_[0-9a-f]*" | sort -u | awk '{ printf "char %s[8];\n", $1 }' > "$OUT/fatbin_syms.c"
gcc -c "$OUT/fatbin_syms.c" -o "$OUT/fatbin_syms.o"
/opt/rocm/lib/llvm/bin/clang++ -O1 -std=c++17 -I"$SRC/include" "$HERE/trace_driver.cpp" "${objs[@]}" "$OUT/hip_stub.o" "$OUT/fatbin_syms.o" -o "$OUT/trace_driver" -lz -lpthread -ldl
"$OUT/trace_driver" "$OUT" "$SRC/ro-map_amd/configs/base.json" > "$OUT/launch_trace.txt"
echo "launch trace: $(wc -l < "$OUT/launch_trace.txt") lines in $OUT/launch_trace.txt"
