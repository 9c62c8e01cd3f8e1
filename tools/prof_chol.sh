#!/bin/bash
# kernel durations of the banded solve benchmark (rocprofv3 --kernel-trace --stats)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${OUT:-$ROOT/out}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_chol
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_chol -- python3 $ROOT/tools/bench_chol.py "$@" > $OUT/prof_chol.log 2>&1
echo "rc=$?"; tail -2 $OUT/prof_chol.log
f=$(find $OUT/prof_chol -name "*kernel_stats.csv" | head -1)
head -8 "$f" | cut -c1-200
find $OUT/prof_chol -name "*_kernel_trace.csv" -delete
