#!/bin/bash
# kernel-trace of one bench step and the idle-gap table of its bundle adjustment
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${OUT:-$ROOT/out}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/trace
timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $OUT/trace -- python3 $ROOT/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-profile > $OUT/trace.log 2>&1
echo "rc=$?"
python3 $ROOT/tools/trace_gaps.py $OUT/trace | tee $OUT/trace_gaps.txt
find $OUT/trace -name "*.csv" -size +1M -delete
