#!/bin/bash
# quick GPU check: selected parity tests (-k "$1"), then a bench with the kernel tables but without the CPU leg; logs go
# to $OUT (default: out/ in the repository)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${OUT:-$ROOT/out}")
mkdir -p "$OUT" && cd "$ROOT" || exit 1
make -C meatmodeler_amd/csrc -j8 > $OUT/make.log 2>&1 || { tail $OUT/make.log; exit 1; }
timeout -k 10 600 python -m pytest tests -m gpu -q --timeout 240 -p no:cacheprovider -k "${1:-link or pipeline}" > $OUT/pytest_quick.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -15 $OUT/pytest_quick.log
if [ $rc -ne 0 ]; then exit 1; fi
timeout -k 10 600 python bench.py --full --no-cpu-baseline ${2:-} > $OUT/bench_quick.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 3000 $OUT/bench_quick.log
