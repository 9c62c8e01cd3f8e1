#!/bin/bash
# end-of-round evidence: parity tests, smoke, bench (--full), rocprofv3 kernel stats, PMC traffic counters; everything
# is written under $OUT (default: out/ in the repository), which tools/collect_profiles.sh reads
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}")
mkdir -p "$OUT" && cd "$ROOT" || exit 1
make -C meatmodeler_amd/csrc -j8 > $OUT/make.log 2>&1 || { tail $OUT/make.log; exit 1; }
timeout -k 10 900 python -m pytest tests -m gpu -q --timeout 300 -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/pytest_gpu.log
if [ $rc -ne 0 ]; then exit 1; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/smoke.log
if [ $rc -ne 0 ]; then exit 1; fi
timeout -k 10 900 python bench.py --full > $OUT/bench_default.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 400 $OUT/bench_default.log
if [ $rc -ne 0 ]; then exit 1; fi
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-profile > $OUT/rocprof.log 2>&1
rc=$?; echo "rocprof rc=$rc"
find $OUT/prof -name "*_kernel_trace.csv" -delete
# (counter collection serialises kernels: the overlapped build + solve runs one after the other there)
export MM_SCHUR_OVERLAP=0
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$ctr
  timeout -k 10 900 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $OUT/pmc_$ctr -- python3 $ROOT/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-profile > $OUT/pmc_$ctr.log 2>&1
  rc=$?; echo "pmc $ctr rc=$rc"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit 1; fi
  python3 $ROOT/tools/pmc_summary.py $OUT/pmc_$ctr $ctr > $OUT/pmc_${ctr}_summary.txt 2>&1
  find $OUT/pmc_$ctr -name "*.csv" -size +2M -delete
done
head -14 $OUT/pmc_FETCH_SIZE_summary.txt
unset MM_SCHUR_OVERLAP
cd $ROOT && ./tools/prof_chol.sh > $OUT/prof_chol_summary.txt 2>&1; tail -4 $OUT/prof_chol_summary.txt | cut -c1-160
cd $ROOT && ./tools/gpu_trace.sh > $OUT/trace_summary.txt 2>&1; head -4 $OUT/trace_summary.txt
cd $ROOT && ./tools/dev/orb_stats.sh > $OUT/orb_kernels.txt 2>&1; tail -8 $OUT/orb_kernels.txt
