#!/bin/bash
# after tools/gpu_evidence.sh: copy the summaries from its output directory $OUT (default: out/, scratch) into profiles/
# (tracked)
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
R=${1:-r01}
grep "^{" $OUT/bench_default.log | tail -1 > profiles/${R}_bench_default.json
# (the output directory may hold several runs' files: take the newest)
newest() { find "$1" -name "$2" -printf '%T@ %p\n' | sort -n | tail -1 | cut -d' ' -f2-; }
cp "$(newest $OUT/prof '*kernel_stats.csv')" profiles/${R}_rocprofv3_kernel_stats.csv
cp $OUT/pmc_FETCH_SIZE_summary.txt profiles/${R}_pmc_fetch_size.txt
cp $OUT/pmc_WRITE_SIZE_summary.txt profiles/${R}_pmc_write_size.txt
python3 tools/pmc_to_json.py profiles/${R}_pmc_fetch_size.txt profiles/${R}_pmc_write_size.txt profiles/${R}_pmc_traffic.json
cp "$(newest $OUT/prof_chol '*kernel_stats.csv')" profiles/${R}_chol_kernel_stats.csv
cp $OUT/trace_gaps.txt profiles/${R}_trace_gaps.txt
grep -v rocprofv3 $OUT/orb_kernels.txt > profiles/${R}_orb_kernels.txt
ls -la profiles | tail -n +2
