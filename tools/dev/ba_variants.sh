#!/bin/bash
# bench.py over compile-time variants of one csrc file: FILE=ba.hip VARIANTS="-DX=1|-DX=2" KERNELS="ba_normal_eq_kernel ba_backsub_points_kernel"
# (logs and bench lines go to $OUT, default: out/ in the repository)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$(realpath -m "${OUT:-$ROOT/out}")
mkdir -p "$OUT" && cd "$ROOT/meatmodeler_amd/csrc" || exit 1
obj=${FILE%.hip}.o
IFS='|' read -ra VS <<< "${VARIANTS}"
for v in "${VS[@]}"; do
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wall -Wno-unused-result $v -c $FILE -o $obj || exit 1
  make > $OUT/make_var.log 2>&1 || { tail $OUT/make_var.log; exit 1; }
  ( cd ../.. && python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/bench_var.json 2>/dev/null; KERNELS="$KERNELS" V="$v" OUT="$OUT" python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_var.json")).read().strip().splitlines()[-1])
ks = {k["kernel"]: k for k in d["kernels_all_launches_extra_step"]}
print("[%s] ms/iteration %.4f nfev %d | " % (os.environ["V"], d["ba"]["ms_per_iteration"], d["ba"]["nfev"]) +
      " ".join("%s %.1f" % (n, ks[n]["avg_us"]) for n in os.environ["KERNELS"].split() if n in ks))
PY
  )
done
rm -f $obj && make > $OUT/make.log 2>&1
