#!/bin/bash
# One GPU machine's worth of checking: the whole GPU suite, the smoke entry, the full bench line.
#   bash tools/gpu_check.sh OUT_DIR        (from the repository root; logs and the bench JSON go to OUT_DIR)
set -o pipefail
OUT=${1:?usage: tools/gpu_check.sh OUT_DIR}
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$OUT/gpu_tests.log" 2>&1; rc=$?
tail -3 "$OUT/gpu_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1; rc=$?
tail -2 "$OUT/smoke.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 700 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"; rc=$?
python3 - "$OUT/bench_full.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
def show(k, r):
    ro = r["roofline"]
    print(f"{k}: {r['value']:.4g} {r['unit']}  {r['ms_per_step']:.4g} ms/step  {ro['kernel']} {ro['avg_kernel_ms']:.4g} ms  frac {ro['frac']:.3f}  verify {r.get('verify')}")
show("headline", d)
for k, r in d.get("also", {}).items():
    show(k, r)
PY
exit $rc
