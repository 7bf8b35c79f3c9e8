#!/bin/bash
# GPU round: parity tests, then a short bench. Stops at the first crash/timeout.
# The logs go to $OUT (default build/gpu_check).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-build/gpu_check}
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -q -m gpu -x ${PYTEST_ARGS} > "$OUT/pytest_gpu.log" 2>&1
rc=$?
echo "pytest rc=$rc"
tail -40 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --steps 20 --warmup 3 ${BENCH_ARGS:---full --no-cpu-baseline} > "$OUT/bench.log" 2>&1
rc2=$?
cat "$OUT/bench.log"
exit $(( rc != 0 ? rc : rc2 ))
