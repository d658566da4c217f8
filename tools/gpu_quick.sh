#!/bin/bash
# GPU-box quick check: the gpu test suite, then one bench line (no CPU baseline).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}  # where the logs and result files go
mkdir -p $OUT
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo TESTS FAILED; tail -40 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --steps 60 --warmup 10 "$@" > $OUT/bench.log 2>&1 || { echo BENCH FAILED; tail -20 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log
