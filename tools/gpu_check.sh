#!/bin/bash
# Round-end style check on the GPU box: gpu tests, the bench line (with CPU baseline), a rocprofv3 kernel
# trace + stats of the bench, and the FETCH_SIZE traffic pass. Usage: tools/gpu_check.sh <tag>
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
tag=${1:-r02}
OUT=${OUT_DIR:-bench_out}  # where the logs and result files go
mkdir -p $OUT/prof
timeout -k 10 600 python3 -u -m pytest tests -m gpu -q -x -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo TESTS FAILED; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python3 bench.py --full > $OUT/bench.log 2>&1 || { echo BENCH FAILED; tail -20 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log
./tools/prof_step.sh "$tag" || exit 1
./tools/pmc_traffic.sh "$tag" || exit 1
echo done
