#!/bin/bash
# A/B two prebuilt libsli.so variants (exp/libsli_a.so, exp/libsli_b.so; exp/ is git-ignored) on one bench line.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}  # where the logs and result files go
mkdir -p $OUT
for v in a b a b; do
  cp exp/libsli_$v.so simplellminference_amd/libsli.so
  timeout -k 10 200 python3 bench.py --full --no-cpu-baseline "$@" > $OUT/ab.log 2>&1 || { tail -5 $OUT/ab.log; exit 1; }
  echo "$v $(tail -1 $OUT/ab.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['roofline']['avg_launch_us'])")"
done
