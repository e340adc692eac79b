#!/bin/bash
# rocprofv3 kernel-trace + stats of a short bench run with its h3 leg (profiles/ summaries are copied from here).
set -u
OUT=${OUT:-out}
mkdir -p $OUT/prof
export TMPDIR=/tmp
timeout -k 10 ${PROF_TIMEOUT:-600} rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- \
  python3 bench.py ${BENCH_ARGS:---full --steps 2 --warmup 1 --no-cpu-baseline} > $OUT/prof_bench.log 2>&1
rc=$?; echo "[rocprof] exit $rc" >> $OUT/status.log; exit $rc
