#!/bin/bash
# One GPU-box session: tests, bench, rocprof kernel trace.  Each GPU step has its own time limit.
# Results go to $LGX_OUT_DIR (default: bench_out/ under the repository root).
set -o pipefail
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
OUT=${LGX_OUT_DIR:-bench_out}
mkdir -p $OUT
STEP=${1:-all}
if [[ $STEP == all || $STEP == tests ]]; then
  timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo "tests failed rc=$?"; tail -30 $OUT/gpu_tests.log; exit 1; }
  tail -3 $OUT/gpu_tests.log
fi
if [[ $STEP == all || $STEP == bench ]]; then
  timeout -k 10 900 python bench.py --full ${BENCH_ARGS:-} > $OUT/bench.json 2> $OUT/bench.err || { echo "bench failed rc=$?"; tail -30 $OUT/bench.err; exit 1; }
  cat $OUT/bench.json
fi
if [[ $STEP == all || $STEP == prof ]]; then
  export TMPDIR=/tmp
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python bench.py --steps 3 --warmup 1 --full --no_cpu_baseline > $OUT/prof_bench.json 2> $OUT/prof.err || { echo "prof failed rc=$?"; tail -30 $OUT/prof.err; exit 1; }
  find $OUT/prof -name "*stats*" | head
fi
