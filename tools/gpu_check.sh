# GPU check: parity tests, then the default bench, then a rocprofv3 kernel trace.
# Output under $OUT_DIR (default: bench_out in the repository).
set -o pipefail
R=$GRAFT_REPO_ROOT
cd $R
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/ -m gpu -q -x --timeout 120 --timeout-method thread > $O/tests.log 2>&1 || { echo TESTS_FAILED; tail -40 $O/tests.log; exit 1; }
tail -2 $O/tests.log
timeout -k 10 300 python bench.py --full ${BENCH_ARGS:---cpu-baseline off} > $O/bench.json 2> $O/bench.err || { echo BENCH_FAILED; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
if [ -n "$PROFILE" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 $R/bench.py --full --cpu-baseline off --steps 10 --warmup 2 > $O/prof.log 2>&1 || { echo PROF_FAILED; tail -20 $O/prof.log; exit 1; }
  head -8 $O/prof/run_kernel_stats.csv | cut -c1-160
fi
