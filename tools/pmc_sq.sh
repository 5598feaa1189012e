# SQ counter passes (one rocprofv3 --pmc run per group) over the cfg2 bench.
# Output under $OUT_DIR/sq (default: bench_out/sq in the repository).
set -o pipefail
R=$GRAFT_REPO_ROOT
S=${OUT_DIR:-$R/bench_out}/sq
mkdir -p $S
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 60 rocprofv3 -L > $S/list.txt 2>&1 || true
i=0
for grp in "$@"; do
  i=$((i+1))
  timeout -s KILL 90 rocprofv3 --pmc $grp --output-format csv -d $S/p$i -o run -- python3 $R/bench.py --full --cpu-baseline off --steps 2 --warmup 1 > $S/p$i.log 2>&1 || { echo "PMC group $i failed: $grp"; tail -3 $S/p$i.log; exit 1; }
done
python3 $R/tools/pmc_sq.py $S/p*
