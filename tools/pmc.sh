# PMC passes (one rocprofv3 --pmc run per counter group, each under its own hard limit).
# Output under $OUT_DIR/pmc (default: bench_out/pmc in the repository).
set -o pipefail
R=$GRAFT_REPO_ROOT
S=${OUT_DIR:-$R/bench_out}/pmc
mkdir -p $S
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 60 rocprofv3 -L > $S/list.txt 2>&1 || true
grep -oE "^[[:space:]]*(SQ|TCC|TCP|GRBM)_[A-Z0-9_]+" $S/list.txt | sort -u > $S/names.txt || true
wc -l $S/names.txt
i=0
for grp in "$@"; do
  i=$((i+1))
  timeout -s KILL 90 rocprofv3 --pmc $grp --output-format csv -d $S/p$i -o run -- python3 $R/bench.py --full --cpu-baseline off --steps 3 --warmup 1 > $S/p$i.log 2>&1 || { echo "PMC group $i failed: $grp"; tail -5 $S/p$i.log; }
done
ls $S
