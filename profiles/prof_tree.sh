#!/bin/bash
# bash profiles/prof_tree.sh <tree under profiles/ab> <tag> [counters...]: kernel trace, then one --pmc pass per counter
set -o pipefail
tree=$1; tag=$2; shift 2
ROOT=$(pwd); OUT=$ROOT/${PROF_OUT:-profiles/out}/$tag; mkdir -p $OUT
cd $ROOT/profiles/ab/$tree || exit 1
export TMPDIR=/tmp
[ -n "$SKIP_KT" ] || timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -o kt -- python3 bench.py --no-cpu-baseline --steps 50 --warmup 5 --steady-steps 0 > $OUT/kt_bench.json 2> $OUT/kt.err || { echo "kernel trace failed $?"; tail -5 $OUT/kt.err; exit 1; }
for c in "$@"; do
  g=${c// /_}; g=${g:0:40}
  timeout -k 10 240 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_$g -o p -- python3 bench.py --steps 5 --warmup 1 --steady-steps 0 --order cold --no-cpu-baseline > $OUT/pmc_$g.json 2> $OUT/pmc_$g.err || { echo "pmc $c failed $?"; tail -5 $OUT/pmc_$g.err; exit 1; }
done
cd $ROOT && python3 profiles/pmc_sum.py $OUT $tag | tee $OUT/summary.txt
