#!/bin/bash
# bash profiles/ab_forms.sh: parent and new tree interleaved, order alternating by round; default form and short form; raw lines kept
set -o pipefail
ROOT=$(pwd); OUT=$ROOT/${PROF_OUT:-profiles/out}/ab; mkdir -p $OUT; : > $OUT/ab_runs.txt
run() {  # tree, form tag, args...
  local t=$1 f=$2; shift 2
  (cd $ROOT/profiles/ab/$t && timeout -k 10 300 python3 bench.py "$@" 2>> $OUT/err_$t.txt | grep '^{' | tail -1 > $OUT/line.json) || return 1
  echo "$t $f $(cat $OUT/line.json)" >> $OUT/ab_runs.txt
  python3 - $t $f $OUT/line.json <<'PY'
import json,sys
t,f,p=sys.argv[1:]
d=json.load(open(p))
print(t,f,'value %.4e'%d['value'],'ms/step %.4f'%d['ms_per_step'],'steady %.4f'%d.get('steady_state',{}).get('ms_per_step',float('nan')),
      {k:round(v['avg_ms']*1e3,1) for k,v in d['kernels'].items()}, d['placement']['outcome'])
PY
}
for r in 1 2 3; do
  if [ $((r % 2)) = 1 ]; then order="parent new"; else order="new parent"; fi
  for t in $order; do run $t default || { echo "FAILED $t default"; tail -5 $OUT/err_$t.txt; exit 1; }; done
  for t in $order; do run $t short --gpus 1 --steps 20 --warmup 5 || { echo "FAILED $t short"; tail -5 $OUT/err_$t.txt; exit 1; }; done
done
