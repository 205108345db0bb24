#!/bin/bash
# one run per tree of the other shapes (profiles/r6_pipelined_loads.md section 4), parent and new alternating
set -o pipefail
ROOT=$(pwd); OUT=$ROOT/${PROF_OUT:-profiles/out}/shapes; mkdir -p $OUT; : > $OUT/shapes.txt
i=0
while read -r name args; do
  i=$((i+1)); if [ $((i % 2)) = 1 ]; then order="parent new"; else order="new parent"; fi
  for t in $order; do
    (cd $ROOT/profiles/ab/$t && timeout -k 10 200 python3 bench.py --no-cpu-baseline --steps 50 --warmup 5 --steady-steps 0 $args < /dev/null 2>> $OUT/err_$t.txt | grep '^{' | tail -1 > $OUT/line.json) || { echo "FAILED $t $name"; tail -5 $OUT/err_$t.txt; exit 1; }
    echo "$name $t $(cat $OUT/line.json)" >> $OUT/shapes.txt
    python3 -c "
import json,sys
d=json.load(open('$OUT/line.json'))
print('%-14s %-6s ms/step %.4f' % ('$name','$t',d['ms_per_step']), {k:round(v['avg_ms']*1e3,1) for k,v in d['kernels'].items()})"
  done
done <<'LIST'
envs12 --envs 12
config1 --config 1
small_sweeps --envs 256 --particles 5000 --mesh 250 --blocks-per-env 2
config3_fixed32 --config 3
config3_float --config 3 --positions float
config4 --config 4
config5 --config 5
LIST
