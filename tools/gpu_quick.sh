#!/bin/bash
# bench on configs[2] (and optionally configs[1]) only, compact output; the JSON lines go to $OUT (default /tmp/lqcov_out)
cd "$(dirname "$0")/.."; OUT=${OUT:-/tmp/lqcov_out}; mkdir -p $OUT
for C in ${CFGS:-cfg3}; do
  timeout 400 python bench.py --full --config $C --steps ${STEPS:-3} --warmup 1 --no-cpu-baseline 2>&1 | tail -1 > $OUT/bench_$C.json
  python -c "
import sys, json
j = json.loads(open('$OUT/bench_$C.json').read())
print('$C', j['value'], j['ms_per_step'], (j.get('golden_rows') or {}).get('rows_identical'), j['roofline']['kernel'], j['roofline']['frac'])
print({k: round(v) for k, v in list(j['roofline']['kernel_ms_one_step'].items())[:16]})
"
done
