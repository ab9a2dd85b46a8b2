#!/bin/bash
# bench.py once per environment setting: tools/sweep_env.sh "VAR=a VAR2=b" "VAR=c" ...
set -e
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for cfg in "$@"; do
  tag=$(echo "$cfg" | tr ' =' '_-')
  env $cfg timeout -k 10 120 python3 bench.py --full --no-cpu-baseline --steps 5 --warmup 2 > "$OUT"/sw_$tag.json 2> "$OUT"/sw_err.log
  echo "$cfg $(python3 -c "import json;d=json.load(open('$OUT/sw_$tag.json'));print(d['value'],d['roofline']['pass_ms'])")"
done
