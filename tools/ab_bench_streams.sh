#!/bin/bash
# Interleaved bench runs (N = 1, the driver's --steps 20 --warmup 5, --full for
# the sustained runs and the lone launch) for stream-layout arms:
# ARM = "name:extra bench args".  One process per run; results go to $O
# (default bench_out/).
set -o pipefail
O=${O:-bench_out}; mkdir -p $O
for round in 1 2; do
  for spec in "$@"; do
    name=${spec%%:*}; extra=${spec#*:}
    timeout -k 10 240 python -u bench.py --full --steps 20 --warmup 5 --no-parity --no-cpu-baseline --no-other-configs \
        --no-bounce $extra > $O/abs_${name}_$round.json 2> $O/abs_${name}_$round.err || exit 1
    python -c "
import json,sys; d=json.load(open('$O/abs_${name}_$round.json'))
print('$name', $round, d['value'], d['ms_per_step'], d['sustained']['value'], d['roofline']['kernel_ms_serial'])"
  done
done
