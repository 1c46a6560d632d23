#!/bin/bash
# GPU-box routine after a kernel change: parity tests, serial-latency probe,
# bench --full (no CPU leg).  Each step has its own time limit; a failing step
# ends the script.  Usage: bash tools/gpu_check.sh <tag> [bench args...]
# Results go to $O (default bench_out/).
set -o pipefail
TAG=${1:-check}; shift
export O=${O:-bench_out}; mkdir -p $O
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
    > $O/tests_$TAG.log 2>&1 || { tail -30 $O/tests_$TAG.log; exit 1; }
tail -1 $O/tests_$TAG.log
timeout -k 10 200 python -u tools/latency_probe.py --blocks 64 --out $O/lat_$TAG.json \
    > $O/lat_$TAG.log 2>&1 || exit 1
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline "$@" > $O/bench_$TAG.json 2> $O/bench_$TAG.err || exit 1
python - "$TAG" <<'EOF'
import json, os, sys
tag, o = sys.argv[1], os.environ["O"]
d = json.load(open(f"{o}/bench_{tag}.json"))
print("bench", d["value"], "Mrays/s", d["ms_per_step"], "ms/step, kernel", d["roofline"]["kernel_ms"],
      "serial kernel", d["roofline"]["kernel_ms_serial"], "| bounce", d["bounce"] and d["bounce"]["value"],
      d["bounce"] and d["bounce"]["ms_per_step"])
for line in open(f"{o}/lat_{tag}.log"):
    if line.startswith("{") or line.startswith("pitch"):
        print(line.strip()[:260])
EOF
