#!/bin/bash
# bench.py without the CPU leg; prints the headline figures and the repeats leg.  Usage: gpurun -- 'bash tools/gpu_bench_repeats.sh [pytest -k expression]'
set -u
export GTX_BENCH_FULL_LINE=1  # bench.py prints its whole record (the default line is the compact one the driver parses)
if [ $# -gt 0 ]; then timeout 900 python -m pytest tests -m gpu -x -q -k "$1" 2>&1 | tail -5; fi
tmp=$(mktemp -d)
python bench.py --full --no-cpu-baseline --steps 10 --warmup 2 > $tmp/bench.json 2> $tmp/bench.err; echo exit $?; tail -3 $tmp/bench.err
python - $tmp/bench.json <<'PY'
import json, sys
j=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
print(j['value'], j['ms_per_step'], j['roofline']['frac'], j['roofline']['kernel_ms'], j['config']['calls_checksum'].get('matches_pinned'))
print(json.dumps(j['config']['extra']['repeats']))
PY
rm -rf $tmp
