#!/bin/bash
# The N > 1 control flow of bench.py on a one-GPU box: two ranks over gloo sharing device 0 (cfg4 shape, exchange, the
# reduce self-check).  Usage: gpurun -- 'bash tools/gpu_two_ranks.sh [reads per rank]'
set -u
export GTX_BENCH_FULL_LINE=1  # bench.py prints its whole record (the default line is the compact one the driver parses)
tmp=$(mktemp -d)
GTX_BENCH_SHARE_DEVICE=1 timeout 600 python bench.py --full --gpus 2 --backend gloo --reads ${1:-2000000} --steps 3 --warmup 1 > $tmp/bench_2rank.json 2> $tmp/bench_2rank.err
echo "two-rank bench exit $?"; tail -3 $tmp/bench_2rank.err; python - $tmp/bench_2rank.json <<'PY'
import json, sys
j = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
print({k: j[k] for k in ("value", "n_gpus", "ms_per_step", "scaling")}, j["config"]["reduce_check"], j["config"]["reduce"])
PY
rm -rf $tmp
