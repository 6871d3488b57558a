#!/bin/bash
# GPU test suite on the in-tree build, then the default bench line with all its legs
# (bench.py --full; its line and stderr go to $LOGS, default logs/).
#   bash tools/gpu_check.sh TAG
set -o pipefail
TAG=${1:-chk}
mkdir -p gpurun_out
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider \
  > gpurun_out/pt_$TAG.log 2>&1 || { tail -40 gpurun_out/pt_$TAG.log; exit 1; }
tail -n 1 gpurun_out/pt_$TAG.log
LOGS=${LOGS:-logs}
mkdir -p $LOGS
timeout -k 10 600 python bench.py --full > $LOGS/bench_$TAG.json 2> $LOGS/bench_$TAG.err || { tail -20 $LOGS/bench_$TAG.err; exit 1; }
python -c "
import json; d = json.loads(open('$LOGS/bench_$TAG.json').read().strip().splitlines()[-1])
print('value', d['value'], 'ms/step', d['ms_per_step'], 'kernel', d['roofline']['avg_kernel_ms'], 'valu frac', d.get('roofline_valu', {}).get('frac'), 'faithful', d.get('faithful_sampling'))"
