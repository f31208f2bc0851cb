#!/bin/bash
# FNN step: parity tests of the step, then the headline bench without the extra legs
export TMPDIR=/tmp
export OUT=${OUT:-tool_out}
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_dp.py tests/test_gpu_golden.py -m gpu -q --timeout 600 2>&1 | tail -3
timeout -k 10 300 python bench.py --full --no-extras --no-cpu-baseline --steps 400 > $OUT/fnn_quick.json 2> $OUT/fnn_quick.err
python - <<PY
import json
d = json.loads(open('$OUT/fnn_quick.json').read().strip().splitlines()[-1])
print('ms/step %.4f' % d['ms_per_step'], '%.2f M ex/s' % (d['value'] / 1e6), {k: round(v * 1e3, 1) for k, v in d['kernel_ms'].items() if v})
PY
