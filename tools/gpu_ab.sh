#!/bin/bash
# A/B of two builds of the library on ONE box: tools/ab/libfnn_A.so (before) against tools/ab/libfnn_B.so (after), alternating
export TMPDIR=/tmp
export OUT=${OUT:-tool_out}
mkdir -p $OUT
for rep in 1 2 3; do
 for v in A B; do
  FNN_HIP_LIB=$PWD/tools/ab/libfnn_$v.so timeout -k 10 300 python bench.py --full ${AB_ARGS:---no-extras --no-cpu-baseline --steps 400} > $OUT/ab_$v.json 2> $OUT/ab_$v.err
  python - <<PY
import json
d = json.loads(open('$OUT/ab_$v.json').read().strip().splitlines()[-1])
print('$v rep $rep', 'ms/step %.4f' % d['ms_per_step'], {k: round(v * 1e3, 1) for k, v in d['kernel_ms'].items() if v and k != 'sort_now'})
PY
 done
done
