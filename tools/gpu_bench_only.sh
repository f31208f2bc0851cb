#!/bin/bash
# the full bench line (every leg) under the clock, then the end-to-end workload at its full size
export TMPDIR=/tmp
export OUT=${OUT:-tool_out}
mkdir -p $OUT
( time timeout -k 10 500 python bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err ) 2> $OUT/bench_default.time || { echo "default bench failed"; tail -5 $OUT/bench_default.err; exit 1; }
tail -4 $OUT/bench_default.time
timeout -k 10 400 python bench.py --workload e2e > $OUT/bench_e2e.log 2> $OUT/bench_e2e.err || { echo "e2e failed"; tail -5 $OUT/bench_e2e.err; exit 1; }
python - <<PY
import json
d = json.loads(open('$OUT/bench_default.log').read().strip().splitlines()[-1])
print('default: %.2f M ex/s' % (d['value'] / 1e6), {k: (v.get('value') if isinstance(v, dict) else v) for k, v in d['extra_workloads'].items()})
e = json.loads(open('$OUT/bench_e2e.log').read().strip().splitlines()[-1])
print('e2e:', e['value'], e.get('phases_s') or {k: v for k, v in e.items() if 'parse' in k or 'phase' in k})
PY
