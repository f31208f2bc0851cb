#!/bin/bash
# rocprofv3 kernel stats of the FNN step in the three precisions (headline leg only), and the default bench line
export TMPDIR=/tmp
export OUT=${OUT:-tool_out}
mkdir -p $OUT
step() { name=$1; secs=$2; shift 2; echo "== $name"; timeout -k 10 $secs "$@" > $OUT/$name.log 2> $OUT/$name.err; rc=$?; echo "   rc=$rc"; if [ $rc -ge 124 ]; then echo killed; exit $rc; fi; }
for prec in bf16 bf16x3 f32; do
  rm -rf $OUT/prof_$prec
  step prof_$prec 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$prec -o fnn -- python3 bench.py --precision $prec --steps 400 --warmup 20 --no-cpu-baseline --no-extras
  find $OUT/prof_$prec -name "*kernel_stats.csv" -exec cp {} $OUT/fnn_${prec}_kernel_stats.csv \;
  head -4 $OUT/fnn_${prec}_kernel_stats.csv | cut -c1-150
done
( time timeout -k 10 500 python bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err ) 2> $OUT/bench_default.time
tail -3 $OUT/bench_default.time
python - <<PY
import json
d = json.loads(open('$OUT/bench_default.log').read().strip().splitlines()[-1])
print('default: %.2f M ex/s' % (d['value'] / 1e6), 'f32 %.2f M' % (d['precision_f32']['value'] / 1e6), 'bf16x3 %.2f M' % (d['precision_bf16x3']['value'] / 1e6),
      {k: (v.get('value') if isinstance(v, dict) else v) for k, v in d['extra_workloads'].items()})
PY
