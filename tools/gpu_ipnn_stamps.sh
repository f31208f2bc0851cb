#!/bin/bash
# per-product stamps of the wide strip kernels (IPNN_STAMPS=1) with the detail of one product's last block of wave 0 (IPNN_STAMP_SEL),
# then the tails (IPNN_STAMPS=2)
export TMPDIR=/tmp
export OUT=${OUT:-tool_out}
mkdir -p $OUT
: > $OUT/ipnn_stamps.txt
for sel in ${STAMP_SELS:-0 1 2 3}; do
  IPNN_STAMPS=1 IPNN_STAMP_SEL=$sel timeout -k 10 200 python bench.py --full --workload ipnn --steps 20 --warmup 5 --no-cpu-baseline > $OUT/ipnn_st.json 2> $OUT/ipnn_st.err || exit 1
  echo "== sel=$sel" >> $OUT/ipnn_stamps.txt; grep "ipnn stamps" $OUT/ipnn_st.err | tail -4 >> $OUT/ipnn_stamps.txt
done
IPNN_STAMPS=2 timeout -k 10 200 python bench.py --full --workload ipnn --steps 20 --warmup 5 --no-cpu-baseline > $OUT/ipnn_st.json 2> $OUT/ipnn_st.err || exit 1
echo "== tails" >> $OUT/ipnn_stamps.txt; grep "ipnn stamps" $OUT/ipnn_st.err | tail -2 >> $OUT/ipnn_stamps.txt
cat $OUT/ipnn_stamps.txt
