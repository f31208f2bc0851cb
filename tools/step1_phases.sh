#!/bin/bash
# per-phase s_memtime stamps of the strip kernel (k_step1) on the bench's ids, the generic and the fixed training instance of the
# bf16 step one after the other -> $OUT/step1_phases.json, $OUT/step1_phases_fixed.json
# (copy to profiles/rNN_step1_phases.json: bench.py quotes the in-step gather figure from the newest).  Diagnostic build.
# "head_us_median": the stretch from P2's last MFMA to P3's first in finer intervals.  The fixed instance with the generic
# form's head: build tools/exp/mlp_stamps.hip with -DFNN_HEAD_DPP=0 -DFNN_HEAD_ONE_TRIP=0 (either alone: that part alone).
set -e
export OUT=${OUT:-tool_out}
mkdir -p $OUT
python3 - <<'PY'
import os
import sys; sys.path.insert(0, '.')
import deep_ctr_amd  # noqa
from deep_ctr_amd import synth
ids = synth.zipf_ids(32 * 4096, synth.field_sizes_ipinyou(), 1.1, 1234)[:4096]
ids.astype('int32').tofile(os.path.join(os.environ['OUT'], 'zipf_ids.bin'))
PY
BIN=tools/exp/mlp_stamps.bin          # (kept out of git; rebuilt when a source is newer)
if [ ! -x $BIN ] || [ tools/exp/mlp_stamps.hip -nt $BIN ] || [ deep-ctr_amd/csrc/fnn_kernels.hip.h -nt $BIN ]; then
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -o $BIN tools/exp/mlp_stamps.hip
fi
timeout -k 10 120 $BIN generic | tee $OUT/step1_phases.txt
timeout -k 10 120 $BIN fixed | tee $OUT/step1_phases_fixed.txt
cat $OUT/step1_phases.json $OUT/step1_phases_fixed.json
