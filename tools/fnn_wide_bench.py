"""Per-step time of the FNN step on wide FM rows (k = rank + 1 >= 17: the layer-by-layer path of fnn_api.hip with k_gather_wide
and the decayed wide row update k_scatdw1 / k_scatdw2) at the iPinYou shape (937,670 rows, 16 fields, batch 4096, hidden
300 / 100), in the three precisions, with the per-segment device times of fnn_prof_* and a FLOP / byte model of the step.
One JSON line on stdout.

  python tools/fnn_wide_bench.py [--steps 200 --warmup 20] [--only NAME,..] [--no-prof]
  python tools/fnn_wide_bench.py --only k101_bf16 --steps 20 --warmup 5 --no-prof    (the run to put under rocprofv3)

Configurations: k51_* / k101_* (the reference's FM50 / FM100 models feeding FNN, python/baseline.py:77-93) x f32 / bf16 / bf16x3.
The timed window and the profiled window are separate runs of the same steps: the profiling events sit between the launches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H1, H2 = 16, 300, 100
CONFIGS = {'k%d_%s' % (k, p): (k, p) for k in (51, 101) for p in ('f32', 'bf16', 'bf16x3')}
SEGMENTS = ('sort', 'gather', 'fwd1', 'fwd2', 'head', 'bwd1', 'gx', 'wgrad', 'reduce', 'scatter', 'finalize', 'update')
PEAK_TFLOPS = {'f32': 157.3, 'bf16': 2516.6, 'bf16x3': 2516.6 / 3}     # MI355X dense MFMA peaks; bf16x3 = three bf16 MFMAs
HBM_TBPS = 8.0


def rup(a, m):
    return (a + m - 1) // m * m


def model(B, K, prec):
    """The step's matrix FLOP and the HBM bytes its kernels must move, from the shapes.  FLOP: the three products of each of the
    two hidden layers (forward, the delta / gx product, the weight gradient) at the reference's sizes (1 + F k, H1, H2) and at
    the padded sizes the kernels run (K1p = rup(F rw + 2, 64), H1p = rup(H1 + 1, 64), H2p = rup(H2 + 1, 64)).  Bytes, per
    segment, each operand counted once (no cache reuse assumed, weights included): the gather reads B F rows of rw floats and
    writes x' in both layouts; fwd1 reads x'; gx writes gx' (f32); wgrad reads x'^T and writes the split-K slabs; the update
    reads the slabs and rewrites masters and shadows; the row update reads gx' at the rows' columns and reads and writes at
    most B F rows."""
    rw = rup(K, 4)
    xdim, K1p, H1p, H2p = 1 + F * K, rup(F * rw + 2, 64), rup(H1 + 1, 64), rup(H2 + 1, 64)
    ts = 2 if prec == 'bf16' else 4
    flop = 6.0 * B * (xdim * H1 + H1 * H2 + H2)
    flop_p = 6.0 * B * (K1p * H1p + H1p * H2p + H2p)
    n1 = K1p * H1p
    by = {
        'gather': B * F * rw * 4 + 2 * B * K1p * ts,
        'fwd1': B * K1p * ts + n1 * ts + B * H1p * ts * 3,
        'gx': B * H1p * ts + n1 * ts + B * K1p * 4,
        'wgrad': B * K1p * ts + 4 * n1 * 4,
        'reduce_update': 4 * n1 * 4 + n1 * 4 * 3 + 2 * n1 * ts,
        'scatter': B * F * rw * 4 + 2 * B * F * rw * 4,
    }
    return {'xdim': xdim, 'K1p': K1p, 'flop': flop, 'flop_padded': flop_p, 'bytes': by, 'bytes_total': sum(by.values())}


def run(names, steps, warmup, B, prof):
    sys.path.insert(0, ROOT)
    import torch
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    from deep_ctr_amd.engine import FNNEngine
    from oracle import fnn_oracle as orc
    sizes = synth.field_sizes_ipinyou()
    D = sum(sizes)
    fo = synth.field_of_row(sizes)
    NB = 8
    ids_h = synth.zipf_ids(NB * B, sizes, 1.1, 99)
    y_h = (np.random.RandomState(3).uniform(size=NB * B) < 0.02).astype(np.float32)
    out = {}
    for name in names:
        K, prec = CONFIGS[name]
        eng = FNNEngine(F, K, H1, H2, max_batch=B, precision=prec, lr=0.001, lambda1=0.0, lambda_fm=0.1)
        eng.set_table(synth.fm_table(D, K, 0.01, 77), fo, -3.0)
        eng.set_dense(orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234))
        ids, y = eng.to_device(ids_h, y_h.astype(np.int32))
        yf = y.float()
        m = (np.random.RandomState(5).uniform(size=(2, max(H1, H2))) < 0.5).astype(np.uint8)
        m1 = torch.as_tensor(m[0, :H1]).to(eng.device)
        m2 = torch.as_tensor(m[1, :H2]).to(eng.device)
        lib, h = eng.lib, eng.h

        def steps_(n):
            for i in range(n):
                j = i % NB
                rc = lib.fnn_train_step(h, ids.data_ptr() + j * B * F * 4, yf.data_ptr() + j * B * 4, B, m1.data_ptr(),
                                        m2.data_ptr(), 0, None, None, 1, None)
                eng._ck(rc)
        with torch.cuda.stream(eng.stream):
            steps_(warmup)
            eng.sync()
            t0 = time.perf_counter()
            steps_(steps)
            eng.sync()
            dt = (time.perf_counter() - t0) / steps
            r = {'k': K, 'precision': prec, 'us_per_step': dt * 1e6, 'examples_per_sec': B / dt}
            if prof:
                eng.prof_enable(True)
                eng.prof_reset()
                steps_(steps)
                eng.sync()
                seg = {s: eng.prof_get(s) for s in SEGMENTS}
                eng.prof_enable(False)
                r['segments_us'] = {s: round(v[0] * 1e3, 2) for s, v in seg.items() if v[1] > 0}
        eng.close()
        md = model(B, K, prec)
        t_mfma = md['flop_padded'] / (PEAK_TFLOPS[prec] * 1e12)
        t_hbm = md['bytes_total'] / (HBM_TBPS * 1e12)
        r['roofline'] = {'flop': md['flop'], 'flop_padded': md['flop_padded'], 'bytes': md['bytes_total'],
                         'bytes_by_segment': md['bytes'], 'K1p': md['K1p'],
                         't_mfma_us': t_mfma * 1e6, 't_hbm_us': t_hbm * 1e6,
                         'bound': 'mfma' if t_mfma > t_hbm else 'hbm',
                         'share_of_roofline': max(t_mfma, t_hbm) / dt,
                         'achieved_tflops': md['flop'] / dt / 1e12}
        out[name] = r
    import torch
    return {'tool': 'fnn_wide_bench', 'n_rows': D, 'fields': F, 'hidden': [H1, H2], 'batch': B, 'steps': steps,
            'warmup': warmup, 'device': torch.cuda.get_device_name(0), 'configs': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--only', default=','.join(CONFIGS))
    ap.add_argument('--no-prof', action='store_true')
    a = ap.parse_args()
    names = a.only.split(',')
    for n in names:
        if n not in CONFIGS:
            raise SystemExit('unknown config %r (%s)' % (n, ', '.join(CONFIGS)))
    print(json.dumps(run(names, a.steps, a.warmup, a.batch, not a.no_prof)))


if __name__ == '__main__':
    main()
