"""Time per example of the dense DAE pre-trainers (include/dae_hip.h) in one process on one GPU: the online trainers dae_dense_epoch_f64 /
dae_dense_epoch (unchanged: the baseline) against the mini-batch trainers dae_dense_batch_f64 / dae_dense_batch at M = 1, 20, 256, at the
reference's layer shapes 300 x 100 and 200 x 300.  Writes profiles/dae_batch_bench.json.

  python tools/dae_batch_bench.py [--n 40960 --repeats 7] [--out profiles/dae_batch_bench.json]

What is timed: one whole call on N examples (>= 20,000) between two device events on the stream the call runs on -- its scratch
allocation, launch and the copy-back of the cost included, as a caller pays them.  Every variant is warmed up once at its shape; then
the variants of a shape alternate inside every repeat, each from the same initial parameters.  Reported: microseconds per example and
examples per second as median and min .. max over the repeats.  The trainers are eight workgroups (f64 online, both mini-batch forms)
or one (f32 online) on a 256-CU part: latency figures of a dependence chain, not a share of any roofline.
The one condition fixed in advance: at M = 20, f64, 300 x 100 the mini-batch call must be faster per example than dae_dense_epoch_f64 by
more than the spread of either (slowest mini-batch repeat < fastest online repeat); `amortised` records whether it held."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((300, 100), (200, 300))
BATCHES = (1, 20, 256)
LR = 0.1


def spread(v):
    v = sorted(v)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1])}


def run(N, repeats):
    import torch
    sys.path.insert(0, ROOT)
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    shapes = {}
    for row, col in SHAPES:
        rng = np.random.RandomState(7 * row + col)
        b = 4 * np.sqrt(6. / (row + col))
        W0, X0 = rng.uniform(-b, b, (row, col)), rng.uniform(0.05, 0.95, (N, row))
        variants = []
        for f64 in (True, False):
            dt, sfx = (torch.float64, '_f64') if f64 else (torch.float32, '')
            W = torch.as_tensor(W0).to(device=dev, dtype=dt).contiguous()
            X = torch.as_tensor(X0).to(device=dev, dtype=dt).contiguous()
            state = dict(W=W, X=X, Wd=W.clone(), bh=torch.zeros(col, dtype=dt, device=dev), bv=torch.zeros(row, dtype=dt, device=dev))
            variants.append(('dae_dense_epoch' + sfx, None, state))
            variants += [('dae_dense_batch' + sfx, M, state) for M in BATCHES]

        def once(name, M, s):
            s['Wd'].copy_(s['W']); s['bh'].zero_(); s['bv'].zero_()
            cost = C.c_double()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if M is None:
                rc = getattr(lib, name)(s['Wd'].data_ptr(), s['bh'].data_ptr(), s['bv'].data_ptr(), s['X'].data_ptr(), N, row, col, LR, 0, C.byref(cost), st)
            else:
                rc = getattr(lib, name)(s['Wd'].data_ptr(), s['bh'].data_ptr(), s['bv'].data_ptr(), s['X'].data_ptr(), None, N, M, row, col, LR, 0,
                                        C.byref(cost), st)
            e1.record(stream)
            if rc != 0:
                raise RuntimeError((lib.dae_last_error() or b'').decode())
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) * 1e3 / N, cost.value

        times = {(n, M): [] for n, M, _ in variants}
        costs = {}
        for rep in range(repeats + 1):                              # repeat 0 warms every variant up at this shape
            for name, M, s in variants:
                us, c = once(name, M, s)
                if rep:
                    times[(name, M)].append(us)
                costs[(name, M)] = c
        res = {}
        for name, M, _ in variants:
            t = times[(name, M)]
            n_steps = N if M is None else (N + M - 1) // M
            res[name if M is None else '%s M=%d' % (name, M)] = {
                'us_per_example': spread(t), 'examples_per_s': spread([1e6 / x for x in t]),
                'mean_cost_per_step': costs[(name, M)] / n_steps}
        shapes['%dx%d' % (row, col)] = res
    on, bt = shapes['300x100']['dae_dense_epoch_f64']['us_per_example'], shapes['300x100']['dae_dense_batch_f64 M=20']['us_per_example']
    return {'tool': 'dae_batch_bench', 'device': torch.cuda.get_device_name(0), 'examples_per_timing': N, 'repeats': repeats, 'lr': LR,
            'timed': 'one whole call between two device events (scratch allocation, launch, cost copy-back included)',
            'occupancy': 'eight workgroups (one for dae_dense_epoch at these f32 shapes) on a 256-CU part: latency figures, not a share of any roofline',
            'shapes': shapes,
            'condition': {'what': 'M = 20, f64, 300 x 100: slowest dae_dense_batch_f64 repeat < fastest dae_dense_epoch_f64 repeat',
                          'online_us_per_example': on, 'batch_us_per_example': bt, 'amortised': bool(bt['max'] < on['min']),
                          'speedup_at_medians': on['median'] / bt['median']}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=40960)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dae_batch_bench.json'))
    a = ap.parse_args()
    if a.n < 20000 or a.repeats < 5:
        raise SystemExit('at least 20,000 examples per timing and five repeats')
    res = run(a.n, a.repeats)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
