"""The solo inner-product step at the reference's 39 columns on the strip kernels against the GEMM path it ran before
(IPNN_STRIP_L0=0: one GEMM launch per product, what every build before the two tile widths ran above 32 fields), in ONE build and
ONE process: FNN_IP_L3 (400 / 400 / 200) and FNN_IP_L7 (1000 / .. / 50), bf16 and f32, relu, keep_prob 0.5, drawn masks, on the
iPinYou table dealt to --fields fields (937,670 rows, k = 11).  Writes profiles/ipnn_fields_strips_solo.json.

  python tools/ipnn_fields_strips_bench.py [--fields 39] [--archs L3,L7] [--batches 10,100,4096] [--repeats 5] [--steps 20] [--out FILE]

The knob is read when a handle is created, so the two handles of a point are made under the two settings and then take turns:
after one warm-up of each, `strips` and `gemm` ALTERNATE inside every repeat; a sample is --steps consecutive steps without a loss
read-back between two events on the handles' stream, divided by --steps.  Median and min-max over the repeats, microseconds per
step.  `beyond_spread`: the medians differ by more than max - min of either.  Every handle's plan (ipnn.plan_query under its
setting) stands beside its point, and both are synchronised afterwards (`sync_errors`)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_online_bench as ob  # noqa: E402
from fm_eval_multi_bench import beyond_spread, clocks  # noqa: E402

K = 11
STACKS = {'L3': [400, 400, 200], 'L7': [1000, 800, 600, 400, 200, 100, 50]}
FORMS = {'strips': None, 'gemm': '0'}                         # IPNN_STRIP_L0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=39)
    ap.add_argument('--archs', default='L3,L7')
    ap.add_argument('--batches', default='10,100,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ipnn_fields_strips_solo.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    F = ob.F = a.fields
    import torch
    synth, D, ids_h, y_h = ob.data(a.steps * 4096)
    from deep_ctr_amd import ipnn
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids_all = torch.as_tensor(ids_h).to(dev).contiguous()
    y_all = torch.as_tensor(np.asarray(y_h, np.float32)).to(dev).contiguous()
    table = synth.fm_table(D, K, 0.01, 77)
    torch.cuda.synchronize()
    res = {'tool': 'ipnn_fields_strips_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'k': K, 'stacks': STACKS,
           'repeats': a.repeats, 'steps_per_sample': a.steps,
           'timing': 'microseconds per step between events on the stream; median / min / max over the repeats, the two forms alternating '
                     'inside every repeat after a warm-up of each; no loss read-back inside a sample',
           'not_measured': ['field counts other than %d' % F, 'value weights', 'the caller\'s masks', 'Adam and FTRL', 'another build of the library'],
           'points': {}}

    def save():
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')

    for arch in a.archs.split(','):
        hidden = STACKS[arch]
        d = [F * K + F * (F - 1) // 2 + 1] + hidden + [1]
        rng = np.random.RandomState(5)
        sc = [min(0.3, 1.5 / np.sqrt(d[i])) for i in range(len(d) - 1)]
        params = (table, 0.1, [rng.uniform(-sc[i], sc[i], (d[i], d[i + 1])).astype(np.float32) for i in range(len(d) - 1)],
                  [np.zeros(d[i + 1], np.float32) for i in range(len(d) - 1)])
        for prec in ('bf16', 'f32'):
            engs, plans = {}, {}
            for form, knob in FORMS.items():
                if knob is None:
                    os.environ.pop('IPNN_STRIP_L0', None)
                else:
                    os.environ['IPNN_STRIP_L0'] = knob
                engs[form] = ipnn.IPNNEngine(F, K, hidden, 'relu', max_batch=4096, precision=prec, lr=1e-4, keep_prob=0.5, stream=stream)
                engs[form].set_params(*params)
                q = engs[form].plan
                plans[form] = {k: q[k] for k in ('strips', 'pairs', 'cut', 'shares_step', 'lds_max', 'stack_fwd', 'stack_bwd', 'wide_fwd', 'tail_fused')}
            os.environ.pop('IPNN_STRIP_L0', None)
            assert plans['strips']['strips'] and not plans['gemm']['strips'], plans
            step0 = 0
            for B in [int(v) for v in a.batches.split(',')]:
                feed = [(ids_all[s * 4096:s * 4096 + B], y_all[s * 4096:s * 4096 + B]) for s in range(a.steps)]
                t = {form: [] for form in FORMS}
                for rep in range(a.repeats + 1):
                    for form, e in engs.items():
                        def steps(e=e):
                            for s, (ids, y) in enumerate(feed):
                                e._ck(e.lib.ipnn_train_step_drawn(e.h, ids.data_ptr(), None, y.data_ptr(), B, 100, step0 + s, None, None))
                        _, dt, _ = clocks(torch, stream, steps)
                        if rep:
                            t[form].append(dt / a.steps)
                    step0 += a.steps
                pt = {form: {'device_us': ob.spread(v), 'plan': plans[form]} for form, v in t.items()}
                s_, g_ = pt['strips']['device_us'], pt['gemm']['device_us']
                pt['ratio_gemm_to_strips_at_medians'] = g_['median'] / s_['median']
                pt['beyond_spread'] = beyond_spread(g_, s_) or beyond_spread(s_, g_)
                pt['sync_errors'] = []
                for form, e in engs.items():
                    try:
                        e.sync()
                    except Exception as ex:
                        pt['sync_errors'].append('%s: %s' % (form, ex))
                name = '%s_%s_B%d' % (arch, prec, B)
                res['points'][name] = pt
                save()
                print('%s: strips %.1f us [%.1f, %.1f], gemm %.1f us [%.1f, %.1f], gemm / strips %.2f%s' % (
                    name, s_['median'], s_['min'], s_['max'], g_['median'], g_['min'], g_['max'], pt['ratio_gemm_to_strips_at_medians'],
                    ''.join(' !! ' + x for x in pt['sync_errors'])), flush=True)
            for e in engs.values():
                e.close()
    save()


if __name__ == '__main__':
    main()
