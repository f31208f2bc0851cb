"""What evaluating several inner-product models on one feed costs in one call (ipnn_eval_multi) against the loop of single-model
evaluations it replaces (ipnn_eval_w per handle), on the iPinYou table: 16 fields, 937,670 rows, Zipf ids, k = 11, max_batch
4,096, at the reference's two stacks -- FNN_IP_L3 (400 / 400 / 200 relu, python/baseline.py:101) and FNN_IP_L7 (1000 / 800 / 600
/ 400 / 200 / 100 / 50 relu, :142).  Writes profiles/ipnn_eval_multi_bench.json.

  python tools/ipnn_eval_multi_bench.py [--shapes L3,L7] [--n 100000,1000000] [--models 1,4,16,64] [--repeats 5] [--out FILE]

One process; the feed (ids, y) is resident on the device; every engine has its own stream, as IPNNEngine makes them.  Per
(shape, N, group): after one warm-up of each, the loop and the call ALTERNATE inside every repeat; the clock is time.perf_counter
around the synchronised call(s) -- the host's launches, allocations and synchronisations are the point.  Median and min-max over
the repeats.  `faster_by_more_than_the_spread`: loop median - call median exceeds max - min of either.  Both sides' metrics are
compared as bits at every point.  The file is rewritten after every point, so that a run cut short keeps what it measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, K, BMAX = 16, 11, 4096
SHAPES = {'L3': [400, 400, 200], 'L7': [1000, 800, 600, 400, 200, 100, 50]}


def spread(v):
    v = sorted(v)
    return {'median': float(np.median(v)), 'min': v[0], 'max': v[-1]}


def beyond_spread(slow, fast):
    s = lambda v: v['max'] - v['min']                               # noqa: E731
    return bool(slow['median'] - fast['median'] > max(s(slow), s(fast)))


def ck(e, rc):
    if rc != 0:
        raise RuntimeError((e.lib.ipnn_last_error(e.h) or b'').decode())


def loop_eval(engs, ids, y, n):
    out = []
    for e in engs:
        v = [C.c_double() for _ in range(3)]
        ck(e, e.lib.ipnn_eval_w(e.h, ids.data_ptr(), None, y.data_ptr(), n, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])))
        out.append(tuple(x.value for x in v))
    return out


def multi_eval(engs, ids, y, n):
    M = len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    a, r, l = (C.c_double * M)(), (C.c_double * M)(), (C.c_double * M)()
    ck(engs[0], engs[0].lib.ipnn_eval_multi(hs, M, ids.data_ptr(), None, y.data_ptr(), n, a, r, l, None, None))
    return [(a[i], r[i], l[i]) for i in range(M)]


def alternate(torch, repeats, fns):
    """{name: wall microseconds} of the variants, alternating inside every repeat after one warm-up of each."""
    t = {name: [] for name in fns}
    last = {}
    for rep in range(repeats + 1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()                                       # both end synchronised
            dt = (time.perf_counter() - t0) * 1e6
            if rep:
                t[name].append(dt)
    return {name: {'wall_us': spread(v)} for name, v in t.items()}, last


def bits(v):
    return np.asarray(v, np.float64).tobytes()


def run(shapes, Ns, Ms, repeats, write):
    import torch
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    from deep_ctr_amd.ipnn import IPNNEngine
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    D = int(sum(sizes))
    ids_h = synth.zipf_ids(max(Ns), sizes, 1.1, 99).astype(np.int32)
    y_h = (np.random.RandomState(3).uniform(size=max(Ns)) < 0.02).astype(np.int32)
    dev = torch.device('cuda', 0)
    ids, y = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev)
    torch.cuda.synchronize()
    table = synth.fm_table(D, K, 0.01, 77)

    def make(hidden, prec, seed):
        e = IPNNEngine(F, K, hidden, 'relu', max_batch=BMAX, precision=prec, keep_prob=1.0)
        rng = np.random.RandomState(seed)
        Ws = [rng.uniform(-1.0, 1.0, (e.d[i], e.d[i + 1])) * min(0.3, 1.5 / np.sqrt(e.d[i])) for i in range(len(e.d) - 1)]
        e.set_params(table, 0.1, Ws, [rng.uniform(-0.1, 0.1, e.d[i + 1]) for i in range(len(e.d) - 1)])
        return e

    res = {'tool': 'ipnn_eval_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'k': K, 'shapes': SHAPES,
           'repeats': repeats, 'max_batch': BMAX,
           'timing': 'microseconds, perf_counter around the synchronised call(s); median / min / max over the repeats, the two '
                     'variants alternating inside every repeat after a warm-up of each',
           'not_measured': ['more than %d models' % max(Ms), 'field counts other than %d' % F, 'wide rows (k >= 17)', 'value weights',
                            'members off the strip kernels'],
           'points': {}}
    for shape in shapes:
        engs = {prec: [make(SHAPES[shape], prec, 100 + m) for m in range(max(Ms))] for prec in ('bf16', 'f32')}
        groups = [('%s_M_%d' % (prec, m), engs[prec][:m]) for prec in ('bf16', 'f32') for m in Ms]
        if max(Ms) >= 4:
            groups.append(('mixed_4_bf16_4_f32', engs['bf16'][:4] + engs['f32'][:4]))
        for N in Ns:
            for name, group in groups:
                t, last = alternate(torch, repeats, {'loop_of_ipnn_eval_w': lambda: loop_eval(group, ids, y, N),
                                                     'ipnn_eval_multi': lambda: multi_eval(group, ids, y, N)})
                pt = dict(t)
                pt['models'], pt['lines'], pt['shape'] = len(group), N, shape
                pt['results_bit_identical'] = bits(last['loop_of_ipnn_eval_w']) == bits(last['ipnn_eval_multi'])
                lo, ca = t['loop_of_ipnn_eval_w']['wall_us'], t['ipnn_eval_multi']['wall_us']
                pt['ratio_loop_to_call_at_medians'] = lo['median'] / ca['median']
                pt['faster_by_more_than_the_spread'] = beyond_spread(lo, ca)
                res['points']['%s_N_%d_%s' % (shape, N, name)] = pt
                write(res)
                print('%s N %d %s: loop %.0f us [%.0f, %.0f], call %.0f us [%.0f, %.0f], ratio %.2f, bits %s' % (
                    shape, N, name, lo['median'], lo['min'], lo['max'], ca['median'], ca['min'], ca['max'],
                    pt['ratio_loop_to_call_at_medians'], pt['results_bit_identical']), flush=True)
        for v in engs.values():
            for e in v:
                e.close()
    return res


def main():
    global F
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='L3,L7')
    ap.add_argument('--n', default='100000,1000000')
    ap.add_argument('--models', default='1,4,16,64')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--fields', type=int, default=F, help='fields of the feed and of every model (default 16; 39: the reference\'s columns)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ipnn_eval_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    F = a.fields

    def write(res):
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')

    res = run(a.shapes.split(','), [int(v) for v in a.n.split(',')], [int(v) for v in a.models.split(',')], a.repeats, write)
    write(res)


if __name__ == '__main__':
    main()
