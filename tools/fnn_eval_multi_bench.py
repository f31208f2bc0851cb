"""What evaluating several FNN models on one feed costs in one call (fnn_eval_multi) against the loop of single-model evaluations
it replaces (fnn_eval per handle), at the iPinYou shape: 16 fields, 937,670 rows, Zipf ids, k = 11, hidden 300 / 100,
max_batch 4,096.  Writes profiles/fnn_eval_multi_bench.json.

  python tools/fnn_eval_multi_bench.py [--n 100000,1000000] [--models 1,4,16,64] [--repeats 5] [--e2e-specs 16] [--out FILE]

One process; the feed (ids, y) is resident on the device; every handle shares one stream (the device clock's events need one).
Per (N, group): after one warm-up of each, the loop and the call ALTERNATE inside every repeat.  Two clocks around each:
  wall   -- time.perf_counter around the synchronised call(s): the host's launches, allocations and synchronisations are the point;
  device -- between two events on the stream.
Median and min-max over the repeats.  `faster_by_more_than_the_spread`: loop median - call median exceeds max - min of either.
Both sides' metrics are compared as bits at every point.  The prediction stage alone (fnn_predict_multi) in its four forms --
FNN_EVAL_ORDER = tile | model times FNN_EVAL_LAUNCH = span | batch -- alternating the same way, their predictions compared as bits.
End to end (--e2e-specs > 0): FNN.run_many on tests/golden/demo with that many specs, against the same driver with
engine.evaluate_many / predict_many replaced by the per-engine loops the driver ran before."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, K, H1, H2, BMAX = 16, 11, 300, 100, 4096
DEV_MEM = 1                                                         # FNN_MEM_DEVICE


def spread(v):
    v = sorted(v)
    return {'median': float(np.median(v)), 'min': v[0], 'max': v[-1]}


def beyond_spread(slow, fast):
    s = lambda v: v['max'] - v['min']                               # noqa: E731
    return bool(slow['median'] - fast['median'] > max(s(slow), s(fast)))


def ck(e, rc):
    if rc != 0:
        raise RuntimeError((e.lib.fnn_last_error(e.h) or b'').decode())


def loop_eval(engs, ids, y, n):
    out = []
    for e in engs:
        v = [C.c_double() for _ in range(3)]
        ck(e, e.lib.fnn_eval(e.h, ids.data_ptr(), y.data_ptr(), n, DEV_MEM, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), None))
        out.append(tuple(x.value for x in v))
    return out


def multi_eval(engs, ids, y, n):
    M = len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    a, r, l = (C.c_double * M)(), (C.c_double * M)(), (C.c_double * M)()
    ck(engs[0], engs[0].lib.fnn_eval_multi(hs, M, ids.data_ptr(), y.data_ptr(), n, a, r, l, None, None))
    return [(a[i], r[i], l[i]) for i in range(M)]


def multi_predict(engs, ids, n, ps):
    M = len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    ck(engs[0], engs[0].lib.fnn_predict_multi(hs, M, ids.data_ptr(), n, (C.c_void_p * M)(*[p.data_ptr() for p in ps])))


def clocks(torch, stream, fn):
    """(wall microseconds, device microseconds, fn's value); the wall clock waits for the stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    v = fn()
    e1.record(stream)
    e1.synchronize()
    return (time.perf_counter() - t0) * 1e6, e0.elapsed_time(e1) * 1e3, v


def alternate(torch, stream, repeats, fns):
    """{name: {'wall_us', 'device_us'}} of the variants, alternating inside every repeat after one warm-up of each."""
    t = {name: ([], []) for name in fns}
    last = {}
    for rep in range(repeats + 1):
        for name, fn in fns.items():
            w, d, last[name] = clocks(torch, stream, fn)
            if rep:
                t[name][0].append(w), t[name][1].append(d)
    return {name: {'wall_us': spread(w), 'device_us': spread(d)} for name, (w, d) in t.items()}, last


def bits(v):
    return np.asarray(v, np.float64).tobytes()


def run(Ns, Ms, repeats):
    import torch
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    from deep_ctr_amd.engine import FNNEngine
    from oracle import fnn_oracle as orc
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    D = int(sum(sizes))
    ids_h = synth.zipf_ids(max(Ns), sizes, 1.1, 99).astype(np.int32)
    y_h = (np.random.RandomState(3).uniform(size=max(Ns)) < 0.02).astype(np.int32)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids, y = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev)
    torch.cuda.synchronize()
    rows, fo = synth.fm_table(D, K, 0.01, 77), synth.field_of_row(sizes)

    def make(prec, seed):
        e = FNNEngine(F, K, H1, H2, max_batch=BMAX, precision=prec, stream=stream)
        e.set_table(rows, fo, -3.0)
        p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=seed)
        p['w3'] = np.random.RandomState(seed).uniform(-0.2, 0.2, H2)
        e.set_dense(p)
        return e

    engs = {prec: [make(prec, 100 + m) for m in range(max(Ms))] for prec in ('bf16', 'f32')}
    groups = [('%s_M_%d' % (prec, m), engs[prec][:m]) for prec in ('bf16', 'f32') for m in Ms]
    groups.append(('mixed_4_bf16_4_f32', engs['bf16'][:4] + engs['f32'][:4]))
    res = {'tool': 'fnn_eval_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'k': K, 'hidden': [H1, H2],
           'repeats': repeats, 'max_batch': BMAX,
           'timing': 'microseconds; wall = perf_counter around the synchronised call(s), device = between events on the stream; '
                     'median / min / max over the repeats, the variants alternating inside every repeat after a warm-up of each',
           'not_measured': ['more than %d models' % max(Ms), 'models on distinct streams (every handle here shares one stream)'],
           'points': {}}
    forms = [(o, g) for o in ('tile', 'model') for g in ('span', 'batch')]
    for N in Ns:
        for name, group in groups:
            M = len(group)
            t, last = alternate(torch, stream, repeats, {'loop_of_fnn_eval': lambda: loop_eval(group, ids, y, N),
                                                         'fnn_eval_multi': lambda: multi_eval(group, ids, y, N)})
            pt = dict(t)
            pt['models'], pt['lines'] = M, N
            pt['results_bit_identical'] = bits(last['loop_of_fnn_eval']) == bits(last['fnn_eval_multi'])
            for clock in ('wall_us', 'device_us'):
                pt['ratio_loop_to_call_at_medians_' + clock] = t['loop_of_fnn_eval'][clock]['median'] / t['fnn_eval_multi'][clock]['median']
                pt['faster_by_more_than_the_spread_' + clock] = beyond_spread(t['loop_of_fnn_eval'][clock], t['fnn_eval_multi'][clock])
            # the prediction stage alone in its four forms
            ps = {f: [torch.empty(N, dtype=torch.float32, device=dev) for _ in group] for f in forms}
            calls = {}
            for f in forms:
                def call(f=f):
                    os.environ['FNN_EVAL_ORDER'], os.environ['FNN_EVAL_LAUNCH'] = f
                    multi_predict(group, ids, N, ps[f])
                calls['%s_%s' % f] = call
            tf, _ = alternate(torch, stream, repeats, calls)
            os.environ.pop('FNN_EVAL_ORDER', None), os.environ.pop('FNN_EVAL_LAUNCH', None)
            torch.cuda.synchronize()
            pt['predict_stage_by_order_and_launch'] = tf
            pt['predict_stage_forms_bit_identical'] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                          for f in forms[1:] for a, b in zip(ps[forms[0]], ps[f]))
            del ps
            res['points']['N_%d_%s' % (N, name)] = pt
            print('N %d %s: wall loop %.0f us, call %.0f us; device loop %.0f us, call %.0f us; predict stage device %s' % (
                N, name, t['loop_of_fnn_eval']['wall_us']['median'], t['fnn_eval_multi']['wall_us']['median'],
                t['loop_of_fnn_eval']['device_us']['median'], t['fnn_eval_multi']['device_us']['median'],
                {k: round(v['device_us']['median']) for k, v in tf.items()}), flush=True)
    for v in engs.values():
        for e in v:
            e.close()
    return res


def end_to_end(n_specs, repeats):
    """FNN.run_many on the demo set: the group evaluation against the per-engine loops the driver ran before, alternating."""
    from deep_ctr_amd import dl_utils, engine
    spec = importlib.util.spec_from_file_location('fnn_script_bench', os.path.join(ROOT, 'deep-ctr_amd', 'FNN.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    specs = ['%g:0.5:0:%g' % (1e-3 * (1 + i % 4), 0.1 / (1 + i // 4)) for i in range(n_specs)]
    group = (engine.evaluate_many, engine.predict_many)
    variants = {'evaluate_many_predict_many': group,
                'per_engine_loops': (lambda engs, ids, y, want_p=False: [e.evaluate(ids, y, want_p) for e in engs],
                                     lambda engs, ids: [e.predict(ids) for e in engs])}
    cwd = os.getcwd()
    os.environ['DEEPCTR_DATA_DIR'] = os.path.join(ROOT, 'tests', 'golden', 'demo')
    os.environ['DEEPCTR_EPOCHS'] = '2'
    t = {k: [] for k in variants}
    hists = {}
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        dl_utils.log_path = os.path.join(d, 'log')
        for rep in range(repeats + 1):
            for name, (ev, pr) in variants.items():
                engine.evaluate_many, engine.predict_many = ev, pr
                out = {}
                t0 = time.perf_counter()
                hists[name] = mod.run_many(['FNN.py', '2997'], specs, out)
                dt = time.perf_counter() - t0
                for e in out['engines']:
                    e.close()
                if rep:
                    t[name].append(dt)
        os.chdir(cwd)
    engine.evaluate_many, engine.predict_many = group
    return {'specs': n_specs, 'epochs': 2, 'seconds': {k: spread(v) for k, v in t.items()},
            'histories_identical': hists['evaluate_many_predict_many'] == hists['per_engine_loops']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='100000,1000000')
    ap.add_argument('--models', default='1,4,16,64')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--e2e-specs', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fnn_eval_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    def write(res):
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')

    res = run([int(v) for v in a.n.split(',')], [int(v) for v in a.models.split(',')], a.repeats)
    write(res)
    if a.e2e_specs > 0:
        res['end_to_end_run_many'] = end_to_end(a.e2e_specs, 3)
        write(res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
