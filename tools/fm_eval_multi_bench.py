"""What evaluating several FM / LR models on one test feed costs in one call (fm_eval_multi) against the loop of single-model
evaluations it replaces (fm_eval_w per handle), at the iPinYou shape of tools/fm_online_bench.py: 16 fields, 937,670 rows, Zipf
ids, rank 10, and the mixed group {LR, FM10, FM50, FM100}.  Writes profiles/fm_eval_multi_bench.json.

  python tools/fm_eval_multi_bench.py [--n 100000,1000000] [--models 1,16,256] [--repeats 5] [--e2e-lines 20000] [--out FILE]

One process; the feed (ids, y) is resident on the device; handles are created with max_batch = 4,096, the chunk of fm_eval_w.
Per (N, group): after one warm-up of each, the loop and the call ALTERNATE inside every repeat.  Two clocks around each:
  wall  -- time.perf_counter around the synchronised call(s): the host allocations, launches and synchronisations are the point;
  device -- between two events on the handles' stream (all handles share one stream here: the events need one).
Median and min-max over the repeats.  `faster_by_more_than_the_spread`: loop median - call median exceeds max - min of either.
Also: both calls' results compared as bits; the prediction stage alone (fm_predict_multi, no stores) as gathered row bytes per
second against the HBM peak; the two grid orders of that stage (FM_EVAL_ORDER=tile | model) alternating.
End to end (--e2e-lines > 0): ipinyou.run_many on a synthetic yzx file, the evaluation through FM.evaluate_many against the same
driver with the evaluation replaced by the per-model `evaluate` loop the driver ran before (ipinyou._eval_auc per model), and the
share of either that is the Python parse of the test file (ipinyou._load_eval), which neither touches."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_online_bench as ob  # noqa: E402

F = ob.F
MIXED = (0, 10, 50, 100)
HBM_PEAK = 8.0e12                                                   # bytes per second, MI355X


def loop_eval(lib, hs, ids, y, n):
    out = []
    for h in hs:
        v = [C.c_double() for _ in range(3)]
        ob.ck(lib, h, lib.fm_eval_w(h, ids.data_ptr(), None, y.data_ptr(), n, *[C.byref(x) for x in v]))
        out.append(tuple(x.value for x in v))
    return out


def multi_eval(lib, hs, ids, y, n):
    M = len(hs)
    arr = (C.c_void_p * M)(*[h.value for h in hs])
    a, r, l = (C.c_double * M)(), (C.c_double * M)(), (C.c_double * M)()
    ob.ck(lib, hs[0], lib.fm_eval_multi(arr, M, ids.data_ptr(), None, y.data_ptr(), n, a, r, l, None))
    return [(a[i], r[i], l[i]) for i in range(M)]


def multi_predict(lib, hs, ids, n):
    M = len(hs)
    arr, p = (C.c_void_p * M)(*[h.value for h in hs]), (C.c_void_p * M)()         # null entries: the gather alone, nothing stored
    ob.ck(lib, hs[0], lib.fm_predict_multi(arr, M, ids.data_ptr(), None, n, p))


def clocks(torch, stream, fn):
    """(wall microseconds, device microseconds, fn's value); fn ends synchronised or the wall clock waits for the stream."""
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
    return {name: {'wall_us': ob.spread(w), 'device_us': ob.spread(d)} for name, (w, d) in t.items()}, last


def beyond_spread(slow, fast):
    s = lambda v: v['max'] - v['min']
    return bool(slow['median'] - fast['median'] > max(s(slow), s(fast)))


def bits(v):
    return np.asarray(v, np.float64).tobytes()


def run(Ns, Ms, repeats):
    import torch
    synth, D, ids_h, y_h = ob.data(max(Ns))
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids = torch.as_tensor(ids_h).to(dev).contiguous()
    y = torch.as_tensor((y_h != 0).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    tables = {r: synth.fm_table(D, r + 1, 0.01, 77) for r in MIXED}
    hs = [ob.make(lib, stream, 11, D, tables[10], max_batch=4096) for _ in range(max(Ms))]
    mixed = [ob.make(lib, stream, r + 1, D, tables[r], max_batch=4096) for r in MIXED]
    groups = [('M_%d' % m, hs[:m]) for m in Ms] + [('mixed_LR_FM10_FM50_FM100', mixed)]
    res = {'tool': 'fm_eval_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'rank': 10,
           'repeats': repeats, 'max_batch': 4096, 'hbm_peak_bytes_per_s': HBM_PEAK,
           'timing': 'microseconds; wall = perf_counter around the synchronised call(s), device = between events on the stream; '
                     'median / min / max over the repeats, the variants alternating inside every repeat after a warm-up of each',
           'not_measured': ['more than %d models' % max(Ms), 'models on distinct streams (every handle here shares one stream)'],
           'points': {}}
    for N in Ns:
        present = int((ids_h[:N] >= 0).sum())
        for name, group in groups:
            M = len(group)
            t, last = alternate(torch, stream, repeats, {'loop_of_fm_eval_w': lambda: loop_eval(lib, group, ids, y, N),
                                                         'fm_eval_multi': lambda: multi_eval(lib, group, ids, y, N)})
            pt = dict(t)
            pt['models'], pt['lines'] = M, N
            pt['results_bit_identical'] = bits(last['loop_of_fm_eval_w']) == bits(last['fm_eval_multi'])
            for clock in ('wall_us', 'device_us'):
                pt['ratio_loop_to_call_at_medians_' + clock] = t['loop_of_fm_eval_w'][clock]['median'] / t['fm_eval_multi'][clock]['median']
                pt['faster_by_more_than_the_spread_' + clock] = beyond_spread(t['loop_of_fm_eval_w'][clock], t['fm_eval_multi'][clock])
            # the prediction stage alone, both grid orders alternating
            orders = {}
            for order in ('tile', 'model'):
                def call(order=order):
                    os.environ['FM_EVAL_ORDER'] = order
                    multi_predict(lib, group, ids, N)
                orders[order] = call
            to, _ = alternate(torch, stream, repeats, orders)
            os.environ.pop('FM_EVAL_ORDER', None)
            pt['predict_stage_device_us_by_grid_order'] = {k: v['device_us'] for k, v in to.items()}
            if name.startswith('M_'):                                # narrow rows: 64 bytes a present field
                by = float(M) * present * 64
                pt['gathered_row_bytes'] = by
                pt['gathered_row_bytes_per_s_at_median'] = {k: by / (v['device_us']['median'] * 1e-6) for k, v in to.items()}
                pt['share_of_hbm_peak'] = {k: v / HBM_PEAK for k, v in pt['gathered_row_bytes_per_s_at_median'].items()}
            res['points']['N_%d_%s' % (N, name)] = pt
            print('N %d %s: wall loop %.0f us, call %.0f us; device loop %.0f us, call %.0f us' % (
                N, name, t['loop_of_fm_eval_w']['wall_us']['median'], t['fm_eval_multi']['wall_us']['median'],
                t['loop_of_fm_eval_w']['device_us']['median'], t['fm_eval_multi']['device_us']['median']), flush=True)
    for h in hs + mixed:
        lib.fm_destroy(h)
    return res


def end_to_end(n_train, n_test, n_models, repeats):
    """run_many on a synthetic yzx pair, evaluate_many against the per-model evaluate loop, alternating."""
    sys.path.insert(0, ROOT)
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import ipinyou, synth
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    ids = synth.zipf_ids(n_train + n_test, sizes, 1.1, 5)
    y = (np.random.RandomState(6).uniform(size=n_train + n_test) < 0.05).astype(np.int32)
    d = tempfile.mkdtemp()
    train, test = os.path.join(d, 'train.yzx.txt'), os.path.join(d, 'test.yzx.txt')
    synth.write_yzx(train, ids[:n_train], y[:n_train])
    synth.write_yzx(test, ids[n_train:], y[n_train:])
    specs = [('FM', 10, 1e-3 * (1 + i % 4), 1e-2 / (1 + i // 4)) for i in range(n_models)]
    new_aucs, load = ipinyou._eval_aucs, ipinyou._load_eval
    spent = {'parse': 0.0}

    def timed_load(*a):
        t0 = time.perf_counter()
        v = load(*a)
        spent['parse'] += time.perf_counter() - t0
        return v
    ipinyou._load_eval = timed_load
    out = {'train_lines': n_train, 'test_lines': n_test, 'models': n_models, 'buffer': 10000, 'seconds': {}}
    variants = {'evaluate_many': new_aucs, 'per_model_evaluate_loop': lambda models, t: [ipinyou._eval_auc(m, t) for m in models]}
    t = {k: ([], []) for k in variants}
    logs = {}
    for rep in range(repeats + 1):
        for name, fn in variants.items():
            ipinyou._eval_aucs = fn
            spent['parse'] = 0.0
            np.random.seed(7)
            t0 = time.perf_counter()
            r = ipinyou.run_many(train, test, specs, buffer=10000, eval_size=100000, echo=False)
            dt = time.perf_counter() - t0
            logs[name] = [m['log'] for m in r]
            for m in r:
                m['model'].close()
            if rep:
                t[name][0].append(dt), t[name][1].append(spent['parse'])
    ipinyou._eval_aucs, ipinyou._load_eval = new_aucs, load
    for name, (tot, parse) in t.items():
        out['seconds'][name] = {'run_many': ob.spread(tot), 'of_which_parsing_the_test_file': ob.spread(parse)}
    out['logs_identical'] = logs['evaluate_many'] == logs['per_model_evaluate_loop']
    for f in (train, test):
        os.remove(f)
    os.rmdir(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='100000,1000000')
    ap.add_argument('--models', default='1,16,256')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--e2e-lines', type=int, default=20000)
    ap.add_argument('--e2e-test-lines', type=int, default=50000)
    ap.add_argument('--e2e-models', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fm_eval_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    res = run([int(v) for v in a.n.split(',')], [int(v) for v in a.models.split(',')], a.repeats)
    if a.e2e_lines > 0:
        res['end_to_end_run_many'] = end_to_end(a.e2e_lines, a.e2e_test_lines, a.e2e_models, 3)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
