"""Time per example of FM / LR pre-training on the reference's online schedule (fm_train_online: batch-1 SGD steps in line order,
one persistent workgroup) against the same schedule run as fm_train_step calls at B = 1, at the iPinYou shape: 16 fields,
937,670 rows, Zipf ids (synth), N = 65,536 lines.  Rank 10 (FM), rank 0 (LR) and rank 100.  Writes profiles/fm_online_bench.json.

  python tools/fm_online_bench.py [--n 65536 --repeats 5 --loop-n 4096] [--ranks 10,0,100] [--out profiles/fm_online_bench.json]
  python tools/fm_online_bench.py --loop-only RANK [--loop-n 500]      (nothing but B = 1 steps: the run to put under
                                                                        `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`)
  python tools/fm_online_bench.py ... --stats RANK=DIR ..              (adds the device time of one B = 1 step's launches from
                                                                        that run's kernel_stats.csv)

What is timed, per rank, in one process, the variants alternating inside every repeat after a warm-up of each:
  online  the whole call on N lines between two device events on the handle's stream (median and min-max over the repeats);
  loop    --loop-n fm_train_step calls at B = 1, a host clock around the loop ending in fm_sync: this INCLUDES the Python /
          ctypes call overhead of every step, and is labelled so.  The device time of a step's launches alone comes from --stats.
One workgroup on a 256-CU part runs the online call: its rate is a latency figure, not a share of any roofline.

Checked at this size before anything is timed: on the first --loop-n lines the table and b after the online call and after the
loop, each against a float64 replay of the schedule (lazy decay, so only touched rows are computed), under the rule of
tests/test_gpu_fm_online.py: err_online <= 2 * err_loop + 2e-7."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16
LR, LAM = 1e-3, {0: 1e-3}          # python/ipinyou.py:133 / :139-140: LR lambda 1e-3, FM lambda 1e-2
FORMS = ('plain',)                  # the forms of the online kernel the library ships


def lam_of(rank):
    return LAM.get(rank, 1e-2)


def replay64(rows, b, ids, y, lr, lam):
    """The online schedule in float64 with the dense decay kept lazy per row: (rows, b) after the lines."""
    val = rows.astype(np.float64)
    last = np.zeros(len(rows), np.int64)
    dec = 1.0 - lr * lam
    for n in range(len(y)):
        live = ids[n][ids[n] >= 0]
        u = np.unique(live)
        val[u] *= (dec ** (n - last[u]))[:, None]
        last[u] = n
        e = val[live]
        S = e[:, 1:].sum(axis=0)
        z = b + e[:, 0].sum() + 0.5 * ((S * S).sum() - (e[:, 1:] * e[:, 1:]).sum())
        delta = 1.0 / (1.0 + np.exp(-z)) - y[n]
        g = np.empty_like(e)
        g[:, 0] = delta
        g[:, 1:] = delta * (S[None, :] - e[:, 1:])
        val[u] *= dec
        last[u] = n + 1
        np.subtract.at(val, live, lr * g)
        b = b * dec - lr * delta
    val *= (dec ** (len(y) - last))[:, None]
    return val, b


def make(lib, stream, K, D, rows, max_batch=1, shared=False):
    h = C.c_void_p()
    if lib.fm_create(F, K, max_batch, 0, C.c_void_p(stream.cuda_stream), C.byref(h)) != 0:
        raise RuntimeError((lib.fm_last_error(None) or b'').decode())
    for rc in (lib.fm_set_table(h, rows.ctypes.data, D), lib.fm_set_b(h, 0.0), lib.fm_set_shared_rows(h, 1 if shared else 0)):
        if rc != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())
    return h


def ck(lib, h, rc):
    if rc != 0:
        raise RuntimeError(lib.fm_last_error(h).decode())


def params(lib, h, D, K):
    rows, b = np.empty((D, K), np.float32), C.c_float()
    ck(lib, h, lib.fm_get_table(h, rows.ctypes.data))
    ck(lib, h, lib.fm_get_b(h, C.byref(b)))
    return rows, float(b.value)


def loop_steps(lib, h, ids, y, n, lr, lam):
    for i in range(n):
        rc = lib.fm_train_step(h, ids.data_ptr() + i * F * 4, y.data_ptr() + i * 4, 1, lr, lam, 1, None, None)
        if rc != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())
    ck(lib, h, lib.fm_sync(h))


def data(N):
    sys.path.insert(0, ROOT)
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    ids = synth.zipf_ids(N, sizes, 1.1, 99).astype(np.int32)
    y = (np.random.RandomState(3).uniform(size=N) < 0.02).astype(np.float32)
    return synth, sum(sizes), ids, y


def spread(v):
    v = sorted(v)
    return {'median': float(np.median(v)), 'min': v[0], 'max': v[-1]}


def run(ranks, N, repeats, loop_n):
    import torch
    synth, D, ids_h, y_h = data(N)
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids, y = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev)
    torch.cuda.synchronize()
    out = {}
    for rank in ranks:
        K, lam = rank + 1, lam_of(rank)
        rows = synth.fm_table(D, K, 0.01, 77)
        # parity on the prefix, each against the float64 replay
        h_on, h_loop = make(lib, stream, K, D, rows), make(lib, stream, K, D, rows)
        ck(lib, h_on, lib.fm_train_online(h_on, ids.data_ptr(), None, y.data_ptr(), loop_n, LR, lam, None, None, None))
        loop_steps(lib, h_loop, ids, y, loop_n, LR, lam)
        ref_rows, ref_b = replay64(rows, 0.0, ids_h[:loop_n], y_h[:loop_n].astype(np.float64), LR, lam)
        errs = {}
        for name, h in (('online', h_on), ('loop', h_loop)):
            got, gb = params(lib, h, D, K)
            errs[name] = float(max(np.abs(got - ref_rows).max(), abs(gb - ref_b)))
        ok = errs['online'] <= 2 * errs['loop'] + 2e-7
        # timing: the variants alternate inside every repeat
        form = lib.fm_online_form(h_on).decode()
        t_on, t_loop = [], []
        for rep in range(repeats + 1):                              # repeat 0 warms both up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ck(lib, h_on, lib.fm_train_online(h_on, ids.data_ptr(), None, y.data_ptr(), N, LR, lam, None, None, None))
            e1.record(stream)
            ck(lib, h_on, lib.fm_sync(h_on))
            t0 = time.perf_counter()
            loop_steps(lib, h_loop, ids, y, loop_n, LR, lam)
            dt = time.perf_counter() - t0
            if rep:
                t_on.append(e0.elapsed_time(e1) * 1e3 / N)
                t_loop.append(dt * 1e6 / loop_n)
        lib.fm_destroy(h_on), lib.fm_destroy(h_loop)
        out['rank_%d' % rank] = {
            'k': K, 'lambda': lam,
            'online_us_per_example': {form: spread(t_on)},
            'loop_b1_us_per_example_host_clock_incl_python_call_overhead': spread(t_loop),
            'prefix_parity': {'lines': loop_n, 'err_online': errs['online'], 'err_loop': errs['loop'],
                              'rule': 'err_online <= 2 * err_loop + 2e-7', 'holds': bool(ok)}}
    return {'tool': 'fm_online_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'lines': N, 'lr': LR,
            'repeats': repeats, 'loop_lines': loop_n, 'forms': list(FORMS),
            'occupancy': 'the online call is ONE workgroup of 256 threads on a 256-CU part: a latency figure, not a share of any roofline',
            'ranks': out}


def loop_only(rank, loop_n):
    import torch
    synth, D, ids_h, y_h = data(loop_n)
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids, y = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev)
    h = make(lib, stream, rank + 1, D, synth.fm_table(D, rank + 1, 0.01, 77))
    loop_steps(lib, h, ids, y, loop_n, LR, lam_of(rank))
    lib.fm_destroy(h)
    print(json.dumps({'tool': 'fm_online_bench', 'loop_only': rank, 'steps': loop_n}))


def step_stats(d):
    """The launches of the B = 1 steps in a rocprofv3 --kernel-trace --stats run: device microseconds per step, by kernel."""
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel_stats.csv under %s' % d)
    kern = {}
    for row in csv.DictReader(open(files[0])):
        name = row['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        if any(s in name for s in ('k_fm', 'k_scat', 'k_sort', 'sort')) and 'k_pack' not in name and 'k_unpack' not in name:
            c, us = kern.get(name, (0, 0.0))
            kern[name] = (c + int(row['Calls']), us + int(row['Calls']) * float(row['AverageNs']) / 1e3)
    steps = max(c for c, _ in kern.values())
    per = {k: round(us / steps, 3) for k, (c, us) in kern.items() if c >= steps}
    return {'steps': steps, 'launches_us_per_step': per, 'device_us_per_step': round(sum(per.values()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--loop-n', type=int, default=4096)
    ap.add_argument('--ranks', default='10,0,100')
    ap.add_argument('--loop-only', type=int, default=None)
    ap.add_argument('--stats', nargs='+', default=[])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fm_online_bench.json'))
    a = ap.parse_args()
    if a.loop_only is not None:
        loop_only(a.loop_only, a.loop_n)
        return
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    res = run([int(r) for r in a.ranks.split(',')], a.n, a.repeats, a.loop_n)
    for pr in a.stats:
        rank, d = pr.split('=', 1)
        r = res['ranks']['rank_%d' % int(rank)]
        r['loop_b1_device'] = step_stats(d)
        on = r['online_us_per_example'][FORMS[0]]
        r['online_vs_b1_device_time'] = {'ratio_at_medians': r['loop_b1_device']['device_us_per_step'] / on['median'],
                                         'ratio_at_online_max': r['loop_b1_device']['device_us_per_step'] / on['max']}
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
