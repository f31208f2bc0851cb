"""What one mini-batch step of several FM / LR models costs in one call (fm_train_step_multi) against the loop of solo steps it
replaces (fm_train_step_w per handle), at the iPinYou shape of tools/fm_online_bench.py: 16 fields, 937,670 rows, Zipf ids,
B = 4,096.  Writes profiles/fm_step_multi_bench.json.

  python tools/fm_step_multi_bench.py [--models 1,2,4,16,64,256] [--repeats 5] [--steps 8] [--parent-lib PATH/libfnn_hip.so] [--out FILE]

One process; the feed (--steps batches of ids, y) is resident on the device; every handle shares one stream (the events need one).
A point is a group of models: SGD rank 10 at M models, the mixed group {LR, FM10, FM50, FM100}, Adam rank 10 at M = 16, and
B = 100 at M = 16 (python/baseline.py's FM batch).  The loop runs on one set of handles and the call on a second set with the same
tables, both over the same batches in the same order, so that after the last repeat the two sets can be compared as bits
(`results_bit_identical`: b of every model, the whole table of the first and the last).  After one warm-up of each, the loop and
the call ALTERNATE inside every repeat (M = 1: the call forwards to the solo step); a sample is --steps consecutive steps without a
loss read-back, divided by --steps:
  wall   -- time.perf_counter around the steps and the stream's synchronisation;
  device -- between two events on the stream.
Median and min-max over the repeats, microseconds per step of the whole group.  `beyond_spread`: loop median - call median exceeds
max - min of either.  --parent-lib: the solo fm_train_step_w of this library against the same entry point of the library built
from the parent commit, alternating, with the verdict "this median inside the parent's min-max" on both clocks (left out, and said
so, without it)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_online_bench as ob  # noqa: E402
from fm_eval_multi_bench import beyond_spread, clocks  # noqa: E402
from fm_online_multi_bench import bind_parent  # noqa: E402

F = ob.F
MIXED = (0, 10, 50, 100)
LR = 1e-3


def set_adam(lib, h):
    ob.ck(lib, h, lib.fm_set_optimizer(h, 1, 0.9, 0.999, 1e-8))


def loop_steps(lib, hs, lams, feed, B):
    for ids, y in feed:
        for h, lam in zip(hs, lams):
            ob.ck(lib, h, lib.fm_train_step_w(h, ids.data_ptr(), None, y.data_ptr(), B, LR, lam, 1, None, None))


def multi_steps(lib, hs, lams, feed, B):
    M = len(hs)
    arr = (C.c_void_p * M)(*[h.value for h in hs])
    lr, lam, mean = (C.c_float * M)(*([LR] * M)), (C.c_float * M)(*lams), (C.c_int * M)(*([1] * M))
    for ids, y in feed:
        ob.ck(lib, hs[0], lib.fm_train_step_multi(arr, M, ids.data_ptr(), None, y.data_ptr(), B, lr, lam, mean, None, None))


def alternate(torch, stream, repeats, steps, fns):
    t = {name: ([], []) for name in fns}
    for rep in range(repeats + 1):
        for name, fn in fns.items():
            w, d, _ = clocks(torch, stream, fn)
            if rep:
                t[name][0].append(w / steps), t[name][1].append(d / steps)
    return {name: {'wall_us': ob.spread(w), 'device_us': ob.spread(d)} for name, (w, d) in t.items()}


def same_bits(lib, a, b, D, ks):
    ok = True
    for i, (x, z) in enumerate(zip(a, b)):
        bx, bz = C.c_float(), C.c_float()
        ob.ck(lib, x, lib.fm_get_b(x, C.byref(bx))), ob.ck(lib, z, lib.fm_get_b(z, C.byref(bz)))
        ok = ok and np.float32(bx.value).tobytes() == np.float32(bz.value).tobytes()
        if i in (0, len(a) - 1):
            rx, rz = ob.params(lib, x, D, ks[i])[0], ob.params(lib, z, D, ks[i])[0]
            ok = ok and bool(np.array_equal(rx.view(np.uint32), rz.view(np.uint32)))
    return bool(ok)


def run(Ms, repeats, steps, parent_lib):
    import torch
    synth, D, ids_h, y_h = ob.data(steps * 4096)
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids_all, y_all = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev).contiguous()
    torch.cuda.synchronize()

    def feed(B):
        return [(ids_all[s * 4096:s * 4096 + B], y_all[s * 4096:s * 4096 + B]) for s in range(steps)]
    tables = {r: synth.fm_table(D, r + 1, 0.01, 77) for r in MIXED}
    res = {'tool': 'fm_step_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'repeats': repeats,
           'steps_per_sample': steps, 'lr': LR,
           'timing': 'microseconds per step of the whole group; wall = perf_counter around the steps and the synchronisation, device '
                     '= between events on the stream; median / min / max over the repeats, the loop and the call alternating inside '
                     'every repeat after a warm-up of each; no loss read-back inside a sample',
           'not_measured': ['more than %d models' % max(Ms), 'models on distinct streams (every handle here shares one stream)',
                            'wide-only groups'],
           'points': {}}

    def point(name, ranks, B, adam=False):
        M = len(ranks)
        sets = [[ob.make(lib, stream, r + 1, D, tables[r], max_batch=4096) for r in ranks] for _ in range(2)]
        if adam:
            for h in sets[0] + sets[1]:
                set_adam(lib, h)
        lams = [ob.lam_of(r) for r in ranks]
        fd = feed(B)
        t = alternate(torch, stream, repeats, steps, {'loop_of_fm_train_step_w': lambda: loop_steps(lib, sets[0], lams, fd, B),
                                                      'fm_train_step_multi': lambda: multi_steps(lib, sets[1], lams, fd, B)})
        pt = dict(t)
        pt['models'], pt['batch'], pt['optimizer'] = M, B, 'adam' if adam else 'sgd'
        pt['results_bit_identical'] = same_bits(lib, sets[0], sets[1], D, [r + 1 for r in ranks])
        for clock in ('wall_us', 'device_us'):
            lo, ca = t['loop_of_fm_train_step_w'][clock], t['fm_train_step_multi'][clock]
            pt['ratio_loop_to_call_at_medians_' + clock] = lo['median'] / ca['median']
            pt['beyond_spread_' + clock] = beyond_spread(lo, ca)
            pt['call_median_inside_loop_spread_' + clock] = bool(lo['min'] <= ca['median'] <= lo['max'])
            pt['examples_per_s_at_call_median_' + clock] = M * B / (ca['median'] * 1e-6)
        res['points'][name] = pt
        print('%s: device loop %.1f us, call %.1f us; wall loop %.1f us, call %.1f us; bits %s' % (
            name, t['loop_of_fm_train_step_w']['device_us']['median'], t['fm_train_step_multi']['device_us']['median'],
            t['loop_of_fm_train_step_w']['wall_us']['median'], t['fm_train_step_multi']['wall_us']['median'],
            pt['results_bit_identical']), flush=True)
        for h in sets[0] + sets[1]:
            lib.fm_destroy(h)

    for m in Ms:
        point('sgd_rank10_B4096_M_%d' % m, [10] * m, 4096)
    point('mixed_LR_FM10_FM50_FM100_B4096', list(MIXED), 4096)
    point('adam_rank10_B4096_M_16', [10] * 16, 4096, adam=True)
    point('sgd_rank10_B100_M_16', [10] * 16, 100)

    if parent_lib:
        par = bind_parent(parent_lib)
        h_n, h_p = ob.make(lib, stream, 11, D, tables[10], max_batch=4096), ob.make(par, stream, 11, D, tables[10], max_batch=4096)
        fd = feed(4096)
        t = alternate(torch, stream, repeats, steps, {'parent': lambda: loop_steps(par, [h_p], [1e-2], fd, 4096),
                                                      'this': lambda: loop_steps(lib, [h_n], [1e-2], fd, 4096)})
        (rp, bp), (rn, bn) = ob.params(par, h_p, D, 11), ob.params(lib, h_n, D, 11)
        for clock in ('device_us', 'wall_us'):                     # the wall clock is the one a host-side change can move
            t['this_median_inside_parent_spread_' + clock] = bool(
                t['parent'][clock]['min'] <= t['this'][clock]['median'] <= t['parent'][clock]['max'])
        t['results_bit_identical'] = bool(bp == bn and np.array_equal(rp.view(np.uint32), rn.view(np.uint32)))
        res['solo_fm_train_step_w_against_parent_library'] = t
        par.fm_destroy(h_p), lib.fm_destroy(h_n)
    else:
        res['solo_fm_train_step_w_against_parent_library'] = 'not measured: no --parent-lib given'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='1,2,4,16,64,256')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fm_step_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    res = run([int(v) for v in a.models.split(',')], a.repeats, a.steps, a.parent_lib)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
