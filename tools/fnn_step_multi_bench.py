"""What one FNN mini-batch step of several models costs in ONE call (fnn_train_step_multi with next_ids) against the loop it
replaces (fnn_prefetch_ids + fnn_train_step per handle), at the headline shape: 16 fields, 937,670 rows, k = 11, hidden 300 / 100,
Zipf ids.  Writes profiles/fnn_step_multi_bench.json.

  python tools/fnn_step_multi_bench.py [--models 1,2,4,16,64] [--batches 100,4096] [--repeats 5] [--steps 8] [--out FILE]

One process; the feed (--steps batches of ids, y) is resident on the device; every handle shares one stream (the events need
one).  A point is (precision, B, M), plus one mixed group of bf16 and f32 handles at each B.  The loop runs on one set of handles
and the call on a second set with the same parameters (model m: its own lr, lambda_fm and masks), both over the same batches in
the same order, so that after the last repeat the two sets can be compared as bits (`results_bit_identical`: every dense tensor of
every model, the whole table of the first and the last).  After one warm-up of each, the loop and the call ALTERNATE inside every
repeat (M = 1: the call forwards to the solo step); a sample is --steps consecutive steps without a loss read-back, divided by
--steps:
  wall   -- time.perf_counter around the steps and the stream's synchronisation;
  device -- between two events on the stream.
Median and min-max over the repeats, microseconds per step of the whole group.  `beyond_spread`: loop median - call median
exceeds max - min of either."""
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

F, K, H1, H2 = ob.F, 11, 300, 100
LOOP, CALL = 'loop_of_fnn_prefetch_ids_and_fnn_train_step', 'fnn_train_step_multi'


def make(torch, stream, prec, m, rows, fo, p):
    """An FNNEngine on the shared stream: model m's hyper-parameters."""
    from deep_ctr_amd.engine import FNNEngine
    e = FNNEngine(F, K, H1, H2, max_batch=4096, precision=prec, lr=1e-3 * (1 + m % 4), lambda1=0.0, lambda_fm=0.1 / (1 + m % 3), stream=stream)
    e.set_table(rows, fo, -3.0)
    e.set_dense(p)
    return e


def loop_steps(engs, masks, feed, B):
    lib = engs[0].lib
    for s, (ids, y) in enumerate(feed):
        nxt = feed[s + 1][0].data_ptr() if s + 1 < len(feed) else None
        for e, (m1, m2) in zip(engs, masks):
            if nxt is not None:
                e._ck(lib.fnn_prefetch_ids(e.h, nxt, B))
            e._ck(lib.fnn_train_step(e.h, ids.data_ptr(), y.data_ptr(), B, m1.data_ptr(), m2.data_ptr(), B, None, None, 1, None))


def multi_steps(engs, masks, feed, B):
    lib, M = engs[0].lib, len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    a1, a2 = (C.c_void_p * M)(*[m1.data_ptr() for m1, _ in masks]), (C.c_void_p * M)(*[m2.data_ptr() for _, m2 in masks])
    for s, (ids, y) in enumerate(feed):
        nxt = feed[s + 1][0].data_ptr() if s + 1 < len(feed) else None
        engs[0]._ck(lib.fnn_train_step_multi(hs, M, ids.data_ptr(), y.data_ptr(), B, a1, a2, B, nxt, B if nxt else 0, None, None))


def alternate(torch, stream, repeats, steps, fns):
    t = {name: ([], []) for name in fns}
    for rep in range(repeats + 1):
        for name, fn in fns.items():
            w, d, _ = clocks(torch, stream, fn)
            if rep:
                t[name][0].append(w / steps), t[name][1].append(d / steps)
    return {name: {'wall_us': ob.spread(w), 'device_us': ob.spread(d)} for name, (w, d) in t.items()}


def same_bits(a, b):
    ok = True
    for i, (x, z) in enumerate(zip(a, b)):
        dx, dz = x.get_dense(), z.get_dense()
        ok = ok and all(np.array_equal(np.asarray(dx[k], np.float32).view(np.uint32), np.asarray(dz[k], np.float32).view(np.uint32)) for k in dx)
        if i in (0, len(a) - 1):
            ok = ok and bool(np.array_equal(x.get_table().view(np.uint32), z.get_table().view(np.uint32)))
    return bool(ok)


def run(Ms, Bs, repeats, steps):
    import torch
    synth, D, ids_h, y_h = ob.data(steps * 4096)
    from deep_ctr_amd import dl_utils
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids_all, y_all = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev).contiguous()
    rows = synth.fm_table(D, K, 0.01, 77)
    fo = synth.field_of_row(synth.field_sizes_ipinyou(n_fields=F))
    dl_utils.seed_global(1234)
    p = dl_utils.init_fnn_weights(1 + F * K, H1, H2, 'tanh')
    rng = np.random.RandomState(5)
    Mmax = max(Ms)
    masks = [(torch.as_tensor((rng.uniform(size=H1) < 0.5).astype(np.uint8)).to(dev), torch.as_tensor((rng.uniform(size=H2) < 0.5).astype(np.uint8)).to(dev))
             for _ in range(Mmax)]
    torch.cuda.synchronize()

    def feed(B):
        return [(ids_all[s * 4096:s * 4096 + B], y_all[s * 4096:s * 4096 + B]) for s in range(steps)]
    res = {'tool': 'fnn_step_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'k': K, 'hidden': [H1, H2],
           'repeats': repeats, 'steps_per_sample': steps,
           'timing': 'microseconds per step of the whole group; wall = perf_counter around the steps and the synchronisation, device '
                     '= between events on the stream; median / min / max over the repeats, the loop and the call alternating inside '
                     'every repeat after a warm-up of each; no loss read-back inside a sample',
           'not_measured': ['more than %d models' % Mmax, 'models on distinct streams (every handle here shares one stream)',
                            'FNN.run_many end to end'],
           'points': {}}

    def point(name, sets, B):
        M = len(sets[0])
        fd, mk = feed(B), masks[:M]
        t = alternate(torch, stream, repeats, steps, {LOOP: lambda: loop_steps(sets[0], mk, fd, B), CALL: lambda: multi_steps(sets[1], mk, fd, B)})
        pt = dict(t)
        pt['models'], pt['batch'] = M, B
        pt['results_bit_identical'] = same_bits(sets[0], sets[1])
        for clock in ('wall_us', 'device_us'):
            lo, ca = t[LOOP][clock], t[CALL][clock]
            pt['ratio_loop_to_call_at_medians_' + clock] = lo['median'] / ca['median']
            pt['beyond_spread_' + clock] = beyond_spread(lo, ca)
            pt['call_median_inside_loop_spread_' + clock] = bool(lo['min'] <= ca['median'] <= lo['max'])
        res['points'][name] = pt
        print('%s: device loop %.1f us, call %.1f us; wall loop %.1f us, call %.1f us; bits %s' % (
            name, t[LOOP]['device_us']['median'], t[CALL]['device_us']['median'], t[LOOP]['wall_us']['median'], t[CALL]['wall_us']['median'],
            pt['results_bit_identical']), flush=True)

    def reset(sets):
        for e in sets[0] + sets[1]:
            e.set_table(rows, fo, -3.0)
            e.set_dense(p)

    pools = {}
    for prec in ('bf16', 'f32'):
        pools[prec] = [[make(torch, stream, prec, m, rows, fo, p) for m in range(Mmax)] for _ in range(2)]
        for B in Bs:
            for M in Ms:
                sets = [pools[prec][0][:M], pools[prec][1][:M]]
                reset(sets)
                point('%s_B%d_M_%d' % (prec, B, M), sets, B)
        if prec == 'bf16' and Mmax > 8:                             # keep eight of them for the mixed group
            for e in pools[prec][0][8:] + pools[prec][1][8:]:
                e.close()
            pools[prec] = [pools[prec][0][:8], pools[prec][1][:8]]
    n = min(4, len(pools['bf16'][0]), len(pools['f32'][0]))
    for B in Bs:
        sets = [[e for pair in zip(pools['bf16'][i][:n], pools['f32'][i][:n]) for e in pair] for i in range(2)]      # bf16, f32, bf16, ...
        reset(sets)
        point('mixed_bf16_f32_B%d_M_%d' % (B, 2 * n), sets, B)
    for prec in pools:
        for e in pools[prec][0] + pools[prec][1]:
            e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='1,2,4,16,64')
    ap.add_argument('--batches', default='100,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fnn_step_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    res = run([int(v) for v in a.models.split(',')], [int(v) for v in a.batches.split(',')], a.repeats, a.steps)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
