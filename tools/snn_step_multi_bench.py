"""What one SNN fine-tune step (FNN_MODE_BAG) of several models costs in ONE call (fnn_bag_train_step_multi with next_ids) against
the loop it replaces (fnn_prefetch_ids + fnn_train_step per handle), at the reference's shape: a bag table of 133,465 x 200
(python/SNN_RBM.py:49, advertiser 2997), 16 columns, hidden 300 / 100.  Writes profiles/snn_step_multi_bench.json.

  python tools/snn_step_multi_bench.py [--models 1,2,4,16,64] [--batches 1000,4096] [--repeats 5] [--steps 8] [--out FILE]

One process; the feed (--steps batches of ids, y) is resident on the device; every handle shares one stream (the events need
one).  The ids are Zipf draws with every column on its own range of rows, so no row lies under two columns of a batch, no float
atomic runs and the two sides can be compared as bits (`results_bit_identical`: every dense tensor and the bag bias of every
model, the whole table of the first and the last) -- a feed with shared rows would agree to the rounding of those atomics only.
A point is (precision, B, M).  The loop runs on one set of handles and the call on a second set with equal parameters (model m:
its own lr, lambda1 and masks), both over the same batches in the same order.  After one warm-up of each, the loop and the call
ALTERNATE inside every repeat (M = 1: the call forwards to the solo step); a sample is --steps consecutive steps without a loss
read-back, divided by --steps:
  wall   -- time.perf_counter around the steps and the stream's synchronisation;
  device -- between two events on the stream.
Median and min-max over the repeats, microseconds per step of the whole group.  `beyond_spread`: loop median - call median
exceeds max - min of either.  Every model holds its own table: 64 models in two sets are 13.7 GB of tables."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_online_bench as ob  # noqa: E402
from fm_eval_multi_bench import beyond_spread  # noqa: E402
from fnn_step_multi_bench import alternate, loop_steps  # noqa: E402

F, X_DIM, H0, H1, H2 = 16, 133465, 200, 300, 100
LOOP, CALL = 'loop_of_fnn_prefetch_ids_and_fnn_train_step', 'fnn_bag_train_step_multi'


def make(stream, prec, m, ww0, bb0, p):
    """A bag-mode FNNEngine on the shared stream: model m's hyper-parameters."""
    from deep_ctr_amd.engine import FNNEngine
    e = FNNEngine(F, 0, H1, H2, max_batch=4096, precision=prec, lr=1e-3 * (1 + m % 4), lambda1=1e-4 * (m % 3), lambda_fm=0.0, reg_all=True,
                  mode='bag', hidden0=H0, stream=stream)
    load(e, ww0, bb0, p)
    return e


def load(e, ww0, bb0, p):
    e.set_table(ww0, np.zeros(ww0.shape[0], np.int32), 0.0)
    e.set_bag_bias(bb0)
    e.set_dense(p)


def multi_steps(engs, masks, feed, B):
    lib, M = engs[0].lib, len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    a1, a2 = (C.c_void_p * M)(*[m1.data_ptr() for m1, _ in masks]), (C.c_void_p * M)(*[m2.data_ptr() for _, m2 in masks])
    for s, (ids, y) in enumerate(feed):
        nxt = feed[s + 1][0].data_ptr() if s + 1 < len(feed) else None
        engs[0]._ck(lib.fnn_bag_train_step_multi(hs, M, ids.data_ptr(), y.data_ptr(), B, a1, a2, B, nxt, B if nxt else 0, None, None))


def same_bits(a, b):
    ok = True
    for i, (x, z) in enumerate(zip(a, b)):
        dx, dz = x.get_dense(), z.get_dense()
        ok = ok and all(np.array_equal(np.asarray(dx[k], np.float32).view(np.uint32), np.asarray(dz[k], np.float32).view(np.uint32)) for k in dx)
        ok = ok and bool(np.array_equal(x.get_bag_bias().view(np.uint32), z.get_bag_bias().view(np.uint32)))
        if i in (0, len(a) - 1):
            ok = ok and bool(np.array_equal(x.get_table().view(np.uint32), z.get_table().view(np.uint32)))
    return bool(ok)


def run(Ms, Bs, repeats, steps):
    import torch
    sys.path.insert(0, ROOT)
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import dl_utils, synth
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    sizes = synth.field_sizes_tiny(X_DIM, n_fields=F)
    ids_h = synth.zipf_ids(steps * 4096, sizes, 1.1, 99).astype(np.int32)
    y_h = (np.random.RandomState(3).uniform(size=steps * 4096) < 0.02).astype(np.float32)
    ids_all, y_all = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev).contiguous()
    dl_utils.seed_global(1234)
    ww0, bb0 = dl_utils.init_weight(X_DIM, H0, 'sigmoid')
    ww1, bb1 = dl_utils.init_weight(H0, H1, 'sigmoid')
    ww2, bb2 = dl_utils.init_weight(H1, H2, 'sigmoid')
    ww0 = np.ascontiguousarray(ww0, dtype=np.float32)
    p = {'w1': ww1, 'b1': bb1, 'w2': ww2, 'b2': bb2, 'w3': np.zeros(H2), 'b3': 0.}
    rng = np.random.RandomState(5)
    Mmax = max(Ms)
    masks = [(torch.as_tensor((rng.uniform(size=H1) < 0.98).astype(np.uint8)).to(dev), torch.as_tensor((rng.uniform(size=H2) < 0.98).astype(np.uint8)).to(dev))
             for _ in range(Mmax)]
    torch.cuda.synchronize()

    def feed(B):
        return [(ids_all[s * 4096:s * 4096 + B], y_all[s * 4096:s * 4096 + B]) for s in range(steps)]
    res = {'tool': 'snn_step_multi_bench', 'device': torch.cuda.get_device_name(0), 'columns': F, 'n_rows': X_DIM, 'hidden': [H0, H1, H2],
           'repeats': repeats, 'steps_per_sample': steps,
           'timing': 'microseconds per step of the whole group; wall = perf_counter around the steps and the synchronisation, device '
                     '= between events on the stream; median / min / max over the repeats, the loop and the call alternating inside '
                     'every repeat after a warm-up of each; no loss read-back inside a sample',
           'feed': 'every column draws from its own rows: no row under two columns of a batch, no float atomics, bits comparable',
           'not_measured': ['more than %d models' % Mmax, 'models on distinct streams (every handle here shares one stream)',
                            'a feed with rows under several columns (the float-atomic branch of the row update)', 'SNN_RBM.run_many end to end'],
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

    for prec in ('bf16', 'f32'):
        pools = [[make(stream, prec, m, ww0, bb0, p) for m in range(Mmax)] for _ in range(2)]
        for B in Bs:
            for M in Ms:
                sets = [pools[0][:M], pools[1][:M]]
                for e in sets[0] + sets[1]:
                    load(e, ww0, bb0, p)
                point('%s_B%d_M_%d' % (prec, B, M), sets, B)
        for e in pools[0] + pools[1]:
            e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='1,2,4,16,64')
    ap.add_argument('--batches', default='1000,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'snn_step_multi_bench.json'))
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
