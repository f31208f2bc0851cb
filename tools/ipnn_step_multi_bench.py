"""What one mini-batch step of several inner-product models costs in ONE call (ipnn_train_step_multi) against the loop it replaces
(ipnn_train_step_drawn per handle), on the iPinYou table: 16 fields, 937,670 rows, k = 11, FNN_IP_L3 (400 / 400 / 200) and
FNN_IP_L7 (1000 / 800 / 600 / 400 / 200 / 100 / 50), relu, keep_prob 0.5, drawn masks.  Writes profiles/ipnn_step_multi_bench.json.

  python tools/ipnn_step_multi_bench.py [--archs L3,L7] [--models 1,2,4,16,64] [--batches 10,100,4096] [--repeats 5] [--steps 8]
                                        [--call-first] [--fields 16] [--out FILE]

--fields: another field count on the same table (synth.field_sizes_ipinyou deals its rows to that many fields): 39 is the
reference's own column count, where layer 0 has 1408 columns.

One process; the feed (--steps batches of ids, y) is resident on the device; every handle shares one stream (the events need
one).  A point is (stack, precision, optimiser, B, M): SGD in both precisions, one Adam row (bf16, M = 16), and one mixed group of
4 bf16 + 4 f32 handles per stack and B.  The loop runs on one set of handles and the call on a second set with the same
parameters (model m: its own lr and seed), both over the same batches in the same order, so that after the last repeat the two
sets can be compared as bits (`results_bit_identical`: b and every dense tensor of every model, the touched rows of the first
and the last; `differences` names what is not), and every handle is synchronised (`sync_errors`: an error word a step left
behind).  After one warm-up of each, the loop and the call ALTERNATE inside every repeat (M = 1: the call forwards to the solo
step); a sample is --steps consecutive steps without a loss read-back, divided by --steps:
  wall   -- time.perf_counter around the steps and the stream's synchronisation;
  device -- between two events on the stream.
Median and min-max over the repeats, microseconds per step of the whole group.  `call_median_below_loop_min`: the call's
median lies below the loop's fastest repeat, which is what B = 10 and 100 have to show from M = 4 on in bf16 (one chain of
launches against M chains on a nearly empty device)."""
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

F, K = ob.F, 11
STACKS = {'L3': [400, 400, 200], 'L7': [1000, 800, 600, 400, 200, 100, 50]}
LOOP, CALL = 'loop_of_ipnn_train_step_drawn', 'ipnn_train_step_multi'


def make(torch, stream, hidden, prec, opt, m, params):
    from deep_ctr_amd.ipnn import IPNNEngine
    e = IPNNEngine(F, K, hidden, 'relu', max_batch=4096, precision=prec, lr=1e-4 * (1 + m % 4), keep_prob=0.5, optimizer=opt, stream=stream)
    e.set_params(*params)
    return e


def loop_steps(engs, feed, B, step0):
    lib = engs[0].lib
    for s, (ids, y) in enumerate(feed):
        for m, e in enumerate(engs):
            e._ck(lib.ipnn_train_step_drawn(e.h, ids.data_ptr(), None, y.data_ptr(), B, 100 + m, step0 + s, None, None))


def multi_steps(engs, feed, B, step0):
    lib, M = engs[0].lib, len(engs)
    hs = (C.c_void_p * M)(*[e.h.value for e in engs])
    seeds = (C.c_uint64 * M)(*[100 + m for m in range(M)])
    for s, (ids, y) in enumerate(feed):
        steps = (C.c_uint64 * M)(*([step0 + s] * M))
        engs[0]._ck(lib.ipnn_train_step_multi(hs, M, ids.data_ptr(), None, y.data_ptr(), B, None, seeds, steps, None, None))


def differences(a, b, ids):
    """What is not the same bits between the two sets: 'model m: tensor (elements that differ, largest difference)'."""
    out = []
    for i, (x, z) in enumerate(zip(a, b)):
        (bx, Wx, cx), (bz, Wz, cz) = x.get_params(), z.get_params()
        pairs = [('b', np.float32(bx).reshape(1), np.float32(bz).reshape(1))]
        pairs += [('W%d' % (t + 1), u, v) for t, (u, v) in enumerate(zip(Wx, Wz))] + [('bias%d' % (t + 1), u, v) for t, (u, v) in enumerate(zip(cx, cz))]
        if i in (0, len(a) - 1):
            pairs.append(('rows', x.get_rows(ids), z.get_rows(ids)))
        for name, u, v in pairs:
            if not np.array_equal(u.view(np.uint32), v.view(np.uint32)):
                out.append('model %d: %s (%d elements, max |d| %.3g)' % (i, name, int((u.view(np.uint32) != v.view(np.uint32)).sum()),
                                                                       float(np.nanmax(np.abs(u.astype(np.float64) - v)))))
    return out


def save(res, out):
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')


def run(archs, Ms, Bs, repeats, steps, out, call_first=False):
    import torch
    synth, D, ids_h, y_h = ob.data(steps * 4096)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids_all = torch.as_tensor(ids_h).to(dev).contiguous()
    y_all = torch.as_tensor(np.asarray(y_h, np.float32)).to(dev).contiguous()
    table = synth.fm_table(D, K, 0.01, 77)
    touched = np.unique(ids_h)
    torch.cuda.synchronize()
    Mmax = max(Ms)

    def feed(B):
        return [(ids_all[s * 4096:s * 4096 + B], y_all[s * 4096:s * 4096 + B]) for s in range(steps)]
    res = {'tool': 'ipnn_step_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'k': K, 'stacks': STACKS,
           'repeats': repeats, 'steps_per_sample': steps, 'first_in_every_repeat': CALL if call_first else LOOP,
           'timing': 'microseconds per step of the whole group; wall = perf_counter around the steps and the synchronisation, device '
                     '= between events on the stream; median / min / max over the repeats, the loop and the call alternating inside '
                     'every repeat after a warm-up of each; no loss read-back inside a sample',
           'not_measured': ['more than %d models' % Mmax, 'members on distinct streams (every handle here shares one stream)',
                            'field counts other than %d' % F, 'wide rows (k > 16) inside a group', 'value weights', 'the caller\'s masks (every point draws them)',
                            'the id grouping and the side chain on a side stream of the group call (built in line only)',
                            'ipnn.train_epoch_many end to end'],
           'points': {}}
    state = {'step': 0}

    def point(name, sets, B):
        M = len(sets[0])
        fd = feed(B)
        t = {LOOP: ([], []), CALL: ([], [])}
        for rep in range(repeats + 1):
            s0 = state['step']
            state['step'] += steps
            turns = ((LOOP, lambda: loop_steps(sets[0], fd, B, s0)), (CALL, lambda: multi_steps(sets[1], fd, B, s0)))
            for key, fn in (turns[::-1] if call_first else turns):
                w, d, _ = clocks(torch, stream, fn)
                if rep:
                    t[key][0].append(w / steps), t[key][1].append(d / steps)
        pt = {key: {'wall_us': ob.spread(w), 'device_us': ob.spread(d)} for key, (w, d) in t.items()}
        pt['models'], pt['batch'] = M, B
        pt['differences'] = differences(sets[0], sets[1], touched)
        pt['results_bit_identical'] = not pt['differences']
        pt['sync_errors'] = []                                       # an error word a step left behind: a pair that gave up, an id out of range
        for k, e in enumerate(sets[0] + sets[1]):
            try:
                e.sync()
            except Exception as ex:
                pt['sync_errors'].append('%s, model %d: %s' % (LOOP if k < M else CALL, k % M, ex))
        for clock in ('wall_us', 'device_us'):
            lo, ca = pt[LOOP][clock], pt[CALL][clock]
            pt['ratio_loop_to_call_at_medians_' + clock] = lo['median'] / ca['median']
            pt['beyond_spread_' + clock] = beyond_spread(lo, ca)
            pt['call_median_below_loop_min_' + clock] = bool(ca['median'] < lo['min'])
        res['points'][name] = pt
        save(res, out)                                               # every point as it falls: a cut-off run keeps what it measured
        print('%s: device loop %.1f (min %.1f) us, call %.1f us; wall loop %.1f (min %.1f) us, call %.1f us; bits %s' % (
            name + ''.join(' !! ' + x for x in pt['differences'] + pt['sync_errors']), pt[LOOP]['device_us']['median'], pt[LOOP]['device_us']['min'], pt[CALL]['device_us']['median'],
            pt[LOOP]['wall_us']['median'], pt[LOOP]['wall_us']['min'], pt[CALL]['wall_us']['median'], pt['results_bit_identical']), flush=True)

    for arch in archs:
        hidden = STACKS[arch]
        d = [F * K + F * (F - 1) // 2 + 1] + hidden + [1]
        rng = np.random.RandomState(5)
        sc = [min(0.3, 1.5 / np.sqrt(d[i])) for i in range(len(d) - 1)]
        params = (table, 0.1, [rng.uniform(-sc[i], sc[i], (d[i], d[i + 1])).astype(np.float32) for i in range(len(d) - 1)],
                  [np.zeros(d[i + 1], np.float32) for i in range(len(d) - 1)])
        kept = {}
        for prec in ('bf16', 'f32'):
            pool = [[make(torch, stream, hidden, prec, 'sgd', m, params) for m in range(Mmax)] for _ in range(2)]
            for B in Bs:
                for M in Ms:
                    point('%s_%s_sgd_B%d_M_%d' % (arch, prec, B, M), [pool[0][:M], pool[1][:M]], B)
            for e in pool[0][4:] + pool[1][4:]:
                e.close()
            kept[prec] = [pool[0][:4], pool[1][:4]]
        n = min(4, Mmax)
        for B in Bs:
            sets = [[e for pair in zip(kept['bf16'][i][:n], kept['f32'][i][:n]) for e in pair] for i in range(2)]      # bf16, f32, bf16, ...
            point('%s_mixed_bf16_f32_sgd_B%d_M_%d' % (arch, B, 2 * n), sets, B)
        for prec in kept:
            for e in kept[prec][0] + kept[prec][1]:
                e.close()
        Ma = min(16, Mmax)
        pool = [[make(torch, stream, hidden, 'bf16', 'adam', m, params) for m in range(Ma)] for _ in range(2)]
        for B in Bs:
            point('%s_bf16_adam_B%d_M_%d' % (arch, B, Ma), pool, B)
        for e in pool[0] + pool[1]:
            e.close()
    return res


def main():
    global F
    ap = argparse.ArgumentParser()
    ap.add_argument('--archs', default='L3,L7')
    ap.add_argument('--models', default='1,2,4,16,64')
    ap.add_argument('--batches', default='10,100,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--call-first', action='store_true', help='inside every repeat the call runs before the loop (default: the loop first)')
    ap.add_argument('--fields', type=int, default=F, help='fields of the feed and of every model (default 16)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ipnn_step_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    F = ob.F = a.fields                                           # (ob.data deals the table's rows to ob.F fields)
    res = run(a.archs.split(','), [int(v) for v in a.models.split(',')], [int(v) for v in a.batches.split(',')], a.repeats, a.steps, a.out, a.call_first)
    save(res, a.out)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
