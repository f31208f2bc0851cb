"""A/B of the FNN step between two builds of libfnn_hip.so loaded into ONE process and alternated: the benchmark's step (bench.py:
bf16, batch 4096, 16 fields x k = 11, hidden 300 / 100, the next batch announced by fnn_prefetch_ids) and fnn_predict at the
same batch.

  python tools/fnn_step_ab.py --parent /path/to/parent/libfnn_hip.so --out profiles/fnn_step_plumbing_ab.json

Three libraries take turns: `parent`, `this` (the tree's) and `parent_copy`, a byte-for-byte copy of the parent's file loaded as a
library of its own -- the null experiment: what two loads of the same code differ by (where the code object lands is fixed for the
life of the process, so it does not average out over runs).  One fresh handle per run, one handle alive at a time, the order
rotating and then mirrored, so that every position of the process's stream / queue rotation sees every library.  A run times, on
the same parameters and inputs: wall time per step over the benchmark's loop (enqueue all, one sync), device time of the same
loop (events on the handle's stream), the host time of the enqueue alone (a shorter loop, so that the queue never pushes back),
then the same for fnn_predict.  The raw runs are written out; the summary says whether this library's median lies inside the
parent's own spread (both loads of it).  Every handle takes the same calls on the same inputs: the tool fails unless all of them
leave the same bits in the table and in every dense tensor.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K, H1, H2 = 16, 11, 300, 100


def load_lib(path):
    from deep_ctr_amd import _capi
    import torch  # noqa: F401  (first: see _capi.load)
    lib = C.CDLL(path)
    for name, (res, args) in _capi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def stats(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--this', default=os.path.join(ROOT, 'deep-ctr_amd', 'libfnn_hip.so'))
    ap.add_argument('--out', required=True)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=10000, help='per timed loop: a third of a second of steps at 30 us')
    ap.add_argument('--enqueue-steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3, help='the order has 6 * rounds runs, a third of them per library')
    args = ap.parse_args()

    import torch
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import _capi, synth
    from deep_ctr_amd import dl_utils as ut
    from deep_ctr_amd.engine import FNNEngine
    tmp = tempfile.mkdtemp()
    shutil.copy(args.parent, os.path.join(tmp, 'libfnn_parent_copy.so'))
    libs = {'parent': load_lib(args.parent), 'this': load_lib(args.this), 'parent_copy': load_lib(os.path.join(tmp, 'libfnn_parent_copy.so'))}
    names = ['parent', 'this', 'parent_copy']
    B, NB = args.batch, 32
    dev = torch.device('cuda', 0)
    sizes = synth.field_sizes_ipinyou()
    rows = synth.fm_table(sum(sizes), K, 0.05, 1234)
    fo = synth.field_of_row(sizes)
    ids = torch.as_tensor(synth.zipf_ids(NB * B, sizes, 1.1, 1234)).to(dev).contiguous()
    y = torch.as_tensor((np.random.RandomState(99).uniform(size=NB * B) < 0.02).astype(np.float32)).to(dev).contiguous()
    ut.seed_global(1234)
    p0 = ut.init_fnn_weights(1 + F * K, H1, H2, 'tanh')
    rs = np.random.RandomState(234)
    m1 = torch.as_tensor((rs.uniform(size=(NB, H1)) < 0.5).astype(np.uint8)).to(dev).contiguous()
    m2 = torch.as_tensor((rs.uniform(size=(NB, H2)) < 0.5).astype(np.uint8)).to(dev).contiguous()
    p_out = torch.empty(B, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def engine(which):
        _capi._lib = libs[which]                       # FNNEngine takes the library from _capi.load()
        eng = FNNEngine(F, K, H1, H2, max_batch=B, precision='bf16', lr=0.001, lambda1=0.0, lambda_fm=0.1)
        assert eng.lib is libs[which]
        eng.set_table(rows, fo, -3.0)
        eng.set_dense(p0)
        return eng

    def timed(eng, call, n, n_enq):
        """wall and device time per call over n calls, host time per call over n_enq calls (enqueue only)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        for i in range(n):
            call(i)
        e1.record(eng.stream)
        eng.sync(); torch.cuda.synchronize(dev)
        wall = (time.perf_counter() - t0) / n
        device = e0.elapsed_time(e1) * 1e-3 / n
        t0 = time.perf_counter()
        for i in range(n_enq):
            call(n + i)
        host = (time.perf_counter() - t0) / n_enq
        eng.sync(); torch.cuda.synchronize(dev)
        return {'wall_us': wall * 1e6, 'device_us': device * 1e6, 'host_enqueue_us_per_call': host * 1e6}

    out = {'what': 'the benchmark\'s FNN step (bf16, batch %d, 16 x 11, 300 / 100, fnn_prefetch_ids + fnn_train_step) and fnn_predict of this tree\'s library '
                   'against the library built from its parent commit and a copy of the latter (null experiment), all loaded into one process; one fresh '
                   'handle per run, the libraries taking turns' % B,
           'steps_per_run': args.steps, 'enqueue_steps': args.enqueue_steps, 'runs_per_library': 2 * args.rounds, 'cases': {}}
    runs = {'step': {n: [] for n in names}, 'predict': {n: [] for n in names}}
    states, order = [], []
    for r in range(args.rounds):
        order += names[r % 3:] + names[:r % 3]
    order += order[::-1]                              # ... and mirrored: every position of the stream / queue rotation sees both
    for which in order:
        eng = engine(which)
        lib, h = eng.lib, eng.h

        def step(i):
            lib.fnn_prefetch_ids(h, ids.data_ptr() + ((i + 1) % NB) * B * F * 4, B)
            b = i % NB
            rc = lib.fnn_train_step(h, ids.data_ptr() + b * B * F * 4, y.data_ptr() + b * B * 4, B, m1.data_ptr() + b * H1, m2.data_ptr() + b * H2, B,
                                    None, None, _capi.FNN_MEM_DEVICE, None)
            if rc != 0:
                raise RuntimeError(lib.fnn_last_error(h).decode())

        def predict(i):
            rc = lib.fnn_predict(h, ids.data_ptr() + (i % NB) * B * F * 4, B, p_out.data_ptr(), _capi.FNN_MEM_DEVICE)
            if rc != 0:
                raise RuntimeError(lib.fnn_last_error(h).decode())

        for i in range(args.warmup):
            step(i)
        runs['step'][which].append(timed(eng, step, args.steps, args.enqueue_steps))
        for i in range(args.warmup):
            predict(i)
        runs['predict'][which].append(timed(eng, predict, args.steps, args.enqueue_steps))
        d = eng.get_dense()
        states.append((eng.get_table().tobytes(), p_out.cpu().numpy().tobytes()) + tuple(np.asarray(d[k]).tobytes() for k in sorted(d)))
        eng.close()
    for kind, rr in runs.items():
        case = {'raw': rr, 'order': order, 'summary': {}}
        for key in ('wall_us', 'device_us', 'host_enqueue_us_per_call'):
            st = {n: stats([x[key] for x in rr[n]]) for n in names}
            st['parent_spread'] = [min(st['parent']['min'], st['parent_copy']['min']), max(st['parent']['max'], st['parent_copy']['max'])]
            st['this_median_inside_parent_spread'] = bool(st['this']['median'] <= st['parent_spread'][1])
            case['summary'][key] = st
        out['cases'][kind] = case
    out['state_bits_equal_over_all_runs'] = bool(all(x == states[0] for x in states))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp, ignore_errors=True)
    for kind, case in out['cases'].items():
        for key, st in case['summary'].items():
            print('%-8s %-26s' % (kind, key) + ''.join('  %s %.1f [%.1f, %.1f]' % (n, st[n]['median'], st[n]['min'], st[n]['max']) for n in names) +
                  '  this median inside the parent\'s spread: %s' % st['this_median_inside_parent_spread'])
    print('state bits equal over all runs:', out['state_bits_equal_over_all_runs'])
    assert out['state_bits_equal_over_all_runs'], "the libraries left different tables / dense tensors"


if __name__ == '__main__':
    main()
