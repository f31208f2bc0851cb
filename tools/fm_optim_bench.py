"""Per-step time of FM / LR pre-training under SGD, Adam and FTRL at the iPinYou shape (937,670 rows, 16 fields, batch 4096),
and the bytes the Adam / FTRL optimiser pass (k_fm_opt_pass in fm_api.hip) must move.  One JSON line on stdout.

  python tools/fm_optim_bench.py [--steps 300 --warmup 30] [--only NAME,..] [--fields N]
  python tools/fm_optim_bench.py --from-stats NAME=DIR ..    (kernel times of separate rocprofv3 --kernel-trace --stats runs,
                                                              one config each: the pass time and its TB/s)

  python tools/fm_optim_bench.py --only fm_sgd --digest        (adds a sha256 of the table, bias and optimiser state after the
                                                              timed steps: two builds of the library, FNN_HIP_LIB, compared bit for bit)

Configurations: fm_sgd / fm_adam / fm_ftrl (rank 10), lr_ftrl (rank 0 = LR); *_dense: the A/B variant of the pass that reads and
clears the whole gradient store G (FM_OPT_DENSE_G=1) instead of the rows the step's stamp marks.  The wide path (k >= 17):
fm50_* / fm100_* (the reference's FM50 / FM100), and fm100_adam_b100 at python/baseline.py's FM batch of 100.

--weights none|uniform|criteo: value weights through fm_train_step_w.  `none`, the default, is the call without weights
(fm_train_step).  `uniform`: the same ids with a weight from [0, 2) per (example, field) -- its step time against `none` of the
same build is what the weights cost.  `criteo`: synth.criteo_like -- the first 13 fields (a third of fewer than 39) are numeric,
ONE row each with a real weight, the rest are categorical with weight 1 (as tools/ipnn_wide_bench.py --weights criteo).

--fields N (1..64, default 16): the same 937,670 rows spread over N fields -- synth.field_sizes_ipinyou(n_fields=N) cycles the
16 iPinYou-like field sizes over the N fields and rescales them to the same total.  16 is the shape above, unchanged.

--shared-rows: fm_set_shared_rows(h, 1) before the steps -- the rank merge claims rows, the update loads their marks.  On the
default ids no row is shared: the step time against a run without the switch is the price of the claims and the mark loads, and
the digest is the same.  --shift FRAC: that fraction of the lines loses its first feature and moves one column left (the last
column becomes -1), as a yzx line with a missing field does: rows then sit under two columns of a batch and take the float
atomics (needs --shared-rows to be right; `shared_rows_last_step` reports how many rows the last step found shared)."""
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, SLOT = 16, 16
# name: (rank, optimizer (FM_OPT_*), lr, lambda, reduce_mean, dense G[, batch]) -- python/baseline.py's recipes: FM Adam 1e-4 /
# eps 1e-8 / 'sum' / lambda 1e-3, LR FTRL 1e-3 / lambda 1e-4; SGD as bench.py's pretrain leg.  No batch: --batch.
CONFIGS = {
    'fm_sgd': (10, 0, 1e-4, 1e-6, 1, False),
    'fm_adam': (10, 1, 1e-4, 1e-3, 0, False),
    'fm_adam_dense': (10, 1, 1e-4, 1e-3, 0, True),
    'fm_ftrl': (10, 2, 1e-3, 1e-3, 1, False),
    'fm_ftrl_dense': (10, 2, 1e-3, 1e-3, 1, True),
    'lr_ftrl': (0, 2, 1e-3, 1e-4, 1, False),
    'lr_ftrl_dense': (0, 2, 1e-3, 1e-4, 1, True),
    'fm50_sgd': (50, 0, 1e-4, 1e-6, 1, False),
    'fm50_adam': (50, 1, 1e-4, 1e-3, 0, False),
    'fm50_ftrl': (50, 2, 1e-3, 1e-3, 1, False),
    'fm100_sgd': (100, 0, 1e-4, 1e-6, 1, False),
    'fm100_adam': (100, 1, 1e-4, 1e-3, 0, False),
    'fm100_ftrl': (100, 2, 1e-3, 1e-3, 1, False),
    'fm100_adam_b100': (100, 1, 1e-4, 1e-3, 0, False, 100),
}


def rup4(k):
    return (k + 3) // 4 * 4


def fwd_bytes(B, K):
    """What the wide forward (k_fm_wide_merge_fwd's example role) must move: the B * F rows of rup(K, 4) floats read once and
    the gradients gx' [B, F, rup(K, 4)] written (the level-1 update reads them back).  Ids, labels and outputs: < 0.1 %."""
    return 2 * B * F * rup4(K) * 4


def pass_bytes(n_rows, K, dense):
    """What the pass must move per step: w, s0 and s1 read and written for every live element; the stamp variant reads one
    int per row (and G of the touched rows only: <= B * F rows, not counted), the dense variant reads and clears G everywhere."""
    return n_rows * K * 4 * (8 if dense else 6) + (0 if dense else n_rows * 4)


def shape():
    sys.path.insert(0, ROOT)
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    return sizes, sum(sizes)


def digest(lib, h, D, K, opt):
    """sha256 of the table, the bias and (Adam / FTRL) both state tensors and the bias's state, as the library returns them."""
    hs = hashlib.sha256()
    rows = np.empty((D, K), np.float32)
    b = C.c_float()
    if lib.fm_get_table(h, rows.ctypes.data) != 0 or lib.fm_get_b(h, C.byref(b)) != 0:
        raise RuntimeError(lib.fm_last_error(h).decode())
    hs.update(rows.tobytes())
    hs.update(np.float32(b.value).tobytes())
    if opt:
        s0, s1, sb, t = np.empty((D, K), np.float32), np.empty((D, K), np.float32), np.empty(2, np.float32), C.c_int64()
        if lib.fm_get_opt_state(h, s0.ctypes.data, s1.ctypes.data, sb.ctypes.data, C.byref(t)) != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())
        for a in (s0, s1, sb):
            hs.update(a.tobytes())
    return hs.hexdigest()


def weight_bytes(B):
    """What the weights add to the forward's traffic: B * F floats read once (fwd_bytes moves 2 * B * F * row bytes)."""
    return B * F * 4


def shift_left(ids, frac, seed=97):
    """A fraction of the lines moves one column left: column j takes column j + 1's id, the last column is empty."""
    ids = ids.copy()
    pick = np.random.RandomState(seed).uniform(size=len(ids)) < frac
    ids[pick, :-1] = ids[pick, 1:]
    ids[pick, -1] = -1
    return ids


def run(names, steps, warmup, B0, want_digest=False, weights='none', shared_rows=False, shift=0.0):
    import torch
    sizes, D = shape()
    from deep_ctr_amd import _capi, synth
    n_num = 0
    if weights == 'criteo':
        n_num = 13 if F >= 39 else F // 3
        D = n_num + sum(sizes[n_num:])
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    NB = 16
    out = {}
    for name in names:
        rank, opt, lr, lam, mean, dense = CONFIGS[name][:6]
        B = CONFIGS[name][6] if len(CONFIGS[name]) > 6 else B0
        ids_h, w_h = synth.zipf_ids(NB * B, sizes, 1.1, 99), None
        if weights == 'criteo':
            ids_h, w_h = synth.criteo_like(NB * B, n_num, sizes[n_num:], seed=99)
        elif weights == 'uniform':
            w_h = np.random.RandomState(98).uniform(0.0, 2.0, size=ids_h.shape).astype(np.float32)
        if shift > 0:
            ids_h = shift_left(ids_h, shift)
        ids = torch.as_tensor(ids_h).to(dev).contiguous()
        wts = None if w_h is None else torch.as_tensor(w_h).to(dev).contiguous()
        y = torch.as_tensor((np.random.RandomState(3).uniform(size=NB * B) < 0.02).astype(np.float32)).to(dev)
        K = rank + 1
        os.environ['FM_OPT_DENSE_G'] = '1' if dense else '0'        # read by fm_create
        h = C.c_void_p()
        if lib.fm_create(F, K, B, 0, C.c_void_p(stream.cuda_stream), C.byref(h)) != 0:
            raise RuntimeError((lib.fm_last_error(None) or b'').decode())
        rows = synth.fm_table(D, K, 0.01, 77)
        for rc in (lib.fm_set_optimizer(h, opt, 0.9, 0.999, 1e-8), lib.fm_set_table(h, rows.ctypes.data, D), lib.fm_set_b(h, 0.0)):
            if rc != 0:
                raise RuntimeError(lib.fm_last_error(h).decode())
        if shared_rows and lib.fm_set_shared_rows(h, 1) != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())

        def steps_(n):
            for i in range(n):
                j = i % NB
                if wts is None:
                    rc = lib.fm_train_step(h, ids.data_ptr() + j * B * F * 4, y.data_ptr() + j * B * 4, B, lr, lam, mean, None, None)
                else:
                    rc = lib.fm_train_step_w(h, ids.data_ptr() + j * B * F * 4, wts.data_ptr() + j * B * F * 4, y.data_ptr() + j * B * 4,
                                             B, lr, lam, mean, None, None)
                if rc != 0:
                    raise RuntimeError(lib.fm_last_error(h).decode())
        steps_(warmup)
        if lib.fm_sync(h) != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())
        t0 = time.perf_counter()
        steps_(steps)
        if lib.fm_sync(h) != 0:
            raise RuntimeError(lib.fm_last_error(h).decode())
        dt = (time.perf_counter() - t0) / steps
        r = {'batch': B, 'us_per_step': dt * 1e6, 'examples_per_sec': B / dt}
        if wts is not None:
            rw = SLOT if K <= 16 else rup4(K)
            r.update({'weight_bytes': weight_bytes(B), 'weight_share_of_forward_bytes': weight_bytes(B) / float(2 * B * F * rw * 4)})
        if shared_rows:
            n_sh = C.c_int64()
            if lib.fm_count_shared_rows(h, C.byref(n_sh)) != 0:
                raise RuntimeError(lib.fm_last_error(h).decode())
            r['shared_rows_last_step'] = int(n_sh.value)
        if want_digest:
            r['sha256'] = digest(lib, h, D, K, opt)
        lib.fm_destroy(h)
        if opt:
            nb = pass_bytes(D, K, dense)
            r.update({'pass_bytes': nb, 'pass_bytes_tbps_at_step_time': nb / dt / 1e12})
        out[name] = r
    res = {'tool': 'fm_optim_bench', 'n_rows': D, 'fields': F, 'batch': B0, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'configs': out}
    if weights != 'none':
        res.update({'weights': weights, 'numeric_fields': n_num})
    if shared_rows or shift > 0:
        res.update({'shared_rows': bool(shared_rows), 'shift': shift})
    return res


def from_stats(pairs):
    """NAME=DIR: the k_fm_opt_pass row (and on the wide path the k_fm_wide_merge_fwd row) of the kernel-stats CSV rocprofv3
    wrote under DIR."""
    import csv
    _, D = shape()
    out = {}
    for pr in pairs:
        name, d = pr.split('=', 1)
        rank, opt, _, _, _, dense = CONFIGS[name][:6]
        B = CONFIGS[name][6] if len(CONFIGS[name]) > 6 else 4096
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            raise SystemExit('no kernel_stats.csv under %s' % d)
        kern = {}
        for row in csv.DictReader(open(files[0])):
            kern[row['Name']] = (int(row['Calls']), float(row['AverageNs']) / 1e3)
        p = [v for k, v in kern.items() if 'k_fm_opt_pass' in k]
        short = lambda k: k.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]     # noqa: E731
        r = {'kernels_us': {short(k): round(v[1], 2) for k, v in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1])[:8]}}
        if p:
            nb = pass_bytes(D, rank + 1, dense)
            r.update({'pass_us': p[0][1], 'pass_calls': p[0][0], 'pass_bytes': nb, 'pass_tbps': nb / (p[0][1] * 1e-6) / 1e12,
                      'share_of_6.29_tbps_copy': nb / (p[0][1] * 1e-6) / 6.29e12})
        w = [v for k, v in kern.items() if 'k_fm_wide_merge_fwd' in k]
        if w:       # the launch also runs the rank merge (16 F small workgroups): its time bounds the forward's from above
            nb = fwd_bytes(B, rank + 1)
            r.update({'wide_fwd_us': w[0][1], 'wide_fwd_bytes': nb, 'wide_fwd_tbps': nb / (w[0][1] * 1e-6) / 1e12,
                      'wide_fwd_share_of_6.29_tbps_copy': nb / (w[0][1] * 1e-6) / 6.29e12})
        out[name] = r
    return {'tool': 'fm_optim_bench', 'kernel_stats': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--only', default=','.join(CONFIGS))
    ap.add_argument('--from-stats', nargs='+', default=None)
    ap.add_argument('--digest', action='store_true')
    ap.add_argument('--fields', type=int, default=16)
    ap.add_argument('--weights', choices=('none', 'uniform', 'criteo'), default='none',
                    help='value weights of the steps (fm_train_step_w); none = the call without weights')
    ap.add_argument('--shared-rows', action='store_true', help='fm_set_shared_rows(h, 1): rows may sit under several columns')
    ap.add_argument('--shift', type=float, default=0.0, help='fraction of the lines moved one column left (shared rows)')
    a = ap.parse_args()
    global F
    F = a.fields
    if a.from_stats:
        print(json.dumps(from_stats(a.from_stats)))
        return
    names = a.only.split(',')
    for n in names:
        if n not in CONFIGS:
            raise SystemExit('unknown config %r (%s)' % (n, ', '.join(CONFIGS)))
    print(json.dumps(run(names, a.steps, a.warmup, a.batch, a.digest, a.weights, a.shared_rows, a.shift)))


if __name__ == '__main__':
    main()
