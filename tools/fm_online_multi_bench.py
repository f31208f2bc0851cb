"""What a pass of FM / LR online pre-training costs when several models take it together (fm_train_online_multi: a workgroup per
model on one feed) at the shape and feed of tools/fm_online_bench.py: 16 fields, 937,670 rows, Zipf ids, N = 65,536 lines.
Writes profiles/fm_online_multi_bench.json.

  python tools/fm_online_multi_bench.py [--n 65536 --repeats 5] [--max-models 256] [--parent-lib PATH/libfnn_hip.so] [--out FILE]

Every time is device time between two events on the launch stream around one whole call, all in one process, after one warm-up
call of everything timed; the variants of a part alternate inside every repeat (median and min-max over the repeats).
  (a) one model: fm_train_online against fm_train_online_multi at M = 1 (rank 10) -- what the new path costs by itself;
  (b) fm_train_online of THIS library against the same entry point of the library built from the parent commit (--parent-lib;
      left out of the result, and said so, without it), at 16 fields rank 10 and rank 100 and at 64 fields rank 127 (1, 2 and 8 row
      pieces per thread) -- the per-example body moved into a function
      both kernels call; the two tables and b are also compared bit for bit after the same calls;
  (c) M = 1, 2, 4, .. 256 models of rank 10 (a table each, equal lr and lambda) and the group {LR, FM10, FM50, FM100}: microseconds
      per line of the call, model-lines per second, and both as ratios to M = 1 of the same run.
The host finds a launch's end by advancing every model's scale line by line (lines x models multiplications) before it
launches, on an idle stream: that time is inside (c)'s interval and grows with M.
All handles share one stream here (the events need one); the Python classes give every model its own, which adds two event
calls per model and call.  Checked before anything is timed: on a prefix, the M = 1 group call leaves the bits of the solo call."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_online_bench as ob  # noqa: E402

F, LR = ob.F, ob.LR
MIXED = (0, 10, 50, 100)


def multi(lib, hs, ranks, ids, y, n):
    M = len(hs)
    arr = (C.c_void_p * M)(*[h.value for h in hs])
    lr, lam = (C.c_float * M)(*[LR] * M), (C.c_float * M)(*[ob.lam_of(r) for r in ranks])
    ob.ck(lib, hs[0], lib.fm_train_online_multi(arr, M, ids.data_ptr(), None, y.data_ptr(), n, lr, lam, None, None, None))


def solo(lib, h, rank, ids, y, n):
    ob.ck(lib, h, lib.fm_train_online(h, ids.data_ptr(), None, y.data_ptr(), n, LR, ob.lam_of(rank), None, None, None))


def make_f(lib, stream, n_fields, K, D, rows):
    """ob.make at another field count."""
    h = C.c_void_p()
    if lib.fm_create(n_fields, K, 1, 0, C.c_void_p(stream.cuda_stream), C.byref(h)) != 0:
        raise RuntimeError((lib.fm_last_error(None) or b'').decode())
    ob.ck(lib, h, lib.fm_set_table(h, rows.ctypes.data, D))
    ob.ck(lib, h, lib.fm_set_b(h, 0.0))
    return h


def timed(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3                                # microseconds


def bind_parent(path):
    from deep_ctr_amd import _capi
    lib = C.CDLL(path)
    for name, (res, args) in _capi.FM_SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def run(N, repeats, max_models, parent_path):
    import torch
    synth, D, ids_h, y_h = ob.data(N)
    from deep_ctr_amd import _capi
    lib = _capi.load()
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ids, y = torch.as_tensor(ids_h).to(dev).contiguous(), torch.as_tensor(y_h).to(dev)
    torch.cuda.synchronize()
    tables = {r: synth.fm_table(D, r + 1, 0.01, 77) for r in MIXED}
    res = {'tool': 'fm_online_multi_bench', 'device': torch.cuda.get_device_name(0), 'fields': F, 'n_rows': D, 'lines': N, 'lr': LR,
           'repeats': repeats, 'timing': 'device events around one whole call, microseconds; median / min / max over the repeats'}

    # the prefix check: M = 1 through the group entry point leaves the bits of the solo call
    pre = min(N, 4096)
    h_s, h_m = ob.make(lib, stream, 11, D, tables[10]), ob.make(lib, stream, 11, D, tables[10])
    solo(lib, h_s, 10, ids, y, pre)
    multi(lib, [h_m], [10], ids, y, pre)
    (rs, bs), (rm, bm) = ob.params(lib, h_s, D, 11), ob.params(lib, h_m, D, 11)
    res['prefix_bit_identity'] = {'lines': pre, 'holds': bool(np.array_equal(rs.view(np.uint32), rm.view(np.uint32)) and bs == bm)}

    # (a) the new path at one model
    t_s, t_m = [], []
    for rep in range(repeats + 1):
        a = timed(torch, stream, lambda: solo(lib, h_s, 10, ids, y, N))
        b = timed(torch, stream, lambda: multi(lib, [h_m], [10], ids, y, N))
        if rep:
            t_s.append(a / N), t_m.append(b / N)
    res['a_one_model_us_per_line'] = {'fm_train_online': ob.spread(t_s), 'fm_train_online_multi_M1': ob.spread(t_m),
                                      'ratio_at_medians': float(np.median(t_m) / np.median(t_s))}
    lib.fm_destroy(h_m)

    # (b) the old entry point, this library against the parent commit's: rank 10 (at most one row piece per thread) and rank 100
    # (two: the gather's loads must all be out before the first is used)
    lib.fm_destroy(h_s)
    if parent_path:
        par = bind_parent(parent_path)
        res['b_fm_train_online_us_per_line'] = {}
        ids64 = torch.as_tensor(synth.zipf_ids(N, synth.field_sizes_ipinyou(n_fields=64), 1.1, 99).astype(np.int32)).to(dev).contiguous()
        for nf, rank in ((F, 10), (F, 100), (64, 127)):
            K = rank + 1
            rows = tables[rank] if rank in tables else synth.fm_table(D, K, 0.01 / 8, 77)
            feed = ids if nf == F else ids64
            h_p, h_n = make_f(par, stream, nf, K, D, rows), make_f(lib, stream, nf, K, D, rows)
            t_new, t_par = [], []
            for rep in range(repeats + 1):
                a = timed(torch, stream, lambda: solo(par, h_p, rank, feed, y, N))
                b = timed(torch, stream, lambda: solo(lib, h_n, rank, feed, y, N))
                if rep:
                    t_par.append(a / N), t_new.append(b / N)
            (rp, bp), (rn, bn) = ob.params(par, h_p, D, K), ob.params(lib, h_n, D, K)
            res['b_fm_train_online_us_per_line']['fields_%d_rank_%d' % (nf, rank)] = {
                'parent_commit': ob.spread(t_par), 'this_commit': ob.spread(t_new),
                'ratio_at_medians': float(np.median(t_new) / np.median(t_par)),
                'calls_compared': repeats + 1, 'b_equal': bool(bp == bn),
                'table_words_differing_after_those_calls': int((rp.view(np.uint32) != rn.view(np.uint32)).sum())}
            par.fm_destroy(h_p), lib.fm_destroy(h_n)
    else:
        res['b_fm_train_online_us_per_line'] = 'not measured: no --parent-lib given'

    # (c) scaling
    counts = [m for m in (1, 2, 4, 8, 16, 32, 64, 128, 256) if m <= max_models]
    hs = [ob.make(lib, stream, 11, D, tables[10]) for _ in range(counts[-1])]
    mixed = [ob.make(lib, stream, r + 1, D, tables[r]) for r in MIXED]
    points = [('M_%d' % m, hs[:m], [10] * m) for m in counts] + [('mixed_LR_FM10_FM50_FM100', mixed, list(MIXED))]
    t = {name: [] for name, _, _ in points}
    for rep in range(repeats + 1):
        for name, group, ranks in points:
            dt = timed(torch, stream, lambda: multi(lib, group, ranks, ids, y, N))
            if rep:
                t[name].append(dt)
    base = float(np.median(t['M_1']))
    scal = {}
    for name, group, ranks in points:
        med = float(np.median(t[name]))
        scal[name] = {'models': len(group), 'ranks': sorted(set(ranks)),
                      'us_per_line_of_the_call': ob.spread([v / N for v in t[name]]),
                      'model_lines_per_second_at_median': len(group) * N / (med * 1e-6),
                      'time_ratio_to_M_1': med / base, 'throughput_ratio_to_M_1': len(group) * base / med}
    res['c_scaling'] = scal
    for h in hs + mixed:
        lib.fm_destroy(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--max-models', type=int, default=256)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fm_online_multi_bench.json'))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit('at least five repeats')
    res = run(a.n, a.repeats, a.max_models, a.parent_lib)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
