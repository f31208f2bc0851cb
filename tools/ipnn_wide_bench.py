"""Per-step time of the inner-product family on wide FM rows (k = rank + 1 >= 17: k_ip_fwd_w / k_ip_bwd_w and the wide sparse-row
update) at the iPinYou shape (937,670 rows, 16 fields, batch 4096): FNN_IP_L3 (hidden 400 / 400 / 200, python/baseline.py's
FNN_IP_L3 recipe) and the plain FNN (hidden 400 / 400) at k = 51 and 101, in f32 and bf16, with SGD and Adam, with the
per-segment device times of ipnn_prof_* and a FLOP / byte model of the step.  One JSON line on stdout.

  python tools/ipnn_wide_bench.py [--steps 100 --warmup 10] [--only NAME,..] [--no-prof]
  python tools/ipnn_wide_bench.py --digest --steps 5 --only l7_k11_bf16_sgd,...   (sha256 of table, layers and b after the steps)
  python tools/ipnn_wide_bench.py --fields 39    (narrow rows on N fields, synth.field_sizes_ipinyou(n_fields=N): the reference's
                                                  39 columns, up to 64; the default configurations are then the NARROW_MANY ones)
  python tools/ipnn_wide_bench.py --weights criteo|random   (value weights through ipnn_train_step_w: `criteo` is
                                                  synth.criteo_like -- the first 13 fields (a third of fewer than 39) are numeric,
                                                  one constant row each for the whole batch, weighted by a value in [0, 2), the
                                                  others categorical with weight 1; `random` keeps the ids and draws every weight
                                                  from [0, 2); `none`, the default, is the call without weights)
  python tools/ipnn_wide_bench.py --dropout none|input|drawn   (who makes the keep-masks of the timed steps: `none`, the default,
                                                  changes nothing -- the resident masks built once at set-up, as always; `input`
                                                  is a training loop's caller: fresh masks every step, torch.rand(...) < keep ->
                                                  uint8 per layer on the device, then passed in; `drawn` is ipnn_train_step_drawn:
                                                  the library draws the masks of (seed 1234, step i) itself.  With --mask-cost the
                                                  device time of making one step's `input` masks is measured on its own.)

The k11 configurations use only what the parent C ABI already had, so the same script digests a build of the parent tree.
The timed window and the profiled window are separate runs of the same steps: the profiling events sit between the launches."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16
HIDDEN = {'l3': [400, 400, 200], 'fnn': [400, 400], 'l7': [1000, 800, 600, 400, 200, 100, 50]}
CONFIGS = {}
for _c in ('l3', 'fnn'):
    for _k in (51, 101):
        for _p in ('f32', 'bf16'):
            for _o in ('sgd', 'adam'):
                CONFIGS['%s_k%d_%s_%s' % (_c, _k, _p, _o)] = (_c, _k, _p, _o)
for _c in ('l7', 'l3'):
    for _p in ('f32', 'bf16'):
        CONFIGS['%s_k11_%s_sgd' % (_c, _p)] = (_c, 11, _p, 'sgd')
WIDE = [n for n in CONFIGS if '_k11_' not in n]
# narrow rows at any field count (--fields 39 / 64: wide rows stop at 32 fields)
NARROW_MANY = []
for _c in ('l3', 'fnn'):
    for _p in ('f32', 'bf16'):
        for _o in ('sgd', 'adam'):
            CONFIGS['%s_k11_%s_%s' % (_c, _p, _o)] = (_c, 11, _p, _o)
            NARROW_MANY.append('%s_k11_%s_%s' % (_c, _p, _o))
SEGMENTS = ('mask_t', 'sort', 'ip_fwd', 'fwd', 'bwd', 'wgrad', 'ip_bwd', 'scatter', 'adam_table', 'update')
PEAK_TFLOPS = {'f32': 157.3, 'bf16': 2516.6}        # MI355X dense MFMA peaks
HBM_TBPS = 8.0


def rup(a, m):
    return (a + m - 1) // m * m


def model(B, K, cls, prec, opt, n_rows):
    """Matrix FLOP of the step (three products per layer: forward, backward-data, weight gradient) at the reference's sizes d and
    at the padded sizes Dp the kernels run, the inner-product layer's own FLOP (P pair products of k forward, twice that
    backward), and the HBM bytes each segment must move, every operand once: the gather reads B F rows and writes a0 in both
    layouts and emb; the backward reads emb and dz0 and writes gx'; the weight gradients read a0^T / the deltas and write the
    split-K slabs; the row update reads gx' and reads / writes at most B F rows; Adam's dense pass streams table, m, v and G
    in and out (eight streams of n_rows rw floats)."""
    pairs = cls != 'fnn'
    rw = rup(K, 4) if K > 16 else 16
    P = F * (F - 1) // 2 if pairs else 0
    hid = HIDDEN[cls]
    d = [F * K + P + 1] + hid + [1]
    Dp = [rup(F * rw + P + 2, 64)] + [rup(h + 1, 64) for h in hid] + [64]
    ts = 2 if prec == 'bf16' else 4
    flop = 6.0 * B * sum(d[i] * d[i + 1] for i in range(len(d) - 1))
    flop_p = 6.0 * B * sum(Dp[i] * Dp[i + 1] for i in range(len(Dp) - 1))
    flop_ip = 6.0 * B * P * K
    nw = sum(Dp[i] * Dp[i + 1] for i in range(len(Dp) - 1))
    by = {
        'ip_fwd': B * F * rw * 4 * 2 + 2 * B * Dp[0] * ts,
        'stack': sum(2 * B * Dp[i] * ts * 2 for i in range(1, len(Dp))) + 2 * nw * ts + B * Dp[0] * 4,
        'wgrad': sum(B * (Dp[i] + Dp[i + 1]) * ts for i in range(len(Dp) - 1)) + 2 * nw * 4,
        'ip_bwd': B * F * rw * 4 + B * Dp[0] * 4 * 2,
        'scatter': B * F * rw * 4 * 3,
        'update': 2 * nw * 4 + 2 * nw * 4 + 2 * nw * ts + (4 * nw * 4 if opt == 'adam' else 0),
    }
    adam_pass = 8 * n_rows * rw * 4 if opt == 'adam' else 0
    return {'d': d, 'Dp': Dp, 'flop': flop, 'flop_padded': flop_p, 'flop_ip': flop_ip, 'bytes_by_segment': by,
            'bytes_step': sum(by.values()), 'bytes_adam_table': adam_pass}


def setup(name, B, NB, D, ids_h, y_h, w_h=None, dropout='none'):
    import torch
    from deep_ctr_amd.ipnn import IPNNEngine
    cls, K, prec, opt = CONFIGS[name]
    hid = HIDDEN[cls]
    eng = IPNNEngine(F, K, hid, 'relu', max_batch=B, precision=prec, lr=1e-4 if opt == 'adam' else 1e-3, keep_prob=0.5,
                     pairs=cls != 'fnn', optimizer=opt, adam_eps=1e-8)
    rng = np.random.RandomState(77)
    table = (rng.uniform(-0.05, 0.05, (D, K))).astype(np.float32)
    d = eng.d
    Ws = [rng.uniform(-0.06, 0.06, (d[i], d[i + 1])).astype(np.float32) for i in range(len(d) - 1)]
    bs = [np.zeros(d[i + 1], np.float32) for i in range(len(d) - 1)]
    eng.set_params(table, 0.1, Ws, bs)
    ids = torch.as_tensor(ids_h).to(eng.device)
    y = torch.as_tensor(y_h).to(eng.device)
    w = None if w_h is None else torch.as_tensor(w_h).to(eng.device)
    mk = [torch.as_tensor((np.random.RandomState(40 + t).uniform(size=(B, d[t])) < 0.5).astype(np.uint8)).to(eng.device)
          for t in range(len(hid) + 1)]
    marr = (C.c_void_p * len(mk))(*[m.data_ptr() for m in mk])
    torch.cuda.synchronize()
    lib, h = eng.lib, eng.h

    keep = 0.5
    wp = (lambda j: None) if w is None else (lambda j: w.data_ptr() + j * B * F * 4)

    def fresh_masks():
        """One step's masks as a caller of the mask-input entry point makes them on the device (three launches a layer)."""
        return [(torch.rand((B, d[t]), device=eng.device) < keep).to(torch.uint8) for t in range(len(hid) + 1)]

    def steps_(n):
        if dropout == 'drawn':
            for i in range(n):
                j = i % NB
                eng._ck(lib.ipnn_train_step_drawn(h, ids.data_ptr() + j * B * F * 4, wp(j), y.data_ptr() + j * B * 4, B, 1234, i, None, None))
            return
        if dropout == 'input':
            for i in range(n):
                j = i % NB
                with torch.cuda.stream(eng.stream):          # the handle's stream: the step follows the masks in order
                    fm = fresh_masks()
                fa = (C.c_void_p * len(fm))(*[m.data_ptr() for m in fm])
                eng._ck(lib.ipnn_train_step_w(h, ids.data_ptr() + j * B * F * 4, wp(j), y.data_ptr() + j * B * 4, B, fa, None, None))
            return
        for i in range(n):
            j = i % NB
            if w is None:
                eng._ck(lib.ipnn_train_step(h, ids.data_ptr() + j * B * F * 4, y.data_ptr() + j * B * 4, B, marr, None, None))
            else:
                eng._ck(lib.ipnn_train_step_w(h, ids.data_ptr() + j * B * F * 4, w.data_ptr() + j * B * F * 4, y.data_ptr() + j * B * 4,
                                              B, marr, None, None))
    steps_.fresh_masks = fresh_masks
    return eng, steps_, (ids, y, mk, w)


def digest(eng, D):
    h = hashlib.sha256()
    h.update(eng.get_rows(np.arange(D)).tobytes())
    b, Ws, bs = eng.get_params()
    for W, bb in zip(Ws, bs):
        h.update(W.tobytes()); h.update(bb.tobytes())
    h.update(np.float32(b).tobytes())
    return h.hexdigest()


def mask_cost_us(eng, fresh_masks, steps):
    """Device time of making one step's masks the caller's way: HIP events around `steps` makings on the handle's stream."""
    import torch
    with torch.cuda.stream(eng.stream):
        for _ in range(3):
            fresh_masks()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fresh_masks()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def run(names, steps, warmup, B, prof, dig, weights='none', dropout='none', mask_cost=False):
    sys.path.insert(0, ROOT)
    import torch
    import deep_ctr_amd  # noqa: F401
    from deep_ctr_amd import synth
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    D = sum(sizes)
    NB = 8
    ids_h, w_h, n_num = synth.zipf_ids(NB * B, sizes, 1.1, 99), None, 0
    if weights == 'criteo':
        n_num = 13 if F >= 39 else F // 3
        D = n_num + sum(sizes[n_num:])
        ids_h, w_h = synth.criteo_like(NB * B, n_num, sizes[n_num:], seed=99)
    elif weights == 'random':
        w_h = np.random.RandomState(98).uniform(0.0, 2.0, size=ids_h.shape).astype(np.float32)
    y_h = (np.random.RandomState(3).uniform(size=NB * B) < 0.02).astype(np.float32)
    out = {}
    for name in names:
        cls, K, prec, opt = CONFIGS[name]
        eng, steps_, keep = setup(name, B, NB, D, ids_h, y_h, w_h, dropout)
        lib, h = eng.lib, eng.h
        if dig:
            steps_(steps)
            eng.sync()
            out[name] = {'k': K, 'precision': prec, 'optimizer': opt, 'steps': steps, 'sha256': digest(eng, D)}
            eng.close()
            continue
        steps_(warmup)
        eng.sync()
        t0 = time.perf_counter()
        steps_(steps)
        eng.sync()
        dt = (time.perf_counter() - t0) / steps
        r = {'class': cls, 'k': K, 'precision': prec, 'optimizer': opt, 'us_per_step': dt * 1e6, 'examples_per_sec': B / dt}
        if mask_cost:
            r['caller_mask_making_us'] = mask_cost_us(eng, steps_.fresh_masks, steps)
        md = model(B, K, cls, prec, opt, D)
        if prof:
            eng._ck(lib.ipnn_prof_enable(h, 1))
            steps_(steps)
            eng.sync()
            seg = {}
            for s in SEGMENTS:
                v = C.c_double()
                eng._ck(lib.ipnn_prof_get(h, s.encode(), C.byref(v)))
                if v.value > 0:
                    seg[s] = round(v.value * 1e3, 2)
            eng._ck(lib.ipnn_prof_enable(h, 0))
            r['segments_us'] = seg
            if 'adam_table' in seg:
                r['adam_table_tbps'] = md['bytes_adam_table'] / (seg['adam_table'] * 1e-6) / 1e12
        eng.close()
        t_mfma = md['flop_padded'] / (PEAK_TFLOPS[prec] * 1e12)
        t_hbm = (md['bytes_step'] + md['bytes_adam_table']) / (HBM_TBPS * 1e12)
        if prof:
            r['segments_note'] = ('HIP events around each segment on its own stream: ip_bwd, scatter and adam_table run on the side '
                                  'stream beside wgrad, so their spans include waiting and overlap; the kernel traces give kernel times')
        r['model'] = dict(md, t_mfma_us=t_mfma * 1e6, t_hbm_us=t_hbm * 1e6, bound='mfma' if t_mfma > t_hbm else 'hbm',
                          share_of_roofline=max(t_mfma, t_hbm) / dt, achieved_tflops=md['flop'] / dt / 1e12)
        out[name] = r
    return {'tool': 'ipnn_wide_bench', 'mode': 'digest' if dig else 'time', 'n_rows': D, 'fields': F, 'batch': B, 'steps': steps,
            'weights': weights, 'numeric_fields': n_num, 'dropout': dropout,
            'warmup': warmup, 'device': torch.cuda.get_device_name(0), 'configs': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--only', default=None)
    ap.add_argument('--fields', type=int, default=16, help='field count (2..64; more than 32: narrow rows only)')
    ap.add_argument('--weights', choices=('none', 'criteo', 'random'), default='none',
                    help='value weights of the steps (ipnn_train_step_w); none = the call without weights')
    ap.add_argument('--dropout', choices=('none', 'input', 'drawn'), default='none',
                    help='keep-masks of the steps: none = the resident masks of set-up (unchanged), input = the caller makes fresh '
                         'ones every step with torch.rand, drawn = the library draws them (ipnn_train_step_drawn)')
    ap.add_argument('--mask-cost', action='store_true', help='also time the making of one step\'s masks with torch.rand on its own')
    ap.add_argument('--no-prof', action='store_true')
    ap.add_argument('--digest', action='store_true', help='sha256 of table, layers and b after --steps steps (no timing)')
    a = ap.parse_args()
    global F
    F = a.fields
    names = (a.only or ','.join(WIDE if F == 16 else NARROW_MANY)).split(',')
    for n in names:
        if n not in CONFIGS:
            raise SystemExit('unknown config %r (%s)' % (n, ', '.join(CONFIGS)))
    print(json.dumps(run(names, a.steps, a.warmup, a.batch, not a.no_prof, a.digest, a.weights, a.dropout, a.mask_cost)))


if __name__ == '__main__':
    main()
