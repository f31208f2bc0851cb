"""The host plumbing the FM group calls share (deep-ctr_amd/csrc/fm_api.hip: ArgRing, GroupCall, plan_step) on the device: every
argument ring wrapped at least once, one front handle through every group call in turn, and one group holding every layout and
update form the step plan knows.  The rule is the group calls' own: a member ends BIT FOR BIT as a twin handle with the same
table and b ends after the same sequence of solo calls.
Shapes: about 300 rows, B = 33 (no multiple of 16 or 8: both roundings of the batch), N = 50 lines, 16 and 17 fields (one and two
groups of 16), k = 1 (LR), 11 (narrow rows), 17 (wide, 16 lanes an example), 65 (wide, 32 lanes), SGD and Adam, a pair of
shared-rows members.  The batches keep every row under one column, where a step is reproducible to the bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fm_online_cases as oc
import fm_shared_cases as sc
from test_gpu_fm_step_multi import Spec, bits, check_group, state, zipf_steps

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi
from deep_ctr_amd.FM import evaluate_many, predict_many, train_online_many, train_step_many

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 18                                                             # rows a column draws from: 8 + 18 F + 1 rows, 297 and 315


def n_rows(F):
    return sc.n_rows_of(F, PER)


def ring_capacity(ring, limit):
    """Elements of a handle's argument ring: its multiplier in fm_api.hip times the header's model limit."""
    hdr = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    src = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "fm_api.hip")).read()
    mult = re.search(r"ArgRing %s\{sizeof\([\w:]+\), (\d+) \* %s\}" % (ring, limit), src)
    return int(mult.group(1)) * int(re.search(r"#define %s (\d+)" % limit, hdr).group(1))


# ------------------------------------------------------------------------------------------------ ring wrap, one test per ring
M_WRAP = 64


def wrap_calls(ring, limit):
    cap = ring_capacity(ring, limit)
    assert cap % M_WRAP == 0
    return cap // M_WRAP + 2                                         # the ring filled once, then two calls into the next round


def wrap_models(max_batch):
    """64 rank-3 models on 16 fields and their twins, each pair with its own table, lr and lambda."""
    specs = [Spec(16, 4, lr=0.02 + 0.001 * i, lam=1e-3 * (i % 5), seed=20 + i % 7, n_rows=n_rows(16), max_batch=max_batch) for i in range(M_WRAP)]
    return [s.model(max_batch) for s in specs], [s.model(max_batch) for s in specs]


def arrays(models):
    M = len(models)
    return ((C.c_void_p * M)(*[m.h.value for m in models]), (C.c_float * M)(*[m.lr for m in models]),
            (C.c_float * M)(*[m.lam for m in models]), (C.c_int * M)(*[m.reduce_mean for m in models]))


def assert_twins(group, twins):
    """b of every model, the table of the first and the last."""
    import torch
    torch.cuda.synchronize()
    for i, (m, t) in enumerate(zip(group, twins)):
        assert m.lib.fm_sync(m.h) == 0 and t.lib.fm_sync(t.h) == 0
        if i in (0, len(group) - 1):
            (rows, b), (trows, tb) = m.get_params(), t.get_params()
            assert np.array_equal(bits(rows), bits(trows)), 'table of model %d' % i
        else:
            b, tb = C.c_float(), C.c_float()
            assert m.lib.fm_get_b(m.h, C.byref(b)) == 0 and t.lib.fm_get_b(t.h, C.byref(tb)) == 0
            b, tb = b.value, tb.value
        assert np.float32(b).tobytes() == np.float32(tb).tobytes(), 'b of model %d' % i
    for m in group + twins:
        m.close()


def test_the_step_ring_wraps(built):
    """4 * 1024 / 64 + 2 fm_train_step_multi calls in a row with nothing read back between them: the host runs ahead of the
    copies, and the wrap has to wait for them.  Three batches in turn, so that a slot read late would hold another batch's ids."""
    import torch
    calls = wrap_calls('step_ring', 'FM_STEP_MAX_MODELS')
    group, twins = wrap_models(16)
    lib, m0 = group[0].lib, group[0]
    feed = [(m0._dev(ids, torch.int32), m0._dev(y, torch.float32)) for ids, _, y in zipf_steps(16, 16, 3, 900, False, per=PER)]
    hs, lr, lam, mean = arrays(group)
    torch.cuda.synchronize()
    for c in range(calls):
        ids, y = feed[c % 3]
        assert lib.fm_train_step_multi(hs, M_WRAP, ids.data_ptr(), None, y.data_ptr(), 16, lr, lam, mean, None, None) == 0
    for c in range(calls):
        ids, y = feed[c % 3]
        for t in twins:
            assert lib.fm_train_step_w(t.h, ids.data_ptr(), None, y.data_ptr(), 16, t.lr, t.lam, t.reduce_mean, None, None) == 0
    assert_twins(group, twins)


def test_the_online_ring_wraps(built):
    """8 * 1024 / 64 + 2 launches as that many fm_train_online_multi calls of 16 lines: shorter than one call cut into as many
    launches (FM_ONLINE_CHUNK lines each, or a fold of the lazy scale per launch), and the ring has to last from call to call."""
    import torch
    calls = wrap_calls('online_ring', 'FM_ONLINE_MAX_MODELS')
    group, twins = wrap_models(1)
    lib, m0 = group[0].lib, group[0]
    feed = []
    for i in range(3):
        _, ids, _, y = oc.build(16, 4, 16, 910 + i, False, n_rows=n_rows(16))
        feed.append((m0._dev(ids, torch.int32), m0._dev(y, torch.float32)))
    hs, lr, lam, _ = arrays(group)
    torch.cuda.synchronize()
    for c in range(calls):
        ids, y = feed[c % 3]
        assert lib.fm_train_online_multi(hs, M_WRAP, ids.data_ptr(), None, y.data_ptr(), 16, lr, lam, None, None, None) == 0
    for c in range(calls):
        ids, y = feed[c % 3]
        for t in twins:
            assert lib.fm_train_online(t.h, ids.data_ptr(), None, y.data_ptr(), 16, t.lr, t.lam, None, None, None) == 0
    assert_twins(group, twins)


def test_the_eval_ring_wraps(built):
    """4 * 1024 / 64 + 2 fm_predict_multi calls in a row, each into its own block of p, nothing synchronised between them."""
    import torch
    calls = wrap_calls('eval_ring', 'FM_EVAL_MAX_MODELS')
    group, twins = wrap_models(16)
    lib, m0 = group[0].lib, group[0]
    feed = [m0._dev(oc.build(16, 4, 16, 920 + i, False, n_rows=n_rows(16))[1], torch.int32) for i in range(3)]
    want = [torch.stack([t.forward(ids) for t in twins]) for ids in feed]
    p = torch.zeros((calls, M_WRAP, 16), dtype=torch.float32, device=m0.device)
    hs = arrays(group)[0]
    torch.cuda.synchronize()
    for c in range(calls):
        p_arr = (C.c_void_p * M_WRAP)(*[p[c, m].data_ptr() for m in range(M_WRAP)])
        assert lib.fm_predict_multi(hs, M_WRAP, feed[c % 3].data_ptr(), None, 16, p_arr) == 0
    torch.cuda.synchronize()
    for c in range(calls):
        assert np.array_equal(bits(p[c].cpu().numpy()), bits(want[c % 3].cpu().numpy())), 'call %d' % c
    assert_twins(group, twins)


# ------------------------------------------------------------------------------------------------ one front handle, every call
def test_one_front_handle_through_every_group_call(built):
    """A plain model in front, a pair of shared-rows members (one grouping class: the second one's marks are the copied ones) and
    an Adam member, each on its own stream.  Twice round: step, online (the SGD members), predict, eval, and a solo step of a
    member, all with the same hs[0] -- its three rings and its one join event in turn.  The twins take the same calls solo."""
    F, B, N = 17, 33, 50
    specs = [Spec(F, 11, lr=0.05, lam=1e-2, seed=1, n_rows=n_rows(F)), Spec(F, 11, lr=0.04, lam=2e-2, seed=2, n_rows=n_rows(F), shared=True, mean=0),
             Spec(F, 17, lr=0.03, lam=0.0, seed=3, n_rows=n_rows(F), shared=True), Spec(F, 11, lr=0.01, lam=1e-3, seed=4, n_rows=n_rows(F), opt='adam')]
    steps = zipf_steps(F, B, 4, 930, True, per=PER)
    lines = []
    for i in range(2):
        _, ids, wts, y = oc.build(F, 4, N, 940 + i, True, n_rows=n_rows(F))
        lines.append((ids, wts, y))

    def run(many):
        models = [s.model(B) for s in specs]
        assert len(set(m.stream.cuda_stream for m in models)) == len(models)
        out = []

        def p_of(outs):
            return [o['p'].cpu().numpy() for o in outs]
        for rnd in range(2):
            ids, wts, y = steps[2 * rnd]
            l_ids, l_wts, l_y = lines[rnd]
            yi = (l_y > 0.5).astype(np.int32)
            if many:
                res = train_step_many(models, ids, y, wts=wts, want_p=True)
                on = train_online_many(models[:3], l_ids, l_y, wts=l_wts, want_p=True)
                ps = [p.cpu().numpy() for p in predict_many(models, l_ids, wts=l_wts)]
                ev = [(r['auc'], r['rmse'], r['logloss']) for r in evaluate_many(models, l_ids, yi, wts=l_wts)]
            else:
                res = [m.train_step(ids, y, want_p=True, wts=wts) for m in models]
                on = [m.train_online(l_ids, l_y, wts=l_wts, want_p=True) for m in models[:3]]
                ps = [m.forward(l_ids, wts=l_wts).cpu().numpy() for m in models]
                ev = [m.evaluate(l_ids, yi, wts=l_wts) for m in models]
            out += p_of(res) + [np.float32(o['loss']) for o in res] + p_of(on) + [np.float32(o['loss_last']) for o in on] + ps
            out += [np.asarray([o['loss'] for o in on], np.float64).view(np.uint32)]
            out += [np.asarray(ev, np.float64).view(np.uint32)]
            out += [np.int32(m.count_shared_rows()) for m in models[1:3]]
            ids, wts, y = steps[2 * rnd + 1]
            out += p_of([models[2].train_step(ids, y, want_p=True, wts=wts)])
        out += [x for m in models for x in state(m)]
        for m in models:
            m.close()
        return out
    got, want = run(True), run(False)
    assert len(got) == len(want)
    for i, (a, c) in enumerate(zip(got, want)):
        assert np.array_equal(bits(a), bits(c)) if np.asarray(a).dtype == np.float32 else np.array_equal(a, c), i


# ------------------------------------------------------------------------------------------------ the plan's corners
@pytest.mark.parametrize("F", [16, 17])
def test_every_layout_and_form_in_one_group_equals_solo(built, F):
    """Narrow, narrow shared, wide at 16 lanes, wide at 32, wide shared, LR and an Adam member, reduce_mean 0 and 1, three steps of
    B = 33: every member's arguments come from the plan its solo step launches.  (tests/test_gpu_fm_step_multi.py's mixed group
    has no Adam member, no k = 65 and 16 fields only.)"""
    R = n_rows(F)
    specs = [Spec(F, 11, lr=0.05, lam=1e-2, seed=1, n_rows=R, mean=1), Spec(F, 11, lr=0.04, lam=2e-2, seed=2, n_rows=R, shared=True, mean=0),
             Spec(F, 17, lr=0.03, lam=1e-2, seed=3, n_rows=R, mean=0), Spec(F, 65, lr=0.02, lam=0.0, seed=4, n_rows=R, mean=1),
             Spec(F, 17, lr=0.03, lam=3e-2, seed=5, n_rows=R, shared=True, mean=1), Spec(F, 1, lr=0.05, lam=1e-3, seed=6, n_rows=R, mean=0),
             Spec(F, 11, lr=0.01, lam=1e-3, seed=7, n_rows=R, opt='adam', mean=1), Spec(F, 65, lr=0.01, lam=0.0, seed=8, n_rows=R, opt='adam', mean=0)]
    got = check_group(specs, zipf_steps(F, 33, 3, 950 + F, F == 17, per=PER))
    assert got[6]['state'][5] == 3 and got[1]['count'] == [0, 0, 0]
