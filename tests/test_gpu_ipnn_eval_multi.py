"""ipnn_predict_multi / ipnn_eval_multi (include/ipnn_hip.h) through ipnn.predict_many / ipnn.evaluate_many: several
inner-product models on one feed in one call, against the solo calls on the same engines.  Every comparison is exact:
np.array_equal on the predictions, == on the three doubles.  The problems are test_gpu_ipnn_shapes.problem's."""
import ctypes as C
import math

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn, synth
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import IPNNEngine

from test_gpu_ipnn_shapes import problem

pytestmark = pytest.mark.gpu

ACTS = ['relu', 'tanh', 'sigmoid']
KEYS = ('auc', 'rmse', 'logloss')


def make(F, K, hidden, prec, act='relu', max_batch=256, pairs=True, seed=0, n_rows=600, set_params=True, **kw):
    table, _, _, params, _, d = problem(F, K, 8, hidden, pairs, seed=seed, n_rows=n_rows)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max_batch, precision=prec, lr=0.01, keep_prob=1.0, pairs=pairs, **kw)
    assert eng.d == d
    if set_params:
        eng.set_params(table, params['b'], params['W'], params['bias'])
    return eng


def feed(F, N, n_rows=600, seed=77):
    sizes = synth.field_sizes_tiny(n_rows, n_fields=F)
    ids = synth.zipf_ids(N, sizes, 1.1, seed).astype(np.int32)
    rng = np.random.RandomState(seed + 1)
    y = (rng.uniform(size=N) < 0.3).astype(np.int32)
    y[0], y[1] = 1, 0
    return ids, y


def weights(ids, seed=5):
    """value weights with zero and negative entries"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-1.5, 1.5, size=ids.shape).astype(np.float32)
    w[rng.uniform(size=ids.shape) < 0.1] = 0.0
    w[0, 0], w[1, 1] = 0.0, -2.0
    return w


def solo(engs, ids, y, wts=None):
    return [(e.predict(ids, wts).cpu().numpy(), e.evaluate(ids, y, wts)) for e in engs]


def assert_same(got, ref, label):
    """got: an entry of evaluate_many(want_p=True); ref: (predictions, metrics) of the solo calls"""
    assert np.array_equal(got['p'].cpu().numpy(), ref[0]), label + ': p'
    for k in KEYS:
        assert got[k] == ref[1][k], '%s: %s %r against %r' % (label, k, got[k], ref[1][k])
    assert 'status' not in got, label


def check(engs, ids, y, wts=None, refs=None):
    refs = refs if refs is not None else solo(engs, ids, y, wts)
    ps = ipnn.predict_many(engs, ids, wts)
    outs = ipnn.evaluate_many(engs, ids, y, wts, want_p=True)
    plain = ipnn.evaluate_many(engs, ids, y, wts)
    assert len(ps) == len(outs) == len(plain) == len(engs)
    for m in range(len(engs)):
        print("[ipnn-eval-multi] model %d of %d, %d lines: p sum %.9g, auc %.17g rmse %.17g logloss %.17g (solo: %.9g, %.17g %.17g %.17g)" % (
            m, len(engs), len(y), float(ps[m].double().sum()), outs[m]['auc'], outs[m]['rmse'], outs[m]['logloss'],
            float(refs[m][0].astype(np.float64).sum()), refs[m][1]['auc'], refs[m][1]['rmse'], refs[m][1]['logloss']))
        assert np.array_equal(ps[m].cpu().numpy(), refs[m][0]), 'predict_many, model %d' % m
        assert_same(outs[m], refs[m], 'evaluate_many, model %d' % m)
        assert 'p' not in plain[m] and all(plain[m][k] == refs[m][1][k] for k in KEYS), 'model %d without p' % m
    for e in engs:
        e.sync()
    return refs


def close(engs):
    for e in engs:
        e.close()


def test_one_f32_class_on_a_ragged_feed(built):
    """max_batch 256, 512, 256: feed batches of 256 lines, N = 700 is two whole ones and 188 lines; the solo calls chunk by
    256, 512 and 256."""
    engs = [make(4, 5, [40, 24], 'f32', ACTS[m], max_batch=mb, seed=10 + m) for m, mb in enumerate([256, 512, 256])]
    try:
        ids, y = feed(4, 700)
        check(engs, ids, y)
    finally:
        close(engs)


def test_one_bf16_class(built):
    engs = [make(16, 11, [300, 100], 'bf16', ACTS[m % 3], max_batch=512, seed=20 + m) for m in range(4)]
    try:
        ids, y = feed(16, 1000)
        check(engs, ids, y)
    finally:
        close(engs)


def test_mixed_list_of_8_fields_with_weights(built):
    """narrow rows, wide rows (k = 20), pairs = 0, a member on the GEMM path (a hidden layer of 1100), both element types: five
    launch classes and one member with its own launches, value weights with zeros and negative entries."""
    engs = [make(8, 5, [40, 24], 'f32', 'relu', seed=30), make(8, 20, [40, 24], 'f32', 'tanh', seed=31),
            make(8, 5, [40, 24], 'bf16', 'sigmoid', pairs=False, seed=32), make(8, 5, [1100, 40], 'f32', 'relu', seed=33),
            make(8, 5, [40, 24], 'bf16', 'tanh', max_batch=512, seed=34), make(8, 20, [64, 24], 'bf16', 'relu', seed=35),
            make(8, 7, [40, 24], 'f32', 'sigmoid', seed=36)]
    try:
        ids, y = feed(8, 600)
        check(engs, ids, y, weights(ids))
        check(engs[:4], ids, y)                        # and the same models without weights: other kernels
    finally:
        close(engs)


def test_mixed_list_of_39_fields_with_weights(built, monkeypatch):
    """39 fields, k = 11: without pairs layer 0 has 640 columns and the stack runs on the strips -- the 16-example forward by
    default, the 8-example one under IPNN_MANY_FWD_MIN=33 -- with pairs it has 1408 and the member runs GEMM launches."""
    engs = [make(39, 11, [60, 30], 'f32', 'relu', pairs=False, seed=40, n_rows=1500),
            make(39, 11, [60, 30], 'bf16', 'tanh', pairs=False, seed=41, n_rows=1500)]
    monkeypatch.setenv('IPNN_MANY_FWD_MIN', '33')
    engs += [make(39, 11, [60, 30], 'f32', 'tanh', pairs=False, seed=42, n_rows=1500),
             make(39, 11, [60, 30], 'bf16', 'relu', pairs=False, seed=43, n_rows=1500),
             make(39, 11, [60, 30], 'f32', 'sigmoid', pairs=True, seed=44, n_rows=1500)]
    monkeypatch.delenv('IPNN_MANY_FWD_MIN')
    try:
        ids, y = feed(39, 300, n_rows=1500)
        check(engs, ids, y, weights(ids))
    finally:
        close(engs)


def test_a_grid_larger_than_the_chip_and_a_second_call(built):
    """twenty bf16 models on 4096 lines: 128 strips each, 2560 strip workgroups in one launch; a second call: the same bits"""
    engs = [make(4, 5, [64, 40], 'bf16', ACTS[m % 3], max_batch=4096, seed=50 + m) for m in range(20)]
    try:
        ids, y = feed(4, 4096)
        refs = check(engs, ids, y)
        check(engs, ids, y, refs=refs)
    finally:
        close(engs)


@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_one_model(built, prec):
    engs = [make(4, 5, [40, 24], prec, 'tanh', seed=60)]
    try:
        ids, y = feed(4, 700)
        check(engs, ids, y)
    finally:
        close(engs)


def test_one_model_reports_as_a_list_does(built):
    """n_models = 1 runs the solo launches: a diverged model, one class in y and an id outside the table are still reported in
    the group call's way, and want_p still gets the predictions."""
    engs = [make(4, 5, [40, 24], 'f32', 'relu', seed=61)]
    try:
        ids, y = feed(4, 700)
        ref = solo(engs, ids, y)[0]
        out = ipnn.evaluate_many(engs, ids, np.ones(700, np.int32))[0]
        assert math.isnan(out['auc']) and out['status'] == _capi.FNN_ERR_RANGE and 'only one class' in out['error']
        assert out['rmse'] > 0 and out['logloss'] > 0
        bad = ids.copy()
        bad[3, 1] = 10 ** 6
        with pytest.raises(FNNError) as ei:
            ipnn.evaluate_many(engs, bad, y)
        assert str(ei.value).endswith(': ipnn_eval_multi: feature id outside [0, n_rows) in model(s) 0')
        assert_same(ipnn.evaluate_many(engs, ids, y, want_p=True)[0], ref, 'after the refusals')
        b, Ws, bs = engs[0].get_params()
        Ws[2][:] = np.nan
        engs[0].set_params(problem(4, 5, 8, [40, 24], True, seed=61)[0], b, Ws, bs)
        out = ipnn.evaluate_many(engs, ids, y, want_p=True)[0]
        assert out['status'] == _capi.FNN_ERR_RANGE and all(math.isnan(out[k]) for k in KEYS)
        assert out['error'] == 'ipnn_eval_multi: predictions NaN or outside [0, 1] in model(s) 0'
        assert bool(out['p'].isnan().any())
    finally:
        close(engs)


@pytest.mark.parametrize("knob", ['one', 'two'])
def test_where_the_metric_groups_are_cut_changes_no_bit(built, monkeypatch, knob):
    """One model's scratch at N = 2000 is 3 x 8192 (predictions, keys, their copy) + 1024 of histograms + 1280: 26,624 bytes,
    two models' 51,456, three models' 77,568.  30,096 holds one model and not two, 60,192 two and not three."""
    engs = [make(4, 5, [40, 24], 'f32' if m != 1 else 'bf16', ACTS[m], seed=70 + m) for m in range(3)]
    try:
        ids, y = feed(4, 2000)
        refs = check(engs, ids, y)
        monkeypatch.setenv('IPNN_EVAL_SCRATCH_BYTES', '30096' if knob == 'one' else '60192')
        check(engs, ids, y, refs=refs)
    finally:
        close(engs)


def test_after_a_train_step_whose_dense_update_is_still_pending(built, monkeypatch):
    """IPNN_UPDATE_SIDE=1 leaves a step's dense update and sparse-row chain running on the side stream; the group call joins
    them, reads the stepped models and changes nothing: a further step on both sets leaves bit-equal parameters and rows."""
    monkeypatch.setenv('IPNN_UPDATE_SIDE', '1')
    spec = [(4, 5, [40, 24], 'f32', 'relu'), (4, 5, [64, 40], 'bf16', 'tanh')]
    engs = [make(*s, seed=80 + m) for m, s in enumerate(spec)]
    twins = [make(*s, seed=80 + m) for m, s in enumerate(spec)]
    try:
        ids, y = feed(4, 700)
        tids, ty = feed(4, 256, seed=91)
        tids2, ty2 = feed(4, 256, seed=93)
        for e in engs + twins:
            e.train_step(tids, ty.astype(np.float32), want_loss=False)
        outs = ipnn.evaluate_many(engs, ids, y, want_p=True)
        refs = solo(twins, ids, y)
        for m in range(2):
            assert_same(outs[m], refs[m], 'model %d' % m)
        for e in engs + twins:
            e.train_step(tids2, ty2.astype(np.float32), want_loss=False)
        rows = np.arange(sum(synth.field_sizes_tiny(600, n_fields=4)))
        for e, t in zip(engs, twins):
            e.sync(), t.sync()
            (b1, W1, c1), (b2, W2, c2) = e.get_params(), t.get_params()
            assert b1 == b2 and all(np.array_equal(u, v) for u, v in zip(W1 + c1, W2 + c2))
            assert np.array_equal(e.get_rows(rows), t.get_rows(rows))
    finally:
        close(engs + twins)


def test_a_diverged_model_costs_the_others_nothing(built):
    engs = [make(4, 5, [40, 24], 'f32', ACTS[m], seed=100 + m) for m in range(3)]
    try:
        b, Ws, bs = engs[1].get_params()
        Ws[1][:] = np.nan
        table = problem(4, 5, 8, [40, 24], True, seed=101)[0]
        engs[1].set_params(table, b, Ws, bs)
        ids, y = feed(4, 700)
        refs = solo([engs[0], engs[2]], ids, y)
        with pytest.raises(FNNError) as ei:
            engs[1].evaluate(ids, y)
        assert ei.value.code == _capi.FNN_ERR_RANGE
        outs = ipnn.evaluate_many(engs, ids, y, want_p=True)
        assert_same(outs[0], refs[0], 'model 0')
        assert_same(outs[2], refs[1], 'model 2')
        assert outs[1]['status'] == _capi.FNN_ERR_RANGE and all(math.isnan(outs[1][k]) for k in KEYS)
        assert outs[1]['error'] == 'ipnn_eval_multi: predictions NaN or outside [0, 1] in model(s) 1'
        # the raw call: FNN_ERR_RANGE, the status array names the model
        rc, st = raw_eval(engs, ids, y)[:2]
        assert rc == _capi.FNN_ERR_RANGE and list(st) == [0, _capi.FNN_ERR_RANGE, 0]
    finally:
        close(engs)


def raw_eval(engs, ids, y, hs=None, fill=-7.0):
    """ipnn_eval_multi itself with recognisable outputs: (rc, status, auc, rmse, logloss, p tensors, message)"""
    import torch
    e0 = engs[0]
    hs = hs if hs is not None else [e.h.value for e in engs]
    M = len(hs)
    ids_t, y_t = e0._dev(ids, torch.int32), e0._dev(y, torch.int32)
    torch.cuda.synchronize()
    ps = [torch.full((ids_t.shape[0],), fill, dtype=torch.float32, device=e0.device) for _ in range(M)]
    auc, rmse, ll = (C.c_double * M)(*[fill] * M), (C.c_double * M)(*[fill] * M), (C.c_double * M)(*[fill] * M)
    st = (C.c_int * M)(*[-7] * M)
    torch.cuda.synchronize()
    rc = e0.lib.ipnn_eval_multi((C.c_void_p * M)(*hs), M, ids_t.data_ptr(), None, y_t.data_ptr(), ids_t.shape[0], auc, rmse, ll, st,
                                (C.c_void_p * M)(*[t.data_ptr() for t in ps]))
    torch.cuda.synchronize()
    return rc, st, auc, rmse, ll, ps, (e0.lib.ipnn_last_error(e0.h) or b'').decode()


def test_one_class_in_y(built):
    import torch
    engs = [make(4, 5, [40, 24], 'f32', ACTS[m], seed=110 + m) for m in range(2)]
    try:
        ids, _ = feed(4, 700)
        y = np.zeros(700, np.int32)
        ref = []
        for e in engs:
            ids_t, y_t = e._dev(ids, torch.int32), e._dev(y, torch.int32)
            auc, rmse, ll = C.c_double(), C.c_double(), C.c_double()
            torch.cuda.synchronize()
            assert e.lib.ipnn_eval(e.h, ids_t.data_ptr(), y_t.data_ptr(), 700, C.byref(auc), C.byref(rmse), C.byref(ll)) == _capi.FNN_ERR_RANGE
            ref.append((rmse.value, ll.value))
        outs = ipnn.evaluate_many(engs, ids, y)
        for m in range(2):
            assert math.isnan(outs[m]['auc']) and (outs[m]['rmse'], outs[m]['logloss']) == ref[m]
            assert outs[m]['status'] == _capi.FNN_ERR_RANGE and 'only one class' in outs[m]['error']
    finally:
        close(engs)


def test_an_id_outside_one_table_only(built):
    engs = [make(4, 5, [40, 24], 'f32', 'relu', seed=120, n_rows=600), make(4, 5, [40, 24], 'f32', 'tanh', seed=121, n_rows=900)]
    try:
        small = sum(synth.field_sizes_tiny(600, n_fields=4))
        assert small < sum(synth.field_sizes_tiny(900, n_fields=4))
        ids, y = feed(4, 700)
        bad = ids.copy()
        bad[300, 2] = small                               # a row of the larger table only
        with pytest.raises(FNNError) as ei:
            ipnn.evaluate_many(engs, bad, y)
        assert ei.value.code == _capi.FNN_ERR_RANGE
        assert str(ei.value).endswith(': ipnn_eval_multi: feature id outside [0, n_rows) in model(s) 0')
        check(engs, ids, y)                               # the flags are cleared: a clean feed succeeds
        ipnn.predict_many(engs, bad)                      # predict_many leaves the flag to the engine's own sync
        with pytest.raises(FNNError) as ei:
            engs[0].sync()
        assert ei.value.code == _capi.FNN_ERR_RANGE
        engs[1].sync()
        engs[0].sync()
    finally:
        close(engs)


def test_refusals_that_need_a_device(built):
    e4 = [make(4, 5, [40, 24], 'f32', ACTS[m], seed=130 + m) for m in range(2)]
    e8 = make(8, 5, [40, 24], 'f32', 'relu', seed=133)
    bare = make(4, 5, [40, 24], 'f32', 'relu', seed=134, set_params=False)
    try:
        ids, y = feed(4, 300)
        h = [e.h.value for e in e4]
        cases = [([h[0], h[1], h[0]], _capi.FNN_ERR_ARG, 'ipnn_eval_multi: model 2: the same handle as model 0'),
                 ([h[0], e8.h.value], _capi.FNN_ERR_ARG, "ipnn_eval_multi: model 1: n_fields or device differs from model 0's"),
                 ([h[0], h[1], bare.h.value], _capi.FNN_ERR_STATE, 'ipnn_eval_multi: model 2: ipnn_set_table has not been called')]
        for hs, code, text in cases:
            rc, st, auc, rmse, ll, ps, msg = raw_eval(e4, ids, y, hs=hs)
            assert rc == code and msg.startswith(text), (rc, msg)
            assert list(st) == [-7] * len(hs) and all(list(a) == [-7.0] * len(hs) for a in (auc, rmse, ll))
            assert all(bool((t == -7.0).all()) for t in ps)
        with pytest.raises(FNNError) as ei:
            ipnn.predict_many([e4[0], e4[1], e4[0]], ids)
        assert ei.value.code == _capi.FNN_ERR_ARG and 'ipnn_predict_multi: model 2: the same handle as model 0' in str(ei.value)
        check(e4, ids, y)
    finally:
        close(e4 + [e8, bare])
