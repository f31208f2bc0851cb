"""The device metrics (fnn::device_metrics of csrc/metrics.hip, behind fnn_eval, fm_eval / fm_eval_w and ipnn_eval / ipnn_eval_w)
on the predictions that a trained or a diverged model makes and the other evaluation tests never do: exact 0.0 and 1.0 (the
logloss clip), large tie groups and the exact ends of the AUC, the block edges of k_metric_keys (2048 examples a block), more
than 2048 x 256 positives (the grid-stride loop of k_metric_auc), labels other than 0 / 1, a single class, and NaN.

Chosen logits reach the metric through the C ABI: an LR model (a rank-0 FM handle) with ONE field, bias 0 and the table
[[1.0], [+inf], [-inf]].  With ids = 0 and wts = z, fm_eval_w evaluates p_t = 1 / (1 + expf(-z_t)) (one field, rank 0: the
forward of fm_api.hip is z = b + wts * row[0]); an infinite logit is row 1 or 2 at weight 1, because a row's 15 padding columns
are zeros and 0 * inf would be NaN.  Every case reads the device's OWN predictions with forward(), computes tests/metrics_ref.py
on them and compares evaluate() with that: the reference never models the device's expf.  Each battery's precondition is asserted
on those predictions (metrics_ref.precondition).

Bounds: the AUC is EQUAL to the reference's (the same integer sum, the same division); RMSE and logloss within 1e-12 relative
(the bar of test_eval_metrics_equal_sklearn at values of order 1, relative because a saturated logloss reaches 10 and more); a
second evaluate returns the same three doubles bit for bit.  Every case prints its deviations."""
import ctypes as C

import numpy as np
import pytest

import metrics_ref as mr

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNEngine, FNNError
from deep_ctr_amd.ipnn import IPNNEngine
from deep_ctr_amd.LR import LR

pytestmark = pytest.mark.gpu
REL = 1e-12
INIT = ['uniform', -0.001, 0.001, [1, 2], None]
ROWS = np.asarray([[1.0], [np.inf], [-np.inf]], np.float32)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def lr_model(rows=ROWS):
    m = LR(4096, [len(rows), 1], INIT, ['sgd', 0.05], [0.0], 'train', 0)
    assert m.max_batch == 4096
    m.set_params(rows, 0.0)
    return m


@pytest.fixture(scope="module")
def lr(built):
    m = lr_model()
    yield m
    m.close()


def feed(m, z):
    """(ids [N, 1], wts [N, 1]) on the device whose logit is z: row 0 (1.0) weighted by z; +-inf is row 1 / 2 weighted by 1."""
    import torch
    z = np.asarray(z, np.float32)
    ids, w = np.zeros((len(z), 1), np.int32), z.reshape(-1, 1).copy()
    for row in (1, 2):
        hit = z == ROWS[row, 0]
        ids[hit, 0], w[hit, 0] = row, 1.0
    return torch.as_tensor(ids).to(m.device), torch.as_tensor(w).to(m.device)


def check(tag, got, again, ref):
    """got / again: (auc, rmse, logloss) of two evaluations; ref: metrics_ref's tuple."""
    d_rmse, d_ll = rel(got[1], ref[1]), rel(got[2], ref[2])
    print("[metrics-edges] %s: n_pos %d auc %.17g (reference %.17g) rmse %.17g logloss %.17g; relative deviation rmse %.2e logloss %.2e"
          % (tag, ref[3], got[0], ref[0], got[1], got[2], d_rmse, d_ll))
    assert got[0] == ref[0], (got[0], ref[0])
    assert d_rmse <= REL and d_ll <= REL, (got, ref)
    assert tuple(again) == tuple(got), (again, got)


_ran = {}


def run_battery(m, name):
    """forward, reference and two evaluations of a battery on the LR model: once per session, shared by the tests below."""
    if name not in _ran:
        z, y = mr.battery(name)
        ids_t, w_t = feed(m, z)
        p = m.forward(ids_t, wts=w_t).cpu().numpy()
        mr.precondition(name, p, y)
        ref = mr.metrics_ref(p, y)
        y = np.array(y)                                             # the battery itself stays read-only
        _ran[name] = (ids_t, w_t, p, ref, m.evaluate(ids_t, y, wts=w_t), m.evaluate(ids_t, y, wts=w_t))
    return _ran[name]


# ------------------------------------------------------------------------------------------------ 1. the batteries
@pytest.mark.parametrize("name", list(mr.BATTERIES))
def test_metrics_equal_reference(lr, name):
    _, _, p, ref, got, again = run_battery(lr, name)
    check(name, got, again, ref)
    if name in mr.EXACT_AUC:
        assert got[0] == mr.EXACT_AUC[name]
    if name == 'saturated':                                         # 36.04 an example: nothing like the 0.7 of a fresh model
        assert got[2] > 5.0


def test_labels_are_zero_or_nonzero(lr):
    """Positives labelled 1, 2, -1, INT32_MAX and INT32_MIN give the doubles of the 0 / 1 run."""
    ids_t, w_t, _, ref, got, _ = run_battery(lr, 'saturated')
    y2 = mr.relabelled(mr.battery('saturated')[1])
    assert set(mr.LABEL_VALUES) <= set(y2.tolist())
    assert tuple(lr.evaluate(ids_t, y2, wts=w_t)) == tuple(got)


# ------------------------------------------------------------------------------------------------ 2. one class, non-finite
def expect_range(call, text=None):
    with pytest.raises(FNNError) as e:
        call()
    assert e.value.code == _capi.FNN_ERR_RANGE, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_single_class_fm(lr):
    ids_t, w_t, _, ref, got, _ = run_battery(lr, 'N2049')
    for y in (np.zeros(2049, np.int32), np.full(2049, 7, np.int32)):
        expect_range(lambda: lr.evaluate(ids_t, y, wts=w_t), 'one class')
        assert tuple(lr.evaluate(ids_t, np.array(mr.battery('N2049')[1]), wts=w_t)) == tuple(got)


def fm_eval_raw(m, ids_t, w_t, y):
    """fm_eval_w itself: (rc, auc, rmse, logloss)."""
    import torch
    y_t = torch.as_tensor(np.ascontiguousarray(y, np.int32)).to(m.device)
    out = [C.c_double(-7.0) for _ in range(3)]
    m.stream.wait_stream(torch.cuda.current_stream(m.device))
    rc = m.lib.fm_eval_w(m.h, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0],
                         *[C.byref(v) for v in out])
    return (rc,) + tuple(v.value for v in out)


def test_nan_logit_is_an_error(lr):
    """One NaN among 9,001 predictions: FNN_ERR_RANGE, the three outputs NaN, the count in the message; the handle evaluates the
    finite battery afterwards.  (Before the count, the NaN's key sorted above every finite p and fmax(NaN, eps) = eps gave it a
    finite logloss term: FNN_OK with a plausible AUC and logloss.)"""
    _, _, _, _, good, _ = run_battery(lr, 'saturated')
    z, y = mr.battery('saturated-nan')
    y = np.array(y)
    ids_t, w_t = feed(lr, z)
    p = lr.forward(ids_t, wts=w_t).cpu().numpy()
    mr.precondition('saturated-nan', p, y)
    with pytest.raises(ValueError):
        mr.metrics_ref(p, y)
    expect_range(lambda: lr.evaluate(ids_t, y, wts=w_t), '1 of 9001')
    rc, auc, rmse, ll = fm_eval_raw(lr, ids_t, w_t, y)
    assert rc == _capi.FNN_ERR_RANGE and np.isnan(auc) and np.isnan(rmse) and np.isnan(ll), (rc, auc, rmse, ll)
    expect_range(lambda: lr.evaluate(ids_t, np.zeros_like(y), wts=w_t), '1 of 9001')      # it outranks the single class
    gi, gw = run_battery(lr, 'saturated')[:2]
    assert tuple(lr.evaluate(gi, np.array(mr.battery('saturated')[1]), wts=gw)) == tuple(good)


def test_nan_table_row_without_weights(built):
    """A diverged model: the table's row is NaN, fm_eval (no weights) predicts NaN for every example."""
    m = lr_model(np.asarray([[np.nan]], np.float32))
    try:
        N = 2049
        ids = np.zeros((N, 1), np.int32)
        y = np.array(mr.battery('N2049')[1])
        assert np.isnan(m.forward(ids).cpu().numpy()).all()
        expect_range(lambda: m.evaluate(ids, y), '%d of %d' % (N, N))
        m.set_params(np.asarray([[0.25]], np.float32), 0.0)
        p = m.forward(ids).cpu().numpy()
        check('after-nan-table', m.evaluate(ids, y), m.evaluate(ids, y), mr.metrics_ref(p, y))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 3. fnn_eval and ipnn_eval
N_OTHER = 1000


def labels(seed):
    y = (np.random.RandomState(seed).uniform(size=N_OTHER) < 0.3).astype(np.int32)
    y[0], y[1] = 1, 0
    return y


def saturated_outputs(tag, set_bias, predict, evaluate, y):
    """Output weights zero, output bias +40, then -120: every prediction exactly 1.0, then 0.0; AUC exactly 0.5.  A NaN bias:
    FNN_ERR_RANGE, and the handle evaluates afterwards.  All-zero and all-non-zero labels: FNN_ERR_RANGE."""
    for bias, want_p in ((40.0, 1.0), (-120.0, 0.0)):
        set_bias(bias)
        p = predict()
        assert p.dtype == np.float32 and (p == np.float32(want_p)).all(), (bias, p[:4])
        ref = mr.metrics_ref(p, y)
        got, again = evaluate(y), evaluate(y)
        check('%s-bias%+d' % (tag, bias), got, again, ref)
        assert got[0] == 0.5
        for one in (np.zeros_like(y), np.full_like(y, -2 ** 31)):
            expect_range(lambda: evaluate(one), 'one class')
        assert evaluate(y) == got
    set_bias(np.nan)
    assert np.isnan(predict()).all()
    expect_range(lambda: evaluate(y), '%d of %d' % (N_OTHER, N_OTHER))
    set_bias(-120.0)
    assert evaluate(y) == got


def test_fnn_eval_saturated_single_class_and_nan(built):
    """fnn_eval's own chunk loop (max_batch 256, N = 1000), with DEVICE and with HOST arrays; want_p equals predict."""
    F, K, H1, H2 = 4, 3, 40, 20
    rng = np.random.RandomState(31)
    sizes = synth.field_sizes_tiny(300, F)
    rows, fo = synth.fm_table(sum(sizes), K, 0.05, 32), synth.field_of_row(sizes)
    ids = synth.zipf_ids(N_OTHER, sizes, 1.1, 33)
    p = {'w1': rng.uniform(-0.2, 0.2, (1 + F * K, H1)), 'b1': rng.uniform(-0.1, 0.1, H1), 'w2': rng.uniform(-0.2, 0.2, (H1, H2)),
         'b2': rng.uniform(-0.1, 0.1, H2), 'w3': np.zeros(H2), 'b3': 0.0}
    eng = FNNEngine(F, K, H1, H2, max_batch=256, precision='f32')
    try:
        eng.set_table(rows, fo, -3.0)
        y = labels(34)

        def set_bias(b):
            eng.set_dense(dict(p, b3=b))

        def ev_device(yy):
            out = eng.evaluate(ids, yy, want_p=True)
            assert np.array_equal(out['p'].cpu().numpy(), eng.predict(ids).cpu().numpy(), equal_nan=True)
            return out['auc'], out['rmse'], out['logloss']

        def ev_host(yy):
            yy = np.ascontiguousarray(yy, np.int32)
            out, ph = [C.c_double() for _ in range(3)], np.full(N_OTHER, -7.0, np.float32)
            eng.sync()
            rc = eng.lib.fnn_eval(eng.h, ids.ctypes.data, yy.ctypes.data, N_OTHER, _capi.FNN_MEM_HOST, C.byref(out[0]), C.byref(out[1]),
                                  C.byref(out[2]), ph.ctypes.data)
            eng._ck(rc)
            assert np.array_equal(ph, eng.predict(ids).cpu().numpy())
            return tuple(v.value for v in out)

        for tag, ev in (('fnn-device', ev_device), ('fnn-host', ev_host)):
            saturated_outputs(tag, set_bias, lambda: eng.predict(ids).cpu().numpy(), ev, y)
    finally:
        eng.close()


def test_ipnn_eval_saturated_single_class_and_nan(built):
    """ipnn_eval's own chunk loop on the smallest inner-product model (2 fields of k = 1, pairs, hidden 40 / 24)."""
    F, K, hidden = 2, 1, [40, 24]
    rng = np.random.RandomState(41)
    sizes = synth.field_sizes_tiny(200, F)
    table = (rng.standard_normal((sum(sizes), K)) * 0.2).astype(np.float32)
    ids = synth.zipf_ids(N_OTHER, sizes, 1.1, 42)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', pairs=True)
    try:
        d = eng.d
        assert d == [4, 40, 24, 1]
        Ws = [rng.uniform(-0.3, 0.3, (d[i], d[i + 1])) for i in range(2)] + [np.zeros((d[2], 1))]
        bs = [rng.uniform(-0.1, 0.1, d[i + 1]) for i in range(2)]
        y = labels(43)

        def evaluate(yy):
            out = eng.evaluate(ids, yy)
            return out['auc'], out['rmse'], out['logloss']

        saturated_outputs('ipnn', lambda b: eng.set_params(table, 0.1, Ws, bs + [np.asarray([b])]),
                          lambda: eng.predict(ids).cpu().numpy(), evaluate, y)
    finally:
        eng.close()
