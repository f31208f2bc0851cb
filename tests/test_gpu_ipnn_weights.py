"""Value weights of the inner-product family (ipnn_train_step_w / ipnn_predict_w / ipnn_eval_w, `wts=` in deep_ctr_amd.ipnn):
e_f = wts[t, f] * table[ids[t, f]] through all six inner-product kernels -- the 16-example pair (k_ip_fwd / k_ip_bwd), the
many-field pair (k_ip_fwd_m / k_ip_bwd_m, 33 .. 64 fields) and the wide pair (k_ip_fwd_w / k_ip_bwd_w, k = 17 .. 128) -- against
the float64 reference of tests/ipnn_weighted_ref.py (the oracle with the one-line definition above).

Bounds are the project's own, unchanged: check_f32_step's for one f32 step, test_fields_bf16_three_steps_track_oracle's for bf16,
test_ipnn_shape_optimiser_steps_vs_oracle's for Adam and FTRL, 1e-12 on the metrics.  The absolute bounds were written for logits
of order 1, so every reference case asserts the reference's own |logits| < 4.  Weights are uniform in [-0.5, 2), different per
example and per field, with exact 0 and exact 1 among them (ipnn_weighted_ref.test_weights); each case prints its worst error as
a fraction of its bound.  Shapes are the smallest that reach each kernel and its edges: B = 1 (one example of a padded batch),
17 / 9 (a partial workgroup) and 257 (a second batch tile), K = 1, a K that is no multiple of 4, and a full slot."""
import pickle

import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import FM
from deep_ctr_amd.ipnn import FNN_IP_L3, IPNNEngine, criteo_feed

import ipnn_weighted_ref as wr
from test_gpu_ipnn_fields import KNOBS
from test_gpu_ipnn_shapes import Bounds, copy_params, cosine, lr_for, oracle_pairs, problem

pytestmark = pytest.mark.gpu

ENVS = {None: {}, 'gemm': {'IPNN_STRIP': '0'}}      # 'gemm': one GEMM launch per product instead of the strip kernels
ENVS.update({k: v for k, v in KNOBS.items() if k})  # 'b16' / 'f8': the other kernel of a many-field handle, where it can run


def check_f32_step_w(eng, prob, wts, act, lr, drop, keep, pairs, label, zero_cols=()):
    """check_f32_step with weights: predict before the step (rtol 2e-4), logits (rtol 2e-4, atol 2e-5), loss (5e-5 relative),
    every W, bias and b and every touched row within 2e-3 of its own change; untouched rows bit-unchanged -- and so is a row
    whose every weight in the batch is an exact 0 (its gradient is a sum of zeros)."""
    table, ids, y, params, masks, d = prob
    bd = Bounds()
    m64 = [m.astype(np.float64) for m in masks] if drop else None
    with oracle_pairs(pairs):
        bd.close('predict', eng.predict(ids, wts).cpu().numpy(), wr.predict_w(params, table, ids, wts, act), 2e-4, 1e-6)
        out = eng.train_step(ids, y, masks if drop else None, want_logits=True, wts=wts)
        p0, t0 = copy_params(params), table.copy()
        loss, logits, _ = wr.sgd_step_w(params, table, ids, wts, y, act, lr, m64, keep)
    assert np.abs(logits).max() < 4.0, "the reference's own logits are not of order 1"
    bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-4, 2e-5)
    bd.close('loss', out['loss'], loss, 0.0, 5e-5 * max(1.0, abs(loss)))
    b, Ws, bs = eng.get_params()
    for t in range(len(Ws)):
        bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 2e-3 * (np.abs(params['W'][t] - p0['W'][t]).max() + 1e-12) + 2e-7)
        bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 2e-3 * (np.abs(params['bias'][t] - p0['bias'][t]).max() + 1e-12) + 2e-7)
    bd.close('b', b, params['b'], 0.0, 2e-3 * abs(params['b'] - p0['b']) + 2e-7)
    rows = eng.get_rows(np.arange(table.shape[0]))
    touched = np.unique(ids)
    tbound = 2e-3 * (np.abs(table - t0).max() + 1e-12) + 2e-7
    bd.close('table', rows[touched], table[touched], 0.0, tbound)
    untouched = np.setdiff1d(np.arange(table.shape[0]), touched)
    assert np.array_equal(rows[untouched], t0[untouched].astype(np.float32)), "a row no example touched moved"
    live = np.unique(ids[np.asarray(wts) != 0])
    dead = np.setdiff1d(touched, live)                       # touched with weight 0 only
    assert np.array_equal(rows[dead], t0[dead].astype(np.float32)), "a row that only zero weights touched moved"
    for c in zero_cols:
        assert set(np.unique(ids[:, c]).tolist()) <= set(dead.tolist())
    bd.report(label)
    return bd, rows, tbound


def run_step_case(monkeypatch, F, K, pairs, hidden, B, act, drop, env, n_rows=1500):
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B, n_rows=n_rows)
    wts = wr.test_weights(B, F, 7 * F + K + B)
    keep, lr = (0.7 if drop else 1.0), lr_for(B)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=lr, keep_prob=keep, pairs=bool(pairs))
    try:
        assert eng.d == prob[5]
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step_w(eng, prob, wts, act, lr, drop, keep, pairs,
                         'w-F%d-K%d-%s-H%s-B%d-%s-%s' % (F, K, 'P' if pairs else 'noP', 'x'.join(map(str, hidden)), B, act, env))
    finally:
        eng.close()


def _ids(cases):
    return ['F%d-K%d-%s-H%s-B%d-%s-%s-%s' % (F, K, 'P' if p else 'noP', 'x'.join(map(str, h)), B, a, 'drop' if dr else 'nodrop', e or 'default')
            for (F, K, p, h, B, a, dr, e) in cases]


# ------------------------------------------------------------------------------------------------ 1. one f32 SGD step
# (F, K, pairs, hidden, B, act, drop, env)
NARROW = [
    (2, 1, 1, [40, 24], 1, 'relu', True, None), (16, 11, 1, [300, 100], 257, 'tanh', True, None), (16, 11, 1, [300, 100], 257, 'tanh', False, 'gemm'),
    (32, 16, 1, [100, 50], 17, 'relu', False, None), (23, 5, 1, [130, 60], 257, 'sigmoid', True, None), (23, 5, 1, [130, 60], 257, 'relu', True, 'gemm'),
    (16, 11, 0, [64, 30], 257, 'tanh', True, None),
]
# default above 32 fields: the 16-example forward while its tile fits the LDS (33 .. 45 fields with pairs), the 4-example backward;
# 'b16' keeps the 16-example backward, 'f8' runs the 8-example forward from 33 fields on.  A layer 0 wider than 1024 columns
# (39 fields and more with pairs) is the GEMM path, the others the strips
MANY = [
    (33, 1, 1, [40, 24], 17, 'relu', True, None), (33, 16, 0, [64, 30], 257, 'tanh', False, None), (39, 11, 1, [60, 30], 257, 'tanh', True, None),
    (39, 16, 1, [64, 63], 1, 'relu', False, None), (46, 11, 1, [50, 30], 257, 'sigmoid', True, None), (46, 1, 1, [40], 1, 'relu', True, None),
    (64, 16, 1, [50, 20], 257, 'relu', True, None), (64, 11, 0, [40], 17, 'tanh', True, None), (64, 1, 1, [40], 17, 'tanh', False, None),
    (39, 11, 1, [60, 30], 257, 'relu', True, 'b16'), (33, 16, 1, [100, 50], 17, 'tanh', True, 'b16'), (64, 11, 0, [40, 20], 257, 'relu', False, 'b16'),
    (39, 11, 1, [60, 30], 257, 'relu', True, 'f8'), (33, 1, 1, [40], 17, 'sigmoid', False, 'f8'), (39, 16, 0, [40, 20], 1, 'tanh', True, 'f8'),
]
WIDE = [
    (2, 17, 1, [40, 24], 1, 'relu', True, None), (16, 51, 1, [100, 50], 257, 'tanh', True, None), (16, 51, 1, [100, 50], 9, 'relu', False, 'gemm'),
    (32, 101, 1, [60, 30], 9, 'relu', True, None), (3, 128, 1, [64, 30], 257, 'sigmoid', False, None), (3, 128, 0, [64, 30], 9, 'tanh', True, None),
]


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop,env", NARROW, ids=_ids(NARROW))
def test_weighted_step_f32_16_example_kernels(built, monkeypatch, F, K, pairs, hidden, B, act, drop, env):
    run_step_case(monkeypatch, F, K, pairs, hidden, B, act, drop, env, n_rows=600)


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop,env", MANY, ids=_ids(MANY))
def test_weighted_step_f32_many_field_kernels(built, monkeypatch, F, K, pairs, hidden, B, act, drop, env):
    run_step_case(monkeypatch, F, K, pairs, hidden, B, act, drop, env)


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop,env", WIDE, ids=_ids(WIDE))
def test_weighted_step_f32_wide_kernels(built, monkeypatch, F, K, pairs, hidden, B, act, drop, env):
    run_step_case(monkeypatch, F, K, pairs, hidden, B, act, drop, env, n_rows=600)


# ------------------------------------------------------------------------------------------------ 2. the Criteo layout
N_NUM, N_CAT = 13, 26


def criteo_problem(B, K, hidden, seed, n_rows=1500, keep_p=0.7):
    """problem() on 39 fields with the ids and weights of synth.criteo_like: rows 0 .. 12 are the numeric fields'."""
    F = N_NUM + N_CAT
    table, _, y, params, masks, d = problem(F, K, B, hidden, True, seed=seed, n_rows=n_rows, keep_p=keep_p)
    ids, wts = synth.criteo_like(B, N_NUM, synth.field_sizes_tiny(n_rows - N_NUM, N_CAT), seed=seed + 1)
    assert ids.max() < table.shape[0]
    return (table, ids, y, params, masks, d), wts


def test_weighted_criteo_layout_full_batch(built):
    """39 = 13 numeric + 26 categorical fields, K = 11, 400 / 400 / 200, one f32 step on a batch of 4096: each numeric field is ONE
    row for the whole batch -- a run of 4096 in its field through the sparse-row update's chunk partials and single owner.  The
    13 numeric rows are compared one by one (each against the table bound of check_f32_step); field 5 carries exact-zero
    weights only, and its row does not move by a bit."""
    F, K, hidden, B = 39, 11, [400, 400, 200], 4096
    prob, wts = criteo_problem(B, K, hidden, seed=390)
    wts[:, 5] = 0.0
    table, ids = prob[0], prob[1]
    t0 = table.copy()
    lr = lr_for(B)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='f32', lr=lr, keep_prob=0.7)
    try:
        eng.set_params(table, prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        bd, rows, tbound = check_f32_step_w(eng, prob, wts, 'relu', lr, True, 0.7, True, 'w-criteo-F39-K11-B4096', zero_cols=(5,))
        assert np.array_equal(rows[5], t0[5].astype(np.float32))
        nb = Bounds()
        for i in range(N_NUM):
            if i != 5:
                assert np.abs(table[i] - t0[i]).max() > 0
                nb.close('numeric row %d' % i, rows[i], table[i], 0.0, tbound)
                print("[ipnn-weights] numeric row %2d: moved %.3e, error %.3f of the bound" %
                      (i, np.abs(table[i] - t0[i]).max(), np.abs(rows[i] - table[i]).max() / tbound))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. bf16, three steps
@pytest.mark.parametrize("layout", ['criteo-F39-K11', 'wide-F16-K51'])
def test_weighted_bf16_three_steps_track_reference(built, layout):
    """test_fields_bf16_three_steps_track_oracle's bounds and lr (0.002, B = 1024) with weights: logits within 5e-2 and loss within
    2 % after each of three steps, every weight's accumulated update with a cosine above 0.99."""
    B, steps, lr = 1024, 3, 0.002
    if layout.startswith('criteo'):
        F, K, hidden = 39, 11, [400, 400, 200]
        (table, ids, y, params, masks, d), wts = criteo_problem(B * steps, K, hidden, seed=61)
    else:
        F, K, hidden = 16, 51, [400, 200]
        table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=62)
        wts = wr.test_weights(B * steps, F, 63)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=lr, keep_prob=0.7)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0 = [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True, wts=wts[sl])
            loss, logits, _ = wr.sgd_step_w(params, table, ids[sl], wts[sl], y[sl], 'relu', lr, [m[sl].astype(np.float64) for m in masks], 0.7)
            assert np.abs(logits).max() < 4.0, "the reference's own step overshoots: the problem is ill-posed"
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 0.0, 5e-2)
            bd.close('loss%d' % s, out['loss'], loss, 0.0, 2e-2 * abs(loss))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.above('cos W%d' % t, cosine(Ws[t] - p0[t], params['W'][t] - p0[t]), 0.99, 0.01)
        bd.report('w-bf16-3steps-' + layout)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. Adam and FTRL
OPT = [(16, 11), (39, 11), (16, 51)]


@pytest.mark.parametrize("opt", ['adam', 'ftrl'])
@pytest.mark.parametrize("F,K", OPT, ids=['narrow-F16-K11', 'many-F39-K11', 'wide-F16-K51'])
def test_weighted_optimiser_steps_vs_reference(built, F, K, opt):
    """Two Adam / FTRL steps with weights, each on a batch of its own, with the bounds of test_ipnn_shape_optimiser_steps_vs_oracle;
    a row no step touched is bit-unchanged under Adam and exactly 0 under FTRL."""
    hidden, B, steps = [40, 24, 12], 160, 2
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=21 + F + K, n_rows=1500)
    wts = wr.test_weights(B * steps, F, 22 + F + K)
    lr = 1e-3 if opt == 'adam' else 1e-2
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=lr, keep_prob=0.7, optimizer=opt, adam_eps=1e-8)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        st = io.adam_state(params, table) if opt == 'adam' else io.ftrl_state(params, table)
        t0, W0 = table.copy(), [w.copy() for w in params['W']]
        never = np.setdiff1d(np.arange(table.shape[0]), np.unique(ids))
        assert len(never) > 0
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True, wts=wts[sl])
            m64 = [m[sl].astype(np.float64) for m in masks]
            if opt == 'adam':
                loss, logits, _ = wr.adam_step_w(params, table, ids[sl], wts[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 5e-4, 5e-5)
            else:
                loss, logits, _ = wr.ftrl_step_w(params, table, ids[sl], wts[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 2e-3, 2e-5)
                bd.close('loss%d' % s, out['loss'], loss, 0.0, 1e-4 * abs(loss))
            assert np.abs(logits).max() < 4.0
        b, Ws, bs = eng.get_params()
        rows = eng.get_rows(np.arange(table.shape[0]))
        if opt == 'adam':
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - W0[t]).max() + 1e-7)
            bd.close('table', rows, table, 0.0, 5e-3 * np.abs(table - t0).max() + 1e-7)
            assert np.array_equal(rows[never], t0[never].astype(np.float32))
        else:
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t]).max() + 1e-7)
                bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 5e-3 * np.abs(params['bias'][t]).max() + 1e-7)
            bd.close('b', b, params['b'], 0.0, 5e-3 * abs(params['b']) + 1e-7)
            bd.close('table', rows, table, 0.0, 5e-3 * np.abs(table).max() + 1e-7)
            assert not rows[never].any()
        bd.report('w-%s-F%d-K%d' % (opt, F, K))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. None is ones; determinism
def _three_steps(F, K, hidden, prec, data, wts):
    table, ids, y, params, masks, d = data
    B, steps = ids.shape[0] // 3, 3
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=max(256, B), precision=prec, lr=0.002, keep_prob=0.7)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        logits = []
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True, wts=None if wts is None else wts[sl])
            logits.append(out['logits'].cpu().numpy().copy())
        b, Ws, bs = eng.get_params()
        return np.concatenate(logits), b, Ws, bs, eng.get_rows(np.arange(table.shape[0]))
    finally:
        eng.close()


def _bit_equal(ra, rb):
    (la, ba, Wa, bsa, rowa), (lb, bb, Wb, bsb, rowb) = ra, rb
    assert np.isfinite(la).all() and np.abs(la).max() > 0
    assert np.array_equal(la, lb), "logits differ"
    assert ba == bb, "b differs"
    assert np.array_equal(rowa, rowb), "the tables differ"
    for t in range(len(Wa)):
        assert np.array_equal(Wa[t], Wb[t]) and np.array_equal(bsa[t], bsb[t]), t


@pytest.mark.parametrize("F,K,prec", [(16, 11, 'f32'), (46, 11, 'bf16'), (39, 11, 'f32'), (16, 51, 'bf16')],
                         ids=['narrow-F16-K11-f32', 'many-F46-K11-bf16', 'f16b4-F39-K11-f32', 'wide-F16-K51-bf16'])
def test_no_weights_is_all_ones_and_runs_are_bit_identical(built, F, K, prec):
    """Three steps with dropout on batches of 300: wts=None and an explicit tensor of ones leave bit-identical logits, layers, b and
    tables (the whole table); two runs with the same random weights are bit-identical too, and differ from the unweighted run."""
    hidden = [100, 50]
    data = problem(F, K, 900, hidden, True, seed=50 + F + K, n_rows=1500)
    base = _three_steps(F, K, hidden, prec, data, None)
    _bit_equal(base, _three_steps(F, K, hidden, prec, data, np.ones((900, F), np.float32)))
    wts = wr.test_weights(900, F, 51 + F)
    ra = _three_steps(F, K, hidden, prec, data, wts)
    _bit_equal(ra, _three_steps(F, K, hidden, prec, data, wts))
    assert not np.array_equal(ra[0], base[0])


# ------------------------------------------------------------------------------------------------ 6. predict and evaluate
def _metrics(y, p):
    """AUC (Mann-Whitney on average ranks: ties count half), RMSE and logloss of float64 predictions, in NumPy."""
    y = np.asarray(y).astype(bool)
    order = np.argsort(p, kind='mergesort')
    ps = p[order]
    ranks = np.empty(len(p), np.float64)
    edges = np.flatnonzero(np.concatenate([[True], ps[1:] != ps[:-1], [True]]))
    for lo, hi in zip(edges[:-1], edges[1:]):
        ranks[order[lo:hi]] = 0.5 * (lo + 1 + hi)
    n1, n0 = int(y.sum()), int((~y).sum())
    auc = (ranks[y].sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * n0)
    eps = np.finfo(np.float64).eps
    pc = np.clip(p, eps, 1 - eps)
    return auc, float(np.sqrt(np.mean((p - y) ** 2))), float(-np.mean(np.where(y, np.log(pc), np.log(1 - pc))))


@pytest.mark.parametrize("F,K", [(16, 11), (39, 11), (16, 51)], ids=['narrow-F16-K11', 'many-F39-K11', 'wide-F16-K51'])
def test_weighted_predict_and_evaluate_over_chunks(built, F, K):
    """predict over N = 2 max_batch + 3 examples with weights equals the reference (the weights of a chunk travel with its ids),
    and evaluate's AUC / RMSE / logloss equal those of the same float32 predictions at 1e-12 (the tolerance of
    test_ipnn_predict_and_eval_vs_sklearn_at_32_fields): ipnn_eval_w cuts its own chunks."""
    hidden, mb = [60, 30], 256
    N = 2 * mb + 3
    table, ids, y, params, masks, d = problem(F, K, N, hidden, True, seed=78 + F, n_rows=1500)
    params['W'][-1] *= 10.0                                 # spread the predictions away from 0.5
    wts = wr.test_weights(N, F, 79 + F)
    yy = (np.random.RandomState(6).uniform(size=N) < 0.3).astype(np.int32)
    eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=mb, precision='f32', lr=0.01, keep_prob=1.0)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        pp = eng.predict(ids, wts).cpu().numpy()
        bd = Bounds()
        bd.close('predict', pp, wr.predict_w(params, table, ids, wts, 'tanh'), 2e-4, 1e-6)
        bd.report('w-predict-F%d-K%d-N%d' % (F, K, N))
        assert np.abs(pp - eng.predict(ids).cpu().numpy()).max() > 1e-3           # the weights matter
        m = eng.evaluate(ids, yy, wts)
        auc, rmse, ll = _metrics(yy, pp.astype(np.float64))
        assert abs(m['auc'] - auc) < 1e-12 and abs(m['rmse'] - rmse) < 1e-12 and abs(m['logloss'] - ll) < 1e-12, (m, auc, rmse, ll)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 7. the reference's classes
def test_fnn_ip_l3_trains_on_the_criteo_feed(built, tmp_path):
    """FNN_IP_L3 at X_feas = 39, seeded from an FM.dump, trains eight steps on what criteo_feed makes of the reference's three feeds
    (v_wts, c_ids, c_wts): the loss falls; forward(ids, wts=w) is eng.predict(ids, w); a wts of another shape raises before
    anything is launched."""
    rank, B, F = 10, 256, N_NUM + N_CAT
    sizes = synth.field_sizes_tiny(2000, N_CAT)
    D = N_NUM + sum(sizes)
    offsets = N_NUM + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rng = np.random.RandomState(6)
    c_ids = synth.zipf_ids(B, sizes, 1.1, 5) - (offsets - N_NUM)              # per-field ids, as the driver feeds them
    v_wts = rng.uniform(0.0, 2.0, size=(B, N_NUM)).astype(np.float32)
    ids, wts = criteo_feed(v_wts, c_ids, np.ones((B, N_CAT), np.float32), offsets)
    assert ids.shape == (B, F) and ids.max() < D and np.array_equal(ids[:, N_NUM:] - offsets, c_ids)
    y = (rng.uniform(size=B) < 0.3).astype(np.float64)
    fm = FM(B, [D, F, rank], ['uniform', -0.01, 0.01, [1, 2], None], ['sgd', 0.05], [1e-3], 'train', 0)
    try:
        for j in range(3):
            fm.train_step(ids, y, want_loss=False)
        rows, b = fm.get_params()
        path = str(tmp_path / 'fm.pkl')
        fm.dump(path)
    finally:
        fm.close()
    assert pickle.load(open(path, 'rb'))['V'].shape == (D, rank)
    m = FNN_IP_L3([], [], B, [D, F, rank, 300, 100, 50, 'relu'], ['uniform', -0.05, 0.05, [3, 4, 5], path], ['sgd', 0.002, 'sum'],
                  [1.0], 'train', B, precision='f32')
    try:
        assert np.array_equal(m.eng.get_rows(np.arange(D)), rows)
        with pytest.raises(ValueError):
            m.train_step(ids, y, wts=wts[:, :N_NUM])
        with pytest.raises(ValueError):
            m.forward(ids, wts=wts[:-1])
        assert np.array_equal(m.eng.get_rows(np.arange(D)), rows)            # nothing ran
        losses = [m.train_step(ids, y, wts=wts)['loss'] for _ in range(8)]
        assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
        p = m.forward(ids, wts=wts).cpu().numpy()
        assert p.shape == (B,) and np.isfinite(p).all()
        assert np.array_equal(p, m.eng.predict(ids, wts).cpu().numpy())
        assert not np.array_equal(p, m.forward(ids).cpu().numpy())
        with pytest.raises(NotImplementedError, match="criteo_feed"):
            m.forward(ids, v_wts=v_wts)
    finally:
        m.eng.close()
