"""The strip kernels and the group launches of the inner-product family on 33 to 64 fields with pairs, where layer 0 is wider than
1024 columns: two LDS tiles of unequal width (ip_strip_plan in ipnn_api.hip; the arithmetic is held by test_ipnn_plan_query).
Every case first asserts, through IPNNEngine.plan, that its engine runs the path it names.

Problems are test_gpu_ipnn_shapes.problem's on 900 rows; the bounds are those of the tests named in each docstring, unchanged.
Against another engine of this library the comparison is exact wherever only launches are regrouped (knobs, group calls).
"""
import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import Drawn, IPNNEngine

from test_gpu_ipnn_eval_multi import ACTS, check, close, feed
from test_gpu_ipnn_shapes import Bounds, check_f32_step, cosine, lr_for, oracle_pairs, padded, problem
from test_gpu_ipnn_step_multi import masks_for, step_both, two_sets
from test_gpu_ipnn_step_plumbing import KNOBS, assert_bits, assert_close, weights_of

pytestmark = pytest.mark.gpu

N_ROWS = 900


def expect_plan(eng, strips=True, shares=None):
    """the engine's own plan: strips (or the GEMM path), and two tile widths wherever layer 0 has more than 1024 columns"""
    q = eng.plan
    assert q['strips'] == strips, q
    if shares is not None:
        assert q['shares_step'] == shares, q
    if strips and q['padded'][0] > 1024:
        assert q['stack_fwd']['cap_a'] >= q['padded'][0] and q['stack_fwd']['lds_bytes'] == 64 * (q['stack_fwd']['cap_a'] + q['stack_fwd']['cap_b'])
    return q


# ------------------------------------------------------------------------------------------------ one f32 step
# (F, K, pairs, hidden, B, act, drop).  B = 300 pads to 512 (a ragged last strip), 17 to 256 (one live strip, one ragged).  45 | 46
# fields is where the forward changes from 16 to 8 examples per workgroup; [1100] at 39 fields fills the 160 KiB (2560 columns),
# [64, 1100, 64] at 33 puts a layer wider than layer 0 into layer 0's tile; without pairs layer 0 stays below 1024 columns.
STEP = [
    (33, 4, 1, [40, 24], 300, 'relu', True), (33, 11, 1, [64, 1100, 64], 300, 'tanh', True), (33, 16, 0, [64, 30], 17, 'sigmoid', True),
    (39, 11, 1, [130, 70, 40], 300, 'relu', True), (39, 11, 1, [1100], 300, 'tanh', True), (39, 4, 1, [1100], 17, 'relu', False),
    (39, 16, 1, [60, 30], 17, 'sigmoid', True), (39, 11, 0, [60, 30], 300, 'relu', True),
    (45, 16, 1, [50, 30], 300, 'relu', True), (45, 4, 1, [40], 17, 'tanh', True),
    (46, 11, 1, [70, 40], 300, 'tanh', True), (46, 16, 1, [50, 30], 17, 'relu', True), (46, 4, 0, [60], 300, 'sigmoid', False),
]


def sid(F, K, pairs, hidden, B, *rest):
    return '-'.join(['F%d-K%d-%s-Dp0_%d-H%s-B%d' % (F, K, 'P' if pairs else 'noP', padded(F, hidden, pairs)[0], 'x'.join(map(str, hidden)), B)] +
                    [str(r) for r in rest])


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop", STEP, ids=[sid(F, K, p, h, B, a, 'drop' if dr else 'nodrop') for (F, K, p, h, B, a, dr) in STEP])
def test_strips_step_f32_vs_oracle(built, F, K, pairs, hidden, B, act, drop):
    """test_fields_step_f32_vs_oracle's checks and bounds (check_f32_step) on engines that run the strip kernels."""
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B, n_rows=N_ROWS)
    keep, lr = (0.7 if drop else 1.0), lr_for(B)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=lr, keep_prob=keep, pairs=bool(pairs))
    try:
        q = expect_plan(eng, shares=True)
        assert (q['padded'][0] > 1024) == bool(pairs) and q['rows_bwd'] == 'many' and q['rows_fwd'] == ('many' if F >= 46 and pairs else 'narrow')
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, act, lr, drop, keep, pairs, sid(F, K, pairs, hidden, B, act))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ bf16, three steps
BF16 = [(39, 11, [300, 70]), (39, 4, [1100]), (46, 16, [320, 40]), (33, 11, [64, 1100, 64])]


@pytest.mark.parametrize("F,K,hidden", BF16, ids=[sid(F, K, 1, h, 1024, 'bf16') for (F, K, h) in BF16])
def test_strips_bf16_three_steps_track_oracle(built, F, K, hidden):
    """test_fields_bf16_three_steps_track_oracle's bounds, batch and lr (B = 1024, lr = 0.002; its docstring says why): logits
    within 5e-2, loss within 2 %, the accumulated update of every weight at a cosine above 0.99 with the oracle's.  64 workgroups
    of pairs: the solo forms with the tail split where the stack has a tail."""
    B, steps, lr = 1024, 3, 0.002
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=11 + F + K, n_rows=N_ROWS)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=lr, keep_prob=0.7)
    bd = Bounds()
    try:
        assert expect_plan(eng)['pairs']
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0 = [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            with oracle_pairs(True):
                loss, logits, _ = io.sgd_step(params, table, ids[sl], y[sl], 'relu', lr, [m[sl].astype(np.float64) for m in masks], 0.7)
            assert np.abs(logits).max() < 4.0, "the oracle's own step overshoots: the problem is ill-posed"
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 0.0, 5e-2)
            bd.close('loss%d' % s, out['loss'], loss, 0.0, 2e-2 * abs(loss))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.above('cos W%d' % t, cosine(Ws[t] - p0[t], params['W'][t] - p0[t]), 0.99, 0.01)
        bd.report(sid(F, K, 1, hidden, B, 'bf16', '3steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ against the GEMM path, and the knobs
HIDDEN, B2, STEPS = [300, 70], 300, 2            # test_gpu_ipnn_step_plumbing's stack: cut = 1 < L = 2, pairs on product 1, a fused tail
_PROB, _DEFAULT = {}, {}


def prob_of(F, K):
    if (F, K) not in _PROB:
        _PROB[(F, K)] = problem(F, K, B2 * STEPS, HIDDEN, seed=31 + F, n_rows=N_ROWS, keep_p=0.5)
    return _PROB[(F, K)]


def run(F, K, feed_kind, prec='bf16', strips=True):
    """test_gpu_ipnn_step_plumbing.run with the engine's plan asserted: two steps on slices of the problem, then predict"""
    table, ids, y, params, masks, d = prob_of(F, K)
    eng = IPNNEngine(F, K, HIDDEN, 'relu', max_batch=B2, precision=prec, lr=0.01, keep_prob=0.5)
    try:
        expect_plan(eng, strips=strips)
        eng.set_params(table, params['b'], params['W'], params['bias'])
        wts = weights_of(ids, 5) if feed_kind == 'wts' else None
        logits = []
        for s in range(STEPS):
            sl = slice(s * B2, (s + 1) * B2)
            m = Drawn(1234, s) if feed_kind == 'drawn' else [mm[sl] for mm in masks]
            out = eng.train_step(ids[sl], y[sl], m, want_logits=True, wts=None if wts is None else wts[sl])
            logits.append(out['logits'].cpu().numpy().copy())
        pr = eng.predict(ids[sl], wts=None if wts is None else wts[sl]).cpu().numpy().copy()
        b, Ws, bs = eng.get_params()
        return {'logits': np.concatenate(logits), 'b': b, 'W': Ws, 'bias': bs, 'rows': eng.get_rows(np.unique(ids)), 'p': pr}
    finally:
        eng.close()


@pytest.mark.parametrize("F,K", [(39, 11), (46, 4)])
def test_strips_f32_against_the_gemm_path(built, monkeypatch, F, K):
    """IPNN_STRIP_L0=0 restores one GEMM launch per product: the same epilogues, the sums regrouped -- assert_close's bound
    (test_gemm_path_f32_against_the_default_form)."""
    ref = run(F, K, 'masks', prec='f32')
    monkeypatch.setenv('IPNN_STRIP_L0', '0')
    assert_close(run(F, K, 'masks', prec='f32', strips=False), ref, prob_of(F, K), 'IPNN_STRIP_L0=0 F%d' % F)


def default_of(feed_kind):
    if feed_kind not in _DEFAULT:
        _DEFAULT[feed_kind] = run(39, 11, feed_kind)
    return _DEFAULT[feed_kind]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda e: '-'.join('%s=%s' % kv for kv in e.items()))
@pytest.mark.parametrize("feed_kind", ['wts', 'drawn'])
def test_strip_forms_are_bit_identical_at_39_fields(built, monkeypatch, feed_kind, knob):
    """(39, 11, [300, 70]) in bf16, B = 300: the default form (pairs on product 1 with a 1408-column tile beside a 320-column one,
    the fused tail, the side stream) against two tail launches, no tail split, one workgroup per strip and one stream."""
    ref = default_of(feed_kind)
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    assert_bits(run(39, 11, feed_kind), ref, (feed_kind, knob))


# ------------------------------------------------------------------------------------------------ the group calls
def member(F, K, hidden, prec, act, opt='sgd', pairs=True, seed=0, lr=0.01, keep=0.7, max_batch=256):
    table, _, _, params, _, d = problem(F, K, 8, hidden, pairs, seed=seed, n_rows=N_ROWS)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max_batch, precision=prec, lr=lr, keep_prob=keep, pairs=pairs, optimizer=opt)
    assert eng.d == d
    eng.set_params(table, params['b'], params['W'], params['bias'])
    return eng


def group_of(F):
    """k, activation, optimiser and element type mixed; [300, 70] in bf16 takes pairs and the tail split in its solo step; a
    member without pairs (layer 0 below 1024 columns: two equal tiles, as up to 32 fields) beside them; and one on the GEMM path
    ([1200] passes the LDS at 39 fields and more), which runs its own step inside the call."""
    return [member(F, 11, [60, 30], 'f32', 'relu', 'sgd', seed=1), member(F, 4, [60, 30], 'bf16', 'tanh', 'adam', seed=2, lr=1e-3),
            member(F, 16, [60, 30], 'bf16', 'sigmoid', 'ftrl', seed=3), member(F, 11, [300, 70], 'bf16', 'relu', 'sgd', seed=4),
            member(F, 11, [60, 30], 'f32', 'tanh', 'adam', seed=5, lr=1e-3), member(F, 11, [60, 30], 'f32', 'relu', pairs=False, seed=6),
            member(F, 4, [1200], 'f32', 'tanh', seed=7)]


@pytest.mark.parametrize("feed_kind", ['wts', 'drawn'])
@pytest.mark.parametrize("F", [39, 46])
def test_group_step_is_the_solo_steps(built, F, feed_kind):
    """train_step_many against twin engines' own train_step, three steps at B = 100 and three at a ragged 77: every loss, logit,
    dense tensor, b and touched row bit for bit (step_both of test_gpu_ipnn_step_multi)."""
    solo, group = two_sets(lambda: group_of(F))
    try:
        for m, e in enumerate(group):
            expect_plan(e, strips=m != 6, shares=m != 6)
        assert group[0].plan['rows_fwd'] == ('many' if F == 46 else 'narrow') and group[5].plan['stack_fwd']['cap_a'] == group[5].plan['stack_fwd']['cap_b']
        for B in (100, 77):
            ids, y = feed(F, B, n_rows=N_ROWS, seed=70 + B)
            y = y.astype(np.float32)
            w = weights_of(ids, 9) if feed_kind == 'wts' else None
            for s in range(3):
                mk = [Drawn(50 + m, s) for m in range(len(solo))] if feed_kind == 'drawn' else [masks_for(e, B, 60 + 7 * s + m) for m, e in enumerate(solo)]
                step_both(solo, group, ids, y, mk, wts=w, label='F%d %s B%d step %d' % (F, feed_kind, B, s))
    finally:
        close(solo + group)


@pytest.mark.parametrize("F", [39, 46])
def test_group_scoring_is_the_solo_scoring(built, F):
    """evaluate_many / predict_many on 1,000 lines at max_batch 256 (check of test_gpu_ipnn_eval_multi: exact against each engine's
    own predict and evaluate), with and without value weights."""
    engs = [member(F, 11, [60, 30], 'f32', ACTS[0], seed=11), member(F, 4, [60, 30], 'bf16', ACTS[1], seed=12),
            member(F, 16, [300, 70], 'bf16', ACTS[2], seed=13, max_batch=512), member(F, 11, [60, 30], 'f32', ACTS[1], seed=14),
            member(F, 4, [1200], 'f32', ACTS[0], seed=15)]
    try:
        for m, e in enumerate(engs):
            assert expect_plan(e, strips=m != 4)['shares_eval'] == (m != 4)
        ids, y = feed(F, 1000, n_rows=N_ROWS)
        check(engs, ids, y)
        check(engs, ids, y, weights_of(ids, 3))
    finally:
        close(engs)


def test_group_step_reports_an_id_outside_the_table_in_field_38(built):
    """Members 0 and 2 hold 900 rows, member 1 holds 1,500: an id of 1,000 in field 38 of the last example is outside the first
    and the third table only.  The call raises FNN_ERR_RANGE naming models 0 and 2, and the engines train afterwards."""
    F, B = 39, 100
    engs = [member(F, 11, [60, 30], 'f32', 'relu', seed=21), None, member(F, 4, [60, 30], 'bf16', 'tanh', seed=23)]
    table, _, _, params, _, _ = problem(F, 11, 8, [60, 30], True, seed=22, n_rows=1500)
    engs[1] = IPNNEngine(F, 11, [60, 30], 'relu', max_batch=256, precision='f32', lr=0.01, keep_prob=0.7)
    engs[1].set_params(table, params['b'], params['W'], params['bias'])
    try:
        for e in engs:
            expect_plan(e, shares=True)
        assert table.shape[0] == 1500
        ids, y = feed(F, B, n_rows=N_ROWS)
        y = y.astype(np.float32)
        bad = ids.copy()
        bad[B - 1, 38] = 1000
        with pytest.raises(FNNError) as ei:
            ipnn.train_step_many(engs, bad, y)
        assert ei.value.code == _capi.FNN_ERR_RANGE
        msg = str(ei.value)
        assert 'ipnn_train_step_multi' in msg and 'model(s) 0, 2' in msg, msg
        out = ipnn.train_step_many(engs, ids, y)
        assert all(np.isfinite(o['loss']) for o in out)
        for e in engs:
            e.sync()
    finally:
        close(engs)
