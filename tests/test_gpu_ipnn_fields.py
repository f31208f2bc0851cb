"""The inner-product step (include/ipnn_hip.h) on 33 to 64 fields of narrow rows (k = 1..16) -- the reference's inner-product
classes are 39-field models (python/FNN_IP_L3.py: X_feas = 13 + len(cat_sizes)) -- against the float64 oracle
(oracle/ipnn_oracle.py), with the problem generator, Bounds and check_f32_step of test_gpu_ipnn_shapes.

Above 32 fields ipnn_create picks, for each direction on its own, between two inner-product kernels, restated in many_of() below:
  f16 / b16   k_ip_fwd / k_ip_bwd, 16 examples per workgroup: a tile of 16 (17 F + Dp0) floats, which fits the 160 KiB of LDS up
              to 45 fields with pairs (159,552 B) and not at 46 (164,736 B)
  f8 / b4     k_ip_fwd_m / k_ip_bwd_m, 8 / 4 examples per workgroup, embeddings only in LDS, a table for the pair -> (i, j) map
The crossovers are measured: the backward's is BWD_MIN = 33 fields (IPM_BWD_MIN_FIELDS), the forward's is the
LDS alone (IPM_FWD_MIN_FIELDS = 65: f8 from 46 fields with pairs, never without).  IPNN_MANY_MIN / IPNN_MANY_FWD_MIN move them, and
the cases marked `b16` / `f8` run the other kernel where it can run.  Every case id starts with that choice, then the stack's path
(strip / strip-duo / gemm: Dp0 >= 1088 and every hidden layer > 1023 go to the GEMM launches) and Dp0.

Bounds are the project's existing ones: test_ipnn_step_f32_vs_oracle for one f32 step, test_ipnn_bf16_wide_stack_tracks_oracle for
bf16, test_adam_steps_vs_oracle / test_ftrl_steps_vs_oracle, test_ipnn_many_steps_track_oracle for twelve steps, and those of
test_ipnn_l7_step_f32_on_the_full_table for the full shape.  Each oracle case prints its worst error as a fraction of its bound.
"""
import pickle

import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.FM import FM
from deep_ctr_amd.ipnn import FNN, FNN_IP_L3, IPNNEngine

from test_gpu_ipnn_shapes import (Bounds, check_f32_step, copy_params, cosine, f32r, lr_for, oracle_pairs, padded, path_of,
                                  problem, lds_ip)

pytestmark = pytest.mark.gpu

BWD_MIN, FWD_MIN = 33, 65            # IPM_BWD_MIN_FIELDS, IPM_FWD_MIN_FIELDS of ipnn_api.hip
LDS_BYTES = 160 * 1024
KNOBS = {None: {}, 'b16': {'IPNN_MANY_MIN': '64'}, 'f8': {'IPNN_MANY_FWD_MIN': '33'}}        # the other kernel, where it can run


def many_of(F, hidden, pairs, many_min):
    """ip_many_choice: above 32 fields, the 8 / 4-example kernel from many_min fields on and wherever the 16-example tile passes
    the LDS."""
    return F > 32 and (F >= max(33, many_min) or lds_ip(F, hidden, pairs) > LDS_BYTES)


def cid(F, K, pairs, hidden, B, prec='f32', *rest, knob=None):
    env = KNOBS[knob]
    fwd = many_of(F, hidden, pairs, int(env.get('IPNN_MANY_FWD_MIN', FWD_MIN)))
    bwd = many_of(F, hidden, pairs, int(env.get('IPNN_MANY_MIN', BWD_MIN)))
    s = '%s%s-%s-F%d-K%d-%s-Dp0_%d-H%s-B%d' % ('f8' if fwd else 'f16', 'b4' if bwd else 'b16', path_of(F, hidden, pairs, prec, B),
                                               F, K, 'P' if pairs else 'noP', padded(F, hidden, pairs)[0], 'x'.join(str(h) for h in hidden), B)
    return '-'.join([s] + [str(r) for r in rest if r not in (None, '')])


def test_choice_restatement():
    """The arithmetic the case ids rest on: the 16-example tile fits at 45 fields with pairs and not at 46; without pairs it fits
    up to 64; layer 0 pads to 1408 columns at 39 fields and 3072 at 64."""
    assert lds_ip(45, [8], 1) == 159552 and lds_ip(46, [8], 1) == 164736 and lds_ip(64, [8], 0) == 139264 and lds_ip(64, [8], 1) == 266240
    assert padded(39, [8], 1)[0] == 1408 and padded(64, [8], 1)[0] == 3072 and padded(64, [8], 0)[0] == 1088
    assert not many_of(32, [8], 1, 33) and many_of(33, [8], 1, 33) and many_of(46, [8], 1, 65) and not many_of(45, [8], 1, 65)
    assert not many_of(64, [8], 0, 65) and many_of(64, [8], 1, 65)
    assert cid(39, 11, 1, [8], 256).startswith('f16b4-') and cid(46, 11, 1, [8], 256).startswith('f8b4-')
    assert cid(45, 11, 1, [8], 256, knob='b16').startswith('f16b16-') and cid(45, 11, 1, [8], 256, knob='f8').startswith('f8b4-')
    assert path_of(39, [400, 400, 200], 1, 'f32', 4096) == 'gemm' and path_of(63, [40], 0, 'f32', 257) == 'strip'


# ------------------------------------------------------------------------------------------------ one f32 step
# (F, K, pairs, hidden, B, act, drop, knob): knob = None is the default choice; 'b16' keeps the 16-example backward wherever its
# tile fits (33 .. 45 fields with pairs, every count but 64 without), 'f8' runs the 8-example forward from 33 fields on: every
# kernel runs on both sides of its crossover and of 45 | 46
STEP = [
    (32, 11, 1, [40, 24], 257, 'relu', True, None),
    (33, 1, 1, [40, 24], 17, 'relu', True, None), (33, 16, 1, [100, 50], 257, 'tanh', True, None), (33, 2, 0, [64, 30], 1, 'sigmoid', False, None),
    (39, 11, 1, [400, 400, 200], 4096, 'relu', True, None), (39, 11, 1, [60, 30], 257, 'tanh', False, None), (39, 2, 1, [1100, 40], 17, 'sigmoid', True, None),
    (39, 11, 0, [300, 100], 4096, 'relu', True, None), (39, 16, 1, [64, 63], 1, 'relu', True, None),
    (45, 16, 1, [50, 30], 257, 'relu', True, None), (45, 1, 1, [40], 17, 'tanh', True, None),
    (46, 16, 1, [50, 30], 257, 'sigmoid', True, None), (46, 2, 1, [40, 20], 4096, 'relu', False, None), (46, 11, 0, [60], 17, 'tanh', True, None),
    (50, 11, 1, [70, 40], 257, 'tanh', True, None), (50, 1, 0, [1100, 30], 17, 'relu', True, None),
    (63, 16, 1, [40, 20], 17, 'relu', True, None), (63, 2, 0, [40], 257, 'sigmoid', True, None), (63, 11, 1, [30], 1, 'tanh', False, None),
    (64, 16, 1, [60, 30], 4096, 'relu', True, None), (64, 11, 1, [50, 20], 257, 'tanh', True, None), (64, 1, 1, [40], 17, 'sigmoid', False, None),
    (64, 16, 0, [300, 100], 257, 'relu', True, None), (64, 2, 1, [64], 1, 'relu', True, None), (64, 16, 0, [40], 4096, 'tanh', False, None),
    # the 16-example kernels above 32 fields (IPNN_MANY_MIN=64), and the handles they cannot serve
    (33, 16, 1, [100, 50], 257, 'tanh', True, 'b16'), (39, 11, 1, [60, 30], 257, 'relu', True, 'b16'), (45, 16, 1, [50, 30], 4096, 'relu', True, 'b16'),
    (45, 1, 1, [40], 17, 'tanh', True, 'b16'), (46, 16, 1, [50, 30], 257, 'sigmoid', True, 'b16'), (63, 16, 0, [40, 20], 257, 'relu', True, 'b16'),
    (64, 11, 1, [50, 20], 17, 'tanh', True, 'b16'),
    # the 8-example forward below its crossover
    (33, 16, 1, [100, 50], 257, 'tanh', True, 'f8'), (39, 11, 1, [60, 30], 4096, 'relu', True, 'f8'), (45, 1, 1, [40], 17, 'sigmoid', True, 'f8'),
    (45, 16, 1, [50, 30], 257, 'relu', False, 'f8'), (39, 2, 0, [40, 20], 257, 'tanh', True, 'f8'), (64, 16, 0, [300, 100], 4096, 'relu', True, 'f8'),
    (63, 11, 0, [64], 1, 'relu', True, 'f8'),
]


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop,mm", STEP,
                         ids=[cid(F, K, p, h, B, 'f32', a, 'drop' if dr else 'nodrop', mm, knob=mm) for (F, K, p, h, B, a, dr, mm) in STEP])
def test_fields_step_f32_vs_oracle(built, monkeypatch, F, K, pairs, hidden, B, act, drop, mm):
    for k, v in KNOBS[mm].items():
        monkeypatch.setenv(k, v)
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B, n_rows=1500)
    keep, lr = (0.7 if drop else 1.0), lr_for(B)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=lr, keep_prob=keep, pairs=bool(pairs))
    try:
        assert eng.d == prob[5]
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, act, lr, drop, keep, pairs, cid(F, K, pairs, hidden, B, 'f32', act, knob=mm))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ bf16, three steps
BF16 = [(39, 11, 1, [400, 400, 200]), (64, 16, 1, [400, 200]), (64, 11, 0, [400, 200]), (39, 1, 1, [1100, 100])]


@pytest.mark.parametrize("F,K,pairs,hidden", BF16, ids=[cid(F, K, p, h, 1024, 'bf16') for (F, K, p, h) in BF16])
def test_fields_bf16_three_steps_track_oracle(built, F, K, pairs, hidden):
    """test_ipnn_bf16_wide_stack_tracks_oracle's bounds after each of three steps on batches of their own: logits within 5e-2,
    loss within 2 %, and after the last step every weight's accumulated update has a cosine above 0.99 with the oracle's.

    The 5e-2 on the logits is an ABSOLUTE bound, written for logits of order 1.  The loss is a sum over the batch, so the step
    length scales with B: at lr = 0.01 and B = 1024 the float64 oracle's own first step overshoots (its logits go from 0.3 to 27
    at 64 fields, 13 at 39; there one bf16 rounding unit is 0.06 .. 0.125, and rounding the oracle's own operands to bf16 moves a
    logit by 0.036) -- an ill-posed problem, not a step anyone trains with.  The steps here use lr = 0.002 (test_gpu_ipnn_shapes
    steps a batch of 4096 at 0.001), and the oracle's logits are asserted to stay below 4 so that the bound means what it says."""
    B, steps, lr = 1024, 3, 0.002
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, pairs, seed=11 + F + K, n_rows=1500)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=lr, keep_prob=0.7, pairs=bool(pairs))
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0 = [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            with oracle_pairs(pairs):
                loss, logits, _ = io.sgd_step(params, table, ids[sl], y[sl], 'relu', lr, [m[sl].astype(np.float64) for m in masks], 0.7)
            assert np.abs(logits).max() < 4.0, "the oracle's own step overshoots: the problem is ill-posed"
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 0.0, 5e-2)
            bd.close('loss%d' % s, out['loss'], loss, 0.0, 2e-2 * abs(loss))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.above('cos W%d' % t, cosine(Ws[t] - p0[t], params['W'][t] - p0[t]), 0.99, 0.01)
        bd.report(cid(F, K, pairs, hidden, B, 'bf16', '3steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ Adam and FTRL, five steps
OPT = [(39, 11, 1, 'adam'), (64, 16, 1, 'adam'), (39, 11, 1, 'ftrl'), (64, 16, 1, 'ftrl'), (64, 3, 0, 'adam'), (64, 3, 0, 'ftrl')]


@pytest.mark.parametrize("F,K,pairs,opt", OPT, ids=[cid(F, K, p, [40, 24, 12], 160, 'f32', o) for (F, K, p, o) in OPT])
def test_fields_optimiser_steps_vs_oracle(built, F, K, pairs, opt):
    """Five Adam / FTRL steps, each on a batch of its own (bounds of test_adam_steps_vs_oracle / test_ftrl_steps_vs_oracle, as
    test_ipnn_shape_optimiser_steps_vs_oracle applies them): every row follows the oracle's dense pass over n_rows x 16; a row no
    step touched is bit-unchanged under Adam and exactly 0 under FTRL -- from step 1 on."""
    hidden, B, steps = [40, 24, 12], 160, 5
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, pairs, seed=21 + F + K, n_rows=4000)
    lr = 1e-3 if opt == 'adam' else 1e-2
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=lr, keep_prob=0.7, optimizer=opt, adam_eps=1e-8, pairs=bool(pairs))
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        st = io.adam_state(params, table) if opt == 'adam' else io.ftrl_state(params, table)
        t0, W0 = table.copy(), [w.copy() for w in params['W']]
        never = np.setdiff1d(np.arange(table.shape[0]), np.unique(ids))
        early = np.setdiff1d(np.unique(ids[:B]), np.unique(ids[B:]))       # touched by the first step only
        assert len(never) > 0 and len(early) > 0
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            m64 = [m[sl].astype(np.float64) for m in masks]
            with oracle_pairs(pairs):
                if opt == 'adam':
                    loss, logits, _ = io.adam_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                    bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 5e-4, 5e-5)
                else:
                    loss, logits, _ = io.ftrl_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                    bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 2e-3, 2e-5)
                    bd.close('loss%d' % s, out['loss'], loss, 0.0, 1e-4 * abs(loss))
            if opt == 'ftrl' and s == 0:
                assert not eng.get_rows(never).any(), "FTRL: a row nobody touched is 0 after step 1"
        b, Ws, bs = eng.get_params()
        rows = eng.get_rows(np.arange(table.shape[0]))
        if opt == 'adam':
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - W0[t]).max() + 1e-7)
            ct = np.abs(table - t0).max()
            bd.close('table', rows, table, 0.0, 5e-3 * ct + 1e-7)
            bd.close('early rows', rows[early], table[early], 0.0, 5e-3 * ct + 1e-7)
            assert np.abs(table[early] - t0[early]).max() > 0 and np.abs(rows[early] - t0[early]).max() > 0
            assert np.array_equal(rows[never], t0[never].astype(np.float32))
        else:
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t]).max() + 1e-7)
                bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 5e-3 * np.abs(params['bias'][t]).max() + 1e-7)
            bd.close('b', b, params['b'], 0.0, 5e-3 * abs(params['b']) + 1e-7)
            bd.close('table', rows, table, 0.0, 5e-3 * np.abs(table).max() + 1e-7)
            bd.close('early rows', rows[early], table[early], 0.0, 5e-3 * np.abs(table).max() + 1e-7)
            assert not rows[never].any()
        bd.report(cid(F, K, pairs, hidden, B, 'f32', opt))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ twelve steps
def test_fields_twelve_steps_at_39_fields(built):
    """test_ipnn_many_steps_track_oracle at F = 39, K = 11: twelve SGD steps with fresh masks and batch lengths; the side-stream
    work of one step (the many-field backward, b, the sparse-row update) overlaps the next step's start."""
    F, K, hidden = 39, 11, [130, 70, 40]
    table, _, _, params, _, d = problem(F, K, 8, hidden, True, seed=31, n_rows=1500)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=0.02, keep_prob=0.7)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0, t0 = [w.copy() for w in params['W']], table.copy()
        rng = np.random.RandomState(77)
        sizes = synth.field_sizes_tiny(1500, n_fields=F)
        touched = set()
        for step in range(12):
            B = int(rng.randint(60, 201))
            ids = synth.zipf_ids(B, sizes, 1.1, 100 + step)
            y = (rng.uniform(size=B) < 0.3).astype(np.float64)
            masks = [(rng.uniform(size=(B, d[t])) < 0.7).astype(np.uint8) for t in range(len(hidden) + 1)]
            out = eng.train_step(ids, y, masks, want_logits=(step == 11))
            loss, logits, _ = io.sgd_step(params, table, ids, y, 'relu', 0.02, [m.astype(np.float64) for m in masks], 0.7)
            touched |= set(np.unique(ids).tolist())
        bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-3, 2e-4)
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - p0[t]).max() + 1e-6)
        tr = np.array(sorted(touched))
        bd.close('table', eng.get_rows(tr), table[tr], 0.0, 5e-3 * np.abs(table - t0).max() + 1e-6)
        bd.report(cid(F, K, 1, hidden, 200, 'f32', '12steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ determinism and store modes
def _three_bf16_steps(F, K, pairs, hidden, data):
    table, ids, y, params, masks, d = data
    B, steps = 4096, 3
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=0.001, keep_prob=0.5, pairs=bool(pairs))
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        logits = []
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            logits.append(out['logits'].cpu().numpy().copy())
        b, Ws, bs = eng.get_params()
        return np.concatenate(logits), b, Ws, bs, eng.get_rows(np.unique(ids))
    finally:
        eng.close()


def _bit_equal(ra, rb):
    (la, ba, Wa, bsa, rowa), (lb, bb, Wb, bsb, rowb) = ra, rb
    assert np.isfinite(la).all() and np.abs(la).max() > 0
    assert np.array_equal(la, lb), "logits differ"
    assert ba == bb, "b differs"
    assert np.array_equal(rowa, rowb), "touched rows differ"
    for t in range(len(Wa)):
        assert np.array_equal(Wa[t], Wb[t]) and np.array_equal(bsa[t], bsb[t]), t


DET = [(39, 11, 1, [400, 400, 200]), (64, 16, 1, [200, 100])]


@pytest.mark.parametrize("F,K,pairs,hidden", DET, ids=[cid(F, K, p, h, 4096, 'bf16') for (F, K, p, h) in DET])
def test_fields_runs_are_bit_identical_in_every_store_mode(built, monkeypatch, F, K, pairs, hidden):
    """bf16, batch 4096, three steps with dropout: logits, every dense tensor, b and the touched rows are BIT-equal between two
    identical runs, between write-through and plain stores (IPNN_WT=0) and with everything on one stream (IPNN_SIDE_STREAM=0)."""
    data = problem(F, K, 4096 * 3, hidden, pairs, seed=77 + F, n_rows=3000, keep_p=0.5)
    base = _three_bf16_steps(F, K, pairs, hidden, data)
    _bit_equal(base, _three_bf16_steps(F, K, pairs, hidden, data))
    monkeypatch.setenv('IPNN_WT', '0')
    _bit_equal(base, _three_bf16_steps(F, K, pairs, hidden, data))
    monkeypatch.delenv('IPNN_WT')
    monkeypatch.setenv('IPNN_SIDE_STREAM', '0')
    _bit_equal(base, _three_bf16_steps(F, K, pairs, hidden, data))


@pytest.mark.parametrize("F,K,B", [(39, 11, 257), (45, 16, 4096)])
def test_fields_both_kernel_pairs_agree(built, monkeypatch, F, K, B):
    """Where both pairs of kernels can run (33 .. 45 fields with pairs) they compute the same sums in the same order: after one f32
    step with dropout the logits, every W and bias and the touched rows are bit-equal; b (a sum of per-workgroup partials of
    another grain) within 2e-3 of its change."""
    hidden = [60, 30]
    table, ids, y, params, masks, d = problem(F, K, B, hidden, True, seed=5 * F + K, n_rows=1500)
    res = []
    for mm in ('33', '64'):                                 # the 8 / 4-example kernels, then the 16-example ones
        monkeypatch.setenv('IPNN_MANY_MIN', mm)
        monkeypatch.setenv('IPNN_MANY_FWD_MIN', mm)
        eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=max(256, B), precision='f32', lr=0.01, keep_prob=0.7)
        try:
            eng.set_params(table, params['b'], params['W'], params['bias'])
            out = eng.train_step(ids, y, masks, want_logits=True)
            b, Ws, bs = eng.get_params()
            res.append((out['logits'].cpu().numpy(), b, Ws, bs, eng.get_rows(np.unique(ids))))
        finally:
            eng.close()
    (la, ba, Wa, bsa, ra), (lb, bb, Wb, bsb, rb) = res
    assert np.array_equal(la, lb) and np.array_equal(ra, rb)
    for t in range(len(Wa)):
        assert np.array_equal(Wa[t], Wb[t]) and np.array_equal(bsa[t], bsb[t]), t
    assert abs(ba - bb) <= 2e-3 * abs(ba - params['b']) + 2e-7


# ------------------------------------------------------------------------------------------------ ids and round trips
def test_fields_id_out_of_range_in_field_63(built):
    """An id past the table in field 63 of the last example: FNN_ERR_RANGE, and the handle trains afterwards."""
    F, K, hidden, B = 64, 11, [40, 20], 257
    prob = problem(F, K, B, hidden, True, seed=64, n_rows=1500)
    table, ids, y, params, masks, d = prob
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='f32', lr=0.01, keep_prob=0.7)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        bad = ids.copy()
        bad[B - 1, 63] = table.shape[0]
        with pytest.raises(FNNError) as ei:
            eng.train_step(bad, y, masks)
        assert ei.value.code == _capi.FNN_ERR_RANGE
        out = eng.train_step(ids, y, masks)
        assert np.isfinite(out['loss'])
        eng.sync()
    finally:
        eng.close()


def test_fields_predict_and_eval_over_more_lines_than_max_batch(built):
    """predict over 2,501 examples at max_batch 1000 against the oracle, ipnn_eval's metrics against sklearn on the same
    predictions (test_ipnn_predict_and_eval_vs_sklearn_at_32_fields at 39 fields)."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    F, K, hidden, N = 39, 11, [300, 100], 2501
    table, ids, y, params, masks, d = problem(F, K, N, hidden, True, seed=78, n_rows=1500)
    params['W'][-1] *= 10.0                                 # spread the predictions away from 0.5
    yy = (np.random.RandomState(6).uniform(size=N) < 0.3).astype(np.int32)
    eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=1000, precision='f32', lr=0.01, keep_prob=1.0)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        pp = eng.predict(ids).cpu().numpy()
        bd = Bounds()
        bd.close('predict', pp, io.predict(params, table, ids, 'tanh'), 2e-4, 1e-6)
        bd.report(cid(F, K, 1, hidden, 1000, 'f32', 'predict-N2501'))
        m = eng.evaluate(ids, yy)
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


@pytest.mark.parametrize("F,K,pairs", [(39, 11, 1), (64, 16, 1), (64, 1, 0)])
def test_fields_set_get_roundtrip(built, F, K, pairs):
    """set_params then get_params / get_rows returns every value bit for bit; a step at lr = 0 leaves them bit-unchanged."""
    hidden, B = [64, 63], 257
    table, ids, y, params, masks, d = problem(F, K, B, hidden, pairs, seed=5 * F + K, n_rows=1500)
    eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=B, precision='f32', lr=0.0, keep_prob=0.7, pairs=bool(pairs))
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        t32 = table.astype(np.float32)
        for when in ('set', 'lr0'):
            b, Ws, bs = eng.get_params()
            assert b == np.float32(params['b']), when
            for t in range(len(Ws)):
                assert np.array_equal(Ws[t], params['W'][t].astype(np.float32)), (when, t)
                assert np.array_equal(bs[t], params['bias'][t].astype(np.float32)), (when, t)
            assert np.array_equal(eng.get_rows(np.arange(table.shape[0])), t32), when
            if when == 'set':
                out = eng.train_step(ids, y, masks, want_logits=True)
                assert np.isfinite(out['logits'].cpu().numpy()).all() and np.isfinite(out['loss'])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("cls,F", [(FNN_IP_L3, 39), (FNN, 64)], ids=['FM39-FNN_IP_L3', 'FM64-FNN'])
def test_fm_pickle_seeds_the_family_and_it_trains(built, tmp_path, cls, F):
    """FM(B, [D, F, 10]) trains a few steps and dumps {'W', 'V', 'b'}; the family class with X_feas = F, rank 10 loads the pickle
    through _init_argv with the FM rows and b bit for bit, trains, evaluates to finite metrics, and its loss falls."""
    rank, B = 10, 256
    sizes = synth.field_sizes_tiny(2000, F)
    D = sum(sizes)
    ids = synth.zipf_ids(B * 4, sizes, 1.1, 5)
    rng = np.random.RandomState(6)
    y = (rng.uniform(size=B * 4) < 0.3).astype(np.float64)
    fm = FM(B, [D, F, rank], ['uniform', -0.01, 0.01, [1, 2], None], ['sgd', 0.05], [1e-3], 'train', 0)
    try:
        for j in range(3):
            fm.train_step(ids[j * B:(j + 1) * B], y[j * B:(j + 1) * B], want_loss=False)
        rows, b = fm.get_params()
        path = str(tmp_path / 'fm.pkl')
        fm.dump(path)
    finally:
        fm.close()
    vm = pickle.load(open(path, 'rb'))
    assert vm['V'].shape == (D, rank)
    hidden = [300, 100, 50][:cls.N_HIDDEN]
    m = cls([], [], B, [D, F, rank] + hidden + ['relu'], ['uniform', -0.05, 0.05, [3, 4, 5], path], ['sgd', 0.002, 'sum'],
            [1.0], 'train', B * 4, precision='f32')
    try:
        assert m.eng.F == F and m.eng.d[0] == F * (rank + 1) + (F * (F - 1) // 2 if cls.PAIRS else 0) + 1
        assert np.array_equal(m.eng.get_rows(np.arange(D)), rows)
        assert m.eng.get_params()[0] == np.float32(b)
        losses = [m.train_step(ids[:B], y[:B])['loss'] for _ in range(8)]
        assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
        met = m.eng.evaluate(ids, y.astype(np.int32))
        assert all(np.isfinite(met[k]) for k in ('auc', 'rmse', 'logloss')), met
        p = m.forward(ids).cpu().numpy()
        assert p.shape == (B * 4,) and np.isfinite(p).all()
        with pytest.raises(NotImplementedError):
            m.forward(ids, v_wts=np.ones((B * 4, 13)))
    finally:
        m.eng.close()


# ------------------------------------------------------------------------------------------------ the full shape
def test_fields_fnn_ip_l3_step_f32_on_the_full_table(built):
    """937,670 rows over 39 fields (synth.field_sizes_ipinyou(39)) x 11, FNN_IP_L3's 400 / 400 / 200, batch 4096 Zipf ids, f32:
    one SGD step against the float64 oracle on the touched rows, at the bounds of test_ipnn_l7_step_f32_on_the_full_table --
    logits rtol 2e-4 (atol 2e-5), loss 5e-5, every dense tensor's and touched row's update within 2e-3 of its size, untouched rows
    bit for bit."""
    F, K, hidden, B = 39, 11, [400, 400, 200], 4096
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    D = sum(sizes)
    assert D == synth.IPINYOU_DIMS
    rng = np.random.RandomState(11)
    table = synth.fm_table(D, K, 0.2, 1234)
    ids = synth.zipf_ids(B, sizes, 1.1, 77)
    y = (rng.uniform(size=B) < 0.3).astype(np.float64)
    d = [F * K + F * (F - 1) // 2 + 1] + hidden + [1]
    params = {'b': float(np.float32(0.1)), 'W': [f32r(rng.uniform(-0.06, 0.06, (d[i], d[i + 1]))) for i in range(len(d) - 1)],
              'bias': [f32r(rng.uniform(-0.1, 0.1, d[i + 1])) for i in range(len(d) - 1)]}
    masks = [(np.random.RandomState(40 + t).uniform(size=(B, d[t])) < 0.5).astype(np.uint8) for t in range(len(hidden) + 1)]
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='f32', lr=1e-3, keep_prob=0.5)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        out = eng.train_step(ids, y, masks, want_logits=True)
        touched = np.unique(ids)
        idc = np.searchsorted(touched, ids)
        tc = table[touched].astype(np.float64)
        t0, p0 = tc.copy(), copy_params(params)
        loss, logits, g = io.sgd_step(params, tc, idc, y, 'relu', 1e-3, [m.astype(np.float64) for m in masks], 0.5)
        bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-4, 2e-5)
        bd.close('loss', out['loss'], loss, 0.0, 5e-5 * max(1.0, abs(loss)))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 2e-3 * (np.abs(params['W'][t] - p0['W'][t]).max() + 1e-12) + 2e-7)
            bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 2e-3 * (np.abs(params['bias'][t] - p0['bias'][t]).max() + 1e-12) + 2e-7)
        bd.close('b', b, params['b'], 0.0, 2e-3 * abs(params['b'] - p0['b']) + 2e-7)
        bd.close('table', eng.get_rows(touched), tc, 0.0, 2e-3 * (np.abs(tc - t0).max() + 1e-12) + 2e-7)
        un = np.setdiff1d(np.random.RandomState(0).randint(0, D, size=20000), touched)
        assert np.array_equal(eng.get_rows(un), table[un])
        bd.report(cid(F, K, 1, hidden, B, 'f32', 'full-table'))
    finally:
        eng.close()
