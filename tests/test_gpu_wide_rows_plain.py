"""The plain (undecayed) update of wide rows -- scatw1_form<false> / scatw2_form<false> of csrc/sparse_rows.hip.h -- at its
consumers, on the hand-built layouts of tests/wide_layouts.py (what each reaches: tests/test_wide_layouts.py), B = 4096 on
N2 = 4096 keys per field and B = 40:
  FM pre-training, k = 17, 18, 128: SGD into the table under the lazy scale (k_fm_scatw1 / k_fm_scatw2_tail), Adam into the
      gradient store, the shared-row marks and float atomics of both levels, the group forms (k_fm_step_scatw*);
  the wide inner-product step (k_ip_scatw1 / k_ip_scatw2), F = 4, k = 17 and 51, SGD and Adam;
  the SNN bag table at h0 = 192 (nq = 48, ngrp = 5) and 316 (nq = 79, ngrp = 3: a run of 1040 is three trips of level 2).

The gradients are formed inside the step, so the references are the float64 restatements the consumers' own tests use
(fm_shared_cases.Trainer, oracle/ipnn_oracle.py, orc.snn_train_step) at those tests' bounds, unwidened.  Those bounds are relative
to the LARGEST change in the table, which here is the row that every example hits: a chunk's partial lost from a run of 24 or
of 1040 entries would hide under it.  So every case also holds each touched row to 1e-2 of that ROW's own largest change (plus
the test's absolute term): a chunk of 32 entries is 1 % of the longest run but the one-row field, which the global bound sees;
f32 rounding of a gradient term is 2^-24 of the term and sums of up to 4096 terms that cancel at random lose a factor of
sqrt(4096) = 64 at the worst, four orders below 1e-2.  Each case prints its worst error as a fraction of both bounds.
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc
from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd.FM import FM

import fm_shared_cases as sc
import wide_layouts as wl
from test_gpu_fm_fields import INIT, check_state, table
from test_gpu_fm_step_multi import Spec, bits, check_group
from test_gpu_ipnn_shapes import Bounds, check_f32_step, f32r, problem
from test_gpu_ipnn_wide import engine as ip_engine
from test_gpu_parity import make_snn_engine, make_snn_problem

pytestmark = pytest.mark.gpu

PER_ROW = 1e-2
SIZES = {'big': (wl.PLAIN_BIG, 4096), 'small': (wl.PLAIN_SMALL, 40)}


def per_row(label, got, ref, before, atol, rows=None):
    """Every row within PER_ROW of its own largest change (+ atol); prints and returns the worst fraction."""
    got, ref, before = (np.asarray(a, np.float64) for a in (got, ref, before))
    if rows is not None:
        got, ref, before = got[rows], ref[rows], before[rows]
    bound = PER_ROW * np.abs(ref - before).max(axis=1, keepdims=True) + atol
    frac = np.abs(got - ref) / bound
    worst = float(frac.max())
    r = int(np.argmax(frac.max(axis=1)))
    print("[wide plain] %s: worst per-row error %.3g of its bound (row %d of %d)" % (label, worst, r, len(got)))
    assert worst <= 1.0, "%s: row %d is at %.3g of 1e-2 of its own change" % (label, r, worst)
    return worst


def feed(size, n_steps, dead=True, seed=21):
    """n_steps batches of the same runs on other examples -> ([(ids, y)], sizes)."""
    codes, B = SIZES[size]
    out = []
    for s in range(n_steps):
        ids, sizes = wl.build(codes, B, seed + s, dead)
        out.append((ids, sc.labels(B, seed + 50 + s)))
    return out, sizes


# ------------------------------------------------------------------------------------------------ FM pre-training
LR_SGD, LAM = 0.05, 1e-2


def fm_model(F, k, B, argv, rows, shared=False):
    m = FM(B, [len(rows), F, k - 1], INIT, argv, [LAM], 'train', 0, shared_rows=shared)
    m.set_params(rows, 0.1)
    return m


def fm_sgd(label, k, steps, n_rows, shared, count=None):
    """SGD steps against the restatement at test_gpu_fm_wide.test_wide_sgd_steps_vs_oracle's bounds (p rtol 5e-5 / atol 1e-6,
    loss 2e-5, rows 2e-3 of the largest change + 2e-7) and the per-row bound -> what the handle computed, as bits."""
    F = steps[0][0].shape[1]
    rows = table(n_rows, F, k - 1, k)
    m = fm_model(F, k, len(steps[0][1]), ['sgd', LR_SGD], rows, shared)
    tr = sc.Trainer(rows, 0.1, 'sgd', LR_SGD, LAM, 1)
    res = []
    try:
        for ids, y in steps:
            out = m.train_step(ids, y, want_p=True)
            data, p = tr.sgd_step(ids, y)
            np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
            assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
            if shared:
                assert m.count_shared_rows() == sc.shared_count(ids) == count
            res += [out['p'].cpu().numpy(), np.float32(out['loss'])]
        got, gb = m.get_params()
    finally:
        m.close()
    change = np.abs(tr.rows - rows).max() + 1e-12
    err = np.abs(got - tr.rows).max()
    print("\n[wide plain] %s: max row error %.3g of its bound" % (label, err / (2e-3 * change + 2e-7)))
    assert err <= 2e-3 * change + 2e-7
    assert abs(gb - tr.b) <= 2e-3 * abs(tr.b - 0.1) + 2e-7
    per_row(label, got, tr.rows, rows, 2e-7)
    return res + [got, np.float32(gb)]


@pytest.mark.parametrize("size", ['big', 'small'])
@pytest.mark.parametrize("k", [17, 18, 128])
def test_fm_sgd_on_hand_built_segments(built, k, size):
    """Two steps (the lazy decay scale is live in the second), and again on a shared-rows handle: no row of these feeds sits
    under two columns, so the marks must change no bit."""
    steps, sizes = feed(size, 2)
    off = fm_sgd('FM sgd k=%d %s' % (k, size), k, steps, sum(sizes), False)
    on = fm_sgd('FM sgd k=%d %s, shared-rows handle' % (k, size), k, steps, sum(sizes), True, count=0)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(on, off))


@pytest.mark.parametrize("k", [17, 128])
def test_fm_sgd_with_the_one_row_under_three_columns(built, k):
    """The row that fills column 0 (a level-2 segment of 128 chunks) also sits 52 times in column 1, where as the smallest id
    it sorts first -- positions 0..51, two chunks: the atomic branch of level 2 -- and 3 times in column 2 -- inside one chunk:
    the atomic branch of level 1.  Held to the restatement as test_gpu_fm_shared.py holds its cases."""
    steps, sizes = feed('big', 2)
    for ids, _ in steps:
        one = ids[0, 0]
        ids[::80, 1][:52] = one
        ids[[5, 1000, 4000], 2] = one
        assert (ids[:, 1] == one).sum() == 52 and wl.owners(ids[:, 1])[0][:2] == (0, 52) and wl.segments(ids[:, 2])[0] == (0, 3)
    fm_sgd('FM sgd k=%d, one row under three columns' % k, k, steps, sum(sizes), True, count=1)


@pytest.mark.parametrize("size", ['big', 'small'])
@pytest.mark.parametrize("k", [17, 18, 128])
def test_fm_adam_on_hand_built_segments(built, k, size):
    """Adam: the update sums the batch's gradient into the gradient store.  After the first step the first moment is 0.1 g:
    every row of it within 1e-2 of the row's own largest entry; three steps at test_gpu_fm_wide.check_state's bounds."""
    steps, sizes = feed(size, 3)
    F, B = steps[0][0].shape[1], len(steps[0][1])
    rows = table(sum(sizes), F, k - 1, k)
    m = fm_model(F, k, B, ['adam', 1e-2, 1e-8], rows)
    tr = sc.Trainer(rows, 0.1, 'adam', 1e-2, LAM, 1)
    tr.rows0 = rows.copy()
    try:
        for s, (ids, y) in enumerate(steps):
            out = m.train_step(ids, y, want_p=True)
            data, p = tr.step(ids, y)
            tol = 5e-5 if s == 0 else 2e-3
            np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=tol, atol=1e-6)
            assert abs(out['loss'] - data) <= tol * max(1.0, abs(data))
            if s == 0:
                print()
                per_row('FM adam k=%d %s, first moment after one step' % (k, size), m.get_opt_state()[0], tr.s0, np.zeros_like(rows), 1e-9)
        check_state(m, tr)
    finally:
        m.close()


def test_fm_group_step_equals_the_solo_steps_on_hand_built_segments(built):
    """train_step_many over k = 17, 18 and 128 on one feed (k_fm_step_scatw1 / k_fm_step_scatw2_tail): every member bit for bit
    what its own train_step calls give (test_gpu_fm_step_multi.check_group)."""
    for size in ('big', 'small'):
        steps, sizes = feed(size, 2)
        F = steps[0][0].shape[1]
        specs = [Spec(F, k, lr=0.03 + 0.01 * i, lam=(0.0, 1e-2, 3e-2)[i], seed=60 + i, n_rows=sum(sizes)) for i, k in enumerate((17, 18, 128))]
        got = check_group(specs, [(ids, None, y.astype(np.float32)) for ids, y in steps])
        assert not np.array_equal(got[0]['state'][0], specs[0].rows().astype(np.float32))


# ------------------------------------------------------------------------------------------------ the wide inner-product step
IP_CODES = {4096: ['one', 'long', 'both', 'many'], 40: ['one', 'sub8', 'dead33', 'pair']}
IP_HIDDEN = [64, 63]


def ip_problem(K, B, n_steps, seed):
    """test_gpu_ipnn_shapes.problem's weights and masks on a table and ids of the layouts; the inner-product family refuses
    ids of -1: further distinct rows stand behind the live ones (dead=False)."""
    feeds = [wl.build(IP_CODES[B], B, seed + s, dead=False) for s in range(n_steps)]
    sizes = feeds[0][1]
    prob = list(problem(4, K, B * n_steps, IP_HIDDEN, True, seed=seed))
    prob[0] = f32r(np.random.RandomState(seed).standard_normal((sum(sizes), K)) * 0.2)
    prob[1] = np.concatenate([f[0] for f in feeds])
    assert prob[1].min() >= 0
    return prob


@pytest.mark.parametrize("B", [4096, 40])
@pytest.mark.parametrize("K", [17, 51])
def test_ip_sgd_on_hand_built_segments(built, K, B):
    """One f32 SGD step, pairs on, no dropout: test_gpu_ipnn_shapes.check_f32_step, and the per-row bound on the table."""
    lr = 0.001 if B >= 4096 else 0.01
    prob = ip_problem(K, B, 1, seed=K + B)
    before = prob[0].copy()
    eng = ip_engine(4, K, IP_HIDDEN, 'tanh', B, 'f32', lr, 1.0, True)
    try:
        assert eng.d == prob[5]
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, 'tanh', lr, False, 1.0, True, 'wide plain: IP sgd K=%d B=%d' % (K, B))
        per_row('IP sgd K=%d B=%d' % (K, B), eng.get_rows(np.arange(len(before))), prob[0], before, 2e-7)
    finally:
        eng.close()


@pytest.mark.parametrize("B", [4096, 40])
@pytest.mark.parametrize("K", [17, 51])
def test_ip_adam_on_hand_built_segments(built, K, B):
    """Three Adam steps (the first moves every element by lr whatever its gradient; the later ones weigh the gradients
    against each other) at test_gpu_ipnn_wide.test_wide_optimiser_steps_vs_oracle's bounds."""
    steps, lr = 3, 1e-3
    table_, ids, y, params, masks, d = ip_problem(K, B, steps, seed=K + B + 1)
    eng = ip_engine(4, K, IP_HIDDEN, 'relu', B, 'f32', lr, 0.7, True, optimizer='adam', adam_eps=1e-8)
    bd = Bounds()
    try:
        eng.set_params(table_, params['b'], params['W'], params['bias'])
        st = io.adam_state(params, table_)
        t0, W0 = table_.copy(), [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            loss, logits, _ = io.adam_step(params, table_, ids[sl], y[sl], 'relu', lr, st, [m[sl].astype(np.float64) for m in masks], 0.7)
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 5e-4, 5e-5)
        b, Ws, bs = eng.get_params()
        rows = eng.get_rows(np.arange(table_.shape[0]))
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - W0[t]).max() + 1e-7)
        bd.close('table', rows, table_, 0.0, 5e-3 * np.abs(table_ - t0).max() + 1e-7)
        never = np.setdiff1d(np.arange(table_.shape[0]), np.unique(ids))
        assert len(never) > 0 and np.array_equal(rows[never], t0[never].astype(np.float32))
        bd.report('wide plain: IP adam K=%d B=%d' % (K, B))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the SNN bag table
SNN_CODES = ['one', 'long', 'both', 'sub8', 'many', 'dead33', 'zipf', 'pair', 'dead0', 'aligned', 'many', 'many', 'dead8', 'zipf',
             'dead1', 'dead40']


def snn_case(label, h0, ids, n_rows, seed):
    """One f32 step against orc.snn_train_step at test_gpu_parity.test_snn_step_f32_vs_oracle's bounds, and the per-row bound."""
    B = len(ids)
    ww0, bb0, _, _, p, r1, r2 = make_snn_problem(8, n_rows=max(n_rows, 600), h0=h0, seed=seed)
    ww0 = (np.random.RandomState(seed).standard_normal((n_rows, h0)) * 0.1).astype(np.float32)
    y = (np.random.RandomState(seed + 1).uniform(size=B) < 0.3).astype(np.float32)
    eng = make_snn_engine(ww0, bb0, p, h0=h0)
    try:
        ww64, bb64 = ww0.astype(np.float64), bb0.astype(np.float64)
        np.testing.assert_allclose(eng.gather(ids).cpu().numpy(), orc.snn_bag(ww64, bb64, ids), rtol=2e-6, atol=1e-7)
        out = eng.train_step(ids, y, r1, r2, want_p=True, want_gx=True)
        p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        ref = orc.snn_train_step(p64, ww64, bb64, ids, y.astype(np.float64), r1.astype(float), r2.astype(float), 0.01, 0.001)
        np.testing.assert_allclose(out['p'].cpu().numpy(), ref['p_drop'], rtol=2e-4, atol=1e-6)
        gs = np.abs(ref['gx']).max()
        np.testing.assert_allclose(out['gx'].cpu().numpy(), ref['gx'], rtol=2e-3, atol=2e-5 * gs + 1e-9)
        assert abs(out['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
        got = eng.get_table()
        upd = np.abs(ww64 - ww0).max() + 1e-12
        err = np.abs(got - ww64).max()
        print("\n[wide plain] %s: max table error %.3g of its bound" % (label, err / (1e-3 * upd + 2e-7)))
        assert err <= 1e-3 * upd + 2e-7
        bupd = np.abs(bb64 - bb0).max() + 1e-12
        assert np.abs(eng.get_bag_bias() - bb64).max() <= 1e-3 * bupd + 2e-7
        touched = np.unique(ids[ids >= 0])
        mask = np.ones(n_rows, bool)
        mask[touched] = False
        assert mask.any() and np.array_equal(got[mask], ww0[mask])
        per_row(label, got, ww64, ww0, 2e-7, rows=touched)
    finally:
        eng.close()


@pytest.mark.parametrize("h0", [192, 316])
def test_snn_bag_step_on_hand_built_segments(built, h0):
    """16 columns, B = 4096: `one` is 128 chunks (7 trips of level 2 at ngrp = 5, 11 at ngrp = 3), `long` 33 chunks (2 and 3)."""
    ids, sizes = wl.build(SNN_CODES, 4096, 31)
    snn_case('SNN bag h0=%d' % h0, h0, ids, sum(sizes), seed=h0)


def test_snn_bag_step_with_a_row_under_two_columns_of_a_line(built):
    """h0 = 316: the row of column 0 also sits in column 1 of 52 lines (the smallest id: positions 0..51 there, two chunks) and in
    column 2 of 3 lines (inside one chunk), every one of them a line that holds it in column 0 too: float atomics in both
    levels, held to the same bounds."""
    ids, sizes = wl.build(SNN_CODES, 4096, 32)
    one = ids[0, 0]
    ids[::80, 1][:52] = one
    ids[[5, 1000, 4000], 2] = one
    assert (ids[:, 1] == one).sum() == 52 and wl.owners(ids[:, 1])[0][:2] == (0, 52) and wl.segments(ids[:, 2])[0] == (0, 3)
    snn_case('SNN bag h0=316, a row under three columns', 316, ids, sum(sizes), seed=7)
