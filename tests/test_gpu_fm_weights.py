"""Value weights of FM / LR pre-training (fm_train_step_w / fm_predict_w / fm_eval_w, `wts=` of deep_ctr_amd.FM and .LR):
e_f = wts[t, f] * row(ids[t, f]) through every forward of fm_api.hip -- fm_body<NF> (k <= 16; NF = 1 .. 4 fields per lane) and
fm_wide_body<L, NC> (k >= 17; L = 16 / 32 lanes per example, NC = 1 .. 4 chunks of 16 fields) -- against the float64 restatement
of tests/fm_weighted_ref.py.

Tables come from test_gpu_fm_fields.table(), batches from its batches() (Zipf duplicates, absent fields, the table's last row in
the last field) and weights from fm_weighted_ref.test_weights (uniform in [-0.5, 2), exact 0 and exact 1 among them); with that
table scaling these weights keep the logits' spread (tests/test_fm_weighted_ref.py), so the bounds are the project's own,
unchanged: sgd_vs_oracle's for SGD and check_state's for Adam / FTRL.  Shapes are the smallest at which each instantiation can
still go wrong: B = 1 (one example of a padded workgroup), 17 / 9 (a partial workgroup), 700 / 257 (many workgroups, the last one
partial), K = 1, a K that is no multiple of 4, a full 64-byte row, the first and last wide ranks of each lane count."""
import pickle

import numpy as np
import pytest

import fm_weighted_ref as wr
import ipnn_weighted_ref as iwr
from oracle import fm_oracle as fo

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import FNN_IP_L3, criteo_feed

from test_gpu_fm_fields import LRS, batches, check_state, model, np_metrics, table

pytestmark = pytest.mark.gpu


def wbatches(sizes, B, n, seed, gap=0, zero_field=None):
    """n (ids, y, wts) batches: test_gpu_fm_fields.batches() and a weight per entry.  Below 6 fields (batches() writes its absent
    entries at fixed columns up to 5) the same recipe with the absent entries fitted to the field count.  zero_field: that
    field's weights are all exact zeros."""
    F, D = len(sizes), sum(sizes)
    if F >= 6:
        bs = batches(sizes, B, n, seed, gap)
    else:
        bs, rng = [], np.random.RandomState(seed)
        for i in range(n):
            ids = synth.zipf_ids(B, sizes, 1.1, seed + 17 * i + 1)
            ids = np.where(ids >= D // 2, ids + gap, ids).astype(np.int32)
            if B > 8:
                ids[3, F - 1] = -1
                ids[4, :] = -1                                     # no field at all: yhat = b
                ids[6, :F - 1] = -1                                # field F - 1 only
            ids[B - 1, F - 1] = D + gap - 1
            bs.append((ids, (rng.uniform(size=B) < 0.3).astype(np.float64)))
    out = []
    for i, (ids, y) in enumerate(bs):
        w = wr.test_weights(B, F, seed + 1000 + i)
        if zero_field is not None:
            w[:, zero_field] = 0.0
        out.append((ids, y, w))
    return out


def sgd_vs_oracle_w(m, rows, b0, bs, lr, lam, reduce_mean, unweighted_oracle=False):
    """test_gpu_fm_fields.sgd_vs_oracle with weights, its bounds unchanged: forward rtol 2e-5 / atol 1e-6; per step p rtol 5e-5 /
    atol 1e-6 and the loss 2e-5 relative; afterwards rows and b within 2e-3 of their own change + 2e-7.  unweighted_oracle: the
    reference is oracle/fm_oracle.py (the weights must then be ones).  Returns the oracle's rows and the device's."""
    ids0, _, w0 = bs[0]
    want = fo.predict(rows, b0, ids0) if unweighted_oracle else wr.predict_w(rows, b0, ids0, w0)
    np.testing.assert_allclose(m.forward(ids0, wts=w0).cpu().numpy(), want, rtol=2e-5, atol=1e-6)
    r, b = rows.copy(), b0
    for ids, y, w in bs:
        out = m.train_step(ids, y, want_p=True, wts=w)
        if unweighted_oracle:
            b, data, p = fo.sgd_step(r, b, ids, y, lr, lam, reduce_mean == 1)
        else:
            b, data, p = wr.sgd_step_w(r, b, ids, w, y, lr, lam, reduce_mean == 1)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
    got, gb = m.get_params()
    change = np.abs(r - rows).max() + 1e-12
    assert np.abs(got - r).max() <= 2e-3 * change + 2e-7
    assert abs(gb - b) <= 2e-3 * abs(b - b0) + 2e-7
    return r, got


# ------------------------------------------------------------------------------------------------ 1. SGD
# path: ((F, rank), ..), the batch sizes rotated over them
PATHS = [
    ('narrow-NF1', ((16, 10), (1, 0), (16, 15), (5, 3)), (1, 17, 700)),
    ('narrow-NF2-4', ((17, 10), (39, 10), (39, 0), (64, 15)), (1, 17, 700)),
    ('wide-L16-NC1', ((2, 16), (16, 50), (16, 63)), (1, 9, 257)),
    ('wide-L16-NC2-3', ((17, 16), (39, 50)), (9, 700)),
    ('wide-L32-NC1', ((3, 64), (16, 100), (16, 127)), (1, 9, 257)),
    ('wide-L32-NC3-4', ((39, 100), (64, 127), (33, 64)), (9, 700)),
]


def _sgd_cases():
    """Every (F, rank) at the batch size its place in the path gives it, every other one at the next size as well; with two
    sizes (NC > 1) at both.  One case of each path (its first shape) runs at lambda = 0 with one field of all-zero weights."""
    cases = []
    for path, shapes, Bs in PATHS:
        for j, (F, rank) in enumerate(shapes):
            take = Bs if len(Bs) == 2 else (Bs[j % 3],) + ((Bs[(j + 1) % 3],) if j % 2 == 0 else ())
            for n, B in enumerate(take):
                cases.append((path, F, rank, B, j == 0 and n == len(take) - 1))
    return cases


SGD_CASES = _sgd_cases()


def sgd_hparams(i, B, zero):
    """(reduce_mean, lambda) of case i: the reductions alternate over the cases of up to 17 examples (every path has both) and
    lambda rotates over {0, 1e-3, 1e-2, 0.05}.  From 257 examples on the loss is the mean: the sum of that many gradients at
    lr = 0.05 diverges in three steps, with or without weights (|logit| > 1e5 in the float64 restatement), and a saturated
    sigmoid checks nothing."""
    small = sum(1 for c in SGD_CASES[:i] if c[3] <= 17)
    return (1 if B > 17 else small % 2), (0.0 if zero else (0.0, 1e-3, 1e-2, 0.05)[(i // 2) % 4])


@pytest.mark.parametrize("path,F,rank,B,zero", SGD_CASES, ids=['%s-F%d-r%d-B%d' % c[:4] + ('-zero' if c[4] else '') for c in SGD_CASES])
def test_weighted_sgd_steps_vs_restatement(built, path, F, rank, B, zero):
    """The forward and three SGD steps.  With lambda = 0, rows no batch touched and rows that only zero weights touched are equal
    to the start bit for bit."""
    i = SGD_CASES.index((path, F, rank, B, zero))
    reduce_mean, lam = sgd_hparams(i, B, zero)
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes) + 24, F, rank, i)
    m = model(F, rank, B, ['sgd', 0.05] + ([] if reduce_mean else ['sum']), lam, rows, 0.1)
    try:
        bs = wbatches(sizes, B, 3, 200 + i, gap=24, zero_field=F - 1 if zero else None)
        _, got = sgd_vs_oracle_w(m, rows, 0.1, bs, 0.05, lam, reduce_mean)
        if lam == 0.0:
            seen, live = np.zeros(len(rows), bool), np.zeros(len(rows), bool)
            for ids, _, w in bs:
                seen[ids[ids >= 0]] = True
                live[ids[(ids >= 0) & (w != 0)]] = True
            assert (~seen).any() and np.array_equal(got[~seen], rows[~seen].astype(np.float32))
            dead = seen & ~live                                        # touched, with weight 0 only
            if zero:
                assert dead.any()
            assert np.array_equal(got[dead], rows[dead].astype(np.float32)), "a row that only zero weights touched moved"
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 2. Adam and FTRL
OPT_CASES = [(opt, F, rank) for opt in ('adam', 'ftrl') for (F, rank) in ((16, 10), (39, 10), (39, 0), (16, 100), (39, 100), (64, 127))]


@pytest.mark.parametrize("opt,F,rank", OPT_CASES, ids=['%s-F%d-r%d' % c for c in OPT_CASES])
def test_weighted_optimiser_steps_vs_restatement(built, opt, F, rank):
    """Four Adam / FTRL steps against TrainerW, with test_fields_optim_steps_vs_oracle's per-step bounds and check_state."""
    i = OPT_CASES.index((opt, F, rank))
    B = (100, 700, 1)[i % 3]
    reduce_mean, lam = i % 2, (0.0, 1e-3, 0.05)[(i // 2) % 3]
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes) + 24, F, rank, 50 + i)
    argv = [opt, LRS[opt]] + ([1e-8] if opt == 'adam' else []) + ([] if reduce_mean else ['sum'])
    m = model(F, rank, B, argv, lam, rows, 0.1)
    try:
        tr = wr.TrainerW(rows, 0.1, opt, LRS[opt], lam, reduce_mean)
        tr.rows0 = rows.copy()
        seen = np.zeros(len(rows), bool)
        for step, (ids, y, w) in enumerate(wbatches(sizes, B, 4, 300 + i, gap=24)):
            out = m.train_step(ids, y, want_p=True, wts=w)
            data, p = tr.step(ids, y, w)
            tol = 5e-5 if step == 0 else 2e-3
            np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=tol, atol=1e-6)
            assert abs(out['loss'] - data) <= tol * max(1.0, abs(data))
            seen[ids[ids >= 0]] = True
        check_state(m, tr)
        if lam == 0.0:
            got, _ = m.get_params()
            assert (~seen).any()
            if opt == 'ftrl':
                assert not got[~seen].any()                            # re-derived from linear = 0
            else:
                assert np.array_equal(got[~seen], rows[~seen].astype(np.float32))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 3. no weights is the old call
@pytest.mark.parametrize("F,rank", [(16, 10), (39, 10), (16, 50), (39, 100)])
def test_none_is_the_unweighted_call_and_ones_track_the_unweighted_oracle(built, F, rank):
    B, lam = 257, 1e-3
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes), F, rank, 7)
    bs = wbatches(sizes, B, 3, 77)
    outs = []
    for kw in ({}, {'wts': None}):
        m = model(F, rank, B, ['sgd', 0.05], lam, rows, 0.1)
        try:
            for ids, y, _ in bs:
                m.train_step(ids, y, **kw)
            outs.append(m.get_params())
        finally:
            m.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    m = model(F, rank, B, ['sgd', 0.05], lam, rows, 0.1)
    try:
        ones = [(ids, y, np.ones(ids.shape, np.float32)) for ids, y, _ in bs]
        _, got = sgd_vs_oracle_w(m, rows, 0.1, ones, 0.05, lam, 1, unweighted_oracle=True)
        gb = m.get_params()[1]
    finally:
        m.close()
    print("[fm-weights] F %d rank %d: all-ones weights %s the unweighted run bit for bit (largest difference %.3e)" %
          (F, rank, "equal" if np.array_equal(got, outs[0][0]) and gb == outs[0][1] else "do NOT equal", np.abs(got - outs[0][0]).max()))


# ------------------------------------------------------------------------------------------------ 4. forward and evaluate over chunks
@pytest.mark.parametrize("F,rank", [(16, 10), (39, 10), (16, 50), (39, 100)])
def test_weighted_forward_and_evaluate_over_chunks(built, F, rank):
    """N = 2 max_batch + 3: the weights of a chunk travel with its ids, in FM.forward and inside fm_eval_w."""
    mb = 256
    N = 2 * mb + 3
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes), F, rank, 9)
    (ids, _, wts), = wbatches(sizes, N, 1, 31)
    y = (np.random.RandomState(10).uniform(size=N) < 0.3).astype(np.int32)
    m = model(F, rank, mb, ['sgd', 0.05], 0.0, rows, -0.2)
    try:
        assert m.max_batch == mb
        p = m.forward(ids, wts=wts).cpu().numpy().astype(np.float64)
        want = wr.predict_w(rows, -0.2, ids, wts)
        print("[fm-weights] forward F %d rank %d: largest relative error %.3e" % (F, rank, np.abs(p / want - 1).max()))
        np.testing.assert_allclose(p, want, rtol=2e-5)
        auc, rmse, ll = m.evaluate(ids, y, wts=wts)
        ea, er, el = np_metrics(p, y)
        assert abs(auc - ea) <= 1e-12 and abs(rmse - er) <= 1e-12 and abs(ll - el) <= 1e-12, ((auc, rmse, ll), (ea, er, el))
        # a reference whose weights lag one chunk behind its ids must NOT match: the check above can tell
        shifted = wr.predict_w(rows, -0.2, ids, np.roll(wts, mb, axis=0))
        assert np.abs(p / shifted - 1).max() > 1e-2
        sa, sr, sl = np_metrics(shifted, y)
        assert abs(rmse - sr) > 1e-6 and abs(ll - sl) > 1e-6
        assert np.abs(p - m.forward(ids).cpu().numpy()).max() > 1e-3            # the weights matter
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 5. arguments
@pytest.mark.parametrize("F,rank", [(16, 10), (39, 100)])
def test_weight_arguments(built, F, rank):
    sizes = synth.field_sizes_tiny(400, F)
    rows = table(sum(sizes), F, rank, 3)
    m = model(F, rank, 64, ['sgd', 0.01], 0.0, rows, 0.0)
    try:
        (ids, y, wts), = wbatches(sizes, 64, 1, 5)
        for bad in (wts[:, :F - 1], wts[:-1], wts.reshape(-1)):
            with pytest.raises(ValueError):
                m.train_step(ids, y, wts=bad)
            with pytest.raises(ValueError):
                m.forward(ids, wts=bad)
            with pytest.raises(ValueError):
                m.evaluate(ids, y.astype(np.int32), wts=bad)
        assert np.array_equal(m.get_params()[0], rows.astype(np.float32))      # nothing ran
        codes = []
        for kw in ({}, {'wts': wts}):
            bad_ids = ids.copy()
            bad_ids[10, F - 1] = len(rows)
            with pytest.raises(FNNError) as e:
                m.train_step(bad_ids, y, **kw)
            codes.append(e.value.code)
            bad_ids[10, F - 1] = -2
            with pytest.raises(FNNError) as e:
                m.forward(bad_ids, **kw)
            codes.append(e.value.code)
        assert codes == [_capi.FNN_ERR_RANGE] * 4
        big = np.zeros((4097, F), np.int32)
        with pytest.raises(FNNError) as e:
            m.train_step(big, np.zeros(4097), wts=np.ones((4097, F), np.float32))
        assert e.value.code == _capi.FNN_ERR_ARG
    finally:
        m.close()


def test_weights_at_absent_fields_and_nan_propagation(built):
    """A NaN weight at an absent field changes no bit of a step; at a present field it reaches that example's prediction."""
    F, rank, B = 39, 10, 64
    sizes = synth.field_sizes_tiny(400, F)
    rows = table(sum(sizes), F, rank, 4)
    (ids, y, wts), = wbatches(sizes, B, 1, 6)
    assert (ids < 0).any()
    bad = wts.copy()
    bad[ids < 0] = np.nan
    outs = []
    for w in (wts, bad):
        m = model(F, rank, B, ['adam', 1e-2, 1e-8], 1e-3, rows, 0.1)
        try:
            p = m.train_step(ids, y, want_p=True, wts=w)['p'].cpu().numpy()
            outs.append((p, m.get_params(), m.get_opt_state()))
            if w is bad:
                t, f = np.argwhere(ids >= 0)[5]
                w2 = wts.copy()
                w2[t, f] = np.nan
                p2 = m.forward(ids, wts=w2).cpu().numpy()
                assert np.isnan(p2[t]) and np.isfinite(np.delete(p2, t)).all()
        finally:
            m.close()
    (p0, (r0, b0), s0), (p1, (r1, b1), s1) = outs
    assert np.isfinite(p0).all() and np.array_equal(p0, p1) and np.array_equal(r0, r1) and b0 == b1
    assert all(np.array_equal(a, c) for a, c in zip(s0[:3], s1[:3]))


# ------------------------------------------------------------------------------------------------ 6. the Criteo shape, end to end
def test_criteo_feed_pretrains_fm_and_seeds_fnn_ip_l3(built, tmp_path):
    """13 numeric fields (one row each, weighted by their value) + 26 categorical fields of about 40 rows, B = 100, rank 10,
    through ipnn.criteo_feed: three Adam steps against TrainerW; the dumped rows seed FNN_IP_L3 at X_feas = 39, whose first
    weighted prediction equals the inner-product family's own float64 reference on those rows."""
    n_num, n_cat, B, rank = 13, 26, 100, 10
    F = n_num + n_cat
    sizes = synth.field_sizes_tiny(40 * n_cat, n_cat)
    D = n_num + sum(sizes)
    offsets = n_num + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rows = table(D, F, rank, 13)
    fm = model(F, rank, B, ['adam', 1e-2, 1e-8, 'sum'], 1e-3, rows, 0.0)
    try:
        tr = wr.TrainerW(rows, 0.0, 'adam', 1e-2, 1e-3, 0)
        tr.rows0 = rows.copy()
        rng = np.random.RandomState(6)
        for s in range(3):
            c_ids = synth.zipf_ids(B, sizes, 1.1, 5 + s) - (offsets - n_num)          # per-field ids, as the driver feeds them
            v_wts = rng.uniform(0.0, 2.0, size=(B, n_num)).astype(np.float32)
            v_wts[rng.uniform(size=v_wts.shape) < 0.05] = 0.0
            ids, wts = criteo_feed(v_wts, c_ids, np.ones((B, n_cat), np.float32), offsets)
            assert ids.shape == (B, F) and ids.max() < D
            y = (rng.uniform(size=B) < 0.3).astype(np.float64)
            out = fm.train_step(ids, y, want_p=True, wts=wts)
            data, p = tr.step(ids, y, wts)
            tol = 5e-5 if s == 0 else 2e-3
            np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=tol, atol=1e-6)
            assert abs(out['loss'] - data) <= tol * max(1.0, abs(data))
        check_state(fm, tr)
        got, b = fm.get_params()
        path = str(tmp_path / 'fm39.pkl')
        fm.dump(path)
    finally:
        fm.close()
    assert pickle.load(open(path, 'rb'))['V'].shape == (D, rank)
    m = FNN_IP_L3([], [], B, [D, F, rank, 40, 24, 12, 'relu'], ['uniform', -0.05, 0.05, [3, 4, 5], path], ['sgd', 0.002, 'sum'],
                  [1.0], 'train', B, precision='f32')
    try:
        assert np.array_equal(m.eng.get_rows(np.arange(D)), got)
        bb, Ws, bs = m.eng.get_params()
        assert bb == np.float32(b)
        params = {'b': bb, 'W': [w.astype(np.float64) for w in Ws], 'bias': [v.astype(np.float64) for v in bs]}
        want = iwr.predict_w(params, got.astype(np.float64), ids, wts, 'relu')
        np.testing.assert_allclose(m.eng.predict(ids, wts).cpu().numpy(), want, rtol=2e-4)
    finally:
        m.eng.close()
