"""The float64 restatement of weighted FM / LR pre-training (tests/fm_weighted_ref.py) against what it restates: oracle/fm_oracle.py
and fm_optim_ref.py at weight 1, a literal transcription of python/FM.py:55-64 (x w, x v and x^2 v^2 as separate terms), and
PyTorch float64 autograd of that literal form (tests/test_oracle_autograd.py is the precedent).  CPU only."""
import numpy as np
import pytest
import torch

import fm_optim_ref as ref
import fm_weighted_ref as wr
from oracle import fm_oracle as fo

from test_gpu_fm_fields import table
from deep_ctr_amd import synth


def problem(B, F, rank, seed, n=60):
    """Rows, bias, ids with repeated rows and absent fields, weights of wr.test_weights, labels."""
    rng = np.random.RandomState(seed)
    rows = rng.standard_normal((n, rank + 1)) * 0.3
    ids = rng.randint(0, n, size=(B, F)).astype(np.int32)
    ids[rng.uniform(size=ids.shape) < 0.1] = -1
    y = (rng.uniform(size=B) < 0.4).astype(np.float64)
    return rows, 0.15, ids, wr.test_weights(B, F, seed + 1).astype(np.float64), y


def literal_logits(W, V, b, ids, x):
    """python/FM.py:55-64 term by term: embedding_lookup_sparse(W, ids, x) + b, _Vx = sum x v, _V2x2 = sum x^2 v^2 (torch or
    NumPy operands; ids >= 0)."""
    yhat = (x * W[ids][..., 0]).sum(1) + b
    Vx = (x[..., None] * V[ids]).sum(1)
    V2x2 = ((x * x)[..., None] * (V * V)[ids]).sum(1)
    return yhat + 0.5 * ((Vx * Vx).sum(1) - V2x2.sum(1))


@pytest.mark.parametrize("F,rank", [(1, 0), (5, 3), (16, 10), (39, 20)])
def test_unit_weights_are_the_unweighted_oracle(F, rank):
    rows, b, ids, _, y = problem(33, F, rank, 3 + F)
    ones = np.ones(ids.shape)
    np.testing.assert_allclose(wr.logits_w(rows, b, ids, ones), fo.logits(rows, b, ids), rtol=1e-13)
    for mean, lam in ((0, 0.0), (1, 0.02)):
        got, want = wr.dense_grad_w(rows, b, ids, ones, y, lam, mean), ref.dense_grad(rows, b, ids, y, lam, mean)
        for a, c in zip(got, want):
            np.testing.assert_allclose(a, c, rtol=1e-13, atol=1e-300)
        r1, r2 = rows.copy(), rows.copy()
        o1, o2 = wr.sgd_step_w(r1, b, ids, ones, y, 0.05, lam, mean == 1), fo.sgd_step(r2, b, ids, y, 0.05, lam, mean == 1)
        np.testing.assert_allclose(r1, r2, rtol=1e-13)
        for a, c in zip(o1, o2):
            np.testing.assert_allclose(a, c, rtol=1e-13)


@pytest.mark.parametrize("F,rank", [(2, 1), (16, 10), (39, 7)])
def test_logits_equal_the_literal_form(F, rank):
    rows, b, ids, wts, _ = problem(41, F, rank, 11 + F)
    live = ids >= 0
    lit = literal_logits(rows[:, :1], rows[:, 1:], b, np.where(live, ids, 0), np.where(live, wts, 0.0))
    np.testing.assert_allclose(wr.logits_w(rows, b, ids, wts), lit, rtol=1e-12)


@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 0.03])
@pytest.mark.parametrize("F,rank", [(3, 0), (16, 10)])
def test_dense_grad_equals_autograd_of_the_literal_form(F, rank, lam, mean):
    """loss = xent (sum | mean) + lambda (l2_loss(W) + l2_loss(V) + l2_loss(b)), l2_loss(t) = sum(t^2) / 2 (python/FM.py:36-41)."""
    rows, b, ids, wts, y = problem(29, F, rank, 21 + F)
    live = ids >= 0
    W = torch.tensor(rows[:, :1], dtype=torch.float64, requires_grad=True)
    V = torch.tensor(rows[:, 1:], dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    z = literal_logits(W, V, tb, torch.tensor(np.where(live, ids, 0), dtype=torch.long),
                       torch.tensor(np.where(live, wts, 0.0), dtype=torch.float64))
    ty = torch.tensor(y)
    xent = torch.clamp(z, min=0) - z * ty + torch.log1p(torch.exp(-torch.abs(z)))
    data = xent.mean() if mean else xent.sum()
    (data + lam * 0.5 * ((W * W).sum() + (V * V).sum() + tb * tb)).backward()
    g, gb, d, p, scale = wr.dense_grad_w(rows, b, ids, wts, y, lam, mean)
    assert abs(d - float(data.detach())) <= 1e-12 * abs(d)
    np.testing.assert_allclose(p, torch.sigmoid(z).detach().numpy(), rtol=1e-12)
    auto = np.concatenate([W.grad.numpy(), V.grad.numpy()], axis=1)
    np.testing.assert_allclose(g, auto, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gb, float(tb.grad), rtol=1e-10)
    assert (scale >= np.abs(g) * (1 - 1e-12)).all()                       # the sum of the |contributions| bounds |g|


def test_a_row_touched_only_with_weight_zero_gets_exactly_lambda_row():
    rows, b, ids, wts, y = problem(25, 6, 4, 31)
    ids[ids == 7] = 8
    ids[3, 2], ids[9, 0] = 7, 7                                           # row 7: twice, both with weight 0
    wts[3, 2], wts[9, 0] = 0.0, -0.0
    for lam in (0.0, 0.02):
        g = wr.dense_grad_w(rows, b, ids, wts, y, lam, 0)[0]
        assert np.array_equal(g[7], lam * rows[7])
        r = rows.copy()
        wr.sgd_step_w(r, b, ids, wts, y, 0.05, lam, False)
        assert np.array_equal(r[7], rows[7] - 0.05 * (lam * rows[7]))


def test_a_nan_weight_at_an_absent_field_changes_nothing():
    rows, b, ids, wts, y = problem(25, 6, 4, 41)
    assert (ids < 0).any()
    bad = wts.copy()
    bad[ids < 0] = np.nan
    assert np.array_equal(wr.logits_w(rows, b, ids, bad), wr.logits_w(rows, b, ids, wts))
    for a, c in zip(wr.dense_grad_w(rows, b, ids, bad, y, 0.01, 1), wr.dense_grad_w(rows, b, ids, wts, y, 0.01, 1)):
        assert np.array_equal(a, c)
    bad[np.argwhere(ids >= 0)[0][0], np.argwhere(ids >= 0)[0][1]] = np.nan    # at a live field it propagates
    assert np.isnan(wr.logits_w(rows, b, ids, bad)).any()


def test_trainer_w_with_unit_weights_is_the_trainer():
    rows, b, ids, _, y = problem(33, 16, 10, 51)
    ones = np.ones(ids.shape)
    for opt, lr in (('adam', 1e-2), ('ftrl', 0.05)):
        a, c = wr.TrainerW(rows, b, opt, lr, 1e-3, 1), ref.Trainer(rows, b, opt, lr, 1e-3, 1)
        for _ in range(3):
            da, dc = a.step(ids, y, ones), c.step(ids, y)
            np.testing.assert_allclose(da[0], dc[0], rtol=1e-13)
        np.testing.assert_allclose(a.rows, c.rows, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(a.s1, c.s1, rtol=1e-12, atol=1e-300)
        assert a.t == c.t and np.array_equal(a.ill, c.ill)


@pytest.mark.parametrize("F,rank", [(1, 0), (2, 16), (16, 10), (17, 15), (39, 50), (64, 127), (16, 100), (39, 0)])
def test_weights_keep_the_magnitudes_the_gpu_bounds_were_set_for(F, rank):
    """test_gpu_fm_weights.py keeps the bounds of test_gpu_fm_fields.py, which were set for logits of that file's table scaling.
    With wr.test_weights on the same tables the logits' standard deviation stays within 15 % of the unweighted one (E x^2 of
    these weights is close to 1); the largest |logit| of the 700 examples is printed beside the unweighted one (the pair term of
    one example can grow by x_i x_j < 4: at 2 fields it reaches 12, elsewhere it stays below 6).  Rank 1 is outside this with or
    without weights, and is not used."""
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes), F, rank, 1)
    ids = synth.zipf_ids(700, sizes, 1.1, 5)
    wts = wr.test_weights(700, F, 6).astype(np.float64)
    zw, z1 = wr.logits_w(rows, 0.1, ids, wts), fo.logits(rows, 0.1, ids)
    assert abs(zw.std() / z1.std() - 1.0) <= 0.15, (zw.std(), z1.std())
    print("[fm-weights] F %d rank %d: std %.3f (unweighted %.3f), max |logit| %.2f (%.2f)" % (F, rank, zw.std(), z1.std(),
                                                                                              np.abs(zw).max(), np.abs(z1).max()))
