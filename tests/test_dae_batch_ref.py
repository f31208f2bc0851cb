"""tests/dae_batch_ref.py, the float64 restatement of the reference's mini-batch dA step (:97-113), held to (1) the online reference
pretrain_ref.run_dense_da at M = 1 without a mask, exactly; (2) torch.autograd on the CPU for the gradients of mean(L) with tied
weights and a keep mask, 1e-12 relative (tests/test_oracle_autograd.py is the precedent); (3) the input regime of the GPU cases:
every reconstruction of the float64 run of every case of DAE_BATCH_CASES stays within [1e-4, 1 - 1e-4], the condition
pretrain_ref.dae_dense_case documents (over all cases the reconstructions span 1.5e-3 .. 1 - 2.9e-4; the test prints it)."""
import numpy as np
import pytest

import dae_batch_ref as br
import pretrain_ref as pr


@pytest.mark.parametrize("row,col,N,skip", [(1, 1, 5, 0), (7, 5, 12, 1), (30, 17, 9, 0), (129, 65, 6, 1)])
def test_batch_of_one_is_the_online_reference(row, col, N, skip):
    c = pr.dae_dense_case(row, col, N, np.float64)
    W, bh, bv, cost = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'], 0.1, skip)
    gW, gbh, gbv, gcost = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], None, 1, 0.1, skip)
    assert np.array_equal(gW, W) and np.array_equal(gbh, bh) and np.array_equal(gbv, bv) and gcost == cost


@pytest.mark.parametrize("masked", [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize("row,col,m", [(1, 1, 1), (9, 4, 3), (33, 20, 20), (64, 70, 7)])
def test_gradients_against_autograd(row, col, m, masked):
    torch = pytest.importorskip("torch")
    c = pr.dae_dense_case(row, col, m, np.float64)
    keep = br.keep_mask(m, row, row + col) if masked else None
    cost, gW, gbh, gbv, _ = br.batch_grads(c['W'], c['bh'], c['bv'], c['X'], keep)
    W, bh, bv = (torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in ('W', 'bh', 'bv'))
    X = torch.tensor(c['X'], dtype=torch.float64)
    Xt = X * torch.tensor((keep != 0).astype(np.float64)) if masked else X
    Y = torch.sigmoid(Xt @ W + bh)
    Z = torch.sigmoid(Y @ W.T + bv)                                         # tied weights: W enters twice
    L = -(X * torch.log(Z) + (1 - X) * torch.log(1 - Z)).sum(dim=1)
    tc = L.mean()
    tc.backward()
    for name, got, ref in (('W', gW, W.grad), ('bhid', gbh, bh.grad), ('bvis', gbv, bv.grad)):
        ref = ref.numpy()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s %dx%d m=%d %s: %.2e" % (name, row, col, m, 'masked' if masked else 'plain', err))
        assert err <= 1e-12
    assert abs(cost - tc.item()) <= 1e-12 * abs(tc.item())


def test_short_last_batch_and_skip():
    """N % M != 0: the last batch takes its own mean; skip_last leaves the parameters as they were before it; N <= M with skip_last
    returns the inputs themselves."""
    c = pr.dae_dense_case(9, 4, 7, np.float64)
    keep = br.keep_mask(7, 9, 1)
    W, bh, bv, cost = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], keep, 3, 0.1, 0)
    W1, bh1, bv1, c1 = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'][:6], keep[:6], 3, 0.1, 0)
    c2, gW, gbh, gbv, _ = br.batch_grads(W1, bh1, bv1, c['X'][6:], keep[6:])                # one example: mean over 1
    assert cost == c1 + c2 and np.array_equal(W, W1 - 0.1 * gW) and np.array_equal(bh, bh1 - 0.1 * gbh) and np.array_equal(bv, bv1 - 0.1 * gbv)
    Ws, bhs, bvs, cs = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], keep, 3, 0.1, 1)
    assert cs == cost and np.array_equal(Ws, W1) and np.array_equal(bhs, bh1) and np.array_equal(bvs, bv1)
    Wn, bhn, bvn, cn = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], keep, 20, 0.1, 1)
    assert Wn is c['W'] and bhn is c['bh'] and bvn is c['bv'] and cn == br.batch_grads(c['W'], c['bh'], c['bv'], c['X'], keep)[0]


def test_case_list_covers_what_the_issue_asks():
    for f64 in (True, False):
        cs = [c for c in br.DAE_BATCH_CASES if c[5] == f64]
        assert {c[:2] for c in cs} == set(br.SHAPES) and {c[2:4] for c in cs} == set(br.BATCHES)
        assert {c[4] for c in cs} == {False, True} and {c[6] for c in cs} == {0, 1}


def test_gpu_cases_stay_out_of_saturation():
    """The float64 run of every GPU parity case (both input roundings): every reconstruction within [1e-4, 1 - 1e-4]."""
    lo, hi = 1.0, 0.0
    seen = set()
    for row, col, M, N, masked, f64, skip in br.DAE_BATCH_CASES:
        key = (row, col, M, N, masked, f64)
        if key in seen:
            continue
        seen.add(key)
        c = pr.dae_dense_case(row, col, N, np.float64 if f64 else np.float32)
        zr = [1.0, 0.0]
        br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], br.keep_mask(N, row, row + col) if masked else None, M, 0.1, 0, zr)
        assert 1e-4 <= zr[0] and zr[1] <= 1 - 1e-4, (key, zr)
        lo, hi = min(lo, zr[0]), max(hi, zr[1])
    print("reconstructions over all GPU cases: %.3e .. 1 - %.3e" % (lo, 1 - hi))
