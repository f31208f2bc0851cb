"""The SNN-DAE pre-training kernels (include/dae_hip.h) at every shape they accept, against oracle/dae_oracle.py's da_grads walked
by tests/pretrain_ref.py: the sparse trainer away from H = 40 / 200, S = 32 (H < S, S < 32, H = 256, bhid_prev, the range error),
the four f32 register tilings of the dense trainer at their edges and one past them (the global-memory form), the float64 split
trainer at its row classes, with fewer columns than workgroups and one past its limits, and the layer-0 / affine kernels.
lr = 0.1 (the reference's), NON-ZERO biases on entry.  f32: 2e-3 of the parameter change, 1e-4 for the cost; f64: 1e-10 (cost 1e-11, as
test_gpu_dae.py).  Each case prints its measured ratios.  Largest measured on an MI355X (error / parameter change):
  sparse_da   f32 2.3e-7 (cost 5.4e-8), f64 1.9e-15
  da f32      W 1.6e-5 (2048 x 1024), bhid 1.1e-4 (7 x 1000), bvis 1.8e-6, cost 8.2e-8
  da f64      W 4.0e-13, bhid 4.2e-13 (512 x 513), bvis 5.9e-14, cost 3.9e-16; the two forms agree as closely
  layer 0     f32 at most 0.096 of its bound (1.2e-7), f64 6.1e-16; affine f64 5.0e-16"""
import ctypes as C

import numpy as np
import pytest

import pretrain_ref as pr

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    dev = torch.device('cuda', 0)
    return torch, dev, torch.cuda.current_stream(dev).cuda_stream


def _t(a, dt):
    torch, dev, _ = _dev()
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()


def _ratio(got, ref, init):
    return float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref - init).max() + 1e-300))


# ------------------------------------------------------------------------------------------ sparse_da
@pytest.mark.parametrize("f64", [False, True], ids=['f32', 'f64'])
@pytest.mark.parametrize("H,S,N", [(1, 1, 30), (8, 32, 60), (65, 7, 80), (200, 31, 50), (256, 32, 40)])
def test_sparse_epoch_shapes(built, H, S, N, f64):
    """dae_sparse_epoch / _f64: H < S (threads that own a bvis slot and no hidden unit), S < 32, H = 1 / 65 / 256.  bhid, bvis, the cost sum
    and bhid_prev (bhid BEFORE the last example; for a call of one example: the input, bit for bit) against the per-example
    reference; the table bit for bit untouched; an id equal to n_rows is FNN_ERR_RANGE (the load is guarded: nothing faults)."""
    torch, dev, st = _dev()
    lib = _capi.load()
    n_rows = 50
    rng = np.random.RandomState(100 * H + S)
    rd = (lambda a: np.asarray(a, np.float64)) if f64 else pr.r32
    b = 4 * np.sqrt(6. / (n_rows + H))
    table = rd(rng.uniform(-b, b, (n_rows, H)))
    idx = np.stack([rng.choice(n_rows, size=S, replace=False) for _ in range(N)]).astype(np.int32)
    x = (rng.uniform(size=(N, S)) < 0.5).astype(np.float64)
    bh0, bv0 = rd(rng.uniform(-0.1, 0.1, H)), rd(rng.uniform(-0.1, 0.1, S))
    bh, bv, prev, cost = pr.run_sparse_da(table, idx, x, bh0, bv0, 0.1)
    dt = torch.float64 if f64 else torch.float32
    fn = lib.dae_sparse_epoch_f64 if f64 else lib.dae_sparse_epoch
    tol, tol_c = (1e-10, 1e-10) if f64 else (pr.TOL, pr.TOL_ERR)

    def call(idx_, x_, n):
        td, bhd, bvd, pvd = _t(table, dt), _t(bh0, dt), _t(bv0, dt), torch.full((H,), 7.0, dtype=dt, device=dev)
        keep = td.clone()
        c = C.c_double(-1.0)
        idd, xd = _t(idx_, torch.int32), _t(x_, dt)
        rc = fn(td.data_ptr(), n_rows, bhd.data_ptr(), bvd.data_ptr(), pvd.data_ptr(), idd.data_ptr(), xd.data_ptr(), n, H, S, 0.1, C.byref(c), st)
        torch.cuda.synchronize()
        assert torch.equal(td, keep)                               # Q1: the table is constant
        return rc, bhd.cpu().numpy(), bvd.cpu().numpy(), pvd.cpu().numpy(), c.value

    rc, g_bh, g_bv, g_prev, g_cost = call(idx, x, N)
    assert rc == 0, lib.dae_last_error()
    r = (_ratio(g_bh, bh, bh0), _ratio(g_bv, bv, bv0), _ratio(g_prev, prev, bh0), abs(g_cost - cost) / cost)
    print("sparse_da %s H=%d S=%d N=%d: error/change bhid %.2e bvis %.2e bhid_prev %.2e, cost %.2e" % (('f64' if f64 else 'f32', H, S, N) + r))
    assert r[0] <= tol and r[1] <= tol and r[2] <= tol and r[3] <= tol_c
    # one example: bhid_prev is the input
    rc, g_bh, g_bv, g_prev, g_cost = call(idx[:1], x[:1], 1)
    assert rc == 0, lib.dae_last_error()
    assert np.array_equal(g_prev.astype(np.float64), bh0)
    c1, bh1, bv1 = pr.sparse_da_example(table, idx[0], bh0, bv0, x[0], 0.1)
    assert _ratio(g_bh, bh1, bh0) <= tol and _ratio(g_bv, bv1, bv0) <= tol and abs(g_cost - c1) <= tol_c * c1
    # an id of n_rows
    bad = idx.copy()
    bad[N // 2, S - 1] = n_rows
    rc = call(bad, x, N)[0]
    assert rc == _capi.FNN_ERR_RANGE and b'n_rows' in lib.dae_last_error()


# ------------------------------------------------------------------------------------------ da, f32
def _dense_f32(row, col, N, skip):
    torch, dev, st = _dev()
    lib = _capi.load()
    c = pr.dae_dense_case(row, col, N, np.float32)
    W, bh, bv, cost = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'], 0.1, skip)
    Wd, bhd, bvd, Xd = (_t(c[k], torch.float32) for k in ('W', 'bh', 'bv', 'X'))
    cs = C.c_double(-1.0)
    rc = lib.dae_dense_epoch(Wd.data_ptr(), bhd.data_ptr(), bvd.data_ptr(), Xd.data_ptr(), N, row, col, 0.1, skip, C.byref(cs), st)
    assert rc == 0, lib.dae_last_error()
    torch.cuda.synchronize()
    return c, (W, bh, bv, cost), (Wd.cpu().numpy(), bhd.cpu().numpy(), bvd.cpu().numpy(), cs.value)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("row,col", pr.DAE_DENSE_F32)
def test_dense_epoch_f32_tiling_edges(built, row, col, skip):
    """k_dae_dense<4,1> at 64 x 64, <8,2> at 65 x 64 / 64 x 65 / 128 x 128, <19,2> at 129 x 128 / 304 x 128, <13,5> at 208 x 320, and one past each
    edge of `fits` (305 x 128, 304 x 129, 209 x 320, 208 x 321), very wide and very tall shapes (7 x 1000, 1500 x 3) and 1 x 1 in the global-memory
    form k_dae_dense_g<float>; both skip_last_update values; non-zero biases on entry."""
    N = pr.dae_dense_steps(row, col)
    c, (W, bh, bv, cost), (gW, gbh, gbv, gcost) = _dense_f32(row, col, N, skip)
    r = (_ratio(gW, W, c['W']), _ratio(gbh, bh, c['bh']), _ratio(gbv, bv, c['bv']), abs(gcost - cost) / abs(cost))
    print("da f32 %dx%d N=%d skip=%d: error/change W %.2e bhid %.2e bvis %.2e, cost %.2e" % ((row, col, N, skip) + r))
    assert r[0] <= pr.TOL and r[1] <= pr.TOL and r[2] <= pr.TOL and r[3] <= pr.TOL_ERR


def test_dense_epoch_f32_largest_shape(built):
    """2048 x 1024, the largest shape the header promises (global-memory form, 45 KB of dynamic LDS), four steps."""
    c, (W, bh, bv, cost), (gW, gbh, gbv, gcost) = _dense_f32(2048, 1024, 4, 0)
    r = (_ratio(gW, W, c['W']), _ratio(gbh, bh, c['bh']), _ratio(gbv, bv, c['bv']), abs(gcost - cost) / abs(cost))
    print("da f32 2048x1024 N=4: error/change W %.2e bhid %.2e bvis %.2e, cost %.2e" % r)
    assert r[0] <= pr.TOL and r[1] <= pr.TOL and r[2] <= pr.TOL and r[3] <= pr.TOL_ERR


def test_dense_epoch_f32_one_example_skipped(built):
    """N = 1 with skip_last_update: the parameters come back bit for bit as they went in, the cost is the example's."""
    c, (W, bh, bv, cost), (gW, gbh, gbv, gcost) = _dense_f32(100, 100, 1, 1)
    assert np.array_equal(W, c['W'])
    assert np.array_equal(gW.astype(np.float64), c['W']) and np.array_equal(gbh.astype(np.float64), c['bh']) and np.array_equal(gbv.astype(np.float64), c['bv'])
    print("da f32 100x100 N=1 skipped: cost %.2e" % (abs(gcost - cost) / cost))
    assert abs(gcost - cost) <= pr.TOL_ERR * cost


# ------------------------------------------------------------------------------------------ da, f64
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("row,col", pr.DAE_DENSE_F64)
def test_dense_epoch_f64_split_classes(built, row, col, skip, monkeypatch):
    """The eight-workgroup trainer at the edges of its rows-per-wave classes (8 | 13 | 19 | 32: 128 / 129, 208 / 209, 304 / 305, 512 rows), with
    fewer columns than workgroups (7, 1: workgroups that own no hidden unit still take part in the exchange), at its limit 512 x 512 and
    one past it either way (513 x 512, 512 x 513: the one-workgroup form); DAE_SPLIT unset and = 0 agree with the oracle and each other."""
    torch, dev, st = _dev()
    lib = _capi.load()
    N = 40
    c = pr.dae_dense_case(row, col, N, np.float64)
    W, bh, bv, cost = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'], 0.1, skip)
    got = {}
    for form in (None, '0'):
        if form is None:
            monkeypatch.delenv('DAE_SPLIT', raising=False)
        else:
            monkeypatch.setenv('DAE_SPLIT', form)
        Wd, bhd, bvd, Xd = (_t(c[k], torch.float64) for k in ('W', 'bh', 'bv', 'X'))
        cs = C.c_double(-1.0)
        rc = lib.dae_dense_epoch_f64(Wd.data_ptr(), bhd.data_ptr(), bvd.data_ptr(), Xd.data_ptr(), N, row, col, 0.1, skip, C.byref(cs), st)
        assert rc == 0, lib.dae_last_error()
        torch.cuda.synchronize()
        got[form] = g = (Wd.cpu().numpy(), bhd.cpu().numpy(), bvd.cpu().numpy(), cs.value)
        r = (_ratio(g[0], W, c['W']), _ratio(g[1], bh, c['bh']), _ratio(g[2], bv, c['bv']), abs(g[3] - cost) / abs(cost))
        print("da f64 %dx%d skip=%d DAE_SPLIT=%s: error/change W %.2e bhid %.2e bvis %.2e, cost %.2e" % ((row, col, skip, form) + r))
        assert r[0] <= 1e-10 and r[1] <= 1e-10 and r[2] <= 1e-10 and r[3] <= 1e-11
    assert np.abs(got[None][0] - got['0'][0]).max() <= 1e-10 * np.abs(c['W']).max()


# ------------------------------------------------------------------------------------------ layer 0, affine
@pytest.mark.parametrize("f64", [False, True], ids=['f32', 'f64'])
@pytest.mark.parametrize("F", [1, 16])
@pytest.mark.parametrize("H", [1, 64, 65, 1000, 1024])
def test_bag_cumsum_sigmoid(built, H, F, f64):
    """Layer 0 of da(): sigmoid(cumsum over the hidden units of the bag sum + b0) -- block sizes 64, 128 and 1024, full and partly
    idle; -1 ids, duplicates, an all -1 row; an id of n_rows is FNN_ERR_RANGE.  f32: 4 (F (k + 1) + 1) 2^-24 sum |terms| before the
    sigmoid for unit k, a quarter of it plus the evaluation's 8 * 2^-24 after; f64: 1e-12."""
    torch, dev, st = _dev()
    lib = _capi.load()
    n, n_rows = 6, 13
    rng = np.random.RandomState(H + F)
    rd = (lambda a: np.asarray(a, np.float64)) if f64 else pr.r32
    W0, b0 = rd(rng.uniform(-2, 2, (n_rows, H)) / np.sqrt(F * H)), rd(rng.uniform(-0.5, 0.5, H))      # the running sum stays O(1): no saturated unit
    ids = pr.bag_ids(n, F, n_rows, H * F + 1)
    ref, pre = pr.cumsum_sigmoid_ref(W0, b0, ids)
    dt = torch.float64 if f64 else torch.float32
    fn = lib.dae_bag_cumsum_sigmoid_f64 if f64 else lib.dae_bag_cumsum_sigmoid
    W0d, b0d, idd = _t(W0, dt), _t(b0, dt), _t(ids, torch.int32)
    out = torch.full((n + 1, H), 7.0, dtype=dt, device=dev)
    assert fn(W0d.data_ptr(), b0d.data_ptr(), H, n_rows, idd.data_ptr(), n, F, out.data_ptr(), st) == 0, lib.dae_last_error()
    got = out.cpu().numpy().astype(np.float64)
    bound = np.full_like(ref, 1e-12) if f64 else pr.sigmoid_bound(pre)
    print("bag_cumsum %s H=%d F=%d: worst error %.2e, error / bound %.3f" % ('f64' if f64 else 'f32', H, F, np.abs(got[:n] - ref).max(),
                                                                           (np.abs(got[:n] - ref) / bound).max()))
    assert (np.abs(got[:n] - ref) <= bound).all()
    assert (got[n] == 7.0).all()                                   # nothing past the n examples
    assert 1e-3 < ref.min() and ref.max() < 1 - 1e-3               # the inputs keep every unit out of saturation
    bad = ids.copy()
    bad[1, F - 1] = n_rows
    bdd = _t(bad, torch.int32)
    assert fn(W0d.data_ptr(), b0d.data_ptr(), H, n_rows, bdd.data_ptr(), n, F, out.data_ptr(), st) == _capi.FNN_ERR_RANGE
    assert b'n_rows' in lib.dae_last_error()


@pytest.mark.parametrize("n,a,b", [(3, 1, 1), (5, 300, 257)])
def test_affine_sigmoid_f64(built, n, a, b):
    torch, dev, st = _dev()
    lib = _capi.load()
    rng = np.random.RandomState(a + b)
    x, W, bias = rng.uniform(0, 1, (n, a)), rng.uniform(-2, 2, (a, b)) / np.sqrt(a), rng.uniform(-0.5, 0.5, b)
    ref = 1.0 / (1.0 + np.exp(-(x @ W + bias)))
    xd, Wd, bd = _t(x, torch.float64), _t(W, torch.float64), _t(bias, torch.float64)
    out = torch.full((n * b + 1,), 7.0, dtype=torch.float64, device=dev)
    assert lib.dae_affine_sigmoid_f64(xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), n, a, b, out.data_ptr(), st) == 0, lib.dae_last_error()
    got = out.cpu().numpy()
    print("affine_sigmoid_f64 %dx%dx%d: worst error %.2e" % (n, a, b, np.abs(got[:-1].reshape(n, b) - ref).max()))
    assert np.abs(got[:-1].reshape(n, b) - ref).max() <= 1e-12 and got[-1] == 7.0
