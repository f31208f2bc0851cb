"""dae_dense_batch / dae_dense_batch_f64 (include/dae_hip.h: the reference's da() at batch_size = M with a keep mask) against the float64
restatement tests/dae_batch_ref.py: the rows-per-wave class edges, fewer columns than workgroups, the limit 512 x 512 and the
reference's 300 x 100; M = 1 .. 256 with N % M != 0 and N < M (a short batch's own mean); with and without a keep mask (density 0.7, one
example fully corrupted); both precisions, both skip_last_update values.  Inputs from pretrain_ref.dae_dense_case (NON-ZERO biases),
lr = 0.1.  Bounds: f64 1e-10 of the parameter change (cost 1e-11), f32 pretrain_ref.TOL / TOL_ERR.  Every call runs with a guard
element of 7.0 behind W, bhid and bvis.  Each case prints its measured ratios.  Largest measured on an MI355X (error / parameter change):
  f64   W 4.6e-14 (305 x 1, M = 256), bhid 1.4e-14, bvis 4.7e-15, cost 3.9e-16
  f32   W 7.4e-05 (1 x 8, M = 256), bhid 4.2e-05, bvis 5.0e-06, cost 3.4e-07
  M = 1 against dae_dense_epoch[_f64]: f64 1.2e-13, f32 7.6e-05;  da() on the demo file: 2.3e-14 of the change"""
import ctypes as C
import os

import numpy as np
import pytest

import dae_batch_ref as br
import pretrain_ref as pr

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    dev = torch.device('cuda', 0)
    return torch, dev, torch.cuda.current_stream(dev).cuda_stream


def _ratio(got, ref, init):
    return float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref - init).max() + 1e-300))


def _guarded(a, dt):
    """The array on the device with one element of 7.0 behind it."""
    torch, dev, _ = _dev()
    t = torch.full((a.size + 1,), 7.0, dtype=dt, device=dev)
    t[:a.size] = torch.as_tensor(np.ascontiguousarray(a).reshape(-1)).to(device=dev, dtype=dt)
    return t


def _call(c, keep, M, f64, skip, N=None):
    """One call on the case's inputs.  Returns (W, bhid, bvis, cost) as the device left them; the guards must have survived."""
    torch, dev, st = _dev()
    lib = _capi.load()
    dt = torch.float64 if f64 else torch.float32
    fn = lib.dae_dense_batch_f64 if f64 else lib.dae_dense_batch
    row, col = c['W'].shape
    N = c['X'].shape[0] if N is None else N
    Wd, bhd, bvd = _guarded(c['W'], dt), _guarded(c['bh'], dt), _guarded(c['bv'], dt)
    Xd = torch.as_tensor(np.ascontiguousarray(c['X'])).to(device=dev, dtype=dt).contiguous()
    Kd = torch.as_tensor(np.ascontiguousarray(keep)).to(dev).contiguous() if keep is not None else None
    cs = C.c_double(-1.0)
    rc = fn(Wd.data_ptr(), bhd.data_ptr(), bvd.data_ptr(), Xd.data_ptr(), Kd.data_ptr() if Kd is not None else None, N, M, row, col, 0.1, skip,
            C.byref(cs), st)
    assert rc == 0, lib.dae_last_error()
    torch.cuda.synchronize()
    W, bh, bv = Wd.cpu().numpy(), bhd.cpu().numpy(), bvd.cpu().numpy()
    assert W[-1] == 7.0 and bh[-1] == 7.0 and bv[-1] == 7.0, "a guard element was overwritten"
    return W[:-1].reshape(row, col), bh[:-1], bv[:-1], cs.value


def _case(row, col, N, f64):
    return pr.dae_dense_case(row, col, N, np.float64 if f64 else np.float32)


@pytest.mark.parametrize("row,col,M,N,masked,f64,skip", br.DAE_BATCH_CASES,
                         ids=["%dx%d-M%d-N%d-%s-%s-skip%d" % (r, c, M, N, 'masked' if k else 'plain', 'f64' if f else 'f32', s)
                              for r, c, M, N, k, f, s in br.DAE_BATCH_CASES])
def test_parity(built, row, col, M, N, masked, f64, skip):
    c = _case(row, col, N, f64)
    keep = br.keep_mask(N, row, row + col) if masked else None
    W, bh, bv, cost = br.run_dense_da_batch(c['W'], c['bh'], c['bv'], c['X'], keep, M, 0.1, skip)
    gW, gbh, gbv, gcost = _call(c, keep, M, f64, skip)
    r = (_ratio(gW, W, c['W']), _ratio(gbh, bh, c['bh']), _ratio(gbv, bv, c['bv']), abs(gcost - cost) / abs(cost))
    print("da batch %s %dx%d M=%d N=%d %s skip=%d: error/change W %.2e bhid %.2e bvis %.2e, cost %.2e"
          % (('f64' if f64 else 'f32', row, col, M, N, 'masked' if masked else 'plain', skip) + r))
    tol, tol_c = (1e-10, 1e-11) if f64 else (pr.TOL, pr.TOL_ERR)
    assert r[0] <= tol and r[1] <= tol and r[2] <= tol and r[3] <= tol_c


@pytest.mark.parametrize("f64", [True, False], ids=['f64', 'f32'])
@pytest.mark.parametrize("row,col", [(300, 100), (129, 65), (512, 512)])
def test_batch_of_one_against_the_online_trainer(built, row, col, f64):
    """M = 1, keep = NULL computes what dae_dense_epoch[_f64] computes on the same inputs, within the parity bounds."""
    torch, dev, st = _dev()
    lib = _capi.load()
    N = 40
    c = _case(row, col, N, f64)
    dt = torch.float64 if f64 else torch.float32
    Wd, bhd, bvd, Xd = (torch.as_tensor(np.ascontiguousarray(c[k])).to(device=dev, dtype=dt).contiguous() for k in ('W', 'bh', 'bv', 'X'))
    cs = C.c_double(-1.0)
    fn = lib.dae_dense_epoch_f64 if f64 else lib.dae_dense_epoch
    assert fn(Wd.data_ptr(), bhd.data_ptr(), bvd.data_ptr(), Xd.data_ptr(), N, row, col, 0.1, 1, C.byref(cs), st) == 0, lib.dae_last_error()
    torch.cuda.synchronize()
    W, bh, bv, cost = Wd.cpu().numpy().astype(np.float64), bhd.cpu().numpy().astype(np.float64), bvd.cpu().numpy().astype(np.float64), cs.value
    gW, gbh, gbv, gcost = _call(c, None, 1, f64, 1)
    r = (_ratio(gW, W, c['W']), _ratio(gbh, bh, c['bh']), _ratio(gbv, bv, c['bv']), abs(gcost - cost) / abs(cost))
    print("da batch M=1 vs online %s %dx%d: difference/change W %.2e bhid %.2e bvis %.2e, cost %.2e" % (('f64' if f64 else 'f32', row, col) + r))
    tol, tol_c = (1e-10, 1e-11) if f64 else (pr.TOL, pr.TOL_ERR)
    assert r[0] <= tol and r[1] <= tol and r[2] <= tol and r[3] <= tol_c


@pytest.mark.parametrize("f64", [True, False], ids=['f64', 'f32'])
@pytest.mark.parametrize("row,col,M,N", [(209, 100, 20, 70), (512, 512, 3, 10)])
def test_all_ones_mask_is_no_mask(built, row, col, M, N, f64):
    c = _case(row, col, N, f64)
    a = _call(c, None, M, f64, 0)
    b = _call(c, np.ones((N, row), np.uint8), M, f64, 0)
    k = np.full((N, row), 255, np.uint8)
    k[::2] = 1
    d = _call(c, k, M, f64, 0)                                     # any non-zero byte keeps
    for x, y, z in zip(a, b, d):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("f64", [True, False], ids=['f64', 'f32'])
@pytest.mark.parametrize("row,col,M,N", [(300, 100, 20, 7), (305, 1, 20, 20), (1, 8, 256, 1)])
def test_one_skipped_batch_returns_the_parameters(built, row, col, M, N, f64):
    """N <= M with skip_last_update: W, bhid, bvis come back bit for bit, the cost is the batch's mean."""
    c = _case(row, col, N, f64)
    keep = br.keep_mask(N, row, 5)
    gW, gbh, gbv, gcost = _call(c, keep, M, f64, 1)
    assert np.array_equal(gW.astype(np.float64), c['W']) and np.array_equal(gbh.astype(np.float64), c['bh']) and np.array_equal(gbv.astype(np.float64), c['bv'])
    cost = br.batch_grads(c['W'], c['bh'], c['bv'], c['X'], keep)[0]
    print("da batch %s %dx%d N=%d <= M=%d skipped: cost %.2e" % ('f64' if f64 else 'f32', row, col, N, M, abs(gcost - cost) / cost))
    assert abs(gcost - cost) <= (1e-11 if f64 else pr.TOL_ERR) * cost


@pytest.mark.parametrize("f64", [True, False], ids=['f64', 'f32'])
def test_two_calls_give_the_same_bits(built, f64):
    c = _case(512, 512, 70, f64)
    keep = br.keep_mask(70, 512, 9)
    a, b = _call(c, keep, 20, f64, 0), _call(c, keep, 20, f64, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("f64", [True, False], ids=['f64', 'f32'])
def test_a_prefix_of_a_longer_buffer(built, f64):
    """N smaller than the X / keep buffers handed in (the guards of _call cover the parameters): the result is that of the prefix."""
    c = _case(129, 65, 50, f64)
    keep = br.keep_mask(50, 129, 2)
    a = _call(c, keep, 20, f64, 0, N=41)
    c2 = dict(c, X=c['X'][:41])
    b = _call(c2, keep[:41], 20, f64, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------ Python
def _demo_layers(golden_dir):
    from oracle import dae_oracle as do
    path = os.path.join(golden_dir, 'demo', 'train.fm.txt')
    lines = do.parse(path)
    x_dim = max(max(ids) for ids, _ in lines) + 1
    rng = np.random.RandomState(21)
    H0, H1 = 40, 64
    results = [rng.uniform(-2, 2, (x_dim, H0)) / np.sqrt(16 * H0), rng.uniform(-0.5, 0.5, H0),
               rng.uniform(-2, 2, (H0, H1)) / np.sqrt(H0), rng.uniform(-0.5, 0.5, H1)]
    X = np.stack([do.propagate(results, ids) for ids, _ in lines])
    return path, results, X


@pytest.fixture(scope='module')
def demo_layers(golden_dir):
    return _demo_layers(golden_dir)


@pytest.mark.parametrize("corruption", [0, 0.3])
def test_da_on_the_demo_file(built, demo_layers, corruption):
    """da(row, col, file, results, batch_size=20, corruption_level) on the demo file's lines propagated through two lower layers, against
    a NumPy walk: oracle.dae_oracle.propagate, the initialisation of :119-127, the keep masks of dl_utils.RandomStreams and
    run_dense_da_batch per pass (skip_last on the last); within 1e-8 of the parameter change."""
    from deep_ctr_amd import dl_utils
    from deep_ctr_amd import sampling_based_denosing_autoencoder as da_mod
    path, results, X = demo_layers
    row, col, epochs, M = 64, 30, 2, 20
    N = X.shape[0]
    rs = np.random.RandomState(123)
    seed = int(rs.randint(2 ** 30))
    b = 4 * np.sqrt(6. / (row + col))
    W0 = rs.uniform(low=-b, high=b, size=(row, col))
    W, bh, bv = W0, np.zeros(col), np.zeros(row)
    op = dl_utils.RandomStreams(seed).binomial(size=(N, row), n=1, p=1 - corruption) if corruption > 0 else None
    for ep in range(epochs):
        keep = op.draw().astype(np.uint8) if op is not None else None
        W, bh, bv, _ = br.run_dense_da_batch(W, bh, bv, X, keep, M, 0.1, 1 if ep == epochs - 1 else 0)
    gW, gb = da_mod.da(row, col, path, results, learning_rate=0.1, training_epochs=epochs, batch_size=M, corruption_level=corruption)
    assert gW.shape == (row, col) and gb.shape == (col,) and gW.dtype == np.float64
    r = (_ratio(gW, W, W0), _ratio(gb, bh, np.zeros(col)))
    print("da() demo corruption=%s: error/change W %.2e b %.2e" % ((corruption,) + r))
    assert r[0] <= 1e-8 and r[1] <= 1e-8


def test_get_da_weights_default_batch_is_unchanged(built, golden_dir):
    """get_da_weights(..., da_batch_size=1) makes the calls it makes without the argument: the same arrays bit for bit."""
    from deep_ctr_amd import sampling_based_denosing_autoencoder as da_mod
    from oracle import dae_oracle as do
    path = os.path.join(golden_dir, 'demo', 'train.fm.txt')
    x_dim = max(max(ids) for ids, _ in do.parse(path)) + 1
    arr = [x_dim, 40, 24, 12]
    a = da_mod.get_da_weights(path, arr, ncases=1200, epochs=1)
    b = da_mod.get_da_weights(path, arr, ncases=1200, epochs=1, da_batch_size=1)
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = da_mod.get_da_weights(path, arr, ncases=1200, epochs=1, da_batch_size=20, corruption_level=0.3)       # the mini-batch route runs
    assert [x.shape for x in c] == [x.shape for x in a] and np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])
    assert not np.array_equal(c[2], a[2]) and all(np.isfinite(x).all() for x in c)
