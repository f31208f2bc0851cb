"""GPU parity of FM pre-training at the wide ranks (16..127, k = rank + 1 >= 17: the reference's FM50 / FM100, python/baseline.py:77-93)
against oracle/fm_oracle.py (SGD) and the float64 restatement in fm_optim_ref.py (Adam, FTRL), through include/fm_hip.h and FM.py.

Rows are drawn with a standard deviation of 0.2 * sqrt(10 / rank): the logit's pair term 1/2 (sum_l S_l^2 - sum_f |v_f|^2) is a
sum of F (F - 1) / 2 * rank products, so this keeps its spread, and the magnitudes sum_l S_l^2 and sum_f |v_f|^2 whose f32
rounding the bounds of test_gpu_fm.py / test_gpu_fm_optim.py were set for, at those of the rank-10 tests (F * rank * std^2 =
16 * 0.4 at every rank).  The bounds are therefore theirs, unchanged; the full-shape test keeps baseline.py's own init range."""
import ctypes as C
import pickle

import numpy as np
import pytest

import fm_optim_ref as ref
from oracle import fm_oracle as fo

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import FM

pytestmark = pytest.mark.gpu
F = 16
INIT = ['uniform', -0.001, 0.001, [1, 2], None]
LRS = {'adam': 1e-2, 'ftrl': 0.05}


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def table(n, rank, seed):
    return f32r(np.random.RandomState(seed).standard_normal((n, rank + 1)) * 0.2 * np.sqrt(10.0 / rank))


def batches(sizes, B, n, seed, gap=0):
    """n Zipf batches (duplicate rows inside a field) with absent fields and the last row; gap > 0: rows [D / 2, D / 2 + gap) of
    a table of D + gap rows are in no batch."""
    out = []
    rng = np.random.RandomState(seed)
    D = sum(sizes)
    nf = len(sizes)
    for i in range(n):
        ids = synth.zipf_ids(B, sizes, 1.1, seed + 17 * i + 1)
        ids = np.where(ids >= D // 2, ids + gap, ids).astype(np.int32)
        if B > 8 and nf == F:
            ids[3, 5] = -1
            ids[4, :7] = -1
        ids[B - 1, nf - 1] = D + gap - 1
        out.append((ids, (rng.uniform(size=B) < 0.3).astype(np.float64)))
    return out


def check_state(m, tr):
    """Rows, bias and both state tensors against the restatement (test_gpu_fm_optim.py's bounds)."""
    got, gb = m.get_params()
    s0, s1, sb, t = m.get_opt_state()
    assert t == tr.t
    if tr.opt == 'adam':
        tol = 5e-3 * np.abs(tr.rows - tr.rows0).max() + 1e-7
        err = np.abs(got - tr.rows)
        assert err[~tr.ill].max() <= tol
        assert (err[tr.ill] <= 2 * tr.lr_sum + tol).all()       # a gradient within f32 noise of 0: any sign is right
        assert abs(gb - tr.b) <= (2 * tr.lr_sum if tr.ill_b else 5e-3 * tr.lr_sum) + 1e-7
    else:
        assert np.abs(got - tr.rows).max() <= 5e-3 * np.abs(tr.rows).max() + 1e-7
        assert abs(gb - tr.b) <= 5e-3 * abs(tr.b) + 1e-7
    for dev, host, dev_b, host_b in ((s0, tr.s0, sb[0], tr.sb0), (s1, tr.s1, sb[1], tr.sb1)):
        assert np.abs(dev - host).max() <= 2e-3 * np.abs(host).max() + 1e-12
        assert abs(float(dev_b) - float(host_b)) <= 2e-3 * abs(float(host_b)) + 1e-9


SGD_CASES = [(rank, B) for rank in (16, 31, 50, 100, 127) for B in (1, 64, 700, 4096)]


@pytest.mark.parametrize("rank,B", SGD_CASES)
def test_wide_sgd_steps_vs_oracle(built, rank, B):
    i = SGD_CASES.index((rank, B))
    reduce_mean, lam = i % 2, (1e-2, 0.0, 0.05, 1e-3)[(i // 2) % 4]
    sizes = synth.field_sizes_tiny(500)
    rows = table(sum(sizes) + 24, rank, i)
    m = FM(B, [len(rows), F, rank], INIT, ['sgd', 0.05] + ([] if reduce_mean else ['sum']), [lam], 'train', 0)
    m.set_params(rows, 0.1)
    bs = batches(sizes, B, 3, 200 + i, gap=24)
    np.testing.assert_allclose(m.forward(bs[0][0]).cpu().numpy(), fo.predict(rows, 0.1, bs[0][0]), rtol=2e-5, atol=1e-6)
    r, b = rows.copy(), 0.1
    for ids, y in bs:                                              # three steps: the lazy decay scale is live
        out = m.train_step(ids, y, want_p=True)
        b, data, p = fo.sgd_step(r, b, ids, y, 0.05, lam, reduce_mean == 1)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
    got, gb = m.get_params()
    change = np.abs(r - rows).max() + 1e-12
    assert np.abs(got - r).max() <= 2e-3 * change + 2e-7
    assert abs(gb - b) <= 2e-3 * abs(b - 0.1) + 2e-7
    if lam == 0.0:                                                 # rows no batch touched: bit-unchanged
        seen = np.zeros(len(rows), bool)
        for ids, _ in bs:
            seen[ids[ids >= 0]] = True
        assert (~seen).any() and np.array_equal(got[~seen], rows[~seen].astype(np.float32))
    m.close()


def test_wide_long_sgd_run_folds_the_decay_scale(built):
    """Rank 50, lr * lambda = 0.5 halves the scale every step: after 30 steps it has been folded back into the rows at least
    once (2^-24 < 2^-30); every row must follow the oracle's dense decay."""
    sizes = synth.field_sizes_tiny(500)
    rows = table(sum(sizes), 50, 9)
    ids, y = batches(sizes, 32, 1, 9)[0]
    m = FM(32, [len(rows), F, 50], INIT, ['sgd', 0.5], [1.0], 'train', 0)
    m.set_params(rows, 0.0)
    r, b = rows.copy(), 0.0
    for _ in range(30):
        m.train_step(ids, y, want_loss=False)
        b, _, _ = fo.sgd_step(r, b, ids, y, 0.5, 1.0, True)
    got, _ = m.get_params()
    np.testing.assert_allclose(got, r, rtol=2e-3, atol=1e-9)
    m.close()


OPT_CASES = [(opt, rank, B) for opt in ('adam', 'ftrl') for rank in (16, 50, 100) for B in (1, 100, 4096)]


@pytest.mark.parametrize("opt,rank,B", OPT_CASES)
def test_wide_optim_steps_vs_oracle(built, opt, rank, B):
    i = OPT_CASES.index((opt, rank, B))
    reduce_mean, lam = i % 2, (0.0, 1e-3, 0.05)[(i // 2) % 3]
    sizes = synth.field_sizes_tiny(500)
    rows = table(sum(sizes) + 24, rank, 50 + i)
    argv = [opt, LRS[opt]] + ([1e-8] if opt == 'adam' else []) + ([] if reduce_mean else ['sum'])
    m = FM(B, [len(rows), F, rank], INIT, argv, [lam], 'train', 0)
    m.set_params(rows, 0.1)
    tr = ref.Trainer(rows, 0.1, opt, LRS[opt], lam, reduce_mean)
    tr.rows0 = rows.copy()
    seen = np.zeros(len(rows), bool)
    for step, (ids, y) in enumerate(batches(sizes, B, 4, 300 + i, gap=24)):
        out = m.train_step(ids, y, want_p=True)
        data, p = tr.step(ids, y)
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
            assert np.array_equal(got[~seen], rows[~seen].astype(np.float32))   # zero gradient, zero moments
    m.close()


def test_wide_sgd_then_adam_folds_the_scale(built):
    """Rank 50: SGD steps leave a lazy decay scale pending (lr * lambda = 0.1); switching to Adam folds it into the rows first."""
    sizes = synth.field_sizes_tiny(400)
    rows = table(sum(sizes), 50, 5)
    m = FM(256, [len(rows), F, 50], INIT, ['sgd', 0.1], [1.0], 'train', 0)
    m.set_params(rows, 0.05)
    tr = ref.Trainer(rows, 0.05, 'sgd', 0.1, 1.0, 1)
    bs = batches(sizes, 256, 6, 7)
    for ids, y in bs[:3]:
        m.train_step(ids, y, want_loss=False)
        tr.sgd_step(ids, y)
    assert m.lib.fm_set_optimizer(m.h, 1, 0.9, 0.999, 1e-8) == 0  # FM_OPT_ADAM
    m.lr, m.lam = 1e-2, 1e-3
    tr.opt, tr.lr, tr.lam, tr.eps = 'adam', 1e-2, 1e-3, 1e-8
    tr.reset_state()
    tr.rows0 = tr.rows.copy()
    for ids, y in bs[3:]:
        m.train_step(ids, y, want_loss=False)
        tr.step(ids, y)
    check_state(m, tr)
    m.close()


def test_wide_set_table_resets_the_state(built):
    sizes = synth.field_sizes_tiny(300)
    rows = table(sum(sizes), 50, 6)
    m = FM(128, [len(rows), F, 50], INIT, ['ftrl', LRS['ftrl']], [1e-3], 'train', 0)
    m.set_params(rows, 0.0)
    tr = ref.Trainer(rows, 0.0, 'ftrl', LRS['ftrl'], 1e-3, 1)
    bs = batches(sizes, 128, 3, 11)
    for ids, y in bs[:2]:
        m.train_step(ids, y, want_loss=False)
    m.set_params(rows, 0.0)
    s0, s1, sb, t = m.get_opt_state()
    assert t == 0 and (s0 == np.float32(0.1)).all() and not s1.any() and sb[0] == np.float32(0.1) and sb[1] == 0
    m.train_step(*bs[2], want_loss=False)
    tr.step(*bs[2])
    check_state(m, tr)
    m.close()


def test_wide_full_shape_adam_step(built):
    """iPinYou shape at the reference's FM100: 937,670 rows x rank 100, batch 4096, python/baseline.py's recipe
    ['adam', 1e-4, 1e-8, 'sum'], lambda 1e-3, as test_full_shape_adam_step runs it at rank 10."""
    sizes = synth.field_sizes_ipinyou()
    rng = np.random.RandomState(8)
    rows = f32r(rng.uniform(-0.01, 0.01, (sum(sizes), 101)))
    m = FM(4096, [len(rows), F, 100], INIT, ['adam', 1e-4, 1e-8, 'sum'], [1e-3], 'train', 0)
    m.set_params(rows, 0.0)
    tr = ref.Trainer(rows, 0.0, 'adam', 1e-4, 1e-3, 0)
    tr.rows0 = rows.copy()
    for ids, y in batches(sizes, 4096, 2, 21):
        out = m.train_step(ids, y)
        data, _ = tr.step(ids, y)
        assert abs(out['loss'] - data) <= 2e-4 * abs(data)
    check_state(m, tr)
    m.close()


@pytest.mark.parametrize("rank,nf", [(16, 1), (16, 16), (127, 1), (127, 16)])
def test_wide_round_trips_are_bit_exact(built, rank, nf):
    sizes = synth.field_sizes_tiny(700, nf)
    D = sum(sizes)
    rows = np.random.RandomState(rank + nf).standard_normal((D, rank + 1)).astype(np.float32)
    m = FM(64, [D, nf, rank], INIT, ['sgd', 0.01], [0.0], 'train', 0)
    m.set_params(rows, -0.25)
    got, b = m.get_params()
    assert np.array_equal(got, rows) and b == np.float32(-0.25)
    want = np.array([D - 1, 0, 5, D // 2, 5], np.int64)
    out = np.empty((len(want), rank + 1), np.float32)
    assert m.lib.fm_get_rows(m.h, want.ctypes.data, len(want), out.ctypes.data) == 0
    assert np.array_equal(out, rows[want])
    ids, y = batches(sizes, 64, 1, 61)[0]                           # an lr = 0 step changes no bit
    m.lr = 0.0
    m.train_step(ids, y)
    got, _ = m.get_params()
    assert np.array_equal(got, rows)
    m.close()


def np_metrics(p, y):
    order = np.argsort(p, kind='stable')
    ps = p[order]
    _, first, counts = np.unique(ps, return_index=True, return_counts=True)
    avg = np.repeat(first + (counts + 1) / 2.0, counts)              # tie-averaged ranks, 1-based
    ranks = np.empty(len(p))
    ranks[order] = avg
    npos = (y != 0).sum()
    nneg = len(y) - npos
    auc = (ranks[y != 0].sum() - npos * (npos + 1) / 2.0) / (npos * nneg)
    rmse = np.sqrt(np.mean((p - (y != 0)) ** 2))
    eps = 2.0 ** -52
    pc = np.clip(p, eps, 1 - eps)
    ll = -np.mean(np.where(y != 0, np.log(pc), np.log(1 - pc)))
    return auc, rmse, ll


def test_wide_eval_vs_numpy(built):
    sizes = synth.field_sizes_tiny(800)
    rows = table(sum(sizes), 100, 9)
    m = FM(1000, [len(rows), F, 100], INIT, ['adam', 1e-3, 1e-8], [0.0], 'train', 0)
    m.set_params(rows, -0.2)
    (ids, _), = batches(sizes, 5000, 1, 31)                        # N > max_batch (1000): five chunks
    y = (np.random.RandomState(10).uniform(size=5000) < 0.3).astype(np.int32)
    p = m.forward(ids).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(p, fo.predict(rows, -0.2, ids), rtol=2e-5, atol=1e-6)
    auc, rmse, ll = m.evaluate(ids, y)
    ea, er, el = np_metrics(p, y)
    assert abs(auc - ea) <= 1e-12 and abs(rmse - er) <= 1e-9 * er and abs(ll - el) <= 1e-9 * el
    m.close()


@pytest.mark.parametrize("opt", ['sgd', 'adam'])
def test_wide_runs_are_bit_identical(built, opt):
    sizes = synth.field_sizes_tiny(2000)
    rows = table(sum(sizes), 100, 12)
    bs = batches(sizes, 4096, 4, 71)
    outs = []
    for _ in range(2):
        m = FM(4096, [len(rows), F, 100], INIT, [opt, 1e-3] + ([1e-8] if opt == 'adam' else []), [1e-3], 'train', 0)
        m.set_params(rows, 0.0)
        losses = [m.train_step(ids, y)['loss'] for ids, y in bs]
        outs.append((m.get_params(), losses))
        m.close()
    (g0, b0), l0 = outs[0]
    (g1, b1), l1 = outs[1]
    assert np.array_equal(g0, g1) and b0 == b1 and l0 == l1


def test_fm_create_limits(built):
    from deep_ctr_amd import _capi
    lib = _capi.load()
    for k in (0, 129):
        h = C.c_void_p()
        assert lib.fm_create(F, k, 64, 0, None, C.byref(h)) == _capi.FNN_ERR_ARG and not h.value
        assert b'1 <= k <= 128' in lib.fm_last_error(None)
    h = C.c_void_p()
    assert lib.fm_create(F, 128, 64, 0, None, C.byref(h)) == 0
    assert lib.fm_destroy(h) == 0


def test_wide_fm_facade_pickle_dump_and_model_file(built, tmp_path):
    """FM(batch, [X_dim, 16, 50], ...) as python/baseline.py's FM50 builds it: pickle init, dump keys and shapes, and
    write_fm_model parsed back bit-exactly by DataFM."""
    from deep_ctr_amd.data_fm import DataFM
    sizes = synth.field_sizes_tiny(600)
    D = sum(sizes)
    m = FM(256, [D, F, 50], ['uniform', -0.001, 0.001, [3, 4], None], ['adam', 1e-4, 1e-8, 'sum'], [1e-3], 'train', 0)
    W0, _ = m.get_params()
    assert W0.shape == (D, 51)
    np.testing.assert_array_equal(W0[:, 1:], np.random.RandomState(4).uniform(-0.001, 0.001, (D, 50)).astype(np.float32))
    for ids, y in batches(sizes, 256, 3, 81):
        m.train_step(ids, y, want_loss=False)
    s0, s1, sb, t = m.get_opt_state()
    assert s0.shape == (D, 51) and t == 3 and s1.any()
    path = str(tmp_path / 'fm50.pickle')
    m.dump(path)
    vm = pickle.load(open(path, 'rb'))
    assert set(vm) == {'W', 'V', 'b'} and vm['W'].shape == (D, 1) and vm['V'].shape == (D, 50) and vm['b'].shape == (1,)
    m2 = FM(256, [D, F, 50], ['uniform', -0.001, 0.001, [3, 4], path], ['adam', 1e-4, 1e-8, 'sum'], [1e-3], 'test', 0)
    got, b = m.get_params()
    got2, b2 = m2.get_params()
    assert np.array_equal(got2, got) and b2 == b
    ids, _ = batches(sizes, 300, 1, 91)[0]
    np.testing.assert_array_equal(m2.forward(ids).cpu().numpy(), m.forward(ids).cpu().numpy())
    fo_row = synth.field_of_row(sizes)
    names = sorted(DataFM.name_field, key=DataFM.name_field.get)
    mpath = str(tmp_path / 'fm.model.txt')
    m.write_fm_model(mpath, fo_row, names)
    d = DataFM(mpath)
    assert d.k == 51 and d.w_0 == np.float64(np.float32(b))
    assert np.array_equal(d.rows.astype(np.float32), got) and np.array_equal(d.field_of_row, fo_row)
    m.close()
    m2.close()
