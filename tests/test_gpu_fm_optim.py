"""GPU parity of FM / LR pre-training under the reference's Adam and FTRL (fm_set_optimizer, include/fm_hip.h) against
the float64 restatement in fm_optim_ref.py, device evaluation (fm_eval) against NumPy, and the LR class.
f32 vs float64: tolerances relative to the size of the parameter change, as in test_gpu_fm.py."""
import pickle

import numpy as np
import pytest

import fm_optim_ref as ref

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

pytestmark = pytest.mark.gpu
F = 16
INIT = ['uniform', -0.001, 0.001, [1, 2], None]
LRS = {'adam': 1e-2, 'ftrl': 0.05}


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def batches(sizes, B, n, seed, gap=0):
    """n Zipf batches with absent fields and the last row; gap > 0: rows [D / 2, D / 2 + gap) of a table of D + gap rows
    are in no batch."""
    out = []
    rng = np.random.RandomState(seed)
    D = sum(sizes)
    for i in range(n):
        ids = synth.zipf_ids(B, sizes, 1.1, seed + 17 * i + 1)
        ids = np.where(ids >= D // 2, ids + gap, ids).astype(np.int32)
        if B > 8:
            ids[3, 5] = -1
            ids[4, :7] = -1
        ids[B - 1, F - 1] = D + gap - 1
        out.append((ids, (rng.uniform(size=B) < 0.3).astype(np.float64)))
    return out


def make(opt, rank, B, reduce_mean, lam, rows, b):
    argv = [opt, LRS[opt]] + ([1e-8] if opt == 'adam' else []) + ([] if reduce_mean else ['sum'])
    if rank == 0:
        m = LR(B, [rows.shape[0], F], INIT, argv, [lam], 'train', 0)
    else:
        m = FM(B, [rows.shape[0], F, rank], INIT, argv, [lam], 'train', 0)
    m.set_params(rows, b)
    return m, ref.Trainer(rows, b, opt, LRS[opt], lam, reduce_mean)


def check_state(m, tr):
    """Rows, bias and both state tensors of the device against the restatement."""
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


CASES = [(opt, rank, B) for opt in ('adam', 'ftrl') for rank in (0, 1, 10, 15) for B in (1, 64, 700, 4096)]


@pytest.mark.parametrize("opt,rank,B", CASES)
def test_fm_optim_steps_vs_oracle(built, opt, rank, B):
    i = CASES.index((opt, rank, B))
    reduce_mean, lam = i % 2, (0.0, 1e-3, 0.05)[(i // 2) % 3]
    rng = np.random.RandomState(i)
    sizes = synth.field_sizes_tiny(500)
    rows = f32r(rng.standard_normal((sum(sizes) + 24, rank + 1)) * 0.2)
    m, tr = make(opt, rank, B, reduce_mean, lam, rows, 0.1)
    tr.rows0 = rows.copy()
    seen = np.zeros(len(rows), bool)
    for step, (ids, y) in enumerate(batches(sizes, B, 4, 100 + i, gap=24)):
        out = m.train_step(ids, y, want_p=True)
        data, p = tr.step(ids, y)
        tol = 5e-5 if step == 0 else 2e-3
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=tol, atol=1e-6)
        assert abs(out['loss'] - data) <= tol * max(1.0, abs(data))
        seen[ids[ids >= 0]] = True
        if step == 0 and lam == 0.0:
            got, _ = m.get_params()
            if opt == 'ftrl':
                assert not got[~seen].any()                        # re-derived from linear = 0
            else:
                assert np.array_equal(got[~seen], rows[~seen].astype(np.float32))   # zero gradient, zero moments
    check_state(m, tr)
    if lam == 0.0:
        got, _ = m.get_params()
        assert (~seen).any()
        if opt == 'ftrl':
            assert not got[~seen].any()
        else:
            assert np.array_equal(got[~seen], rows[~seen].astype(np.float32))
    m.close()


def test_sgd_then_adam_folds_the_scale(built):
    """SGD steps leave a lazy decay scale pending (lr * lambda = 0.1); switching to Adam folds it into the rows first."""
    sizes = synth.field_sizes_tiny(400)
    rows = f32r(np.random.RandomState(5).standard_normal((sum(sizes), 11)) * 0.2)
    m = FM(256, [len(rows), F, 10], INIT, ['sgd', 0.1], [1.0], 'train', 0)
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


def test_set_table_resets_the_state(built):
    sizes = synth.field_sizes_tiny(300)
    rows = f32r(np.random.RandomState(6).standard_normal((sum(sizes), 5)) * 0.2)
    m, tr = make('ftrl', 4, 128, 1, 1e-3, rows, 0.0)
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


def test_full_shape_adam_step(built):
    """iPinYou shape: 937,670 rows x rank 10, batch 4096, lambda 1e-3 (python/baseline.py's FM recipe, reduce_sum)."""
    sizes = synth.field_sizes_ipinyou()
    rng = np.random.RandomState(8)
    rows = f32r(rng.uniform(-0.01, 0.01, (sum(sizes), 11)))
    m = FM(4096, [len(rows), F, 10], INIT, ['adam', 1e-4, 1e-8, 'sum'], [1e-3], 'train', 0)
    m.set_params(rows, 0.0)
    tr = ref.Trainer(rows, 0.0, 'adam', 1e-4, 1e-3, 0)
    tr.rows0 = rows.copy()
    for ids, y in batches(sizes, 4096, 2, 21):
        out = m.train_step(ids, y)
        data, _ = tr.step(ids, y)
        assert abs(out['loss'] - data) <= 2e-4 * abs(data)
    check_state(m, tr)
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


@pytest.mark.parametrize("rank", [0, 10])
def test_fm_eval_vs_numpy(built, rank):
    sizes = synth.field_sizes_tiny(800)
    rows = f32r(np.random.RandomState(9).standard_normal((sum(sizes), rank + 1)) * 0.3)
    m = (LR(1000, [len(rows), F], INIT, ['ftrl', 1e-3], [0.0], 'train', 0) if rank == 0 else
         FM(1000, [len(rows), F, rank], INIT, ['adam', 1e-3, 1e-8], [0.0], 'train', 0))
    m.set_params(rows, -0.2)
    (ids, _), = batches(sizes, 5000, 1, 31)                        # N > max_batch (1000): five chunks
    y = (np.random.RandomState(10).uniform(size=5000) < 0.3).astype(np.int32)
    p = m.forward(ids).cpu().numpy().astype(np.float64)
    auc, rmse, ll = m.evaluate(ids, y)
    ea, er, el = np_metrics(p, y)
    assert abs(auc - ea) <= 1e-12 and abs(rmse - er) <= 1e-9 * er and abs(ll - el) <= 1e-9 * el
    m.close()


def test_lr_matches_rank0_oracle_dump_and_pickle_init(built, tmp_path):
    """python/baseline.py's LR recipe (FTRL 1e-3, lambda 1e-4): LR = the rank-0 FM; dump keys {'W', 'b'} of the reference's
    shapes ([X_dim, 1], [1]); a dumped model seeds a new LR exactly."""
    sizes = synth.field_sizes_tiny(600)
    D = sum(sizes)
    m = LR(512, [D, F], ['uniform', -0.05, 0.05, [3, 4], None], ['ftrl', 1e-3], [1e-4], 'train', 0)
    W0, b0 = m.get_params()
    assert W0.shape == (D, 1) and b0 == 0.0
    np.testing.assert_array_equal(W0, np.random.RandomState(3).uniform(-0.05, 0.05, (D, 1)).astype(np.float32))
    tr = ref.Trainer(f32r(W0), 0.0, 'ftrl', 1e-3, 1e-4, 1)
    for ids, y in batches(sizes, 512, 3, 41):
        out = m.train_step(ids, y, want_p=True)
        data, p = tr.step(ids, y)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=2e-3, atol=1e-6)
    check_state(m, tr)
    path = str(tmp_path / 'lr.p')
    m.dump(path)
    vm = pickle.load(open(path, 'rb'))
    assert set(vm) == {'W', 'b'} and vm['W'].shape == (D, 1) and vm['b'].shape == (1,)
    m2 = LR(512, [D, F], ['uniform', -0.05, 0.05, [3, 4], path], ['ftrl', 1e-3], [1e-4], 'test', 0)
    W2, b2 = m2.get_params()
    W1, b1 = m.get_params()
    assert np.array_equal(W2, W1) and b2 == b1
    ids, _ = batches(sizes, 300, 1, 51)[0]
    np.testing.assert_array_equal(m2.forward(ids).cpu().numpy(), m.forward(ids).cpu().numpy())
    m.close()
    m2.close()
