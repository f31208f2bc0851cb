"""GPU parity of FM / LR pre-training at 17 to 64 fields (fm_create's n_fields range beyond one lane per field) on both row layouts
(k <= 16: 64-byte rows, a lane owns fields f, f + 16, ..; k >= 17: wide rows, 16 fields at a time) against oracle/fm_oracle.py
(SGD) and the float64 restatement in fm_optim_ref.py (Adam, FTRL), through include/fm_hip.h and FM.py / LR.py, and the hand-off
of such models to the FNN step, the inner-product family and the fm.model.txt reader.

Rows are drawn with a standard deviation of sqrt(6.4 / (F * rank)): the logit's pair term is a sum of F (F - 1) / 2 * rank
products, and F * rank * std^2 = 6.4 keeps its spread and the magnitudes whose f32 rounding the bounds of test_gpu_fm.py,
test_gpu_fm_optim.py and test_gpu_fm_wide.py were set for (16 fields x rank 10 x 0.2^2).  Rank 0 (LR) keeps the linear term's
spread: 0.2 * sqrt(16 / F).  The bounds are theirs, unchanged."""
import ctypes as C
import pickle

import numpy as np
import pytest

import fm_optim_ref as ref
from oracle import fm_oracle as fo
from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

pytestmark = pytest.mark.gpu
INIT = ['uniform', -0.001, 0.001, [1, 2], None]
LRS = {'adam': 1e-2, 'ftrl': 0.05}
FIELDS = (17, 26, 32, 39, 64)
RANKS = (0, 10, 15, 50, 100, 127)


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def table(n, F, rank, seed):
    sd = 0.2 * np.sqrt(16.0 / F) if rank == 0 else np.sqrt(6.4 / (F * rank))
    return f32r(np.random.RandomState(seed).standard_normal((n, rank + 1)) * sd)


def model(F, rank, B, argv, lam, rows, b, mode='train'):
    m = LR(B, [len(rows), F], INIT, argv, [lam], mode, 0) if rank == 0 else FM(B, [len(rows), F, rank], INIT, argv, [lam], mode, 0)
    m.set_params(rows, b)
    return m


def batches(sizes, B, n, seed, gap=0):
    """n Zipf batches (duplicate rows inside a field) with absent fields below and above 16 and the table's last row in field
    F - 1; gap > 0: rows [D / 2, D / 2 + gap) of a table of D + gap rows are in no batch."""
    out = []
    rng = np.random.RandomState(seed)
    D, nf = sum(sizes), len(sizes)
    for i in range(n):
        ids = synth.zipf_ids(B, sizes, 1.1, seed + 17 * i + 1)
        ids = np.where(ids >= D // 2, ids + gap, ids).astype(np.int32)
        if B > 8:
            ids[3, 5] = -1
            ids[4, :7] = -1
            ids[5, 16:] = -1                                      # every field a lane's second row comes from
            ids[6, :nf - 1] = -1                                  # field F - 1 only
            ids[7, 16::3] = -1
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


def sgd_vs_oracle(m, rows, b0, bs, lr, lam, reduce_mean):
    """Forward, then one step per batch against fo.sgd_step (test_gpu_fm_wide.py's bounds); returns the oracle's rows."""
    np.testing.assert_allclose(m.forward(bs[0][0]).cpu().numpy(), fo.predict(rows, b0, bs[0][0]), rtol=2e-5, atol=1e-6)
    r, b = rows.copy(), b0
    for ids, y in bs:
        out = m.train_step(ids, y, want_p=True)
        b, data, p = fo.sgd_step(r, b, ids, y, lr, lam, reduce_mean == 1)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
    got, gb = m.get_params()
    change = np.abs(r - rows).max() + 1e-12
    assert np.abs(got - r).max() <= 2e-3 * change + 2e-7
    assert abs(gb - b) <= 2e-3 * abs(b - b0) + 2e-7
    return r, got


# every field count with every rank, each field count at every batch size (1, 700 = 43.75 workgroups of 16 / 87.5 of 8, 4096)
SGD_CASES = [(F, rank, (1, 700, 4096)[(i + j) % 3]) for i, F in enumerate(FIELDS) for j, rank in enumerate(RANKS)]


@pytest.mark.parametrize("F,rank,B", SGD_CASES, ids=['F%d-r%d-B%d' % c for c in SGD_CASES])
def test_fields_sgd_steps_vs_oracle(built, F, rank, B):
    i = SGD_CASES.index((F, rank, B))
    reduce_mean, lam = i % 2, (1e-2, 0.0, 0.05, 1e-3)[(i // 2) % 4]
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes) + 24, F, rank, i)
    m = model(F, rank, B, ['sgd', 0.05] + ([] if reduce_mean else ['sum']), lam, rows, 0.1)
    bs = batches(sizes, B, 3, 200 + i, gap=24)
    _, got = sgd_vs_oracle(m, rows, 0.1, bs, 0.05, lam, reduce_mean)
    if lam == 0.0:                                                 # rows no batch touched: bit-unchanged
        seen = np.zeros(len(rows), bool)
        for ids, _ in bs:
            seen[ids[ids >= 0]] = True
        assert (~seen).any() and np.array_equal(got[~seen], rows[~seen].astype(np.float32))
    m.close()


OPT_CASES = [(opt, F, rank) for opt in ('adam', 'ftrl') for F in (26, 39, 64) for rank in (0, 10, 100)]


@pytest.mark.parametrize("opt,F,rank", OPT_CASES, ids=['%s-F%d-r%d' % c for c in OPT_CASES])
def test_fields_optim_steps_vs_oracle(built, opt, F, rank):
    i = OPT_CASES.index((opt, F, rank))
    B = (100, 4096, 1)[i % 3]
    reduce_mean, lam = i % 2, (0.0, 1e-3, 0.05)[(i // 2) % 3]
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes) + 24, F, rank, 50 + i)
    argv = [opt, LRS[opt]] + ([1e-8] if opt == 'adam' else []) + ([] if reduce_mean else ['sum'])
    m = model(F, rank, B, argv, lam, rows, 0.1)
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


def edge_ids(sizes, B, which, seed):
    ids = synth.zipf_ids(B, sizes, 1.1, seed).astype(np.int32)
    F = len(sizes)
    if which == 'high_only':                                       # only fields >= 16: no lane's first row
        ids[:, :16] = -1
    elif which == 'last_only':                                     # field F - 1 alone
        ids[:, :F - 1] = -1
    else:                                                          # 'low_only': fields 16.. absent
        ids[:, 16:] = -1
    return ids


EDGE_CASES = [(F, rank, which) for F in (39, 64) for rank in (10, 50, 100) for which in ('high_only', 'last_only', 'low_only')]


@pytest.mark.parametrize("F,rank,which", EDGE_CASES, ids=['F%d-r%d-%s' % c for c in EDGE_CASES])
def test_fields_lane_ownership_edges(built, F, rank, which):
    """Batches whose present fields sit only at or above 16, only in field F - 1, or only below 16; B = 700 is no multiple of
    the examples per workgroup (16, or 8 at rank > 63)."""
    i = EDGE_CASES.index((F, rank, which))
    B = 700
    sizes = synth.field_sizes_tiny(600, F)
    rows = table(sum(sizes), F, rank, 70 + i)
    m = model(F, rank, B, ['sgd', 0.05], 1e-3, rows, -0.1)
    rng = np.random.RandomState(i)
    bs = [(edge_ids(sizes, B, which, 90 + i + s), (rng.uniform(size=B) < 0.3).astype(np.float64)) for s in range(2)]
    sgd_vs_oracle(m, rows, -0.1, bs, 0.05, 1e-3, 1)
    m.close()


@pytest.mark.parametrize("F,rank", [(39, 10), (64, 10), (39, 50), (64, 100)])
def test_fields_range_error_in_the_last_field(built, F, rank):
    """An id outside [-1, n_rows) in field F - 1 (a lane's fourth, third or second row, or a later 16-field chunk of the wide
    path) is reported as FNN_ERR_RANGE, by the step and by a prediction."""
    sizes = synth.field_sizes_tiny(400, F)
    rows = table(sum(sizes), F, rank, 3)
    m = model(F, rank, 64, ['sgd', 0.01], 0.0, rows, 0.0)
    ids, y = batches(sizes, 64, 1, 5)[0]
    ids[10, F - 1] = len(rows)
    with pytest.raises(FNNError) as e:
        m.train_step(ids, y)
    assert e.value.code == _capi.FNN_ERR_RANGE
    ids[10, F - 1] = -2
    with pytest.raises(FNNError) as e:
        m.forward(ids)
    assert e.value.code == _capi.FNN_ERR_RANGE
    m.close()


@pytest.mark.parametrize("rank", [10, 50])
def test_fields_long_sgd_run_folds_the_decay_scale(built, rank):
    """39 fields, lr * lambda = 0.5 halves the scale every step: after 30 steps it has been folded back into the rows at least
    once (2^-24 < 2^-30); every row must follow the oracle's dense decay.  lr = 0.05, lambda = 10 (the 16-field tests' lr = 0.5,
    lambda = 1 lets the pair term's gradient, a sum over 38 other fields, run away to 1e16 and test f32 rounding of that)."""
    F = 39
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes), F, rank, 9)
    ids, y = batches(sizes, 32, 1, 9)[0]
    m = model(F, rank, 32, ['sgd', 0.05], 10.0, rows, 0.0)
    r, b = rows.copy(), 0.0
    for _ in range(30):
        m.train_step(ids, y, want_loss=False)
        b, _, _ = fo.sgd_step(r, b, ids, y, 0.05, 10.0, True)
    got, _ = m.get_params()
    np.testing.assert_allclose(got, r, rtol=2e-3, atol=1e-9)
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


@pytest.mark.parametrize("rank", [0, 10, 100])
def test_fields_eval_vs_numpy(built, rank):
    F = 26
    sizes = synth.field_sizes_tiny(800, F)
    rows = table(sum(sizes), F, rank, 9)
    m = model(F, rank, 1000, ['adam', 1e-3, 1e-8], 0.0, rows, -0.2)
    (ids, _), = batches(sizes, 5000, 1, 31)                        # N > max_batch (1000): five chunks
    y = (np.random.RandomState(10).uniform(size=5000) < 0.3).astype(np.int32)
    p = m.forward(ids).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(p, fo.predict(rows, -0.2, ids), rtol=2e-5, atol=1e-6)
    auc, rmse, ll = m.evaluate(ids, y)
    ea, er, el = np_metrics(p, y)
    assert abs(auc - ea) <= 1e-12 and abs(rmse - er) <= 1e-9 * er and abs(ll - el) <= 1e-9 * el
    m.close()


@pytest.mark.parametrize("rank", [0, 10, 100, 127])
def test_fields_round_trips_are_bit_exact(built, rank):
    F = 64
    sizes = synth.field_sizes_tiny(900, F)
    D = sum(sizes)
    rows = np.random.RandomState(rank + F).standard_normal((D, rank + 1)).astype(np.float32)
    m = model(F, rank, 64, ['sgd', 0.01], 0.0, rows, -0.25)
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


@pytest.mark.parametrize("F,rank,opt", [(39, 10, 'adam'), (39, 100, 'adam'), (64, 10, 'sgd'), (64, 50, 'adam'), (64, 100, 'ftrl')])
def test_fields_runs_are_bit_identical(built, F, rank, opt):
    """Two handles fed the same batches end with the same table, bias, loss values and optimiser state, bit for bit."""
    sizes = synth.field_sizes_tiny(2000, F)
    rows = table(sum(sizes), F, rank, 12)
    bs = batches(sizes, 4096, 3, 71)
    outs = []
    for _ in range(2):
        m = model(F, rank, 4096, [opt, 1e-3] + ([1e-8] if opt == 'adam' else []), 1e-3, rows, 0.0)
        losses = [m.train_step(ids, y)['loss'] for ids, y in bs]
        outs.append((m.get_params(), losses, m.get_opt_state() if opt != 'sgd' else None))
        m.close()
    (g0, b0), l0, s0 = outs[0]
    (g1, b1), l1, s1 = outs[1]
    assert np.array_equal(g0, g1) and b0 == b1 and l0 == l1
    if s0 is not None:
        assert all(np.array_equal(a, c) for a, c in zip(s0[:3], s1[:3])) and s0[3] == s1[3]


def test_fields_fm_pickle_seeds_fnn_ip_l3(built, tmp_path):
    """FM([D, 26, 10]) trains a few steps and dumps {'W', 'V', 'b'}; FNN_IP_L3 with X_feas 26, rank 10 loads that pickle through
    _init_argv with the FM rows bit for bit, and trains a step."""
    from deep_ctr_amd.ipnn import FNN_IP_L3
    F, rank, B = 26, 10, 256
    sizes = synth.field_sizes_tiny(1500, F)
    D = sum(sizes)
    ids = synth.zipf_ids(B * 4, sizes, 1.1, 5)
    y = (np.random.RandomState(6).uniform(size=B * 4) < 0.3).astype(np.float64)
    fm = FM(B, [D, F, rank], ['uniform', -0.01, 0.01, [1, 2], None], ['sgd', 0.05], [1e-3], 'train', 0)
    try:
        for j in range(3):
            fm.train_step(ids[j * B:(j + 1) * B], y[j * B:(j + 1) * B], want_loss=False)
        rows, b = fm.get_params()
        path = str(tmp_path / 'fm26.pkl')
        fm.dump(path)
    finally:
        fm.close()
    m = FNN_IP_L3([], [], B, [D, F, rank, 300, 100, 50, 'relu'], ['uniform', -0.05, 0.05, [3, 4, 5], path], ['sgd', 0.001, 'sum'],
                  [1.0], 'train', 0, precision='f32')
    assert np.array_equal(m.eng.get_rows(np.arange(D)), rows)
    assert m.eng.get_params()[0] == np.float32(b)
    out = m.train_step(ids[3 * B:], y[3 * B:])
    assert np.isfinite(out['loss'])


def test_fields_fm_rows_feed_the_wide_fnn_gather(built):
    """FM rows at 39 fields, rank 50 -> FNNEngine(n_fields=39, k=51) (wide rows, 39 x 52 = 2028 layer-one columns): fnn_gather
    gives x[0] = w_0, x[1 + f K + l] = row[l] bit for bit."""
    from deep_ctr_amd.engine import FNNEngine
    F, rank, B = 39, 50, 500
    K = rank + 1
    sizes = synth.field_sizes_tiny(1200, F)
    D = sum(sizes)
    fm = model(F, rank, 256, ['adam', 1e-3, 1e-8], 1e-3, table(D, F, rank, 4), 0.05)
    for ids, y in batches(sizes, 256, 3, 41):
        fm.train_step(ids, y, want_loss=False)
    rows, b = fm.get_params()
    fm.close()
    ids, _ = batches(sizes, B, 1, 43)[0]
    eng = FNNEngine(F, K, 64, 8, max_batch=B, precision='f32')
    try:
        eng.set_table(rows, synth.field_of_row(sizes), b)
        eng.set_dense(orc.init_fnn_weights(1 + F * K, 64, 8))
        want = orc.gather(rows.astype(np.float64), ids, b).astype(np.float32)
        assert np.array_equal(eng.gather(ids).cpu().numpy(), want)
        assert want[0, 0] == np.float32(b) and np.array_equal(want[B - 1, 1 + (F - 1) * K:], rows[D - 1])
    finally:
        eng.close()


def test_fields_fm_model_file_round_trip(built, tmp_path):
    """write_fm_model with 39 field names -> ingest.FMModel.load returns the same rows and field_of_row."""
    from deep_ctr_amd import ingest
    F, rank = 39, 10
    sizes = synth.field_sizes_tiny(700, F)
    D = sum(sizes)
    fo_row = synth.field_of_row(sizes)
    names = ['f%02d' % f for f in range(F)]
    m = model(F, rank, 128, ['sgd', 1e-2], 1e-3, table(D, F, rank, 8), 0.0)
    for ids, y in batches(sizes, 128, 2, 51):
        m.train_step(ids, y, want_loss=False)
    path = str(tmp_path / 'fm39.model.txt')
    m.write_fm_model(path, fo_row, names)
    got, b = m.get_params()
    m.close()
    fm_file = ingest.FMModel.load(path, names)
    try:
        assert fm_file.k == rank + 1 and fm_file.n_rows == D and fm_file.w0 == np.float64(np.float32(b))
        rows, feat, fo_back = fm_file.arrays()
        assert np.array_equal(rows.astype(np.float32), got) and np.array_equal(fo_back, fo_row)
        assert np.array_equal(feat, np.arange(D))
    finally:
        fm_file.close()


def test_fields_full_shape_adam_step(built):
    """937,670 rows over 39 fields (the iPinYou-like sizes cycled and rescaled) x rank 10, batch 4096, python/baseline.py's recipe
    ['adam', 1e-4, 1e-8, 'sum'], lambda 1e-3, as test_full_shape_adam_step runs it at 16 fields."""
    F = 39
    sizes = synth.field_sizes_ipinyou(n_fields=F)
    assert sum(sizes) == synth.IPINYOU_DIMS
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
