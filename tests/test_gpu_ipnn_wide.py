"""The inner-product step (include/ipnn_hip.h) on wide rows: k = rank + 1 from 17 to 128 (FM50 / FM100 seeds), 2..32 fields, with
and without the pair products, against the float64 oracle (oracle/ipnn_oracle.py).

Wide handles keep rows of rw = rup(k, 4) floats; layer 0 holds the F field columns f rw + l, the pair products, b and the ones
column: Dp0 = rup(F rw + P + 2, 64).  The inner-product layer runs k_ip_fwd_w / k_ip_bwd_w (8 examples per workgroup) and the
sparse-row update the bag table's wide scatter; the deep stack is shared with the narrow path and picks the strip kernels or one
GEMM per product by maxD as there.  Every case id starts with the path the restatement below predicts (as the shapes file does).

Bounds are those of tests/test_gpu_ipnn.py and tests/test_gpu_ipnn_shapes.py (check_f32_step and the bf16 / optimiser bounds
there).  Each oracle case prints its worst error as a fraction of its bound.
"""
import pickle

import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import FNN, FNN_IP_L3, IPNNEngine

from test_gpu_ipnn_shapes import Bounds, check_f32_step, copy_params, cosine, f32r, lr_for, oracle_pairs, problem

pytestmark = pytest.mark.gpu

N_CU = 256          # MI355X


def rup(a, m):
    return (a + m - 1) // m * m


def npairs(F, pairs):
    return F * (F - 1) // 2 if pairs else 0


def padded(F, K, hidden, pairs):
    """h->Dp of ipnn_create for a wide handle: layer 0 holds F fields of rup(k, 4) floats, the pairs, b and the ones column."""
    return [rup(F * rup(K, 4) + npairs(F, pairs) + 2, 64)] + [rup(h + 1, 64) for h in hidden] + [64]


def path_of(F, K, hidden, pairs, prec, B):
    """ip_run's choice: strip_lds = 2 RT 16 maxD sizeof(T) <= 128 KiB (RT = 2 for bf16), StripDuo for bf16 when both workgroups
    of every strip fit the chip."""
    maxD = max(padded(F, K, hidden, pairs))
    RT, ts = (2, 2) if prec == 'bf16' else (1, 4)
    if 2 * RT * 16 * maxD * ts > 128 * 1024:
        return 'gemm'
    return 'strip-duo' if RT == 2 and 2 * (rup(B, 256) // 32) <= N_CU else 'strip'


def case_id(F, K, pairs, hidden, B, prec='f32', *rest):
    s = '%s-F%d-K%d-%s-Dp0_%d-H%s-B%d' % (path_of(F, K, hidden, pairs, prec, B), F, K, 'P' if pairs else 'noP',
                                          padded(F, K, hidden, pairs)[0], 'x'.join(str(h) for h in hidden), B)
    return '-'.join([s] + [str(r) for r in rest if r not in (None, '')])


def engine(F, K, hidden, act='relu', B=256, prec='f32', lr=0.01, keep=0.7, pairs=True, **kw):
    return IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision=prec, lr=lr, keep_prob=keep, pairs=bool(pairs), **kw)


# ------------------------------------------------------------------------------------------------ one f32 step
# (F, K, pairs, hidden, B, act, drop): F = 8, k = 51 (Dp0 = 448) and F = 2 stay on the strips; F = 16, k = 101 (Dp0 = 1792),
# F = 23 and F = 32, k = 128 (Dp0 = 4608, the widest layer 0) take one GEMM per product
STEP = [
    (2, 17, 1, [40, 24], 17, 'relu', True), (2, 128, 1, [64, 63], 4096, 'tanh', True), (8, 51, 1, [130, 70], 257, 'tanh', True),
    (8, 20, 1, [100], 33, 'sigmoid', False), (16, 101, 1, [300, 100], 300, 'sigmoid', True), (16, 51, 1, [200, 100], 1, 'relu', True),
    (23, 101, 1, [64], 257, 'relu', True), (32, 128, 1, [100, 50], 300, 'tanh', True), (32, 17, 1, [120, 60], 257, 'sigmoid', True),
    # pairs = 0: the plain FNN class
    (2, 51, 0, [40, 20], 257, 'tanh', True), (16, 101, 0, [300, 100], 300, 'relu', True), (23, 20, 0, [100], 17, 'sigmoid', False),
    (32, 128, 0, [64, 63], 17, 'sigmoid', True),
]


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop", STEP,
                         ids=[case_id(F, K, p, h, B, 'f32', a, 'drop' if dr else 'nodrop') for (F, K, p, h, B, a, dr) in STEP])
def test_wide_step_f32_vs_oracle(built, F, K, pairs, hidden, B, act, drop):
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B)
    keep, lr = (0.7 if drop else 1.0), lr_for(B)
    eng = engine(F, K, hidden, act, B, 'f32', lr, keep, pairs)
    try:
        assert eng.d == prob[5]
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, act, lr, drop, keep, pairs, case_id(F, K, pairs, hidden, B, 'f32', act))
    finally:
        eng.close()


def test_wide_step_without_side_stream_or_write_through(built, monkeypatch):
    """The same wide step in line on one stream (IPNN_SIDE_STREAM=0) and with plain stores (IPNN_WT=0): both against the oracle."""
    F, K, hidden, B = 16, 51, [130, 70], 300
    for env in ({'IPNN_SIDE_STREAM': '0'}, {'IPNN_WT': '0'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        prob = problem(F, K, B, hidden, True, seed=9)
        eng = engine(F, K, hidden, 'relu', B, 'f32', 0.01, 0.7)
        try:
            eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
            check_f32_step(eng, prob, 'relu', 0.01, True, 0.7, True, case_id(F, K, 1, hidden, B, 'f32', *env.keys()))
        finally:
            eng.close()
        for k in env:
            monkeypatch.delenv(k)


# ------------------------------------------------------------------------------------------------ bf16, three steps
BF16 = [(16, 51, 1, [400, 200]), (16, 101, 1, [400, 200]), (8, 101, 0, [300, 100])]


@pytest.mark.parametrize("F,K,pairs,hidden", BF16, ids=[case_id(F, K, p, h, 1024, 'bf16') for (F, K, p, h) in BF16])
def test_wide_bf16_tracks_oracle(built, F, K, pairs, hidden):
    """test_ipnn_bf16_wide_stack_tracks_oracle's bounds over three steps: logits within 5e-2 and the loss within 2 % at every
    step, every weight update's cosine with the oracle's > 0.99 at the end.  The rows are scaled by sqrt(16 / k) so that a pair
    product (a sum of k terms) keeps the magnitude it has in the narrow tests the absolute logit bound was set on: with problem()'s
    rows as they are, the step-1 logits of F = 16, k = 51 / 101 (|logit| larger by the pair sums) reach 1.22 / 1.36 of the bound
    while every run is bit-reproducible and the f32 path holds its bounds."""
    B, steps = 1024, 3
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, pairs, seed=11 + F + K)
    table = f32r(table * np.sqrt(16.0 / K))
    eng = engine(F, K, hidden, 'relu', B, 'bf16', 0.01, 0.7, pairs)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0 = [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            with oracle_pairs(pairs):
                loss, logits, _ = io.sgd_step(params, table, ids[sl], y[sl], 'relu', 0.01, [m[sl].astype(np.float64) for m in masks], 0.7)
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 0.0, 5e-2)
            bd.close('loss%d' % s, out['loss'], loss, 0.0, 2e-2 * abs(loss))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.above('cos W%d' % t, cosine(Ws[t] - p0[t], params['W'][t] - p0[t]), 0.99, 0.01)
        bd.report(case_id(F, K, pairs, hidden, B, 'bf16', '3steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ Adam and FTRL
OPT = [(16, 51, 'adam'), (16, 101, 'adam'), (16, 51, 'ftrl'), (16, 101, 'ftrl')]


@pytest.mark.parametrize("F,K,opt", OPT, ids=[case_id(F, K, 1, [40, 24, 12], 160, 'f32', o) for (F, K, o) in OPT])
def test_wide_optimiser_steps_vs_oracle(built, F, K, opt):
    """test_ipnn_shape_optimiser_steps_vs_oracle on wide rows: five Adam / FTRL steps on batches of their own, so that rows an
    early step touched keep moving through the dense pass over n_rows x rw; every row follows the oracle, a row no step touched
    is bit-unchanged under Adam and exactly 0 under FTRL."""
    hidden, B, steps = [40, 24, 12], 160, 5
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=21 + F + K)
    lr = 1e-3 if opt == 'adam' else 1e-2
    eng = engine(F, K, hidden, 'relu', B, 'f32', lr, 0.7, optimizer=opt, adam_eps=1e-8)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        st = io.adam_state(params, table) if opt == 'adam' else io.ftrl_state(params, table)
        t0, W0 = table.copy(), [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            m64 = [m[sl].astype(np.float64) for m in masks]
            if opt == 'adam':
                loss, logits, _ = io.adam_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 5e-4, 5e-5)
            else:
                loss, logits, _ = io.ftrl_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 2e-3, 2e-5)
                bd.close('loss%d' % s, out['loss'], loss, 0.0, 1e-4 * abs(loss))
        b, Ws, bs = eng.get_params()
        rows = eng.get_rows(np.arange(table.shape[0]))
        never = np.setdiff1d(np.arange(table.shape[0]), np.unique(ids))
        early = np.setdiff1d(np.unique(ids[:B]), np.unique(ids[B:]))
        assert len(never) > 0 and len(early) > 0
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
        bd.report(case_id(F, K, 1, hidden, B, 'f32', opt))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ twelve SGD steps
def test_wide_many_steps_k101_track_oracle(built):
    """test_ipnn_many_steps_track_oracle at F = 16, k = 101 (Dp0 = 1792, the GEMM path): twelve SGD steps with fresh masks and
    batch lengths over a small table, so that ids repeat inside every batch (the sorted segments of the scatter span chunks)."""
    F, K, hidden = 16, 101, [130, 70, 40]
    table, _, _, params, _, d = problem(F, K, 8, hidden, True, seed=31, n_rows=300)
    eng = engine(F, K, hidden, 'relu', 256, 'f32', 0.02, 0.7)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0, t0 = [w.copy() for w in params['W']], table.copy()
        rng = np.random.RandomState(77)
        sizes = synth.field_sizes_tiny(300, n_fields=F)
        touched, dup = set(), 0
        for step in range(12):
            B = int(rng.randint(60, 201))
            ids = synth.zipf_ids(B, sizes, 1.1, 100 + step)
            dup += B * F - len(np.unique(ids))
            y = (rng.uniform(size=B) < 0.3).astype(np.float64)
            masks = [(rng.uniform(size=(B, d[t])) < 0.7).astype(np.uint8) for t in range(len(hidden) + 1)]
            out = eng.train_step(ids, y, masks, want_logits=(step == 11))
            loss, logits, _ = io.sgd_step(params, table, ids, y, 'relu', 0.02, [m.astype(np.float64) for m in masks], 0.7)
            touched |= set(np.unique(ids).tolist())
        assert dup > 1000
        bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-3, 2e-4)
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - p0[t]).max() + 1e-6)
        tr = np.array(sorted(touched))
        bd.close('table', eng.get_rows(tr), table[tr], 0.0, 5e-3 * np.abs(table - t0).max() + 1e-6)
        bd.report(case_id(F, K, 1, hidden, 200, 'f32', '12steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ bit-exactness
@pytest.mark.parametrize("F,K,pairs", [(2, 17, 1), (16, 101, 1), (32, 128, 1), (23, 51, 0)],
                         ids=lambda v: str(v))
def test_wide_roundtrip_and_zero_lr_bit_exact(built, F, K, pairs):
    """set_params then get_params / get_rows returns every value bit for bit (the rows packed at stride rup(k, 4) and back, the
    layer-1 rows remapped to the wide layout and back); a step at lr = 0 leaves the table, W, biases and b bit-unchanged."""
    hidden, B = [64, 63], 257
    table, ids, y, params, masks, d = problem(F, K, B, hidden, pairs, seed=5 * F + K)
    eng = engine(F, K, hidden, 'tanh', B, 'f32', 0.0, 0.7, pairs)
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
            sel = np.array([table.shape[0] - 1, 0, 5, 0, table.shape[0] - 1])
            assert np.array_equal(eng.get_rows(sel), t32[sel]), when
            if when == 'set':
                eng.train_step(ids, y, masks)
    finally:
        eng.close()


@pytest.mark.parametrize("prec,opt", [('f32', 'sgd'), ('bf16', 'sgd'), ('f32', 'adam'), ('bf16', 'ftrl')])
def test_wide_runs_are_bit_identical(built, prec, opt):
    """Two identical runs of four steps (repeated ids, dropout) give bit-identical logits, tables, layers and b: the wide scatter
    sums in a fixed order and uses no float atomics."""
    F, K, hidden, B, steps = 16, 101, [200, 100], 512, 4
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=3, n_rows=400)
    res = []
    for _ in range(2):     # (bf16 here takes the GEMM path: the write-through stores of k_ip_fwd_w feed it directly)
        eng = engine(F, K, hidden, 'relu', B, prec, 1e-3, 0.7, optimizer=opt)
        try:
            eng.set_params(table, params['b'], params['W'], params['bias'])
            lg = []
            for s in range(steps):
                sl = slice(s * B, (s + 1) * B)
                lg.append(eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)['logits'].cpu().numpy().copy())
            b, Ws, bs = eng.get_params()
            res.append((np.concatenate(lg), b, Ws, bs, eng.get_rows(np.arange(table.shape[0]))))
        finally:
            eng.close()
    (la, ba, Wa, bsa, ra), (lb, bb, Wb, bsb, rb) = res
    assert np.isfinite(la).all() and np.abs(ra - table).max() > 0
    assert np.array_equal(la, lb) and ba == bb and np.array_equal(ra, rb)
    for t in range(len(Wa)):
        assert np.array_equal(Wa[t], Wb[t]) and np.array_equal(bsa[t], bsb[t]), t


# ------------------------------------------------------------------------------------------------ errors and eval
def test_wide_out_of_range_id_is_reported(built):
    """An id outside [0, n_rows) in a wide step is FNN_ERR_RANGE at the step's sync; the handle then steps on."""
    F, K, hidden, B = 16, 101, [64], 64
    table, ids, y, params, masks, d = problem(F, K, B, hidden, True, seed=2)
    eng = engine(F, K, hidden, 'relu', B, 'f32', 0.01, 1.0)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        bad = ids.copy()
        bad[5, 3] = table.shape[0] + 7
        with pytest.raises(FNNError) as ei:
            eng.train_step(bad, y)
        assert ei.value.code == _capi.FNN_ERR_RANGE
        out = eng.train_step(ids, y)
        assert np.isfinite(out['loss'])
    finally:
        eng.close()


def test_wide_predict_and_eval_equal_oracle_and_sklearn(built):
    """predict on a wide handle (16 fields, k = 101) equals the oracle; ipnn_eval over 9,001 examples in three max_batch chunks
    gives sklearn's AUC / RMSE / logloss on the same float32 predictions at 1e-12."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    F, K, hidden = 16, 101, [300, 100]
    table, ids, y, params, masks, d = problem(F, K, 3000, hidden, True, seed=78)
    ids = np.concatenate([ids, ids, ids, ids[:1]])
    yy = (np.random.RandomState(6).uniform(size=len(ids)) < 0.3).astype(np.int32)
    eng = engine(F, K, hidden, 'relu', 3000, 'f32', 0.01, 1.0)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        pp = eng.predict(ids).cpu().numpy()
        bd = Bounds()
        bd.close('predict', pp, io.predict(params, table, ids, 'relu'), 2e-4, 1e-6)
        bd.report('predict-F16-K101')
        m = eng.evaluate(ids, yy)
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ FM -> FNN_IP_L3 / FNN
@pytest.mark.parametrize("cls,rank", [(FNN_IP_L3, 50), (FNN, 50), (FNN_IP_L3, 100)], ids=['FNN_IP_L3_50', 'FNN50', 'FNN_IP_L3_100'])
def test_fm_pickle_seeds_the_wide_family(built, tmp_path, cls, rank):
    """The hand-off this path exists for (python/baseline.py): FM at rank `rank` trains a few steps and dumps {'W', 'V', 'b'};
    FNN_IP_L3 / FNN of the same rank load that pickle through _init_argv (its rows bit for bit), train three steps and track the
    oracle started from the same pickle and the same initial layers (the one-f32-step bounds on the logits and the loss)."""
    from deep_ctr_amd.FM import FM
    F, B = 16, 256
    sizes = synth.field_sizes_tiny(1500, n_fields=F)
    X_dim = sum(sizes)
    ids = synth.zipf_ids(B * 4, sizes, 1.1, 5)
    yl = (np.random.RandomState(6).uniform(size=B * 4) < 0.3).astype(np.float64)
    fm = FM(B, [X_dim, F, rank], ['uniform', -0.01, 0.01, [1, 2], None], ['sgd', 0.05], [1e-3], 'train', 0)
    try:
        for j in range(4):
            fm.train_step(ids[j * B:(j + 1) * B], yl[j * B:(j + 1) * B], want_loss=False)
        path = str(tmp_path / ('fm%d.pkl' % rank))
        fm.dump(path)
    finally:
        fm.close()
    vm = pickle.load(open(path, 'rb'))
    rows = np.concatenate([vm['W'], vm['V']], axis=1)
    assert rows.shape == (X_dim, rank + 1)
    hidden = [300, 100, 50] if cls is FNN_IP_L3 else [300, 100]
    m = cls([], [], B, [X_dim, F, rank] + hidden + ['relu'], ['uniform', -0.05, 0.05, [3, 4, 5], path], ['sgd', 0.001, 'sum'],
            [1.0], 'train', 0, precision='f32')
    bd = Bounds()
    try:
        assert np.array_equal(m.eng.get_rows(np.arange(X_dim)), rows.astype(np.float32))
        b, Ws, bs = m.eng.get_params()
        assert b == np.float32(vm['b'][0])
        params = {'b': float(b), 'W': [w.astype(np.float64) for w in Ws], 'bias': [x.astype(np.float64) for x in bs]}
        table = rows.astype(np.float64)
        pairs = cls.PAIRS
        for s in range(3):
            sl = slice(s * B, (s + 1) * B)
            out = m.eng.train_step(ids[sl], yl[sl], want_logits=True)
            with oracle_pairs(pairs):
                loss, logits, _ = io.sgd_step(params, table, ids[sl], yl[sl], 'relu', 0.001)
            bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 2e-4, 2e-5)
            bd.close('loss%d' % s, out['loss'], loss, 0.0, 5e-5 * max(1.0, abs(loss)))
        touched = np.unique(ids[:3 * B])
        bd.close('rows', m.eng.get_rows(touched), table[touched], 0.0, 2e-3 * np.abs(table - rows).max() + 1e-7)
        out_path = str(tmp_path / 'ip.pkl')
        m.dump(out_path)
        back = pickle.load(open(out_path, 'rb'))
        assert back['V'].shape == (X_dim, rank) and back['h1_w'].shape == (m.eng.d[0], hidden[0])
        bd.report('%s-rank%d' % (cls.__name__, rank))
    finally:
        m.eng.close()


# ------------------------------------------------------------------------------------------------ full shape
def test_wide_full_shape_f32_step(built):
    """One f32 SGD step at the iPinYou size of python/baseline.py's FNN_IP_L3 recipe on FM100 rows: 937,670 x 101 table, 16
    fields, hidden 400 / 400 / 200, batch 4096, keep 0.5.  The oracle runs on the touched rows (ids remapped through the sorted
    list of them); the one-f32-step bounds: logits rtol 2e-4, the loss to 5e-5, every dense and touched-row update within 2e-3
    of its size; a sample of untouched rows bit for bit."""
    F, K, hidden, B = 16, 101, [400, 400, 200], 4096
    sizes = synth.field_sizes_ipinyou()
    D = sum(sizes)
    rng = np.random.RandomState(11)
    table = (np.random.RandomState(1234).standard_normal((D, K)) * 0.05).astype(np.float32)
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
        loss, logits, _ = io.sgd_step(params, tc, idc, y, 'relu', 1e-3, [m.astype(np.float64) for m in masks], 0.5)
        bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-4, 2e-5)
        bd.close('loss', out['loss'], loss, 0.0, 5e-5 * max(1.0, abs(loss)))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 2e-3 * (np.abs(params['W'][t] - p0['W'][t]).max() + 1e-12) + 2e-7)
            bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 2e-3 * (np.abs(params['bias'][t] - p0['bias'][t]).max() + 1e-12) + 2e-7)
        bd.close('b', b, params['b'], 0.0, 2e-3 * abs(params['b'] - p0['b']) + 2e-7)
        bd.close('table', eng.get_rows(touched), tc, 0.0, 2e-3 * (np.abs(tc - t0).max() + 1e-12) + 2e-7)
        cand = np.setdiff1d(np.random.RandomState(0).randint(0, D, size=20000), touched)
        assert np.array_equal(eng.get_rows(cand), table[cand])
        bd.report(case_id(F, K, 1, hidden, B, 'f32', 'fullsize'))
    finally:
        eng.close()


def test_wide_write_through_equals_plain_stores_bf16(built, monkeypatch):
    """IPNN_WT=0 (plain stores) and the default write-through stores of the wide kernels give bit-identical logits, rows and
    layers over three bf16 steps on both stack paths (a store that reads its data registers late would show here)."""
    for F, K, hidden in ((16, 101, [200, 100]), (8, 51, [200, 100])):
        table, ids, y, params, masks, d = problem(F, K, 512 * 3, hidden, True, seed=4, n_rows=400)
        res = []
        for wt in ('1', '0'):
            monkeypatch.setenv('IPNN_WT', wt)
            eng = engine(F, K, hidden, 'relu', 512, 'bf16', 1e-3, 0.7)
            try:
                eng.set_params(table, params['b'], params['W'], params['bias'])
                lg = [eng.train_step(ids[s * 512:(s + 1) * 512], y[s * 512:(s + 1) * 512], [m[s * 512:(s + 1) * 512] for m in masks],
                                     want_logits=True)['logits'].cpu().numpy().copy() for s in range(3)]
                b, Ws, bs = eng.get_params()
                res.append((np.concatenate(lg), b, Ws, eng.get_rows(np.arange(table.shape[0]))))
            finally:
                eng.close()
        (la, ba, Wa, ra), (lb, bb, Wb, rb) = res
        assert np.array_equal(la, lb) and ba == bb and np.array_equal(ra, rb), (F, K)
        for t in range(len(Wa)):
            assert np.array_equal(Wa[t], Wb[t]), (F, K, t)
