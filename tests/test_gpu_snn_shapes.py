"""The SNN fine-tune step (FNN_MODE_BAG, python/SNN_RBM.py:238-291) at the shapes fnn_create accepts beyond the layout every
other bag-mode test uses (16 columns, hidden 300 / 100, tanh): 2..64 columns, h0 from 192 to 316, every hidden pair the strip
kernel is built for, all three activations and precisions, max_batch above 4096 for predict and eval, and a table large
enough for 64-bit sort keys -- against the float64 oracle.

Bag mode runs on the strip kernel only.  Every case id starts with the instance the restatement of strip_shape_ok and
step1_sel (fnn_api.hip) below predicts:
  cx4-c5x2-nw8  k_step1<T, 5, 2, 4, true, 8>   h0 <= 252 (K1p = rup(h0 + 1, 64) = 256), hidden 256..319 / 64..127
  cx5-c5x2-nw8  k_step1<T, 5, 2, 5, true, 8>   h0 >= 256 (K1p = 320), the same hidden pairs
  cx4-c1x1      k_step1<T, 1, 1, 4, true>      h0 <= 252, hidden <= 63 / <= 63 (four waves)
  ...-nw4       the four-wave forms of the first two under FNN_STEP1_WAVES=4
The strip keeps 16 x F ids in LDS and sums each example's rows in groups of 16 columns (P0, BAGL = 16), and so does
k_bag_ref (fnn_gather).  The grouping tags a row that several columns of a batch hold with atomicMax(tag_first[row],
stamp << 6 | column), and such rows take the float-atomic branch of the row update: with many columns on a small table
that branch is the main path.  The ones column that carries b1 (row h0 of w1), the masked columns past H1 / H2 and the
columns of b2 and b3 move with h0, H1 and H2.

Bounds are those of test_gpu_parity.test_snn_step_f32_vs_oracle (f32), the random sweep's tol 8 for bf16x3 and those of
test_snn_step_bf16_tracks_oracle for bf16.  Each one-step case prints its worst error as a fraction of its bound.  The
oracle's row update is snn_update_vec (checked against the per-example loop in tests/test_oracle.py), so that 4096 lines of
64 columns stay cheap.
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi
from deep_ctr_amd.engine import FNNEngine, FNNError
from test_gpu_parity import make_snn_engine, make_snn_problem, snn_active_ids
from test_gpu_shapes import Bounds

pytestmark = pytest.mark.gpu

DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')


def rup(a, m):
    return (a + m - 1) // m * m


def instance_of(h0, H1, H2, waves=8):
    """The bag branch of strip_shape_ok and step1_sel's choice of k_step1 instance; None: fnn_create refuses the pair."""
    cx, c1, c2 = rup(h0 + 1, 64) // 64, rup(H1 + 1, 64) // 64, rup(H2 + 1, 64) // 64
    if c1 == 5 and c2 == 2 and cx in (4, 5):
        return 'cx%d-c5x2-nw%d' % (cx, waves)
    if c1 == 1 and c2 == 1 and cx == 4:
        return 'cx4-c1x1'
    return None


def case_id(F, h0, H1, H2, B=None, *rest, waves=8):
    s = '%s-F%d-h%d-H%dx%d' % (instance_of(h0, H1, H2, waves), F, h0, H1, H2)
    if B is not None:
        s += '-B%d' % B
    return '-'.join([s] + [str(r) for r in rest if r not in (None, '', 'tanh', 'f32')])


def lr_for(B):
    """test_gpu_shapes.lr_for: the loss is a sum over the batch, so 4096 examples and more step at lr = 0.001."""
    return 0.001 if B >= 4096 else 0.01


def edge_empties(B, F):
    return [(0, 0), (B // 2, F - 1), (B - 1, F - 1), (B // 3, min(16, F - 1))]


def problem(F, h0, H1, H2, B, layout, n_rows, kind='', seed=0):
    kw = {}
    if layout == 'fields':
        kw['empty'] = edge_empties(B, F)
        if kind == 'dup':
            kw['dup_col'] = F - 1
    prob = make_snn_problem(B, n_rows=n_rows, h0=h0, seed=seed, n_fields=F, h1=H1, h2=H2, layout=layout, **kw)
    prob[5][0] = prob[6][0] = 1                                # one-unit layers stay live
    return prob


def engine(prob, F, h0, H1, H2, prec='f32', acti='tanh', lr=0.01, lam1=0.001, max_batch=4096):
    ww0, bb0, ids, y, p, r1, r2 = prob
    return make_snn_engine(ww0, bb0, p, prec=prec, lr=lr, lam1=lam1, h0=h0, max_batch=max_batch, n_fields=F, h1=H1, h2=H2,
                           acti=acti)


def compact(ids, rows):
    """ids remapped to positions in `rows` (sorted unique), -1 kept."""
    return np.where(ids >= 0, np.searchsorted(rows, ids), -1).astype(ids.dtype)


def check_step(eng, prob, lr, lam1, prec='f32', acti='tanh', label='', touched=None, ids_dev=None):
    """One step against orc.snn_train_step, tensor by tensor: fnn_gather, p_drop, gx, the loss, the whole table (or, with
    `touched`, the touched rows: the oracle then runs on a table of those rows only), the bag bias, the six dense tensors and
    (f32) the predictions after the step.  Returns the oracle's state after the step."""
    ww0, bb0, ids, y, p, r1, r2 = prob
    ids_o = ids if touched is None else compact(ids, touched)
    ww64 = (ww0 if touched is None else ww0[touched]).astype(np.float64)
    w_before = ww64.copy()
    bb64 = bb0.astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    bg, bd = Bounds(), Bounds()
    bg.close('gather', eng.gather(ids).cpu().numpy(), orc.snn_bag(ww64, bb64, ids_o), 2e-6, 1e-7)
    bg.report(label + ' fnn_gather')
    out = eng.train_step(ids if ids_dev is None else ids_dev, y, r1, r2, want_p=True, want_gx=True)
    ref = orc.snn_train_step(p64, ww64, bb64, ids_o, y.astype(np.float64), r1.astype(float), r2.astype(float), lr, lam1,
                             acti, vec=True)
    got_p, got_gx = out['p'].cpu().numpy(), out['gx'].cpu().numpy()
    tab = eng.get_table() if touched is None else eng.get_rows(touched)
    upd = np.abs(ww64 - w_before).max() + 1e-12
    if prec == 'bf16':
        bd.close('p_drop', got_p, ref['p_drop'], 0.0, 3e-2)
        bd.close('loss', out['loss'], ref['loss'], 0.0, 3e-2 * ref['loss'])
        bd.close('table', tab, ww64, 0.0, 8e-2 * upd + 1e-6)
    else:
        tol = 8.0 if prec == 'bf16x3' else 1.0
        bd.close('p_drop', got_p, ref['p_drop'], 2e-4 * tol, 1e-6 * tol)
        gs = np.abs(ref['gx']).max()
        bd.close('gx', got_gx, ref['gx'], 2e-3 * tol, 2e-5 * gs * tol + 1e-9)
        bd.close('loss', out['loss'], ref['loss'], 0.0, 2e-5 * tol * max(1.0, abs(ref['loss'])))
        bd.close('table', tab, ww64, 0.0, 1e-3 * tol * upd + 2e-7)
        bupd = np.abs(bb64 - bb0).max() + 1e-12
        bd.close('bag bias', eng.get_bag_bias(), bb64, 0.0, 1e-3 * tol * bupd + 2e-7)
        d = eng.get_dense()
        for k in DENSE:
            scale = np.abs(p64[k] - p[k]).max() + 1e-12
            bd.close(k, d[k], p64[k], 0.0, 1e-3 * tol * scale + 1e-7)
        bd.close('b3', d['b3'], p64['b3'], 0.0, 1e-3 * tol * (abs(p64['b3'] - p['b3']) + 1e-12) + 1e-7)
        if prec == 'f32':
            bd.close('predict', eng.predict(ids).cpu().numpy(), orc.snn_predict(p64, ww64, bb64, ids_o, acti), 3e-4, 1e-6)
    bd.report(label)
    return ww64, bb64, p64


# ------------------------------------------------------------------------------------------------ one step, f32
# (F, h0, H1, H2, B, layout, n_rows, kind): the column counts, h0, hidden pairs, batch boundaries, both id layouts and table
# sizes rotate over the cases; the small hidden pairs sit at h0 <= 252, where the strip kernel has them
STEP = [
    (2, 192, 300, 100, 257, 'fields', 600, ''), (3, 200, 63, 63, 17, 'active', 80, ''),
    (13, 252, 1, 1, 4096, 'fields', 3000, ''), (17, 256, 256, 64, 1, 'active', 300, ''),
    (31, 300, 319, 127, 15, 'fields', 1000, ''), (39, 316, 300, 100, 4095, 'active', 3000, ''),
    (64, 192, 32, 17, 257, 'active', 120, ''), (64, 300, 300, 100, 4096, 'fields', 3000, 'dup'),
    (2, 316, 256, 64, 4096, 'active', 80, ''), (3, 252, 319, 127, 257, 'fields', 600, ''),
    (13, 200, 32, 17, 15, 'fields', 1000, ''), (17, 192, 63, 63, 4095, 'active', 600, ''),
    (31, 256, 300, 100, 17, 'active', 120, ''), (39, 200, 1, 1, 1, 'active', 300, ''),
    (64, 252, 63, 63, 4096, 'active', 3000, ''), (13, 316, 319, 127, 257, 'active', 80, ''),
    (39, 192, 256, 64, 257, 'fields', 300, 'dup'), (17, 200, 300, 100, 15, 'fields', 80, ''),
]
# (F, h0, H1, H2, B, layout, n_rows, kind, precision, activation, waves)
CASES = [c + ('f32', 'tanh', 8) for c in STEP]
CASES += [                                                   # bf16 pairs (tol 8) and bf16: both cx, the small-hidden instance
    (17, 300, 300, 100, 257, 'active', 600, '', 'bf16x3', 'tanh', 8),
    (39, 200, 63, 63, 257, 'fields', 1000, '', 'bf16x3', 'tanh', 8),
    (64, 256, 319, 127, 4096, 'active', 3000, '', 'bf16x3', 'tanh', 8),
    (3, 192, 1, 1, 17, 'active', 80, '', 'bf16x3', 'tanh', 8),
    (17, 300, 300, 100, 512, 'active', 600, '', 'bf16', 'tanh', 8),
    (39, 252, 63, 63, 512, 'fields', 1000, '', 'bf16', 'tanh', 8),
    (64, 200, 256, 64, 512, 'active', 600, '', 'bf16', 'tanh', 8),
]
CASES += [                                                   # sigmoid and linear on layer one, at cx = 4 and cx = 5
    (F_, h0_, H1_, H2_, 257, lay, n_, '', 'f32', a, 8)
    for (F_, h0_, H1_, H2_, lay, n_) in ((13, 200, 300, 100, 'active', 600), (39, 300, 256, 64, 'fields', 1000))
    for a in ('sigmoid', 'linear')
]
CASES += [                                                   # FNN_STEP1_WAVES=4: the four-wave forms of both hidden-300 instances
    (13, 200, 300, 100, 4096, 'active', 3000, '', 'f32', 'tanh', 4),
    (39, 300, 319, 127, 257, 'fields', 1000, '', 'f32', 'tanh', 4),
]


@pytest.mark.parametrize("F,h0,H1,H2,B,layout,n_rows,kind,prec,acti,waves", CASES,
                         ids=[case_id(*c[:5], c[5], c[7], c[8], c[9], waves=c[10]) for c in CASES])
def test_snn_step_vs_oracle(built, monkeypatch, F, h0, H1, H2, B, layout, n_rows, kind, prec, acti, waves):
    assert instance_of(h0, H1, H2) is not None
    if waves == 4:
        monkeypatch.setenv('FNN_STEP1_WAVES', '4')              # read by fnn_create
    else:
        monkeypatch.delenv('FNN_STEP1_WAVES', raising=False)
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    prob = problem(F, h0, H1, H2, B, layout, n_rows, kind, seed=F * 7 + h0 + B)
    lr = lr_for(B)
    eng = engine(prob, F, h0, H1, H2, prec=prec, acti=acti, lr=lr)
    try:
        check_step(eng, prob, lr, 0.001, prec=prec, acti=acti,
                   label=case_id(F, h0, H1, H2, B, layout, prec, acti, waves=waves))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ shared rows over steps
def shared_rows(ids):
    """Rows that several columns of this batch hold, and the highest such column."""
    cols = {}
    for f in range(ids.shape[1]):
        for r in np.unique(ids[:, f]):
            if r >= 0:
                cols.setdefault(int(r), []).append(f)
    sh = {r: c for r, c in cols.items() if len(c) > 1}
    return len(sh), max((max(c) for c in sh.values()), default=-1)


def test_five_steps_at_64_columns_on_a_small_table(built):
    """64 columns on a table of 150 rows: in every step most touched rows sit in several columns (also beyond column 15, so
    the tag uses all six column bits) and take the float-atomic branch, and every step advances the stamp.  Once through
    train_step with the next batch announced (fnn_prefetch_ids), once through train_epoch; both against the oracle's five
    steps, at the bounds of test_snn_same_row_in_several_columns, and against each other."""
    import torch
    F, h0, H1, H2, B, steps = 64, 200, 300, 100, 300, 5
    ww0, bb0, ids, y, p, r1, r2 = make_snn_problem(steps * B, n_rows=150, h0=h0, seed=31, n_fields=F, layout='active')
    for j in range(steps):
        n, top = shared_rows(ids[j * B:(j + 1) * B])
        assert n > 50 and top >= 48, (j, n, top)
    rng = np.random.RandomState(8)
    M1 = (rng.uniform(size=(steps, H1)) < 0.9).astype(np.uint8)
    M2 = (rng.uniform(size=(steps, H2)) < 0.9).astype(np.uint8)
    ww64, bb64 = ww0.astype(np.float64), bb0.astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    losses = []
    for j in range(steps):
        sl = slice(j * B, (j + 1) * B)
        ref = orc.snn_train_step(p64, ww64, bb64, ids[sl], y[sl].astype(np.float64), M1[j].astype(float),
                                 M2[j].astype(float), 0.01, 0.001, vec=True)
        losses.append(ref['loss'])
    a = make_snn_engine(ww0, bb0, p, h0=h0, n_fields=F)
    b = make_snn_engine(ww0, bb0, p, h0=h0, n_fields=F)
    try:
        dev = [torch.as_tensor(ids[j * B:(j + 1) * B]).to(a.device).contiguous() for j in range(steps)]
        for j in range(steps):
            if j + 1 < steps:
                a.prefetch_ids(dev[j + 1])
            out = a.train_step(dev[j], y[j * B:(j + 1) * B], M1[j], M2[j])
            assert abs(out['loss'] - losses[j]) <= 5e-5 * max(1.0, abs(losses[j])), j
        ids_d, y_d = b.to_device(ids, y.astype(np.int32))
        b.train_epoch(ids_d, y_d.float(), B, M1, M2)
        upd, bupd = np.abs(ww64 - ww0).max(), np.abs(bb64 - bb0).max()
        res = []
        for e in (a, b):
            tab, bias, d = e.get_table(), e.get_bag_bias(), e.get_dense()
            assert np.abs(tab - ww64).max() <= 1e-3 * upd + 3e-7
            assert np.abs(bias - bb64).max() <= 1e-3 * bupd + 3e-7
            for k in DENSE:
                assert np.abs(d[k] - p64[k]).max() <= 1e-3 * (np.abs(p64[k] - p[k]).max() + 1e-12) + 1e-7, k
            assert abs(d['b3'] - p64['b3']) <= 1e-3 * abs(p64['b3'] - p['b3']) + 1e-7
            res.append((tab, bias, d))
        # the float atomics of the shared rows add in any order: the runs differ by a few ulps per step, carried on
        assert np.abs(res[0][0] - res[1][0]).max() <= 1e-4 * upd + 1e-7
        assert np.abs(res[0][1] - res[1][1]).max() <= 1e-4 * bupd + 1e-7
        for k in DENSE:
            assert np.abs(res[0][2][k] - res[1][2][k]).max() <= 1e-4 * np.abs(p64[k] - p[k]).max() + 1e-7, k
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ boundaries, bit-exact
ROUND = [(2, 192, 63, 63), (64, 252, 1, 1), (13, 256, 256, 64), (39, 316, 319, 127), (17, 192, 319, 127), (31, 252, 256, 64)]


@pytest.mark.parametrize("F,h0,H1,H2", ROUND, ids=[case_id(*c) for c in ROUND])
def test_set_get_roundtrip_bit_exact(built, F, h0, H1, H2):
    """fnn_set_dense / fnn_get_dense remap w1 [h0, H1] and b1 (row h0 of the padded w1, the ones column), w2 / b2 and w3 / b3
    into blocks padded to K1p / H1p / H2p; fnn_set_bag_bias / fnn_get_bag_bias, fnn_get_table and fnn_get_rows keep h0
    floats of rows rw wide: all bit for bit."""
    ww0, bb0, ids, y, p, r1, r2 = problem(F, h0, H1, H2, 8, 'fields', 1000, seed=F + h0)
    eng = engine((ww0, bb0, ids, y, p, r1, r2), F, h0, H1, H2)
    try:
        d = eng.get_dense()
        for k in DENSE:
            assert np.array_equal(d[k], p[k].astype(np.float32)), k
        assert d['b3'] == np.float32(p['b3'])
        assert np.array_equal(eng.get_bag_bias(), bb0)
        assert np.array_equal(eng.get_table(), ww0)
        sel = np.array([ww0.shape[0] - 1, 0, ww0.shape[0] // 2, 1])
        assert np.array_equal(eng.get_rows(sel), ww0[sel])
    finally:
        eng.close()


@pytest.mark.parametrize("F", [2, 64])
def test_gather_beyond_max_batch(built, F):
    """fnn_gather (k_bag_ref: groups of 16 columns) against orc.snn_bag at 2 and 64 columns, 1000 lines on a handle of
    max_batch 256: device pointers in one launch, host pointers in max_batch chunks; rtol 2e-6 as test_snn_step_f32_vs_oracle."""
    import ctypes as C
    B, h0 = 1000, 300
    prob = problem(F, h0, 300, 100, B, 'active', 600, seed=F)
    ww0, bb0, ids, y, p, r1, r2 = prob
    eng = engine(prob, F, h0, 300, 100, max_batch=256)
    try:
        ref = orc.snn_bag(ww0.astype(np.float64), bb0.astype(np.float64), ids)
        np.testing.assert_allclose(eng.gather(ids).cpu().numpy(), ref, rtol=2e-6, atol=1e-7)
        x = np.empty((B, h0), np.float32)
        ids32 = np.ascontiguousarray(ids, np.int32)
        rc = eng.lib.fnn_gather(eng.h, ids32.ctypes.data_as(C.c_void_p), B, x.ctypes.data_as(C.c_void_p), _capi.FNN_MEM_HOST)
        assert rc == 0
        np.testing.assert_allclose(x, ref, rtol=2e-6, atol=1e-7)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ predict and evaluate
PRED = [(39, 300, 300, 100, 1000, 2501, 'tanh'), (17, 252, 63, 63, 8192, 8192, 'sigmoid')]


@pytest.mark.parametrize("F,h0,H1,H2,max_batch,N,acti", PRED, ids=[case_id(*c[:4], None, 'mb%d' % c[4], 'N%d' % c[5], c[6]) for c in PRED])
def test_predict_and_eval_vs_oracle(built, F, h0, H1, H2, max_batch, N, acti):
    """fnn_predict (acti_type on both hidden layers) against orc.snn_predict on the engine's own state after a step, and
    fnn_eval's AUC / RMSE / logloss against sklearn on the returned p at 1e-12: 2,501 lines in max_batch chunks of 1000,
    and 8,192 in one call on a handle of max_batch 8192."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    prob = problem(F, h0, H1, H2, N, 'active', 1000, seed=N)
    ww0, bb0, ids, y, p, r1, r2 = prob
    eng = engine(prob, F, h0, H1, H2, acti=acti, max_batch=max_batch)
    try:
        eng.train_step(ids[:300], y[:300], r1, r2)
        pr = eng.predict(ids).cpu().numpy()
        d = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in eng.get_dense().items()}
        ref = orc.snn_predict(d, eng.get_table().astype(np.float64), eng.get_bag_bias().astype(np.float64), ids, acti)
        np.testing.assert_allclose(pr, ref, rtol=3e-4, atol=1e-6)
        yy = y.astype(np.int32)
        m = eng.evaluate(ids, yy, want_p=True)
        pp = m['p'].cpu().numpy()
        np.testing.assert_array_equal(pp, pr)
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


@pytest.mark.parametrize("announced", [False, True])
def test_refused_large_batch_leaves_no_state(built, announced):
    """Bag mode trains through the three-launch path only: train_step with 4097 lines on a handle of max_batch 8192 is
    FNN_ERR_ARG and leaves the table, the bag bias and the dense tensors as they were.  A valid 4096-line step on the same
    handle then matches the oracle -- also when fnn_prefetch_ids announced that batch before the refused call."""
    import torch
    F, h0, H1, H2 = 31, 256, 300, 100
    prob = problem(F, h0, H1, H2, 4097 + 4096, 'active', 3000, seed=77)
    ww0, bb0, ids, y, p, r1, r2 = prob
    eng = engine(prob, F, h0, H1, H2, lr=0.001, max_batch=8192)
    try:
        big = torch.as_tensor(ids[:4097]).to(eng.device).contiguous()
        ok = torch.as_tensor(ids[4097:]).to(eng.device).contiguous()
        if announced:
            eng.prefetch_ids(ok)
        with pytest.raises(FNNError) as ei:
            eng.train_step(big, y[:4097], r1, r2)
        assert ei.value.code == _capi.FNN_ERR_ARG and 'B <= 4096' in str(ei.value)
        eng.sync()
        assert np.array_equal(eng.get_table(), ww0) and np.array_equal(eng.get_bag_bias(), bb0)
        d = eng.get_dense()
        for k in DENSE:
            assert np.array_equal(d[k], p[k].astype(np.float32)), k
        assert d['b3'] == np.float32(p['b3'])
        check_step(eng, (ww0, bb0, ids[4097:], y[4097:], p, r1, r2), 0.001, 0.001, ids_dev=ok,
                   label=case_id(F, h0, H1, H2, 4096, 'after-refusal', 'announced' if announced else ''))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 64-bit sort keys
def test_step_with_64bit_sort_keys(built):
    """A bag table of 1,100,000 rows (h0 = 192: 845 MB in f32) makes n_rows * 4096 exceed 2^32, so the grouping runs on 64-bit
    keys.  One f32 step with rows shared between columns and the last row in three columns, against the oracle on a table of
    the touched rows only; a seeded sample of untouched rows keeps its bits."""
    F, h0, H1, H2, B, n_rows = 17, 192, 300, 100, 1000, 1100000
    ww0 = np.random.default_rng(0).standard_normal((n_rows, h0), dtype=np.float32) * np.float32(0.1)
    _, bb0, _, y, p, r1, r2 = make_snn_problem(B, n_rows=600, h0=h0, seed=23, n_fields=F)
    ids = snn_active_ids(B, n_rows, F, 24)
    top = n_rows - 1
    ids[5, 0] = ids[9, 3] = ids[11, 0] = top
    ids[9, 0] = ids[12, 1] = 7
    touched = np.unique(ids[ids >= 0])
    assert touched[-1] == top
    eng = make_snn_engine(ww0, bb0, p, h0=h0, n_fields=F)
    try:
        assert eng.n_rows * 4096 > 2 ** 32
        check_step(eng, (ww0, bb0, ids, y, p, r1, r2), 0.01, 0.001, touched=touched,
                   label=case_id(F, h0, H1, H2, B, 'key64'))
        rng = np.random.RandomState(5)
        sample = np.setdiff1d(rng.randint(0, n_rows, 4000), touched)[:2000]
        assert np.array_equal(eng.get_rows(sample), ww0[sample])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ data parallelism
def test_virtual_two_rank_dp_at_39_columns_small_hidden(built):
    """test_virtual_two_rank_dp_bag_mode on the small-hidden instance at 39 columns: fnn_step_begin on each half, buckets
    summed as the all-reduce would, fnn_step_end; dense tensors and the bag bias equal the single-engine full-batch step, rows
    only one half touches equal the full-batch result on that rank."""
    import torch
    F, h0, H1, H2 = 39, 200, 63, 63
    ww0, bb0, ids, y, p, r1, r2 = make_snn_problem(512, n_rows=1000, h0=h0, seed=9, dup_col=4, n_fields=F, h1=H1, h2=H2)
    full = make_snn_engine(ww0, bb0, p, h0=h0, n_fields=F, h1=H1, h2=H2)
    full.train_step(ids, y, r1, r2)
    ref_dense, ref_rows, ref_bb = full.get_dense(), full.get_table(), full.get_bag_bias()
    full.close()
    ranks = [make_snn_engine(ww0, bb0, p, h0=h0, n_fields=F, h1=H1, h2=H2) for _ in range(2)]
    try:
        halves = [slice(0, 256), slice(256, 512)]
        buckets = [e.step_begin(ids[h], y[h], r1, r2, b_size=512) for e, h in zip(ranks, halves)]
        for e in ranks:
            e.sync()
        tot = buckets[0] + buckets[1]
        for b in buckets:
            b.copy_(tot)
        torch.cuda.synchronize()
        for e in ranks:
            e.step_end()
            e.sync()
        for e in ranks:
            d = e.get_dense()
            for k in DENSE:
                scale = np.abs(d[k] - p[k].astype(np.float32)).max() + 1e-12
                assert np.abs(d[k] - ref_dense[k]).max() <= 5e-4 * scale + 1e-7, k
            bscale = np.abs(ref_bb - bb0).max() + 1e-12
            assert np.abs(e.get_bag_bias() - ref_bb).max() <= 5e-4 * bscale + 1e-7
        t0, t1 = set(np.unique(ids[halves[0]])), set(np.unique(ids[halves[1]]))
        only0, only1 = np.array(sorted(t0 - t1 - {-1})), np.array(sorted(t1 - t0 - {-1}))
        assert len(only0) and len(only1)
        np.testing.assert_allclose(ranks[0].get_table()[only0], ref_rows[only0], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(ranks[1].get_table()[only1], ref_rows[only1], rtol=1e-5, atol=2e-7)
    finally:
        for e in ranks:
            e.close()


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [(200, 255, 64), (200, 64, 63), (200, 63, 64), (200, 320, 128), (256, 63, 63)]
ACCEPTED = [(200, 256, 64), (200, 319, 127), (316, 256, 64), (256, 319, 127)]


@pytest.mark.parametrize("h0,H1,H2", REFUSED, ids=['h%d-H%dx%d' % c for c in REFUSED])
def test_hidden_pairs_outside_the_strip_kernel_are_refused(built, h0, H1, H2):
    """fnn_create refuses a bag handle whose hidden pair the strip kernel is not built for, and its message states the ranges
    strip_shape_ok accepts: hidden1 256..319 with hidden2 64..127, or both <= 63 at h0 <= 252."""
    assert instance_of(h0, H1, H2) is None
    with pytest.raises(FNNError) as ei:
        FNNEngine(17, 0, H1, H2, max_batch=256, precision='f32', mode='bag', hidden0=h0, reg_all=True, lambda_fm=0.0)
    msg = str(ei.value)
    assert ei.value.code == _capi.FNN_ERR_ARG and '256..319' in msg and '64..127' in msg and '<= 63' in msg, msg


@pytest.mark.parametrize("h0,H1,H2", ACCEPTED, ids=[case_id(17, *c) for c in ACCEPTED])
def test_hidden_pairs_at_the_edges_are_accepted(built, h0, H1, H2):
    eng = FNNEngine(17, 0, H1, H2, max_batch=256, precision='f32', mode='bag', hidden0=h0, reg_all=True, lambda_fm=0.0)
    eng.close()


def test_bag_step_without_the_strip_kernel_is_refused(built, monkeypatch):
    """FNN_NO_FUSE=1 turns the strip kernel off, and bag mode has no layer-by-layer form: train_step and predict fail with
    FNN_ERR_ARG and a message that names the cause."""
    monkeypatch.setenv('FNN_NO_FUSE', '1')
    prob = problem(13, 200, 300, 100, 64, 'active', 300, seed=2)
    ww0, bb0, ids, y, p, r1, r2 = prob
    eng = engine(prob, 13, 200, 300, 100)
    try:
        for call in (lambda: eng.train_step(ids, y, r1, r2), lambda: eng.predict(ids)):
            with pytest.raises(FNNError) as ei:
                call()
            assert ei.value.code == _capi.FNN_ERR_ARG and 'FNN_NO_FUSE' in str(ei.value), str(ei.value)
        assert np.array_equal(eng.get_table(), ww0)
    finally:
        eng.close()
