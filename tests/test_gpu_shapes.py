"""The FNN step at the shapes fnn_create accepts beyond the default layout (16 fields, k = 11, hidden 300 / 100): field counts
2..64, k = rank + 1 in 1..15, hidden sizes 1..4095 / 1..255, all three precisions, against the float64 oracle.

Both code paths depend on the shape.  Every case id starts with the path the restatement of strip_shape_ok (fnn_api.hip) below
predicts:
  strip  the fused strip kernel: K1p = rup(16 F, 64) = 256 (F = 13..16) and hidden sizes padding to 320 / 128 (256..319 /
         64..127) or to 64 / 64 (<= 63 / <= 63).  Its gather writes w_0 into slot k of field 0 and 1.0 into slot k of field 1
         (float4 k >> 2, lane k & 3), so each k takes its own lane and quarter of the 16-float row.
  layer  the layer-by-layer kernels (k_gather, the tiled GEMMs at any padded size, k_head) for every other shape.
Pad slots, the w_0 slot and the ones slot only go wrong visibly on a LATER step or in the host remap of w1 (row k carries
w1[0, :], row 16 + k carries b1), hence the multi-step and bit-exact round-trip tests beside the one-step checks.

Bounds are those of test_gpu_parity._check_step (f32: tol 1, the table included), the random sweep's for bf16x3 (tol 8, table
40) and test_train_step_bf16_vs_oracle's for bf16.  Each one-step case prints its worst error as a fraction of its bound.
The oracle's row update is the vectorised closed form (scatter_sgd_vec, checked against the sequential loop in
tests/test_oracle.py), so that 4096-example batches at 39 or 64 fields stay cheap.
"""
import os

import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNEngine

pytestmark = pytest.mark.gpu

DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')


def rup(a, m):
    return (a + m - 1) // m * m


def path_of(F, H1, H2):
    """strip_shape_ok of fnn_api.hip for FM mode (K1p = rup(16 F, 64), H1p = rup(H1 + 1, 64), H2p = rup(H2 + 1, 64))."""
    cx, c1, c2 = rup(16 * F, 64) // 64, rup(H1 + 1, 64) // 64, rup(H2 + 1, 64) // 64
    return 'strip' if cx == 4 and ((c1 == 5 and c2 == 2) or (c1 == 1 and c2 == 1)) else 'layer'


def case_id(F, K, H1, H2, B=None, *rest):
    s = '%s-F%d-K%d-H%dx%d' % (path_of(F, H1, H2), F, K, H1, H2)
    if B is not None:
        s += '-B%d' % B
    return '-'.join([s] + [str(r) for r in rest if r not in (None, '', 'tanh')])


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def edge_empties(B, F):
    """Empty entries in field 0 (it carries w_0), field 1 (the ones slot) and the last field."""
    return [(0, 0), (B // 2, 1), (B - 1, F - 1), (B // 3, 0), (B // 3, 1)]


def make_problem(F, K, H1, H2, B, n_rows=1000, seed=0, dup_col=None, empty=()):
    sizes = synth.field_sizes_tiny(n_rows, n_fields=F)
    rows = synth.fm_table(sum(sizes), K, 0.05, seed)
    fo = synth.field_of_row(sizes)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 1)
    if dup_col is not None:
        ids[:, dup_col] = ids[0, dup_col]
    for (t, f) in empty:
        ids[t, f] = -1
    rng = np.random.RandomState(seed + 2)
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    y[0] = 1.0
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p['w3'] = rng.uniform(-0.2, 0.2, H2)
    p['b1'] = rng.uniform(-0.1, 0.1, H1)
    p['b2'] = rng.uniform(-0.1, 0.1, H2)
    p['b3'] = 0.05
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
    r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
    r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
    r1[0] = r2[0] = 1                              # one-unit layers stay live
    return rows, fo, ids, y, p, r1, r2


def make_engine(F, K, H1, H2, rows, fo, p, prec='f32', acti='tanh', max_batch=4096, lr=0.01, lam1=0.02, lamfm=0.1, w0=-3.0,
                reg_all=False):
    eng = FNNEngine(F, K, H1, H2, max_batch=max_batch, precision=prec, acti_type=acti, lr=lr, lambda1=lam1, lambda_fm=lamfm,
                    reg_all=reg_all)
    eng.set_table(rows, fo, w0)
    eng.set_dense(p)
    return eng


def lr_for(B):
    """The loss is a SUM over the batch (python/FNN_wnzh.py:173): at lr = 0.01 one 4096-example step moves a row hit by most
    of the batch from 0.05 to about 5 and drives the output unit into saturation, which measures f32 rounding of a step no
    run takes.  4096 examples and more step at lr = 0.001, as the other tests at that batch do (the reference's default)."""
    return 0.001 if B >= 4096 else 0.01


def oracle_step(rows64, p64, ids, y, r1, r2, lr, lam1, lamfm, acti='tanh', w0=-3.0, b_size=None, reg_all=False):
    """One step of the float64 oracle, in place on rows64 / p64: (gx, loss, p_drop, grads)."""
    x = orc.gather_vec(rows64, ids, w0)
    gx, _, loss, p_drop, g = orc.train_call(p64, x, y.astype(np.float64), r1.astype(np.float64), r2.astype(np.float64),
                                            lr, lam1, acti, reg_all)
    orc.scatter_sgd_vec(rows64, ids, gx, lr, lamfm, b_size)
    return gx, loss, p_drop, g


class Bounds(object):
    """assert_allclose-style checks that also keep the worst |got - ref| / (atol + rtol |ref|) seen."""

    def __init__(self):
        self.worst, self.where = 0.0, ''

    def close(self, name, got, ref, rtol, atol):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        r = float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()) if got.size else 0.0
        if not r <= self.worst:
            self.worst, self.where = r, name
        assert r <= 1.0, "%s: max error %.3g of its bound (max |d| %.3e)" % (name, r, float(np.abs(got - ref).max()))

    def report(self, label):
        print("\n[shapes] %s: worst error %.3f of the bound (%s)" % (label, self.worst, self.where))


def compare_step(bd, prec, rows, lr, got_p, got_loss, tab, d, oracle, got_gx=None):
    """What check_step asserts about one step's outputs, on the Bounds `bd`.  rows: the table before the step; tab / d: the table
    and fnn_get_dense after it; oracle: (rows64, p64, gx, loss, p_drop, g), the oracle's state after its step and what oracle_step
    returned.  got_gx None (a call that returns no gx) leaves the gx bound out; every other bound is check_step's."""
    rows64, p64, gx, loss, p_drop, g = oracle
    gscale = np.abs(gx).max()
    if prec == 'bf16':
        bd.close('p_drop', got_p, p_drop, 0.0, 2e-2)
        if got_gx is not None:
            bd.close('gx', got_gx, gx, 0.0, 5e-2 * gscale)
        bd.close('loss', got_loss, loss, 0.0, 2e-2 * loss)
        bd.close('table', tab, rows64, 0.0, 5e-2 * np.abs(rows64 - rows).max() + 1e-6)
    else:
        tol, tt = (8.0, 40.0) if prec == 'bf16x3' else (1.0, 1.0)
        bd.close('p_drop', got_p, p_drop, 1e-4 * tol, 1e-6 * tol)
        if got_gx is not None:
            bd.close('gx', got_gx, gx, 2e-3 * tol, 2e-5 * gscale * tol + 1e-9)
        bd.close('loss', got_loss, loss, 0.0, 2e-5 * tol * max(1.0, abs(loss)))
        bd.close('table', tab, rows64, 1e-5 * tt, 2e-7 * tt)
        for k in DENSE:
            bd.close(k, d[k], p64[k], 1e-5 * tol, 1e-3 * lr * np.abs(g[k]).max() * tol + 1e-7)
        bd.close('b3', d['b3'], p64['b3'], 0.0, 1e-5 * tol)


def check_step(eng, prob, lr, lam1, lamfm, prec='f32', acti='tanh', b_size=0, label=''):
    """test_gpu_parity._check_step for any shape, at its bounds (f32: tol 1; bf16x3: tol 8, table 40; bf16: the bounds of
    test_train_step_bf16_vs_oracle): p_drop, gx, the loss, the whole table and every dense tensor."""
    rows, fo, ids, y, p, r1, r2 = prob
    rows64 = rows.astype(np.float64).copy()
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    out = eng.train_step(ids, y, r1, r2, b_size=b_size, want_p=True, want_gx=True)
    gx, loss, p_drop, g = oracle_step(rows64, p64, ids, y, r1, r2, lr, lam1, lamfm, acti, b_size=b_size if b_size > 0 else None)
    bd = Bounds()
    compare_step(bd, prec, rows, lr, out['p'].cpu().numpy(), out['loss'], eng.get_table(), eng.get_dense(),
                 (rows64, p64, gx, loss, p_drop, g), got_gx=out['gx'].cpu().numpy())
    bd.report(label)
    return rows64, p64


# ------------------------------------------------------------------------------------------------ one step, strip shapes
# F in {13, 16} x k in {1, 2, 4, 5, 12, 15}; the four hidden pairs the strip kernel is built for rotate over them, and so do the
# batch boundaries, the empty entries in fields 0 / 1 / last and a duplicate-heavy column
STRIP = [
    (13, 1, 300, 100, 257, 'empty'), (13, 2, 256, 64, 17, 'empty'), (13, 4, 319, 127, 1, ''), (13, 5, 63, 63, 257, 'dup'),
    (13, 12, 300, 100, 4096, 'empty'), (13, 15, 256, 64, 257, 'empty'),
    (16, 1, 319, 127, 257, 'dup'), (16, 2, 63, 63, 257, 'empty'), (16, 4, 300, 100, 17, 'empty'), (16, 5, 256, 64, 4096, 'dup'),
    (16, 12, 319, 127, 257, 'empty'), (16, 15, 63, 63, 1, 'empty'),
]


def _kw(kind, B, F):
    return {'empty': {'empty': edge_empties(B, F)}, 'dup': {'dup_col': F - 1, 'empty': [(B - 1, 0)]}, '': {}}[kind]


@pytest.mark.parametrize("F,K,H1,H2,B,kind", STRIP, ids=[case_id(*c) for c in STRIP])
def test_strip_shape_step_f32_both_paths(built, monkeypatch, F, K, H1, H2, B, kind):
    """One f32 step through the strip kernel and again with FNN_NO_FUSE=1 (the layer-by-layer kernels): both against the
    oracle, and against each other as tightly as test_layer_by_layer_path_matches_strip_kernel asserts."""
    assert path_of(F, H1, H2) == 'strip'
    prob = make_problem(F, K, H1, H2, B, seed=F * 100 + K, **_kw(kind, B, F))
    rows, fo, ids, y, p, r1, r2 = prob
    outs = []
    for nofuse in (None, '1'):
        if nofuse is None:
            monkeypatch.delenv('FNN_NO_FUSE', raising=False)
        else:
            monkeypatch.setenv('FNN_NO_FUSE', nofuse)
        eng = make_engine(F, K, H1, H2, rows, fo, p, lr=lr_for(B))
        try:
            check_step(eng, prob, lr_for(B), 0.02, 0.1, label=case_id(F, K, H1, H2, B, kind, 'f32', 'nofuse' if nofuse else 'fused'))
            outs.append((eng.get_table(), eng.get_dense(), eng.predict(ids).cpu().numpy()))
        finally:
            eng.close()
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-6)
    for k in DENSE:
        np.testing.assert_allclose(outs[0][1][k], outs[1][1][k], rtol=1e-5, atol=1e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ one step, any shape
# (F, K, H1, H2, B, precision, activation, kind, max_batch, b_size)
STEP = []
for _i, (_F, _K) in enumerate([(f, k) for f in (2, 3, 12, 17, 39, 64) for k in (1, 11, 15)]):   # field counts x ranks
    STEP.append((_F, _K, 300, 100, (1, 17, 257)[_i % 3], 'f32', 'tanh', ('empty', 'dup', 'empty')[_i % 3], 4096, 0))
STEP += [                                                                   # hidden sizes, paired
    (12, 4, 1, 1, 257, 'f32', 'tanh', 'empty', 4096, 0),
    (16, 11, 64, 63, 257, 'f32', 'tanh', 'dup', 4096, 0),
    (17, 3, 65, 64, 17, 'f32', 'tanh', 'empty', 4096, 0),
    (13, 7, 255, 65, 257, 'f32', 'tanh', 'empty', 4096, 0),
    (16, 15, 320, 128, 257, 'f32', 'tanh', 'dup', 4096, 0),
    (39, 2, 500, 255, 257, 'f32', 'tanh', 'empty', 4096, 0),
    (64, 15, 4095, 255, 257, 'f32', 'tanh', 'empty', 4096, 0),              # the longest reductions: F k = 960, H1 = 4095
    (16, 11, 4095, 1, 17, 'f32', 'tanh', '', 4096, 0),
]
STEP += [                                                                   # batches: 4096, above 4096, a global b_size
    (39, 11, 300, 100, 4096, 'f32', 'tanh', 'dup', 4096, 0),
    (17, 15, 300, 100, 5000, 'f32', 'tanh', 'empty', 8192, 0),
    (3, 15, 65, 64, 257, 'f32', 'tanh', 'empty', 4096, 264),
]
STEP += [                                                                   # activations, on a strip shape with k != 11 and a layer shape
    (F_, K_, H1_, H2_, 257, 'f32', a, 'empty', 4096, 0) for (F_, K_, H1_, H2_) in ((13, 15, 256, 64), (39, 4, 65, 64))
    for a in ('tanh', 'sigmoid', 'linear')
]
STEP += [                                                                   # bf16x3 (16-bit pairs) at the random sweep's bounds
    (13, 1, 300, 100, 257, 'bf16x3', 'tanh', 'empty', 4096, 0),
    (16, 15, 319, 127, 257, 'bf16x3', 'sigmoid', 'dup', 4096, 0),
    (13, 5, 63, 63, 17, 'bf16x3', 'tanh', 'empty', 4096, 0),
    (2, 1, 300, 100, 257, 'bf16x3', 'tanh', 'empty', 4096, 0),
    (64, 15, 300, 100, 257, 'bf16x3', 'linear', 'empty', 4096, 0),
    (17, 11, 500, 255, 4096, 'bf16x3', 'tanh', 'dup', 4096, 0),
]
STEP += [                                                                   # bf16 at test_train_step_bf16_vs_oracle's bounds
    (16, 1, 300, 100, 512, 'bf16', 'tanh', 'dup', 4096, 0),
    (13, 5, 63, 63, 512, 'bf16', 'tanh', 'empty', 4096, 0),
    (39, 15, 500, 255, 512, 'bf16', 'tanh', 'empty', 4096, 0),
]


@pytest.mark.parametrize("F,K,H1,H2,B,prec,acti,kind,max_batch,b_size", STEP,
                         ids=[case_id(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], 'bs%d' % c[9] if c[9] else '') for c in STEP])
def test_shape_step_vs_oracle(built, monkeypatch, F, K, H1, H2, B, prec, acti, kind, max_batch, b_size):
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    prob = make_problem(F, K, H1, H2, B, seed=7 * F + K + B, **_kw(kind, B, F))
    rows, fo, ids, y, p, r1, r2 = prob
    eng = make_engine(F, K, H1, H2, rows, fo, p, prec=prec, acti=acti, max_batch=max_batch, lr=lr_for(B))
    try:
        check_step(eng, prob, lr_for(B), 0.02, 0.1, prec=prec, acti=acti, b_size=b_size,
                   label=case_id(F, K, H1, H2, B, kind, prec, acti))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ state across steps
MULTI = [(16, 1, 300, 100), (13, 15, 300, 100), (39, 5, 500, 65)]


@pytest.mark.parametrize("F,K,H1,H2", MULTI, ids=[case_id(*c) for c in MULTI])
def test_multi_step_sequence_with_prefetch(built, F, K, H1, H2):
    """Five consecutive f32 steps, the middle ones announcing the next batch (fnn_prefetch_ids), against the oracle's steps
    (as test_multi_step_sequence_f32): a pad slot, the w_0 slot or the ones slot leaking into the table or into w1's pad rows
    shows in the later steps' losses, the table, the dense tensors and the predictions."""
    import torch
    steps, B = 5, 200
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, steps * B, seed=K + 60, dup_col=2,
                                               empty=edge_empties(steps * B, F))
    eng = make_engine(F, K, H1, H2, rows, fo, p, lr=0.002, lam1=0.0, lamfm=0.1)
    rows64 = rows.astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    ms = orc.TheanoMaskStream(H1, H2, 0.5)
    dev_ids = [torch.as_tensor(ids[j * B:(j + 1) * B]).to(eng.device).contiguous() for j in range(steps)]
    try:
        for j in range(steps):
            sl = slice(j * B, (j + 1) * B)
            if 1 <= j < steps - 1:
                eng.prefetch_ids(dev_ids[j + 1])
            m1, m2 = ms.next()
            out = eng.train_step(dev_ids[j], y[sl], m1.astype(np.uint8), m2.astype(np.uint8))
            _, loss, _, _ = oracle_step(rows64, p64, ids[sl], y[sl], m1, m2, 0.002, 0.0, 0.1)
            assert abs(out['loss'] - loss) <= 1e-4 * abs(loss), j
        np.testing.assert_allclose(eng.get_table(), rows64, rtol=1e-4, atol=1e-6)
        d = eng.get_dense()
        for k in DENSE:
            np.testing.assert_allclose(d[k], p64[k], rtol=1e-4, atol=1e-6, err_msg=k)
        pr = eng.predict(ids).cpu().numpy()
        np.testing.assert_allclose(pr, orc.predict(p64, orc.gather_vec(rows64, ids, -3.0)), rtol=2e-4, atol=1e-6)
    finally:
        eng.close()


def test_train_epoch_equals_the_step_loop_at_another_shape(built):
    """FNNEngine.train_epoch against the per-step loop (as test_train_epoch_equals_the_step_loop) at 13 fields, k = 15: full
    batches, a short last batch, shadowed features, a start in the middle of the epoch -- bit for bit."""
    F, K, H1, H2 = 13, 15, 300, 100
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 1030, seed=45, dup_col=5, empty=edge_empties(1030, F))
    rng = np.random.RandomState(3)
    M1 = (rng.uniform(size=(11, H1)) < 0.5).astype(np.uint8)
    M2 = (rng.uniform(size=(11, H2)) < 0.5).astype(np.uint8)
    sh = np.array([[5, fo[7], 7], [5, fo[411], 411], [250, fo[2], 2], [1029, fo[900], 900]], np.int32)
    a, b = make_engine(F, K, H1, H2, rows, fo, p), make_engine(F, K, H1, H2, rows, fo, p)
    try:
        for j in range(11):
            lo, hi = j * 100, min(1030, (j + 1) * 100)
            part = sh[(sh[:, 0] >= lo) & (sh[:, 0] < hi)].copy()
            if len(part):
                part[:, 0] -= lo
                a.set_shadowed(part)
            a.train_step(ids[lo:hi], y[lo:hi], M1[j], M2[j], b_size=hi - lo, want_loss=False)
        ids_d, y_d = b.to_device(ids, y.astype(np.int32))
        yf = y_d.float()
        b.train_epoch(ids_d, yf, 100, M1, M2, 0, 4, sh)
        b.train_epoch(ids_d, yf, 100, M1, M2, 4, None, sh)
        da, db = a.get_dense(), b.get_dense()
        bad = [k for k in da if not np.array_equal(da[k], db[k])]
        assert not bad and np.array_equal(a.get_table(), b.get_table()), bad
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ boundaries, bit-exact
ROUND = [(2, 1, 65, 3), (2, 15, 65, 3), (64, 1, 65, 3), (64, 15, 65, 3)]


@pytest.mark.parametrize("F,K,H1,H2", ROUND, ids=[case_id(*c) for c in ROUND])
def test_set_get_roundtrip_bit_exact(built, F, K, H1, H2):
    """fnn_set_dense / fnn_get_dense remap w1 between the reference's 1 + F k rows and the padded F x 16 layout (w1[0, :] on
    row k, b1 on row 16 + k); fnn_set_table / fnn_get_table / fnn_get_rows keep k of the 16 floats: all bit for bit."""
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 8, seed=F + K)
    eng = make_engine(F, K, H1, H2, rows, fo, p)
    try:
        assert np.array_equal(eng.get_table(), rows)
        sel = np.array([rows.shape[0] - 1, 0, rows.shape[0] // 2, 1])
        assert np.array_equal(eng.get_rows(sel), rows[sel])
        d = eng.get_dense()
        for k in DENSE:
            assert np.array_equal(d[k], p[k].astype(np.float32)), k
        assert d['b3'] == np.float32(p['b3'])
    finally:
        eng.close()


GATHER = [(2, 1, 300, 100), (64, 15, 300, 100), (13, 5, 300, 100)]


@pytest.mark.parametrize("F,K,H1,H2", GATHER, ids=[case_id(*c) for c in GATHER])
def test_gather_beyond_max_batch_exact(built, F, K, H1, H2):
    """fnn_gather (k_gather_ref: the reference-layout tile, 65,600 bytes of LDS at 64 fields x k = 15) against orc.gather, for
    1000 examples on a handle of max_batch 256: device pointers in one launch, host pointers in max_batch chunks."""
    import ctypes as C
    B = 1000
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, B, seed=4, empty=edge_empties(B, F))
    eng = make_engine(F, K, H1, H2, rows, fo, p, max_batch=256)
    try:
        ref = orc.gather(rows.astype(np.float64), ids, -3.0).astype(np.float32)
        assert np.array_equal(eng.gather(ids).cpu().numpy(), ref)
        x = np.empty((B, 1 + F * K), np.float32)
        ids32 = np.ascontiguousarray(ids, np.int32)
        rc = eng.lib.fnn_gather(eng.h, ids32.ctypes.data_as(C.c_void_p), B, x.ctypes.data_as(C.c_void_p), _capi.FNN_MEM_HOST)
        assert rc == 0 and np.array_equal(x, ref)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ predict and evaluate
PRED = [(13, 2, 256, 64), (64, 15, 65, 64)]


@pytest.mark.parametrize("acti", ['tanh', 'sigmoid', 'linear'])
@pytest.mark.parametrize("F,K,H1,H2", PRED, ids=[case_id(*c) for c in PRED])
def test_predict_vs_oracle(built, F, K, H1, H2, acti):
    """fnn_predict (acti_type on both hidden layers, no masks) against orc.predict on the engine's own state after a step,
    for 1000 examples on a handle of max_batch 256 (predict walks max_batch chunks), at the bounds of test_other_activations."""
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 1000, seed=12 + K, empty=edge_empties(1000, F))
    eng = make_engine(F, K, H1, H2, rows, fo, p, acti=acti, max_batch=256)
    try:
        eng.train_step(ids[:200], y[:200], r1, r2)
        pr = eng.predict(ids).cpu().numpy()
        d = {k: (f32r(v) if isinstance(v, np.ndarray) else v) for k, v in eng.get_dense().items()}
        ref = orc.predict(d, orc.gather_vec(eng.get_table().astype(np.float64), ids, -3.0), acti)
        np.testing.assert_allclose(pr, ref, rtol=1e-4, atol=1e-6)
    finally:
        eng.close()


def test_eval_metrics_equal_sklearn_at_39_fields(built):
    """fnn_eval on a layer shape (39 fields, k = 11, hidden 500 / 255): 9,001 examples in three max_batch chunks with tie
    groups, AUC / RMSE / logloss against sklearn on the same float32 predictions at 1e-12 (test_eval_metrics_equal_sklearn)."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    F, K, H1, H2 = 39, 11, 500, 255
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 3000, seed=78)
    p['w3'] = f32r(np.random.RandomState(5).uniform(-0.5, 0.5, H2))
    ids = np.concatenate([ids, ids, ids, ids[:1]])
    yy = (np.random.RandomState(6).uniform(size=len(ids)) < 0.3).astype(np.int32)
    eng = make_engine(F, K, H1, H2, rows, fo, p)
    try:
        m = eng.evaluate(ids, yy, want_p=True)
        pp = m['p'].cpu().numpy()
        np.testing.assert_array_equal(pp, eng.predict(ids).cpu().numpy())
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ FNN.py at another FM rank
def test_fnn_script_at_fm_rank_4(built, tmp_path, monkeypatch):
    """FNN.py takes k from the FM model file (python/FNN_wnzh.py:66-76): a demo set of rank 4 (k = 5, the strip kernel at
    16 fields) through `mod.run` for two f32 epochs; test AUC and logloss per epoch within 1e-4 of the oracle's run of the same
    flow (orc.run_epochs with the arguments tests/golden/make_golden.py passes for epoch.npz)."""
    import importlib.util
    from deep_ctr_amd import dl_utils
    n_train = 1200
    demo = synth.make_demo(str(tmp_path / 'demo'), n_train=n_train, n_test=400, n_feat=1000, rank=4, seed=20261015, w0=-3.0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('DEEPCTR_DATA_DIR', str(tmp_path / 'demo'))
    monkeypatch.setenv('DEEPCTR_EPOCHS', '2')
    monkeypatch.delenv('DEEPCTR_PRECISION', raising=False)
    monkeypatch.setattr(dl_utils, 'log_path', str(tmp_path / 'log'))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('fnn_script_rank4', os.path.join(root, 'deep-ctr_amd', 'FNN.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.run(['FNN.py'])
    F, K, H1, H2 = 16, 5, 300, 100
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    ids, yl = demo['ids'], demo['y']
    ref = orc.run_epochs(p, demo['rows'].astype(np.float64), demo['w0'], ids[:n_train], yl[:n_train], ids[n_train:],
                         yl[n_train:], 100, 0.001, 0.0, 0.1, 0.5, 2, H1, H2)
    assert len(hist) == len(ref) == 2
    for h, r in zip(hist, ref):
        assert abs(h['test_auc'] - r['test_auc']) <= 1e-4
        assert abs(h['test_logloss'] - r['test_logloss']) <= 1e-4


# ------------------------------------------------------------------------------------------------ data parallelism
def test_virtual_two_rank_dp_at_13_fields_k5(built):
    """Two engines stand for two ranks (as test_virtual_two_rank_dp_equals_single_gpu_dense) on the strip shape 13 fields,
    k = 5: the flat bucket's layout follows K1p / H1p / H2p; dense tensors equal the single-engine full-batch step."""
    import torch
    F, K, H1, H2 = 13, 5, 300, 100
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 512, seed=42, dup_col=6, empty=edge_empties(512, F))
    kw = dict(lr=0.01, lam1=0.05, lamfm=0.1)
    full = make_engine(F, K, H1, H2, rows, fo, p, **kw)
    full.train_step(ids, y, r1, r2)
    ref_dense, ref_rows = full.get_dense(), full.get_table()
    full.close()
    ranks = [make_engine(F, K, H1, H2, rows, fo, p, **kw) for _ in range(2)]
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
                assert np.abs(d[k] - ref_dense[k]).max() <= 2e-4 * scale + 1e-7, k
            assert abs(d['b3'] - ref_dense['b3']) < 1e-6
        t0, t1 = set(np.unique(ids[halves[0]])), set(np.unique(ids[halves[1]]))
        only0, only1 = np.array(sorted(t0 - t1 - {-1})), np.array(sorted(t1 - t0 - {-1}))
        np.testing.assert_allclose(ranks[0].get_rows(only0), ref_rows[only0], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(ranks[1].get_rows(only1), ref_rows[only1], rtol=1e-5, atol=2e-7)
        assert np.array_equal(ranks[0].get_rows(only1), rows[only1])
    finally:
        for e in ranks:
            e.close()
