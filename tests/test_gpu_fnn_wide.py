"""The FNN step on wide FM rows: FNN_MODE_FM with k = rank + 1 in 17..128 (ranks 16..127, the reference's FM50 / FM100 models,
python/baseline.py:77-93, read by python/FNN_wnzh.py:66-78), against oracle/fnn_oracle.py in all three precisions.

Wide handles keep rows of rw = rup(k, 4) floats; x' holds field f at columns f*rw.., w_0 at column F*rw and the ones column
that carries b1 at F*rw + 1, and every step takes the layer-by-layer kernels (k_gather_wide, the generic GEMMs, the decayed
wide row update k_scatdw1 / k_scatdw2).  Pad lanes, the w_0 column and the ones column only go wrong visibly on a LATER step
or in the host remap of w1, hence the multi-step and bit-exact round-trip tests beside the one-step checks.

Bounds: the one-step checks are test_gpu_shapes.check_step itself, at that file's bounds for each precision, unwidened.  The
longer layer-one contraction (F k up to 3,939 terms against 176 at the default shape) does not grow the magnitudes those bounds
were set for: the rows keep the standard deviation 0.05 of every other test, and the Glorot init of w1 (python/FNN_wnzh.py:
106-130, scale sqrt(6 / (1 + F k + H1))) shrinks w1 as F k grows, so the pre-activations keep a spread of 0.2..0.3 at every k
(0.17 at the default shape).  Each case prints its worst error as a fraction of its bound.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNEngine, FNNError

from test_gpu_shapes import DENSE, check_step, edge_empties, f32r, lr_for, make_engine, make_problem, oracle_step

pytestmark = pytest.mark.gpu


def rup(a, m):
    return (a + m - 1) // m * m


def cid(F, K, H1, H2, B=None, prec=None):
    s = 'F%d-K%d-pad%d-H%dx%d' % (F, K, rup(K, 4) - K, H1, H2)
    if B is not None:
        s += '-B%d' % B
    return s + ('-' + prec if prec else '')


# ------------------------------------------------------------------------------------------------ one step
# (F, K, H1, H2, B, precision): every k of {17, 20, 51, 101, 128} (pad widths 3, 0, 1, 3, 0), both field counts, every
# precision, and B = 4096 at the largest shape (39 x 101: F * rw = 4056) in all three precisions
STEP = [
    (16, 17, 300, 100, 100, 'f32'), (39, 17, 300, 100, 1, 'bf16'), (16, 17, 64, 63, 4096, 'bf16x3'),
    (16, 20, 300, 100, 4096, 'f32'), (39, 20, 300, 100, 100, 'bf16x3'),
    (39, 51, 300, 100, 100, 'f32'), (16, 51, 300, 100, 1, 'bf16x3'), (16, 51, 300, 100, 100, 'bf16'),
    (39, 101, 300, 100, 4096, 'f32'), (39, 101, 300, 100, 4096, 'bf16'), (39, 101, 300, 100, 4096, 'bf16x3'),
    (16, 101, 300, 100, 100, 'f32'), (16, 101, 500, 255, 100, 'bf16'),
    (16, 128, 300, 100, 100, 'f32'), (16, 128, 300, 100, 4096, 'bf16x3'), (16, 128, 300, 100, 1, 'bf16'),
]


@pytest.mark.parametrize("F,K,H1,H2,B,prec", STEP, ids=[cid(*c) for c in STEP])
def test_wide_step_vs_oracle(built, F, K, H1, H2, B, prec):
    """One step (p_drop, gx in the reference layout, the loss, the whole table, the dense tensors) on Zipf ids -- rows repeat
    inside a field, at B = 4096 in runs of hundreds of entries, far longer than a WCH = 32 chunk of the row update -- with empty
    entries in field 0 (w_0's neighbour), field 1 and the last field."""
    prob = make_problem(F, K, H1, H2, B, seed=3 * F + K + B, empty=edge_empties(B, F))
    eng = make_engine(F, K, H1, H2, prob[0], prob[1], prob[4], prec=prec, lr=lr_for(B))
    try:
        check_step(eng, prob, lr_for(B), 0.02, 0.1, prec=prec, label=cid(F, K, H1, H2, B, prec))
    finally:
        eng.close()


# (F, K, H1, H2, B, precision, max_batch): above 4096 keys per field -- N2 = 8192 (k_sort<8>, 256 chunks of the row update per
# field) and 16384 (k_sort<16>, 512 chunks), and the generic GEMMs on a wide K1p with more than 4096 rows
STEP_ABOVE_4096 = [(16, 51, 300, 100, 5000, 'f32', 8192), (3, 128, 64, 63, 9000, 'bf16x3', 16384)]


@pytest.mark.parametrize("F,K,H1,H2,B,prec,max_batch", STEP_ABOVE_4096, ids=[cid(*c[:6]) + '-of-%d' % c[6] for c in STEP_ABOVE_4096])
def test_wide_step_above_4096_keys_vs_oracle(built, F, K, H1, H2, B, prec, max_batch):
    """test_wide_step_vs_oracle's check (check_step at its bounds for the precision) on 5000 and 9000 examples."""
    prob = make_problem(F, K, H1, H2, B, seed=3 * F + K + B, empty=edge_empties(B, F))
    eng = make_engine(F, K, H1, H2, prob[0], prob[1], prob[4], prec=prec, max_batch=max_batch, lr=lr_for(B))
    try:
        check_step(eng, prob, lr_for(B), 0.02, 0.1, prec=prec, label=cid(F, K, H1, H2, B, prec))
    finally:
        eng.close()


def test_wide_decay_of_a_row_hit_many_times(built):
    """lambda_fm > 0 with c = 1 - 2 lambda_fm lr / b_size = 0.975: column 3 holds one row in all 200 examples (a segment over
    seven chunks of the row update, c^200 = 0.006), the Zipf columns hold runs of every length.  The table equals the
    reference's sequential loop (orc.train_step -> scatter_sgd) at f32 tolerance."""
    F, K, H1, H2, B = 16, 51, 300, 100, 200
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, B, seed=5, dup_col=3, empty=edge_empties(B, F))
    lr, lamfm, bs = 0.01, 5.0, 4
    c = 1 - 2 * lamfm * lr / bs
    assert c ** B < 0.01
    eng = make_engine(F, K, H1, H2, rows, fo, p, lr=lr, lam1=0.0, lamfm=lamfm)
    try:
        out = eng.train_step(ids, y, r1, r2, b_size=bs)
        rows64 = rows.astype(np.float64)
        p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        ref = orc.train_step(p64, rows64, -3.0, ids, y.astype(np.float64), r1.astype(float), r2.astype(float), lr, 0.0, lamfm,
                             b_size=bs)
        assert abs(out['loss'] - ref['loss']) <= 2e-5 * abs(ref['loss'])
        got = eng.get_table()
        np.testing.assert_allclose(got, rows64, rtol=1e-5, atol=2e-7)
        # the decay is live: the same gradients without it (lambda_fm = 0) leave that row far outside the tolerance
        r = ids[0, 3]
        nodecay = orc.scatter_sgd(rows.astype(np.float64), ids, ref['gx'], lr, 0.0, bs)
        assert np.abs(nodecay[r] - rows64[r]).max() > 1e3 * (2e-7 + 1e-5 * np.abs(rows64[r]).max())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ state across steps
MULTI = [(16, 51, 300, 100, 'f32'), (39, 101, 300, 100, 'f32'), (16, 128, 64, 63, 'f32'), (16, 17, 300, 100, 'bf16x3')]


@pytest.mark.parametrize("F,K,H1,H2,prec", MULTI, ids=[cid(c[0], c[1], c[2], c[3], None, c[4]) for c in MULTI])
def test_wide_multi_step_sequence_with_prefetch(built, F, K, H1, H2, prec):
    """Five consecutive steps, the middle ones announcing the next batch (fnn_prefetch_ids), against the oracle's steps (as
    test_gpu_shapes.test_multi_step_sequence_with_prefetch): a pad lane, the w_0 column or the ones column leaking into the
    table or into w1 shows in the later steps' losses, the table, the dense tensors and the predictions."""
    import torch
    steps, B = 5, 200
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, steps * B, seed=K + 60, dup_col=2,
                                               empty=edge_empties(steps * B, F))
    eng = make_engine(F, K, H1, H2, rows, fo, p, prec=prec, lr=0.002, lam1=0.0, lamfm=0.1)
    rows64 = rows.astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    ms = orc.TheanoMaskStream(H1, H2, 0.5)
    dev_ids = [torch.as_tensor(ids[j * B:(j + 1) * B]).to(eng.device).contiguous() for j in range(steps)]
    tol = 1e-4 if prec == 'f32' else 8e-4
    try:
        for j in range(steps):
            sl = slice(j * B, (j + 1) * B)
            if 1 <= j < steps - 1:
                eng.prefetch_ids(dev_ids[j + 1])
            m1, m2 = ms.next()
            out = eng.train_step(dev_ids[j], y[sl], m1.astype(np.uint8), m2.astype(np.uint8))
            _, loss, _, _ = oracle_step(rows64, p64, ids[sl], y[sl], m1, m2, 0.002, 0.0, 0.1)
            assert abs(out['loss'] - loss) <= tol * abs(loss), j
        tab = eng.get_table()
        np.testing.assert_allclose(tab, rows64, rtol=tol, atol=1e-6)
        d = eng.get_dense()
        for k in DENSE:
            np.testing.assert_allclose(d[k], p64[k], rtol=tol, atol=1e-6, err_msg=k)
        pr = eng.predict(ids).cpu().numpy()
        np.testing.assert_allclose(pr, orc.predict(p64, orc.gather_vec(rows64, ids, -3.0)), rtol=2 * tol, atol=1e-6)
    finally:
        eng.close()


def test_wide_train_epoch_equals_the_step_loop(built):
    """FNNEngine.train_epoch against the per-step loop at 16 fields, k = 51: full batches, a short last batch, shadowed
    features, a start in the middle of the epoch -- bit for bit (as test_gpu_shapes does at k = 15)."""
    F, K, H1, H2 = 16, 51, 300, 100
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


@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_wide_runs_are_bit_identical(built, prec):
    """Two engines, the same three 4096-example steps at 16 fields, k = 101: the row update has no float atomics and sums in a
    fixed order, so tables and dense tensors are bit-identical."""
    F, K, H1, H2, B = 16, 101, 300, 100, 4096
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 3 * B, seed=77, empty=edge_empties(3 * B, F))
    outs = []
    for _ in range(2):
        eng = make_engine(F, K, H1, H2, rows, fo, p, prec=prec, lr=0.001)
        try:
            for j in range(3):
                eng.train_step(ids[j * B:(j + 1) * B], y[j * B:(j + 1) * B], r1, r2, want_loss=False)
            outs.append((eng.get_table(), eng.get_dense()))
        finally:
            eng.close()
    assert not np.array_equal(outs[0][0], rows)
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


# ------------------------------------------------------------------------------------------------ layouts, bit-exact
ROUND = [(2, 17, 65, 3), (16, 20, 65, 3), (39, 101, 65, 3), (16, 128, 65, 3), (64, 64, 65, 3)]


@pytest.mark.parametrize("F,K,H1,H2", ROUND, ids=[cid(*c) for c in ROUND])
def test_wide_set_get_roundtrip_bit_exact(built, F, K, H1, H2):
    """fnn_set_dense / fnn_get_dense remap w1 between the reference's 1 + F k rows and the padded layout (row 1 + f k + l <->
    f rw + l, w1[0, :] <-> the w_0 column F rw, b1 <-> the ones column F rw + 1); fnn_set_table / fnn_get_table /
    fnn_get_rows keep k of the rw floats: all bit for bit."""
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


GATHER = [(64, 64), (39, 101), (16, 128), (16, 17)]


@pytest.mark.parametrize("F,K", GATHER, ids=['F%d-K%d' % c for c in GATHER])
def test_wide_gather_exact(built, F, K):
    """fnn_gather (k_gather_ref with rows of rw floats, 8 examples per tile: 133,152 bytes of LDS at 64 fields x k = 64, the
    largest tile the F rw <= 4096 bound admits) against orc.gather bit for bit, for 1000 examples on a handle of max_batch 256:
    device pointers in one launch, host pointers in max_batch chunks."""
    B = 1000
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, 65, 3, B, seed=4, empty=edge_empties(B, F))
    eng = make_engine(F, K, 65, 3, rows, fo, p, max_batch=256)
    try:
        ref = orc.gather(rows.astype(np.float64), ids, -3.0).astype(np.float32)
        assert np.array_equal(eng.gather(ids).cpu().numpy(), ref)
        x = np.empty((B, 1 + F * K), np.float32)
        ids32 = np.ascontiguousarray(ids, np.int32)
        rc = eng.lib.fnn_gather(eng.h, ids32.ctypes.data_as(C.c_void_p), B, x.ctypes.data_as(C.c_void_p), _capi.FNN_MEM_HOST)
        assert rc == 0 and np.array_equal(x, ref)
    finally:
        eng.close()


def test_wide_out_of_range_id_is_reported(built):
    """An id outside [-1, n_rows) raises FNN_ERR_RANGE through the error flag of the wide gather (as k_gather does)."""
    F, K, H1, H2, B = 16, 51, 300, 100, 64
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, B, seed=8)
    eng = make_engine(F, K, H1, H2, rows, fo, p)
    try:
        bad = ids.copy()
        bad[7, 4] = rows.shape[0]
        with pytest.raises(FNNError) as ei:
            eng.predict(bad).cpu()
            eng.sync()
        assert ei.value.code == _capi.FNN_ERR_RANGE
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ shadowed features
def test_wide_shadowed_features_vs_oracle(built):
    """fnn_set_shadowed on a wide handle (16 fields, k = 51): lines with 0..3 features per field, a feature listed twice, a row
    that only ever appears shadowed -- against orc.train_step_feats (the reference's update loop over every listed feature)."""
    F, K, H1, H2, B = 16, 51, 300, 100, 300
    rng = np.random.RandomState(B)
    sizes = synth.field_sizes_tiny(1000)
    offs = np.cumsum([0] + sizes[:-1])
    rows, fo, _, _, p, r1, r2 = make_problem(F, K, H1, H2, 8, seed=B)
    feats = []                                              # feature id == row id here
    for t in range(B):
        ft = []
        for f in range(F):
            n = 1 if rng.uniform() < 0.8 else int(rng.randint(0, 4))
            pick = list(offs[f] + rng.randint(0, min(sizes[f], 5), size=n))
            if n == 3 and rng.uniform() < 0.5:
                pick[2] = pick[0]
            ft += pick
        rng.shuffle(ft)
        feats.append([int(v) for v in ft])
    fbig = int(np.argmax(sizes))
    rare = int(offs[fbig] + sizes[fbig] - 1)
    feats[0] = [rare] + feats[0] + [int(offs[fbig])]
    ident = {int(r): int(r) for r in range(rows.shape[0])}
    field_of = {int(r): int(fo[r]) for r in range(rows.shape[0])}
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    lr, lam1, lamfm = 0.01, 0.0, 0.1
    rows64 = rows.astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    ref = orc.train_step_feats(p64, rows64, -3.0, feats, ident, field_of, F, y.astype(np.float64), r1.astype(float),
                               r2.astype(float), lr, lam1, lamfm)
    ids = ref['ids'].astype(np.int32)
    shadow = []
    for t, ft in enumerate(feats):
        seen = {}
        for feat in ft:
            if field_of[feat] in seen:
                shadow.append((t, field_of[feat], seen[field_of[feat]]))
            seen[field_of[feat]] = feat
    assert len(shadow) > B // 20
    eng = make_engine(F, K, H1, H2, rows, fo, p, lr=lr, lam1=lam1, lamfm=lamfm)
    try:
        eng.set_shadowed(np.asarray(shadow, np.int32))
        out = eng.train_step(ids, y, r1, r2, want_gx=True)
        got = eng.get_table()
        change = np.abs(rows64 - rows).max()
        assert np.abs(got - rows64).max() <= 3e-4 * change + 2e-7
        assert abs(out['loss'] - ref['loss']) <= 2e-5 * abs(ref['loss'])
        main_rows = set(int(v) for v in ids[ids >= 0])
        only_shadow = np.array(sorted(set(s[2] for s in shadow) - main_rows))
        assert len(only_shadow) > 0 and np.all(np.abs(got[only_shadow] - rows[only_shadow]).max(axis=1) > 0)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ data parallelism
def test_wide_virtual_two_rank_dp_split_api(built):
    """Two engines stand for two ranks of the portable split API (fnn_step_begin / the caller's all-reduce of the bucket /
    fnn_step_end) at 16 fields, k = 51, as test_gpu_shapes.test_virtual_two_rank_dp_at_13_fields_k5: dense tensors equal the
    single-engine full-batch step, rows only one rank touched equal its update, rows only the other touched stay put."""
    import torch
    F, K, H1, H2 = 16, 51, 300, 100
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
            e.step_scatter()
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


@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
def test_wide_native_dp_sparse_local(built, payload):
    """The native data-parallel step (fnn_dp_init_custom, FNN_DP_SPARSE_LOCAL) on a wide handle: the layer-by-layer path
    issues the collective of the payload in force.  One rank whose all-reduce is the identity computes exactly the
    single-process step: tables and dense tensors bit-identical after two steps."""
    F, K, H1, H2, B = 16, 51, 300, 100, 300
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 2 * B, seed=31, empty=edge_empties(2 * B, F))
    calls = []
    outs = []
    for dp in (False, True):
        eng = make_engine(F, K, H1, H2, rows, fo, p)
        try:
            if dp:
                eng.dp_init_custom(0, 1, lambda v: calls.append(v.numel()), None, sparse='local')
                eng.dp_set_payload(payload)
            for j in range(2):
                eng.train_step(ids[j * B:(j + 1) * B], y[j * B:(j + 1) * B], r1, r2, b_size=B, want_loss=False)
            eng.sync()
            outs.append((eng.get_table(), eng.get_dense()))
        finally:
            eng.close()
    assert len(calls) == 2
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


def test_wide_refuses_the_slot_layout_exchange(built):
    """FNN_DP_SPARSE_EXCHANGE, fnn_sparse_grad and fnn_step_scatter_global carry 16-float slots: a wide handle refuses them
    with FNN_ERR_ARG and a message instead of mis-indexing."""
    import torch
    F, K, H1, H2, B = 16, 51, 300, 100, 64
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, B, seed=9)
    eng = make_engine(F, K, H1, H2, rows, fo, p)
    try:
        with pytest.raises(FNNError) as ei:
            eng.dp_init_custom(0, 2, lambda v: None, lambda a, b: None, sparse='exchange')
        assert ei.value.code == _capi.FNN_ERR_ARG and 'wide rows' in str(ei.value)
        eng.step_begin(ids, y, r1, r2)
        with pytest.raises(FNNError) as ei:
            eng.sparse_grad(B)
        assert ei.value.code == _capi.FNN_ERR_ARG and 'wide rows' in str(ei.value)
        ids_g = torch.as_tensor(ids, dtype=torch.int32).to(eng.device).contiguous()
        gxp_g = torch.zeros((B, F * 52), dtype=torch.float32, device=eng.device)
        with pytest.raises(FNNError) as ei:
            eng.step_scatter_global(ids_g, gxp_g)
        assert ei.value.code == _capi.FNN_ERR_ARG and 'wide rows' in str(ei.value)
        eng.step_end()
        eng.sync()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ limits
def test_wide_create_limits(built):
    """k = 17 and 128 are accepted (and 39 fields x k = 101: F rw = 4056); k = 129 is refused; k = 16 is still refused with
    `k = rank+1` in the message; F rw above 4096 is refused with the bound in the message."""
    for F, K in ((16, 17), (16, 128), (39, 101), (64, 64)):
        FNNEngine(F, K, 300, 100, max_batch=256, precision='f32').close()
    for F, K, msg in ((16, 129, 'k = rank+1'), (16, 16, 'k = rank+1'), (40, 101, '4096'), (64, 65, '4096'),
                      (33, 128, '4096')):
        with pytest.raises(FNNError) as ei:
            FNNEngine(F, K, 300, 100, max_batch=256, precision='f32')
        assert ei.value.code == _capi.FNN_ERR_ARG and msg in str(ei.value), (F, K, str(ei.value))


# ------------------------------------------------------------------------------------------------ predict and evaluate
def test_wide_eval_equals_sklearn_and_the_oracle(built):
    """fnn_eval on a wide handle (16 fields, k = 101): 9,001 examples in three max_batch chunks with tie groups; AUC / RMSE /
    logloss against sklearn on the same float32 predictions at 1e-12, the predictions against orc.predict."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    F, K, H1, H2 = 16, 101, 300, 100
    rows, fo, ids, y, p, r1, r2 = make_problem(F, K, H1, H2, 3000, seed=78)
    p['w3'] = f32r(np.random.RandomState(5).uniform(-0.5, 0.5, H2))
    ids = np.concatenate([ids, ids, ids, ids[:1]])
    yy = (np.random.RandomState(6).uniform(size=len(ids)) < 0.3).astype(np.int32)
    eng = make_engine(F, K, H1, H2, rows, fo, p)
    try:
        m = eng.evaluate(ids, yy, want_p=True)
        pp = m['p'].cpu().numpy()
        np.testing.assert_array_equal(pp, eng.predict(ids).cpu().numpy())
        np.testing.assert_allclose(pp, orc.predict(p, orc.gather_vec(rows.astype(np.float64), ids, -3.0)), rtol=1e-4, atol=1e-6)
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ FNN.py
def _load_script(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, 'deep-ctr_amd', 'FNN.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _script_env(monkeypatch, tmp_path, data_dir, epochs, precision=None):
    from deep_ctr_amd import dl_utils
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('DEEPCTR_DATA_DIR', str(data_dir))
    monkeypatch.setenv('DEEPCTR_EPOCHS', str(epochs))
    if precision:
        monkeypatch.setenv('DEEPCTR_PRECISION', precision)
    else:
        monkeypatch.delenv('DEEPCTR_PRECISION', raising=False)
    monkeypatch.setattr(dl_utils, 'log_path', str(tmp_path / 'log'))


@pytest.mark.parametrize("rank,prec", [(50, 'f32'), (100, 'bf16x3')])
def test_fnn_script_at_wide_fm_rank(built, tmp_path, monkeypatch, rank, prec):
    """FNN.py takes k from the FM model file (python/FNN_wnzh.py:66-76): a demo set of rank 50 (k = 51) or 100 (k = 101)
    through `mod.run` for two epochs; test AUC and logloss per epoch within 1e-4 of the oracle's run of the same flow, as
    test_gpu_shapes.test_fnn_script_at_fm_rank_4."""
    n_train = 1200
    demo = synth.make_demo(str(tmp_path / 'demo'), n_train=n_train, n_test=400, n_feat=1000, rank=rank, seed=20261016, w0=-3.0)
    _script_env(monkeypatch, tmp_path, tmp_path / 'demo', 2, None if prec == 'f32' else prec)
    hist = _load_script('fnn_script_rank%d' % rank).run(['FNN.py'])
    F, K, H1, H2 = 16, rank + 1, 300, 100
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    ids, yl = demo['ids'], demo['y']
    ref = orc.run_epochs(p, demo['rows'].astype(np.float64), demo['w0'], ids[:n_train], yl[:n_train], ids[n_train:],
                         yl[n_train:], 100, 0.001, 0.0, 0.1, 0.5, 2, H1, H2)
    assert len(hist) == len(ref) == 2
    for h, r in zip(hist, ref):
        assert abs(h['test_auc'] - r['test_auc']) <= 1e-4, (h, r)
        assert abs(h['test_logloss'] - r['test_logloss']) <= 1e-4, (h, r)


def test_fm50_pretraining_feeds_the_fnn_script(built, tmp_path, monkeypatch):
    """The pipeline the wide path exists for: FM pre-training at rank 50 (FM.py, python/baseline.py's FM50) for a few steps,
    FM.write_fm_model, then FNN.py on that file.  The script trains and evaluates one epoch, within 1e-4 of orc.run_epochs
    started from the rows DataFM reads back; the first step of an FNNEngine built the way the script builds it matches
    orc.train_step from the same rows at the one-step f32 bounds."""
    from deep_ctr_amd.FM import FM
    from deep_ctr_amd.data_fm import DataFM
    n_train = 1000
    demo = synth.make_demo(str(tmp_path / 'demo'), n_train=n_train, n_test=300, n_feat=800, rank=50, seed=7, w0=-3.0)
    ids, yl = demo['ids'], demo['y']
    m = FM(100, [len(demo['rows']), 16, 50], ['uniform', -0.001, 0.001, [1, 2], None], ['sgd', 0.05], [1e-3], 'train', 0)
    m.set_params(demo['rows'], demo['w0'])
    for j in range(5):
        m.train_step(ids[j * 100:(j + 1) * 100], yl[j * 100:(j + 1) * 100].astype(np.float64), want_loss=False)
    got, _ = m.get_params()
    assert not np.array_equal(got, demo['rows'].astype(np.float32))
    names = sorted(DataFM.name_field, key=DataFM.name_field.get)
    m.write_fm_model(str(tmp_path / 'demo' / 'fm.model.txt'), demo['field_of_row'], names, demo['feat_ids'])
    m.close()
    d = DataFM(str(tmp_path / 'demo' / 'fm.model.txt'))
    assert d.k == 51
    rows, fo_row, w0 = d.table()
    tr_ids, tr_y = d.load_ids(str(tmp_path / 'demo' / 'train.fm.txt'))
    te_ids, te_y = d.load_ids(str(tmp_path / 'demo' / 'test.fm.txt'))

    _script_env(monkeypatch, tmp_path, tmp_path / 'demo', 1)
    hist = _load_script('fnn_script_fm50').run(['FNN.py'])
    F, K, H1, H2 = 16, 51, 300, 100
    p0 = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p0 = {k: (f32r(v) if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    ref = orc.run_epochs(p, np.asarray(rows, np.float64), w0, tr_ids, tr_y, te_ids, te_y, 100, 0.001, 0.0, 0.1, 0.5, 1, H1, H2)
    assert len(hist) == len(ref) == 1
    assert abs(hist[0]['test_auc'] - ref[0]['test_auc']) <= 1e-4, (hist, ref)
    assert abs(hist[0]['test_logloss'] - ref[0]['test_logloss']) <= 1e-4, (hist, ref)

    r1, r2 = orc.TheanoMaskStream(H1, H2, 0.5).next()
    y0 = tr_y[:100].astype(np.float32)
    eng = FNNEngine(F, K, H1, H2, max_batch=4096, precision='f32', lr=0.001, lambda1=0.0, lambda_fm=0.1)
    try:
        eng.set_table(rows, fo_row, w0)
        eng.set_dense(p0)
        rows64 = np.asarray(rows, np.float64).copy()
        pp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
        out = eng.train_step(tr_ids[:100], y0, r1.astype(np.uint8), r2.astype(np.uint8), want_p=True)
        st = orc.train_step(pp, rows64, w0, tr_ids[:100], y0.astype(np.float64), r1.astype(float), r2.astype(float), 0.001, 0.0,
                            0.1)
        np.testing.assert_allclose(out['p'].cpu().numpy(), st['p_drop'], rtol=1e-4, atol=1e-6)
        assert abs(out['loss'] - st['loss']) <= 2e-5 * max(1.0, abs(st['loss']))
        np.testing.assert_allclose(eng.get_table(), rows64, rtol=1e-5, atol=2e-7)
        dd = eng.get_dense()
        for k in DENSE:
            np.testing.assert_allclose(dd[k], pp[k], rtol=1e-5, atol=1e-7 + 1e-3 * 0.001 * np.abs(st['grads'][k]).max(), err_msg=k)
    finally:
        eng.close()
