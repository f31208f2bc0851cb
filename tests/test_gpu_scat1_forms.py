"""Level 1 of the sparse-row update on 16-float rows has two forms: scat1q_body (a thread per 16-byte quarter-column of a chunk
of 16 sorted entries; the default) and scat1_body (a lane per slot; FNN_SCAT1_FORM=slot).  They fold every slot's entries in the
same order with the same f64 operations, so they must agree bit for bit -- and the default one must track the float64 oracle
and repeat itself.

The ids are hand-built so that every kind of chunk occurs in a batch of 40 (the rest of the field's sorted keys are dead):
  field A  one row for all 40 examples: its segment [0, 40) opens in chunk 0, passes wholly through chunk 1 and ends in the
           middle of chunk 2 -- both kinds of partial sum and one registered owner;
  field B  three rows hit 16 / 8 / 16 times: a segment that is exactly a chunk, one that is exactly the first sub-batch of 8
           of chunk 1, one that straddles chunks 1 | 2;
  field C  distinct rows, two pairs of which one straddles the 8 | 8 border inside chunk 0, and three ids of -1.
Run at 3 fields (the layer-by-layer kernels: standalone k_scat1 over 256 keys per field) and as the first three of 16 fields
(the three-launch step: the scatter role of k_step2 over 4096 keys per field), at K = 4, 5, 11, 15 live slots per row (last
quarter full, one live lane, three live lanes, four quarters), in f32 and bf16, with and without fnn_prefetch_ids.
fnn_create takes K = rank + 1 up to 15 on 16-float rows (two pad slots carry w_0 and the bias), so rows with all 16 slots
live (rank 15) run through FM pre-training, which shares k_scat1: plain SGD and Adam (the sums land in the gradient store).
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine

gpu = pytest.mark.gpu

B = 40
SIZES3 = [5, 7, 60]                                             # rows of fields A, B, C
SIZES16 = SIZES3 + [11, 4, 70, 9, 4, 7, 24, 20, 30, 35, 12, 5, 15]
KS = [4, 5, 11, 15]
LR, LAM1, LAMFM, W0 = 0.01, 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def hand_ids(F, seed):
    """ids int32 [40, F]: fields 0..2 as the module docstring says (which example holds which entry is drawn from `seed`),
    further fields zipf-distributed."""
    sizes = SIZES3 if F == 3 else SIZES16
    rng = np.random.RandomState(seed)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 100)
    offA, offB, offC = 0, SIZES3[0], SIZES3[0] + SIZES3[1]
    ids[:, 0] = offA + 3
    colB = np.repeat([offB + 1, offB + 2, offB + 5], [16, 8, 16])
    ids[:, 1] = colB[rng.permutation(B)]
    distinct = np.sort(rng.choice(SIZES3[2], size=35, replace=False)) + offC
    sortedC = []
    for r in distinct:                                          # sorted positions 7, 8 and 18, 19 hold a pair each
        sortedC.append(r)
        if len(sortedC) in (8, 19):
            sortedC.append(r)
    assert len(sortedC) == 37
    colC = np.array(sortedC + [-1, -1, -1], np.int32)
    ids[:, 2] = colC[rng.permutation(B)]
    return ids


def segments(col):
    """[s, e) of every row's run in the field's sorted order (ids of -1 sort to the end and are dropped)."""
    v = np.sort(col[col >= 0])
    cut = np.flatnonzero(np.diff(v)) + 1
    return list(zip(np.r_[0, cut], np.r_[cut, len(v)]))


def test_hand_built_ids_have_the_layout_the_cases_rely_on():
    for F in (3, 16):
        for seed in (1, 2):
            ids = hand_ids(F, seed)
            assert segments(ids[:, 0]) == [(0, 40)]
            assert segments(ids[:, 1]) == [(0, 16), (16, 24), (24, 40)]
            segC = segments(ids[:, 2])
            assert (7, 9) in segC and (18, 20) in segC and len(segC) == 35 and (ids[:, 2] < 0).sum() == 3
            fo = synth.field_of_row(SIZES3 if F == 3 else SIZES16)
            for f in range(F):
                live = ids[:, f][ids[:, f] >= 0]
                assert np.all(fo[live] == f)


def make_problem(F, K, seed=5):
    sizes = SIZES3 if F == 3 else SIZES16
    H1, H2 = (20, 10) if F == 3 else (300, 100)
    rows = synth.fm_table(sum(sizes), K, 0.05, seed)
    fo = synth.field_of_row(sizes)
    rng = np.random.RandomState(seed + 2)
    y = (rng.uniform(size=(2, B)) < 0.3).astype(np.float32)
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p['w3'] = rng.uniform(-0.2, 0.2, H2)
    p['b1'] = rng.uniform(-0.1, 0.1, H1)
    p['b2'] = rng.uniform(-0.1, 0.1, H2)
    p['b3'] = 0.05
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
    r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
    r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
    r1[0] = r2[0] = 1
    ids = [hand_ids(F, 1), hand_ids(F, 2)]
    return dict(F=F, K=K, H1=H1, H2=H2, rows=rows, fo=fo, ids=ids, y=y, p=p, r1=r1, r2=r2)


def slot_splitk(F, prec):
    """fnn_create ties the default split-K of the weight gradients to the form on handles that take the three-launch step
    (16 fields here): 8 beside the quarter-column role in f32 and bf16, 4 otherwise.  The slices change the summation order of
    the dense gradients, so the slot arm runs at the split-K the default arm chooses by itself: the arms differ in the
    scatter body only."""
    return '8' if F == 16 and prec in ('f32', 'bf16') else None


def run(monkeypatch, pb, form, prec, prefetch=False, no_fuse=False, shadow=None, steps=2, splitk=None):
    """`steps` training steps (the second consumes the rows the first wrote) -> (table, dense tensors)."""
    import torch
    if splitk is None:
        monkeypatch.delenv('FNN_SPLITK', raising=False)
    else:
        monkeypatch.setenv('FNN_SPLITK', splitk)
    if form is None:
        monkeypatch.delenv('FNN_SCAT1_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
    if no_fuse:
        monkeypatch.setenv('FNN_NO_FUSE', '1')
    else:
        monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    eng = FNNEngine(pb['F'], pb['K'], pb['H1'], pb['H2'], max_batch=256, precision=prec, lr=LR, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids']]
        for s in range(steps):
            if prefetch and s + 1 < steps:
                eng.prefetch_ids(dev_ids[s + 1])
            if shadow is not None:
                eng.set_shadowed(shadow)
            eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_loss=False)
        eng.sync()
        return eng.get_table(), eng.get_dense()
    finally:
        eng.close()


def assert_same_bits(a, b):
    assert np.array_equal(a[0], b[0]), "table: %d of %d floats differ" % ((a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[1]['b3'] == b[1]['b3']


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("F", [3, 16])
def test_forms_are_bit_identical(built, monkeypatch, F, K, prec, prefetch):
    pb = make_problem(F, K)
    slot = run(monkeypatch, pb, 'slot', prec, prefetch, splitk=slot_splitk(F, prec))
    quarter = run(monkeypatch, pb, None, prec, prefetch)          # the default
    assert not np.array_equal(quarter[0], pb['rows'])             # the steps did move the rows
    assert_same_bits(slot, quarter)


@gpu
@pytest.mark.parametrize("F", [3, 16])
def test_forms_are_bit_identical_layer_by_layer(built, monkeypatch, F):
    """FNN_NO_FUSE=1: standalone k_scat1 over the batch's own N2 = 256 keys per field."""
    pb = make_problem(F, 11)
    slot = run(monkeypatch, pb, 'slot', 'f32', no_fuse=True)
    quarter = run(monkeypatch, pb, 'quarter', 'f32', no_fuse=True)
    assert_same_bits(slot, quarter)


@gpu
@pytest.mark.parametrize("F", [3, 16])
def test_forms_are_bit_identical_with_shadowed_features(built, monkeypatch, F):
    """A shadowed-feature list: (row, t) keys behind the B regular ones, which lengthen field A's and field B's segments
    and add rows to field C."""
    offB, offC = SIZES3[0], SIZES3[0] + SIZES3[1]
    shadow = np.array([(3, 0, 3), (3, 0, 1), (5, 1, offB + 2), (9, 1, offB + 5), (9, 2, offC + 59), (11, 2, offC + 0),
                       (39, 0, 3), (39, 2, offC + 59)], np.int32)
    pb = make_problem(F, 11)
    slot = run(monkeypatch, pb, 'slot', 'f32', shadow=shadow, splitk=slot_splitk(F, 'f32'))
    quarter = run(monkeypatch, pb, None, 'f32', shadow=shadow)
    plain = run(monkeypatch, pb, None, 'f32')
    assert not np.array_equal(plain[0], quarter[0])               # the list was used
    assert_same_bits(slot, quarter)


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("F", [3, 16])
def test_quarter_form_vs_oracle(built, monkeypatch, F, K):
    """One f32 step of the default form against the float64 oracle, the table at the bounds of
    tests/test_gpu_parity.py::_check_step (rtol 1e-5, atol 2e-7)."""
    pb = make_problem(F, K)
    table, dense = run(monkeypatch, pb, None, 'f32', steps=1)
    rows64 = pb['rows'].astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pb['p'].items()}
    ids, y = pb['ids'][0], pb['y'][0]
    x = orc.gather_vec(rows64, ids, W0)
    gx, _, loss, p_drop, g = orc.train_call(p64, x, y.astype(np.float64), pb['r1'].astype(np.float64),
                                            pb['r2'].astype(np.float64), LR, LAM1, 'tanh')
    orc.scatter_sgd_vec(rows64, ids, gx, LR, LAMFM, None)
    err = np.abs(table - rows64) / (2e-7 + 1e-5 * np.abs(rows64))
    print("F=%d K=%d: worst table error %.3g of its bound" % (F, K, err.max()))
    np.testing.assert_allclose(table, rows64, rtol=1e-5, atol=2e-7)
    for k in DENSE:
        gs = LR * np.abs(g[k]).max()
        np.testing.assert_allclose(dense[k], p64[k], rtol=1e-5, atol=1e-3 * gs + 1e-7, err_msg=k)


@gpu
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_quarter_form_repeats_itself(built, monkeypatch, prec):
    pb = make_problem(16, 11)
    a = run(monkeypatch, pb, None, prec, prefetch=True)
    b = run(monkeypatch, pb, None, prec, prefetch=True)
    assert_same_bits(a, b)


@gpu
@pytest.mark.parametrize("opt", [['sgd', 0.05], ['adam', 0.01, 1e-8]], ids=['sgd', 'adam'])
def test_forms_are_bit_identical_all_16_slots_live(built, monkeypatch, opt):
    """K = 16 (rank 15): every lane of all four quarters is live.  FM pre-training on the hand-built ids, two steps."""
    from deep_ctr_amd.FM import FM
    n_rows = sum(SIZES3)
    rows = synth.fm_table(n_rows, 16, 0.05, 3)
    y = (np.random.RandomState(4).uniform(size=(2, B)) < 0.3).astype(np.float32)
    ids = [hand_ids(3, 1), hand_ids(3, 2)]
    res = []
    for form in ('slot', 'quarter'):
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
        m = FM(B, [n_rows, 3, 15], ['uniform', -0.001, 0.001, [1, 2], None], opt, [0.01], 'train', 0)
        try:
            m.set_params(rows, 0.1)
            for s in range(2):
                m.train_step(ids[s], y[s], want_loss=False)
            res.append(m.get_params())
        finally:
            m.close()
    assert not np.array_equal(res[1][0], rows)
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
