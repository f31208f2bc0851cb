"""Level 1 of the sparse-row update on 16-float rows has a third form, scat1h_body (FNN_SCAT1_FORM=half): a thread owns a 16-byte
quarter-column of one HALF of a chunk of 16 sorted entries, the upper half starts its f64 fold from the sums the lower half leaves
open (handed over between two adjacent lanes).  It folds every slot's entries in the order and with the operations of scat1q_body
(quarter) and scat1_body (slot), so the three must agree bit for bit, on the table and on every dense tensor.

The ids are hand-built so that every case of the hand-over occurs in a batch of 40 (sorted positions; chunks are [0, 16),
[16, 32), [32, 48), their halves split at 8, 24, 40):
  field A  one row for all 40 examples: [0, 40) carries a non-zero sum over the borders 8, 24 and 40, passes wholly through chunk
           1, leaves both kinds of partial sum and one registered owner;
  field B  [0, 8) ends exactly at the border (the carry is zero), [8, 16) starts at the border and closes the chunk, [16, 17) is a
           single entry, six more single entries, a pair at 23 and 24 -- and nothing else: 25 live entries and 15 ids of -1, the
           upper half of chunk 1 holds exactly one live entry, which the lower half's carry completes;
  field C  distinct rows but for a pair at 7 and 8 (the whole segment inside chunk 0, written by the upper half with the lower
           half's carry) and a pair at 15 and 16 (across a chunk border: two partial sums); 37 live entries and three ids of
           -1: the upper half of the last chunk is all dead.
Run at 16 fields (the three-launch step: the scatter role of k_step2 over 4096 keys per field) with and without
fnn_prefetch_ids, and at 3 fields (the layer-by-layer kernels: stand-alone k_scat1), at K = 4, 5, 11, 15, in f32 and bf16;
through FM pre-training at rank 15 (all 16 slots live) and through the inner-product step (which refuses ids of -1: the dead
entries become further distinct rows that sort behind the live ones).  FNN_SPLITK is the same in all arms, so that only the
scatter body differs.  One case at batch 4096 with Zipf(1.1) ids on a small table has the long multi-chunk segments of real ids.
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine

gpu = pytest.mark.gpu

B = 40
LENS_B = [8, 8, 1] + [1] * 6 + [2]                              # run lengths of field B's rows in sorted order: 25 live
LENS_C = [1] * 7 + [2] + [1] * 6 + [2] + [1] * 20               # field C: 37 live
SIZES3 = [5, len(LENS_B) + 15, len(LENS_C) + 3]                 # rows of fields A, B, C (B and C: room for rows in place of the ids of -1)
TAIL13 = [11, 4, 70, 9, 4, 7, 24, 20, 30, 35, 12, 5, 15]
SIZES16 = SIZES3 + TAIL13
ZIPF_SIZES16 = [5, 7, 60] + TAIL13                              # tests/test_gpu_scat1_forms.py's SIZES16
KS = [4, 5, 11, 15]
LR, LAM1, LAMFM, W0 = 0.01, 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
FORMS = ('half', 'quarter', 'slot')


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def column(off, lens, dead):
    """A field's 40 entries in sorted order: row off + i taken lens[i] times, then ids of -1 -- or, dead=False, further distinct
    rows behind the live ones."""
    live = np.repeat(off + np.arange(len(lens)), lens)
    n = B - len(live)
    rest = np.full(n, -1) if dead else off + len(lens) + np.arange(n)
    return np.r_[live, rest].astype(np.int32)


def hand_ids(F, seed, dead=True):
    """ids int32 [40, F]: fields 0..2 as the module docstring says (which example holds which entry is drawn from `seed`),
    further fields zipf-distributed."""
    sizes = SIZES3 if F == 3 else SIZES16
    rng = np.random.RandomState(seed)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 100)
    offB, offC = SIZES3[0], SIZES3[0] + SIZES3[1]
    ids[:, 0] = 3
    ids[:, 1] = column(offB, LENS_B, dead)[rng.permutation(B)]
    ids[:, 2] = column(offC, LENS_C, dead)[rng.permutation(B)]
    return ids


def segments(col):
    """[s, e) of every row's run in the field's sorted order (ids of -1 sort to the end and are dropped)."""
    v = np.sort(col[col >= 0])
    cut = np.flatnonzero(np.diff(v)) + 1
    return [(int(s), int(e)) for s, e in zip(np.r_[0, cut], np.r_[cut, len(v)])]


def test_hand_built_ids_have_the_layout_the_cases_rely_on():
    for F in (3, 16):
        for seed in (1, 2):
            ids = hand_ids(F, seed)
            assert segments(ids[:, 0]) == [(0, 40)]                          # over 8 | 8 borders at 8, 24, 40; through chunk 1
            segB = segments(ids[:, 1])
            assert segB[:3] == [(0, 8), (8, 16), (16, 17)]                   # zero carry; opens at the border, closes the chunk; one entry
            assert segB[-1] == (23, 25) and len(segB) == 10                  # the pair at 23, 24
            assert (ids[:, 1] >= 0).sum() == 25 and (ids[:, 1] < 0).sum() == 15   # chunk 1's upper half: one live entry (24)
            segC = segments(ids[:, 2])
            assert (7, 9) in segC and (15, 17) in segC and len(segC) == 35   # inside chunk 0 over its border; over a chunk border
            assert all(e - s == 1 for s, e in segC if (s, e) not in ((7, 9), (15, 17)))
            assert (ids[:, 2] >= 0).sum() == 37 and (ids[:, 2] < 0).sum() == 3    # [40, 48) of the last chunk is all dead
            fo = synth.field_of_row(SIZES3 if F == 3 else SIZES16)
            for f in range(F):
                live = ids[:, f][ids[:, f] >= 0]
                assert np.all(fo[live] == f)
    full = hand_ids(3, 1, dead=False)                                        # the inner-product step's ids: same runs, no -1
    assert full.min() >= 0 and np.all(synth.field_of_row(SIZES3)[full] == np.arange(3))
    assert segments(full[:, 1])[:10] == segments(hand_ids(3, 1)[:, 1]) and len(segments(full[:, 1])) == 25
    assert segments(full[:, 2])[:35] == segments(hand_ids(3, 1)[:, 2]) and len(segments(full[:, 2])) == 38


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


def run(monkeypatch, pb, form, prec, prefetch=False, steps=2, max_batch=256):
    """`steps` training steps (the second consumes the rows the first wrote) -> (table, dense tensors)."""
    import torch
    monkeypatch.setenv('FNN_SPLITK', '4')                         # the same slices in every arm: only the scatter body differs
    monkeypatch.setenv('FNN_SCAT1_FORM', form)
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    eng = FNNEngine(pb['F'], pb['K'], pb['H1'], pb['H2'], max_batch=max_batch, precision=prec, lr=LR, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids']]
        for s in range(steps):
            if prefetch and s + 1 < steps:
                eng.prefetch_ids(dev_ids[s + 1])
            eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_loss=False)
        eng.sync()
        return eng.get_table(), eng.get_dense()
    finally:
        eng.close()


def assert_same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s, table: %d of %d floats differ" % (what, (a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), (what, k)
    assert a[1]['b3'] == b[1]['b3'], what


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
@pytest.mark.parametrize("K", KS)
def test_three_forms_are_bit_identical_in_the_three_launch_step(built, monkeypatch, K, prec, prefetch):
    pb = make_problem(16, K)
    half, quarter, slot = [run(monkeypatch, pb, form, prec, prefetch) for form in FORMS]
    assert not np.array_equal(half[0], pb['rows'])                # the steps did move the rows
    assert_same_bits(half, quarter, 'half against quarter')
    assert_same_bits(half, slot, 'half against slot')


@gpu
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
@pytest.mark.parametrize("K", KS)
def test_three_forms_are_bit_identical_layer_by_layer(built, monkeypatch, K, prec):
    """3 fields: stand-alone k_scat1 over the batch's own N2 = 256 keys per field."""
    pb = make_problem(3, K)
    half, quarter, slot = [run(monkeypatch, pb, form, prec) for form in FORMS]
    assert not np.array_equal(half[0], pb['rows'])
    assert_same_bits(half, quarter, 'half against quarter')
    assert_same_bits(half, slot, 'half against slot')


@gpu
def test_three_forms_are_bit_identical_all_16_slots_live(built, monkeypatch):
    """K = 16 (rank 15): every lane of all four quarters is live.  FM pre-training (plain SGD) on the hand-built ids, two steps."""
    from deep_ctr_amd.FM import FM
    n_rows = sum(SIZES3)
    rows = synth.fm_table(n_rows, 16, 0.05, 3)
    y = (np.random.RandomState(4).uniform(size=(2, B)) < 0.3).astype(np.float32)
    ids = [hand_ids(3, 1), hand_ids(3, 2)]
    res = []
    for form in FORMS:
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
        m = FM(B, [n_rows, 3, 15], ['uniform', -0.001, 0.001, [1, 2], None], ['sgd', 0.05], [0.01], 'train', 0)
        try:
            m.set_params(rows, 0.1)
            for s in range(2):
                m.train_step(ids[s], y[s], want_loss=False)
            res.append(m.get_params())
        finally:
            m.close()
    assert not np.array_equal(res[0][0], rows)
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and res[0][1] == other[1]


@gpu
def test_three_forms_are_bit_identical_in_the_inner_product_step(built, monkeypatch):
    """FNN_IP_L3-shaped step on 3 fields, K = 11, f32, no dropout: k_scat1 on the side stream of the inner-product family."""
    from deep_ctr_amd.ipnn import IPNNEngine
    F, K, hidden = 3, 11, [30, 20]
    n_rows = sum(SIZES3)
    rng = np.random.RandomState(8)
    table = f32r(rng.standard_normal((n_rows, K)) * 0.2)
    d = [F * K + F * (F - 1) // 2 + 1] + hidden + [1]
    Ws = [f32r(rng.uniform(-0.3, 0.3, (d[i], d[i + 1]))) for i in range(len(d) - 1)]
    bs = [f32r(rng.uniform(-0.1, 0.1, d[i + 1])) for i in range(len(d) - 1)]
    y = (rng.uniform(size=(2, B)) < 0.3).astype(np.float32)
    ids = [hand_ids(3, 1, dead=False), hand_ids(3, 2, dead=False)]
    res = []
    for form in FORMS:
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
        eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=256, precision='f32', lr=0.01, keep_prob=1.0)
        try:
            eng.set_params(table, 0.1, Ws, bs)
            for s in range(2):
                eng.train_step(ids[s], y[s], None, want_loss=False)
            eng.sync()
            res.append((eng.get_rows(np.arange(n_rows)), eng.get_params()))
        finally:
            eng.close()
    assert not np.array_equal(res[0][0], table.astype(np.float32))
    for rows_o, (b_o, Ws_o, bs_o) in res[1:]:
        assert np.array_equal(res[0][0], rows_o)
        assert res[0][1][0] == b_o
        assert all(np.array_equal(a, b) for a, b in zip(res[0][1][1], Ws_o))
        assert all(np.array_equal(a, b) for a, b in zip(res[0][1][2], bs_o))


@gpu
def test_half_and_quarter_are_bit_identical_on_zipf_ids_at_batch_4096(built, monkeypatch):
    """One bf16 step of 4096 examples with Zipf(1.1) ids on a 16-field table of 322 rows: segments of hundreds of entries over
    many chunks beside short ones."""
    Bz, F, K, H1, H2 = 4096, 16, 11, 300, 100
    rows = synth.fm_table(sum(ZIPF_SIZES16), K, 0.05, 5)
    rng = np.random.RandomState(7)
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p['w3'] = rng.uniform(-0.2, 0.2, H2)
    p['b3'] = 0.05
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
    r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
    r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
    pb = dict(F=F, K=K, H1=H1, H2=H2, rows=rows, fo=synth.field_of_row(ZIPF_SIZES16), ids=[synth.zipf_ids(Bz, ZIPF_SIZES16, 1.1, 9)],
              y=(rng.uniform(size=(1, Bz)) < 0.3).astype(np.float32), p=p, r1=r1, r2=r2)
    half = run(monkeypatch, pb, 'half', 'bf16', steps=1, max_batch=Bz)
    quarter = run(monkeypatch, pb, 'quarter', 'bf16', steps=1, max_batch=Bz)
    assert not np.array_equal(half[0], rows)
    assert_same_bits(half, quarter, 'half against quarter')
