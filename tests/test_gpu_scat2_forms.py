"""Level 2 of the sparse-row update on 16-float rows has a second form, scat2w_body (FNN_SCAT2_FORM=wave): one 64-lane wave per
registered owner of a multi-chunk segment instead of a 256-thread workgroup, the first owner record read speculatively beside
the owner count.  It adds a segment's partial sums in the order and with the f64 operations of scat2_body (block), so the two
must agree bit for bit, on the table and on every dense tensor; FNN_SCAT1_FORM and FNN_SPLITK are the same in both arms.

The ids are hand-built in sorted positions (chunks of 16 sorted entries; an owner is a segment that lies in more than one chunk).
Batch 40 (three-launch step at 16 fields, stand-alone k_scat2 at 3):
  field 0  one row for all 40 examples: one owner of 3 chunks;
  field 1  distinct rows but for a pair at positions 15 | 16 (one owner of 2 chunks); 37 live entries, three ids of -1 behind them;
  field 2  40 distinct rows: no owner.
Batch 4096, 16 fields:
  field 0  one row for all 4096 entries: 256 chunks, four batches of 64, four terms in every one of the sixteen sums;
  field 1  a run of 1040 from position 8: 66 chunks, the second batch holds two;
  field 2  a run of 250 from position 10: 17 chunks, only the first sum has a second term;
  field 3  runs of 16 aligned to the chunks: no owner;
  field 4  runs of 16 from position 8: 255 owners of two chunks;
  fields 5..10  runs of 12 (or 20): every second one crosses a chunk border, 170 owners each;
  field 11 distinct rows; fields 12..15 Zipf(1.1) on small tables.
More than 1024 owners: at 256 workgroups the wave loop takes a second iteration, at FNN_SCAT2_WGS=16 some twenty.
The oracle comparison (one f32 step, batch 40) uses the bounds of tests/test_gpu_scat1_forms.py::test_quarter_form_vs_oracle.
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine

gpu = pytest.mark.gpu

B = 40
LENS1 = [1] * 15 + [2] + [1] * 20                               # field 1 of the small batch: 37 live, the pair at 15 | 16
SIZES3 = [5, len(LENS1) + 3, B]                                 # (field 1: room for rows in place of the ids of -1)
TAIL13 = [11, 4, 70, 9, 4, 7, 24, 20, 30, 35, 12, 5, 15]
SIZES16 = SIZES3 + TAIL13
ZIPF_SIZES16 = [5, 7, 60] + TAIL13
BZ = 4096
BIG_SIZES = [B, BZ, BZ, 256, 272] + [352] * 6 + [BZ, 24, 20, 30, 35]
KS = [4, 5, 11, 15]
LR, LAM1, LAMFM, W0 = 0.01, 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
FORMS = ('wave', 'block')


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def column(off, lens, n, dead):
    """A field's n entries in sorted order: row off + i taken lens[i] times, then ids of -1 -- or, dead=False, further distinct
    rows behind the live ones."""
    live = np.repeat(off + np.arange(len(lens)), lens)
    rest = np.full(n - len(live), -1) if dead else off + len(lens) + np.arange(n - len(live))
    return np.r_[live, rest].astype(np.int32)


def hand_ids(F, seed, dead=True):
    """ids int32 [40, F]: fields 0..2 as the module docstring says (which example holds which entry is drawn from `seed`),
    further fields zipf-distributed."""
    sizes = SIZES3 if F == 3 else SIZES16
    rng = np.random.RandomState(seed)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 100)
    ids[:, 0] = 3
    ids[:, 1] = column(SIZES3[0], LENS1, B, dead)[rng.permutation(B)]
    ids[:, 2] = column(SIZES3[0] + SIZES3[1], [1] * B, B, dead)[rng.permutation(B)]
    return ids


def runs(n, length, lead):
    """Run lengths that fill n sorted positions: `lead` single entries, runs of `length`, single entries to the end."""
    k = (n - lead) // length
    return [1] * lead + [length] * k + [1] * (n - lead - k * length)


def big_ids(seed, run_len=12):
    """ids int32 [4096, 16] on BIG_SIZES as the module docstring says."""
    rng = np.random.RandomState(seed)
    ids = synth.zipf_ids(BZ, BIG_SIZES, 1.1, seed + 100)
    off = np.r_[0, np.cumsum(BIG_SIZES)]
    lens = {0: [BZ], 1: [1] * 8 + [1040] + [1] * (BZ - 1048), 2: [1] * 10 + [250] + [1] * (BZ - 260),
            3: runs(BZ, 16, 0), 4: runs(BZ, 16, 8), 11: [1] * BZ}
    for f in range(5, 11):
        lens[f] = runs(BZ, run_len, 0)
    for f, ln in lens.items():
        assert len(ln) <= BIG_SIZES[f]
        ids[:, f] = column(off[f], ln, BZ, True)[rng.permutation(BZ)]
    return ids


def distinct_ids(seed):
    """ids int32 [40, 16] on BIG_SIZES: 40 distinct rows in the fields that have them, ids of -1 for the rest of a smaller field --
    no segment of two entries anywhere, so no owner."""
    rng = np.random.RandomState(seed)
    off = np.r_[0, np.cumsum(BIG_SIZES)]
    ids = np.full((B, 16), -1, dtype=np.int32)
    for f, size in enumerate(BIG_SIZES):
        n = min(B, size)
        ids[:n, f] = off[f] + rng.permutation(size)[:n]
        ids[:, f] = ids[rng.permutation(B), f]
    return ids


def segments(col):
    """[s, e) of every row's run in the field's sorted order (ids of -1 sort to the end and are dropped)."""
    v = np.sort(col[col >= 0])
    cut = np.flatnonzero(np.diff(v)) + 1
    return [(int(s), int(e)) for s, e in zip(np.r_[0, cut], np.r_[cut, len(v)])]


def owners(col):
    """(s, e, chunks) of every segment that lies in more than one chunk of 16 sorted entries: what level 1 registers."""
    return [(s, e, ((e - 1) >> 4) - (s >> 4) + 1) for s, e in segments(col) if (e - 1) >> 4 > s >> 4]


def test_hand_built_ids_have_the_layout_the_cases_rely_on():
    for F in (3, 16):
        for seed in (1, 2):
            ids = hand_ids(F, seed)
            assert owners(ids[:, 0]) == [(0, 40, 3)]
            assert owners(ids[:, 1]) == [(15, 17, 2)] and len(segments(ids[:, 1])) == 36
            assert (ids[:, 1] >= 0).sum() == 37 and (ids[:, 1] < 0).sum() == 3
            assert owners(ids[:, 2]) == [] and len(segments(ids[:, 2])) == 40
            fo = synth.field_of_row(SIZES3 if F == 3 else SIZES16)
            for f in range(F):
                live = ids[:, f][ids[:, f] >= 0]
                assert np.all(fo[live] == f)
    full = hand_ids(3, 1, dead=False)                                        # the inner-product step's ids: same runs, no -1
    assert full.min() >= 0 and np.all(synth.field_of_row(SIZES3)[full] == np.arange(3))
    assert owners(full[:, 1]) == [(15, 17, 2)] and len(segments(full[:, 1])) == 39
    fo = synth.field_of_row(BIG_SIZES)
    count = {}
    for run_len in (12, 20):
        ids = big_ids(3, run_len)
        assert all(np.all(fo[ids[:, f][ids[:, f] >= 0]] == f) for f in range(16))
        assert owners(ids[:, 0]) == [(0, 4096, 256)]                          # four batches of 64 chunks
        assert owners(ids[:, 1]) == [(8, 1048, 66)]                           # the second batch holds two chunks
        assert owners(ids[:, 2]) == [(10, 260, 17)]                           # only S_0 has a second term
        assert owners(ids[:, 3]) == [] and len(segments(ids[:, 3])) == 256
        o4 = owners(ids[:, 4])
        assert len(o4) == 255 and all(c == 2 and e - s == 16 and s % 16 == 8 for s, e, c in o4)
        for f in range(5, 11):
            of = owners(ids[:, f])
            assert all(e - s == run_len and c == 2 for s, e, c in of)
            assert len(of) == (170 if run_len == 12 else 204)       # 12: every second run crosses a border; 20: every run
        assert owners(ids[:, 11]) == []
        count[run_len] = sum(len(owners(ids[:, f])) for f in range(16))
    assert count[12] > 1024 and count[20] > 1024 and count[12] != count[20]   # a second iteration of 1024 waves; two owner counts
    d = distinct_ids(4)
    assert all(owners(d[:, f]) == [] and len(segments(d[:, f])) == min(B, BIG_SIZES[f]) for f in range(16))
    assert np.all(fo[d[d >= 0]] == np.nonzero(d >= 0)[1])


def dense_params(F, K, H1, H2, rng):
    p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
    p['w3'] = rng.uniform(-0.2, 0.2, H2)
    p['b1'] = rng.uniform(-0.1, 0.1, H1)
    p['b2'] = rng.uniform(-0.1, 0.1, H2)
    p['b3'] = 0.05
    p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
    r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
    r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
    r1[0] = r2[0] = 1
    return p, r1, r2


def make_problem(F, K, seed=5):
    sizes = SIZES3 if F == 3 else SIZES16
    H1, H2 = (20, 10) if F == 3 else (300, 100)
    rng = np.random.RandomState(seed + 2)
    y = [(rng.uniform(size=B) < 0.3).astype(np.float32) for _ in range(2)]
    p, r1, r2 = dense_params(F, K, H1, H2, rng)
    return dict(F=F, K=K, H1=H1, H2=H2, rows=synth.fm_table(sum(sizes), K, 0.05, seed), fo=synth.field_of_row(sizes),
                ids=[hand_ids(F, 1), hand_ids(F, 2)], y=y, p=p, r1=r1, r2=r2)


_big = {}


def big_problem(sizes=None, ids=None, key='big'):
    """The batch-4096 problem, built once (16 fields, K = 11, 300 x 100)."""
    if key not in _big:
        sizes = sizes or BIG_SIZES
        rng = np.random.RandomState(7)
        ids = ids or [big_ids(3), distinct_ids(4), big_ids(5, 20)]
        p, r1, r2 = dense_params(16, 11, 300, 100, rng)
        y = [(rng.uniform(size=len(i)) < 0.3).astype(np.float32) for i in ids]
        _big[key] = dict(F=16, K=11, H1=300, H2=100, rows=synth.fm_table(sum(sizes), 11, 0.05, 5), fo=synth.field_of_row(sizes),
                         ids=ids, y=y, p=p, r1=r1, r2=r2)
    return _big[key]


def run(monkeypatch, pb, form, prec, prefetch=False, steps=2, max_batch=256, wgs=None):
    """`steps` training steps on one handle (each consumes the rows the one before wrote) -> (table, dense tensors)."""
    import torch
    monkeypatch.setenv('FNN_SPLITK', '4')                         # the same slices in every arm: only the level-2 body differs
    monkeypatch.setenv('FNN_SCAT1_FORM', 'half')
    monkeypatch.setenv('FNN_SCAT2_FORM', form)
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    if wgs is None:
        monkeypatch.delenv('FNN_SCAT2_WGS', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT2_WGS', str(wgs))
    eng = FNNEngine(pb['F'], pb['K'], pb['H1'], pb['H2'], max_batch=max_batch, precision=prec, lr=LR, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids'][:steps]]
        for s in range(steps):
            if prefetch and s + 1 < steps:
                eng.prefetch_ids(dev_ids[s + 1])
            eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_loss=False)
        eng.sync()
        return eng.get_table(), eng.get_dense()
    finally:
        eng.close()


def assert_same_bits(a, b, what='wave against block'):
    assert np.array_equal(a[0], b[0]), "%s, table: %d of %d floats differ" % (what, (a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), (what, k)
    assert a[1]['b3'] == b[1]['b3'], what


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
@pytest.mark.parametrize("K", KS)
def test_forms_are_bit_identical_in_the_three_launch_step(built, monkeypatch, K, prec, prefetch):
    pb = make_problem(16, K)
    wave, block = [run(monkeypatch, pb, form, prec, prefetch) for form in FORMS]
    assert not np.array_equal(wave[0], pb['rows'])                # the steps did move the rows
    assert_same_bits(wave, block)


@gpu
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
@pytest.mark.parametrize("K", KS)
def test_forms_are_bit_identical_layer_by_layer(built, monkeypatch, K, prec):
    """3 fields: stand-alone k_scat2 over the batch's own N2 = 256 keys per field (48 owner records allocated)."""
    pb = make_problem(3, K)
    wave, block = [run(monkeypatch, pb, form, prec) for form in FORMS]
    assert not np.array_equal(wave[0], pb['rows'])
    assert_same_bits(wave, block)


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("F", [3, 16])
def test_wave_form_vs_oracle(built, monkeypatch, F, K):
    """One f32 step of the wave form against the float64 oracle, at the bounds of
    tests/test_gpu_scat1_forms.py::test_quarter_form_vs_oracle (table: rtol 1e-5, atol 2e-7)."""
    pb = make_problem(F, K)
    table, dense = run(monkeypatch, pb, 'wave', 'f32', steps=1)
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
@pytest.mark.parametrize("wgs", [None, 16], ids=['wgs256', 'wgs16'])
@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_forms_are_bit_identical_on_long_segments_at_batch_4096(built, monkeypatch, prec, wgs):
    """One step: segments of 256, 66 and 17 chunks beside more than 1275 short owners -- two iterations of the wave loop, many at 16 workgroups."""
    pb = big_problem()
    wave, block = [run(monkeypatch, pb, form, prec, steps=1, max_batch=BZ, wgs=wgs) for form in FORMS]
    assert not np.array_equal(wave[0], pb['rows'])
    assert_same_bits(wave, block)


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
def test_forms_are_bit_identical_over_three_batches_on_one_handle(built, monkeypatch, prefetch):
    """The batch above, then 40 examples of distinct ids (no owner: the records of the first batch are stale and the speculative
    read must ignore them), then a batch with another owner count."""
    pb = big_problem()
    wave, block = [run(monkeypatch, pb, form, 'bf16', prefetch, steps=3, max_batch=BZ) for form in FORMS]
    assert_same_bits(wave, block)
    one = run(monkeypatch, pb, 'wave', 'bf16', prefetch, steps=1, max_batch=BZ)
    two = run(monkeypatch, pb, 'wave', 'bf16', prefetch, steps=2, max_batch=BZ)
    assert not np.array_equal(one[0], two[0]) and not np.array_equal(two[0], wave[0])      # every batch moved rows


@gpu
def test_forms_are_bit_identical_on_zipf_ids_at_batch_4096(built, monkeypatch):
    """One bf16 step of 4096 examples with Zipf(1.1) ids on a 16-field table of 322 rows."""
    pb = big_problem(ZIPF_SIZES16, [synth.zipf_ids(BZ, ZIPF_SIZES16, 1.1, 9)], key='zipf')
    wave, block = [run(monkeypatch, pb, form, 'bf16', steps=1, max_batch=BZ) for form in FORMS]
    assert not np.array_equal(wave[0], pb['rows'])
    assert_same_bits(wave, block)


@gpu
@pytest.mark.parametrize("opt", [['sgd', 0.05], ['adam', 0.01, 1e-8], ['ftrl', 0.05]], ids=['sgd', 'adam', 'ftrl'])
def test_forms_are_bit_identical_all_16_slots_live(built, monkeypatch, opt):
    """K = 16 (rank 15): every slot is live.  FM pre-training on the hand-built ids, two steps: k_fm_scat2_tail, with lr = -1 and the
    gradient store as the target under Adam and FTRL."""
    from deep_ctr_amd.FM import FM
    n_rows = sum(SIZES3)
    rows = synth.fm_table(n_rows, 16, 0.05, 3)
    y = (np.random.RandomState(4).uniform(size=(2, B)) < 0.3).astype(np.float32)
    ids = [hand_ids(3, 1), hand_ids(3, 2)]
    res = []
    monkeypatch.setenv('FNN_SCAT1_FORM', 'half')
    for form in FORMS:
        monkeypatch.setenv('FNN_SCAT2_FORM', form)
        m = FM(B, [n_rows, 3, 15], ['uniform', -0.001, 0.001, [1, 2], None], opt, [0.01], 'train', 0)
        try:
            m.set_params(rows, 0.1)
            for s in range(2):
                m.train_step(ids[s], y[s], want_loss=False)
            res.append(m.get_params())
        finally:
            m.close()
    assert not np.array_equal(res[0][0], rows)
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@gpu
def test_forms_are_bit_identical_in_the_inner_product_step(built, monkeypatch):
    """FNN_IP_L3-shaped step on 3 fields, K = 11, f32, no dropout: k_scat2 on the side stream of the inner-product family (which
    refuses ids of -1: the dead entries become further distinct rows that sort behind the live ones)."""
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
    monkeypatch.setenv('FNN_SCAT1_FORM', 'half')
    for form in FORMS:
        monkeypatch.setenv('FNN_SCAT2_FORM', form)
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
    rows_o, (b_o, Ws_o, bs_o) = res[1]
    assert np.array_equal(res[0][0], rows_o)
    assert res[0][1][0] == b_o
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1][1], Ws_o))
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1][2], bs_o))
