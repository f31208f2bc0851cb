"""The grouping of a batch's (row, example) keys runs in two phases: sorted runs (sortA_body), then a merge by rank (sortB_body).
FNN_SORT_RUNS=4 (the default of the FNN step on FM rows and of the inner-product step) leaves 4 runs of 1024 keys per field for
the merge, FNN_SORT_RUNS=16 (the default in bag mode and in FM pre-training) the 16 wave runs of 256.  Keys
are distinct, so both forms must write the identical `rec` -- and with it every row, dense tensor, loss and gx' bit for bit.

The strip kernel, and with it the three-launch step whose launches 2 and 3 carry the two phases as roles, takes 13 to 16 fields of
16-float rows; an engine of 4 fields steps layer by layer with a sort of its own.  So the hand-built columns are run both as a
4-field engine and as the first four of 13 fields:
  field 0  4 rows: every segment spans all the runs its batch fills;
  field 1  all ids distinct;
  field 2  beyond 1024 examples: 512 rows twice each, then one row whose segment starts exactly at key 1024 of the sorted order;
  field 3  Zipf ids with every seventh id -1.
Batches of 40 (all keys in one wave run), 300 (crosses a wave run), 1029 (crosses a workgroup's run of 1024) and 4096 (full), with
fnn_prefetch_ids (the roles inside launches 2 and 3) and without (k_sortA / k_sortB).
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine

gpu = pytest.mark.gpu

HAND = [4, 5000, 5000, 50]                                       # rows of the hand-built fields
REST = [11, 4, 70, 9, 40, 7, 24, 20, 30, 12, 5, 15]              # fields 4 .. 15: Zipf
LR, LAM1, LAMFM, W0 = 0.01, 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
K = 11
BS = [40, 300, 1029, 4096]


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def sizes_of(F):
    return (HAND + REST)[:F]


def hand_ids(B, F, seed):
    sizes = sizes_of(F)
    off = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.RandomState(seed)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 100)
    ids[:, 0] = off[0] + rng.randint(0, 4, size=B)
    ids[:, 1] = off[1] + rng.permutation(sizes[1])[:B]
    if B > 1024:
        n = min(40, B - 1024)
        col = np.concatenate([np.repeat(np.arange(512), 2), np.full(n, 600), 700 + np.arange(B - 1024 - n)])
        ids[:, 2] = off[2] + col[rng.permutation(B)]
    ids[::7, 3] = -1
    return ids


def segments(col):
    v = np.sort(col[col >= 0])
    cut = np.flatnonzero(np.diff(v)) + 1
    return list(zip(np.r_[0, cut], np.r_[cut, len(v)]))


def test_hand_built_ids_have_the_layout_the_cases_rely_on():
    for F in (4, 13):
        fo = synth.field_of_row(sizes_of(F))
        for B in BS:
            ids = hand_ids(B, F, 1)
            assert len(np.unique(ids[:, 0])) == 4
            assert len(np.unique(ids[:, 1])) == B
            if B > 1024:
                seg = segments(ids[:, 2])
                assert any(s == 1024 and e - s == min(40, B - 1024) for s, e in seg)
            assert (ids[:, 3] < 0).sum() == len(range(0, B, 7))
            for f in range(F):
                live = ids[:, f][ids[:, f] >= 0]
                assert np.all(fo[live] == f)
    ids = hand_ids(4096, 13, 1)                                  # field 0 at 4096: every row has entries in all four quarters
    for r in range(4):
        assert all(((ids[q * 1024:(q + 1) * 1024, 0]) == r).any() for q in range(4))


def make_problem(B, F, H1=40, H2=20, seed=5):
    sizes = sizes_of(F)
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
    return dict(B=B, F=F, H1=H1, H2=H2, rows=rows, fo=fo, ids=[hand_ids(B, F, 1), hand_ids(B, F, 2)], y=y, p=p, r1=r1, r2=r2)


_PROBLEMS = {}


def problem_of(B, F):
    if (B, F) not in _PROBLEMS:
        _PROBLEMS[(B, F)] = make_problem(B, F)
    return _PROBLEMS[(B, F)]


def set_runs(monkeypatch, runs):
    if runs is None:
        monkeypatch.delenv('FNN_SORT_RUNS', raising=False)         # the default: 4
    else:
        monkeypatch.setenv('FNN_SORT_RUNS', str(runs))


def run(monkeypatch, pb, runs, prec='f32', prefetch=False, shadow=None, steps=2):
    """`steps` training steps -> (table, dense tensors, losses, gx' of every step)."""
    import torch
    set_runs(monkeypatch, runs)
    lr = 0.001 if pb['B'] >= 4096 else LR
    eng = FNNEngine(pb['F'], K, pb['H1'], pb['H2'], max_batch=4096, precision=prec, lr=lr, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids']]
        loss, gx = [], []
        for s in range(steps):
            if prefetch and s + 1 < steps:
                eng.prefetch_ids(dev_ids[s + 1])
            if shadow is not None:
                eng.set_shadowed(shadow)
            out = eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_gx=True)
            loss.append(out['loss'])
            gx.append(out['gx'].cpu().numpy())
        eng.sync()
        return eng.get_table(), eng.get_dense(), loss, gx
    finally:
        eng.close()


def assert_same_bits(a, b):
    assert np.array_equal(a[0], b[0]), "table: %d of %d floats differ" % ((a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[1]['b3'] == b[1]['b3']
    assert a[2] == b[2], "loss"
    for s in range(len(a[3])):
        assert np.array_equal(a[3][s], b[3][s]), "gx' of step %d" % s


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("F", [4, 13])
def test_run_counts_are_bit_identical(built, monkeypatch, F, B, prefetch):
    pb = problem_of(B, F)
    r16 = run(monkeypatch, pb, 16, prefetch=prefetch)
    r4 = run(monkeypatch, pb, None, prefetch=prefetch)
    assert not np.array_equal(r4[0], pb['rows'])                  # the steps did move the rows
    assert_same_bits(r16, r4)


@gpu
def test_run_counts_are_bit_identical_bf16_at_16_fields(built, monkeypatch):
    """hidden 300 / 100 in bf16 at 16 fields: the benchmark's instances of launches 2 and 3."""
    pb = make_problem(1029, 16, 300, 100)
    r16 = run(monkeypatch, pb, 16, prec='bf16', prefetch=True)
    r4 = run(monkeypatch, pb, 4, prec='bf16', prefetch=True)
    assert not np.array_equal(r4[0], pb['rows'])
    assert_same_bits(r16, r4)


@gpu
def test_run_counts_are_bit_identical_with_shadowed_features(built, monkeypatch):
    """A shadowed-feature list sends the step through the layer-by-layer kernels; the switch must not disturb them."""
    pb = problem_of(300, 13)
    off = np.concatenate([[0], np.cumsum(sizes_of(13))])
    shadow = np.array([(3, 0, 1), (3, 0, 2), (5, 1, off[1] + 7), (9, 3, off[3] + 2), (299, 0, 3)], np.int32)
    r16 = run(monkeypatch, pb, 16, shadow=shadow)
    r4 = run(monkeypatch, pb, None, shadow=shadow)
    plain = run(monkeypatch, pb, None)
    assert not np.array_equal(plain[0], r4[0])                    # the list was used
    assert_same_bits(r16, r4)


@gpu
@pytest.mark.parametrize("runs", [4, 16])
def test_step_vs_oracle(built, monkeypatch, runs):
    """One f32 step at 1029 examples against the float64 oracle, at the bounds of tests/test_gpu_parity.py::_check_step
    (table rtol 1e-5, atol 2e-7): two forms that were wrong alike would pass the comparisons above."""
    pb = problem_of(1029, 13)
    table, dense, _, _ = run(monkeypatch, pb, runs, steps=1)
    rows64 = pb['rows'].astype(np.float64)
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pb['p'].items()}
    ids, y = pb['ids'][0], pb['y'][0]
    x = orc.gather_vec(rows64, ids, W0)
    gx, _, loss, p_drop, g = orc.train_call(p64, x, y.astype(np.float64), pb['r1'].astype(np.float64),
                                            pb['r2'].astype(np.float64), LR, LAM1, 'tanh')
    orc.scatter_sgd_vec(rows64, ids, gx, LR, LAMFM, None)
    err = np.abs(table - rows64) / (2e-7 + 1e-5 * np.abs(rows64))
    print("FNN_SORT_RUNS=%d: worst table error %.3g of its bound" % (runs, err.max()))
    np.testing.assert_allclose(table, rows64, rtol=1e-5, atol=2e-7)
    for k in DENSE:
        gs = LR * np.abs(g[k]).max()
        np.testing.assert_allclose(dense[k], p64[k], rtol=1e-5, atol=1e-3 * gs + 1e-7, err_msg=k)


@gpu
@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
def test_run_counts_are_bit_identical_in_bag_mode(built, monkeypatch, prefetch):
    """Bag rows: column 1 repeats column 0, so every row of column 0 sits in two columns of the batch and takes the tag_shared
    path (float atomics).  Both columns then add the same sum to such a row, so the result does not depend on their order."""
    import torch
    from test_gpu_parity import make_snn_engine, make_snn_problem
    F, h0, B, H1, H2 = 13, 200, 300, 40, 20
    probs = []
    for seed in (1, 2):
        pr = list(make_snn_problem(B, n_rows=600, h0=h0, seed=seed, n_fields=F, h1=H1, h2=H2))
        pr[2][:, 1] = pr[2][:, 0]
        pr[5][0] = pr[6][0] = 1
        probs.append(pr)
    res = []
    for runs in (16, 4):
        set_runs(monkeypatch, runs)
        eng = make_snn_engine(probs[0][0], probs[0][1], probs[0][4], h0=h0, n_fields=F, h1=H1, h2=H2)
        try:
            dev_ids = [torch.as_tensor(pr[2]).to(eng.device).contiguous() for pr in probs]
            loss, gx = [], []
            for s in range(2):
                if prefetch and s == 0:
                    eng.prefetch_ids(dev_ids[1])
                out = eng.train_step(dev_ids[s], probs[s][3], probs[0][5], probs[0][6], want_gx=True)
                loss.append(out['loss'])
                gx.append(out['gx'].cpu().numpy())
            eng.sync()
            res.append((eng.get_table(), eng.get_dense(), loss, gx, eng.get_bag_bias()))
        finally:
            eng.close()
    assert not np.array_equal(res[1][0], probs[0][0])
    assert_same_bits(res[0], res[1])
    assert np.array_equal(res[0][4], res[1][4])


def ipnn_state(eng, n_rows):
    b, Ws, bs = eng.get_params()
    return [np.float32(b)] + list(Ws) + list(bs) + [eng.get_rows(np.arange(n_rows))]


def ipnn_both(monkeypatch, F, K_, hidden, B, n_rows, seed, act):
    from deep_ctr_amd.ipnn import IPNNEngine
    from test_gpu_ipnn_shapes import problem
    table, ids, y, params, masks, d = problem(F, K_, B, hidden, True, seed=seed, n_rows=n_rows)
    res = []
    for runs in (16, 4):
        set_runs(monkeypatch, runs)
        eng = IPNNEngine(F, K_, hidden, act, max_batch=B, precision='f32', lr=0.01, keep_prob=0.7)
        try:
            eng.set_params(table, params['b'], params['W'], params['bias'])
            outs = [eng.train_step(ids, y, masks, want_logits=True) for _ in range(2)]
            res.append((ipnn_state(eng, table.shape[0]), [o['loss'] for o in outs], [o['logits'].cpu().numpy() for o in outs]))
        finally:
            eng.close()
    assert not np.array_equal(res[1][0][-1], table.astype(np.float32))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert res[0][1] == res[1][1]
    for a, b in zip(res[0][2], res[1][2]):
        assert np.array_equal(a, b)


@gpu
def test_run_counts_are_bit_identical_inner_product_step(built, monkeypatch):
    ipnn_both(monkeypatch, 2, 1, [64, 63], 257, 600, 5, 'tanh')


@gpu
def test_run_counts_are_bit_identical_with_64bit_keys(built, monkeypatch):
    """n_rows * 4096 > 2^32: 64-bit sort keys (tests/test_gpu_ipnn_shapes.py::test_ipnn_step_with_64bit_sort_keys_at_32_fields)."""
    n_rows = 1100000
    assert n_rows * 4096 > 2 ** 32
    ipnn_both(monkeypatch, 32, 5, [64, 32], 1029, n_rows, 91, 'relu')


@gpu
@pytest.mark.parametrize("rank", [3, 20], ids=['narrow-rows', 'wide-rows'])
def test_run_counts_are_bit_identical_fm_pretraining(built, monkeypatch, rank):
    from deep_ctr_amd.FM import FM
    B, sizes = 300, HAND[:3]
    n_rows = sum(sizes)
    rows = synth.fm_table(n_rows, rank + 1, 0.05, 3)
    y = (np.random.RandomState(4).uniform(size=(2, B)) < 0.3).astype(np.float32)
    ids = [np.ascontiguousarray(hand_ids(B, 4, s)[:, :3]) for s in (1, 2)]
    res = []
    for runs in (16, 4):
        set_runs(monkeypatch, runs)
        m = FM(B, [n_rows, 3, rank], ['uniform', -0.001, 0.001, [1, 2], None], ['sgd', 0.05], [0.01], 'train', 0)
        try:
            m.set_params(rows, 0.1)
            for s in range(2):
                m.train_step(ids[s], y[s], want_loss=False)
            res.append(m.get_params())
        finally:
            m.close()
    assert not np.array_equal(res[1][0], rows)
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
