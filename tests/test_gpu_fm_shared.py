"""GPU parity of FM / LR pre-training with rows shared between columns of a batch (fm_set_shared_rows; FM(..., shared_rows=True)):
a row under several columns must receive every column's contribution, on both row layouts, under SGD, Adam and FTRL, with and
without value weights, and a batch that shares nothing must leave a mode-on handle bit-equal to a mode-off one.

Reference: the float64 restatement of tests/fm_weighted_ref.py (fm_shared_cases.Trainer), which test_fm_shared_ref.py holds to
float64 autograd of python/FM.py:55-64 on such ids.  Bounds: those of the existing FM tests, unchanged -- predictions rtol 5e-5 /
atol 1e-6 and loss 2e-5 relative (test_gpu_fm_fields.py), rows after SGD 2e-3 * max|change| + 2e-7 (sgd_vs_oracle), Adam / FTRL
check_state's with its `ill` mask, which may cover at most 1 % of the touched elements.  fm_count_shared_rows is asserted equal
to the NumPy count after every step, which is how a case proves it reached the atomic path.  Batches: fm_shared_cases."""
import numpy as np
import pytest

import fm_shared_cases as sc
from test_gpu_fm_fields import INIT, batches, check_state, table

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import ipinyou, synth
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

pytestmark = pytest.mark.gpu
LR_SGD = 0.05
PER = 12


def model(F, rank, B, argv, lam, rows, b, shared=True):
    if rank == 0:
        m = LR(B, [len(rows), F], INIT, argv, [lam], 'train', 0, shared_rows=shared)
    else:
        m = FM(B, [len(rows), F, rank], INIT, argv, [lam], 'train', 0, shared_rows=shared)
    m.set_params(rows, b)
    return m


def sgd_case(F, rank, steps, lam=1e-2, reduce_mean=1, n_rows=None, seed=0, counts=None):
    """steps: [(ids, wts | None, y)].  Every step's predictions, loss and shared-row count, then rows and bias."""
    n_rows = n_rows or sc.n_rows_of(F, PER)
    rows, b0 = table(n_rows, F, rank, seed), 0.1
    B = max(len(s[2]) for s in steps)
    m = model(F, rank, B, ['sgd', LR_SGD] + ([] if reduce_mean else ['sum']), lam, rows, b0)
    tr = sc.Trainer(rows, b0, 'sgd', LR_SGD, lam, reduce_mean)
    for i, (ids, wts, y) in enumerate(steps):
        out = m.train_step(ids, y, want_p=True, wts=wts)
        data, p = tr.sgd_step(ids, y, wts)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
        want = sc.shared_count(ids)
        assert m.count_shared_rows() == want and (counts is None or want == counts[i]), (i, want)
    got, gb = m.get_params()
    change = np.abs(tr.rows - rows).max() + 1e-12
    err = np.abs(got - tr.rows).max()
    print("[fm-shared] F %d rank %d: max row error %.3g of bound %.3g" % (F, rank, err, 2e-3 * change + 2e-7))
    assert err <= 2e-3 * change + 2e-7
    assert abs(gb - tr.b) <= 2e-3 * abs(tr.b - b0) + 2e-7
    m.close()
    return got, tr


@pytest.mark.parametrize("reduce_mean", [0, 1], ids=['sum', 'mean'])
def test_narrow_rows_shared_between_columns(built, reduce_mean):
    """k = 11, 5 columns, B = 67: a row under 2 columns, under all 5, twice on a line, a line of shared rows only, -1 ids."""
    steps = [(sc.basic_batch(67, 5, PER, 10 + i), None, sc.labels(67, 20 + i)) for i in range(3)]
    sgd_case(5, 10, steps, reduce_mean=reduce_mean, seed=1, counts=[3, 3, 3])


@pytest.mark.parametrize("rank", [0, 3, 4, 14, 15])
def test_narrow_rows_every_live_quarter_count(built, rank):
    """k = 1 (LR), 4, 5, 15, 16: one to four live quarters of the 64-byte row, with and without pad lanes in the last."""
    steps = [(sc.basic_batch(67, 5, PER, 30 + rank + i), None, sc.labels(67, 40 + i)) for i in range(2)]
    sgd_case(5, rank, steps, lam=(0.0, 1e-2)[rank % 2], seed=2 + rank, counts=[3, 3])


@pytest.mark.parametrize("rank", [10, 50], ids=['narrow', 'wide'])
def test_hot_row_takes_level_2_and_level_1_adds(built, rank):
    """B = 300: a row whose column-0 segment spans several chunks (a level-2 add) and whose column-2 segment lies inside one (a
    level-1 add); rows whose column-1 segments end on the 8|8 border and on the chunk border; single-entry segments."""
    steps = [(sc.hot_batch(300, 5, PER, 50 + i), None, sc.labels(300, 60 + i)) for i in range(2)]
    sgd_case(5, rank, steps, seed=3, counts=[3, 3])


@pytest.mark.parametrize("F", [17, 39, 64])
def test_narrow_rows_beyond_16_columns(built, F):
    steps = []
    for i in range(2):
        ids = sc.basic_batch(67, F, PER, 70 + F + i)
        sc.place(ids, 3, [(20, 0), (21, F - 1)])                             # columns 0 and F - 1: at 64 the top of the 6-bit tag
        steps.append((ids, None, sc.labels(67, 80 + i)))
    sgd_case(F, 10, steps, seed=4, counts=[4, 4])


@pytest.mark.parametrize("F,rank", [(3, 50), (3, 100), (18, 50)], ids=['k51', 'k101', 'k51-18cols'])
def test_wide_rows_shared_between_columns(built, F, rank):
    steps = [(sc.basic_batch(67, F, PER, 90 + F + i), None, sc.labels(67, 95 + i)) for i in range(2)]
    sgd_case(F, rank, steps, seed=5, counts=[3, 3])


@pytest.mark.parametrize("opt,F,rank,seed", sc.OPT_CASES, ids=['%s-F%d-r%d' % c[:3] for c in sc.OPT_CASES])
def test_adam_and_ftrl_with_shared_rows(built, opt, F, rank, seed):
    rows = table(sc.n_rows_of(F, sc.OPT_PER), F, rank, seed)
    bs = sc.opt_batches(F, seed)
    lr = sc.OPT_LRS[opt]
    m = model(F, rank, sc.OPT_B, [opt, lr] + ([1e-8] if opt == 'adam' else []), 1e-3, rows, 0.1)
    tr = sc.Trainer(rows, 0.1, opt, lr, 1e-3, 1)
    tr.rows0 = rows.copy()
    for ids, y in bs:
        out = m.train_step(ids, y, want_p=True)
        data, p = tr.step(ids, y)
        np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - data) <= 2e-5 * max(1.0, abs(data))
        assert m.count_shared_rows() == sc.shared_count(ids) == 3
    t = sc.touched(bs, len(rows))
    assert tr.ill[t].sum() <= 0.01 * tr.ill[t].size
    check_state(m, tr)
    m.close()


@pytest.mark.parametrize("rank", [10, 50], ids=['narrow', 'wide'])
def test_reference_feed_pads_as_last_row_with_weight_zero(built, rank):
    """python/ipinyou.py:42-65's own arrays: pads are (last row, weight 0), so the pad row sits under every column of nearly
    every line.  Its gradient is exactly 0: it must end where the restatement puts it (the L2 decay alone)."""
    F, steps = 5, []
    n_rows = sc.n_rows_of(F, PER)
    for i in range(2):
        ids = sc.basic_batch(67, F, PER, 110 + i)
        wts = (ids >= 0).astype(np.float32)
        steps.append((np.where(ids < 0, n_rows - 1, ids).astype(np.int32), wts, sc.labels(67, 120 + i)))
    got, tr = sgd_case(F, rank, steps, seed=6, counts=[4, 4])
    want = table(n_rows, F, rank, 6)[-1] * (1.0 - LR_SGD * 1e-2) ** 2
    assert np.abs(got[-1] - want).max() <= 2e-7 and np.abs(tr.rows[-1] - want).max() <= 1e-15


def test_non_unit_weights_on_shared_rows(built):
    rng = np.random.RandomState(7)
    steps = []
    for i in range(2):
        ids = sc.basic_batch(67, 5, PER, 130 + i)
        wts = rng.uniform(-0.5, 2.0, size=ids.shape).astype(np.float32)
        wts[rng.uniform(size=ids.shape) < 0.1] = 0.0
        steps.append((ids, wts, sc.labels(67, 140 + i)))
    sgd_case(5, 10, steps, seed=7, counts=[3, 3])


def test_64bit_sort_keys(built):
    """n_rows * 4096 > 2^32 (tests/test_gpu_sort_runs.py's key-width case): the claim runs in the 64-bit rank merge."""
    n_rows = 1100000
    assert n_rows * 4096 > 2 ** 32
    steps = []
    for i in range(2):
        ids = sc.basic_batch(67, 5, PER, 150 + i)
        ids = np.where(ids >= sc.S_ROWS, ids + (n_rows - sc.n_rows_of(5, PER)), ids).astype(np.int32)   # the background at the table's top
        steps.append((ids, None, sc.labels(67, 160 + i)))
    assert max(s[0].max() for s in steps) >= n_rows - PER - 1
    sgd_case(5, 3, steps, n_rows=n_rows, seed=8, counts=[3, 3])


def test_stale_marks_do_not_outlive_their_step(built):
    """Rows shared in step 1 sit under one column in step 2 (their marks are stale and must not be honoured: the single rounded
    store again); step 3 shares nothing."""
    s1 = sc.basic_batch(67, 5, PER, 170)
    s2 = sc.background(67, 5, PER, 171)
    sc.place(s2, 0, [(1, 0), (2, 0)]), sc.place(s2, 1, [(3, 4)]), sc.place(s2, 2, [(4, 2), (5, 2), (6, 2)])
    sc.place(s2, 4, [(7, 1), (8, 3)])                                        # another row is shared now
    s3 = sc.background(67, 5, PER, 172)
    sc.place(s3, 0, [(1, 1)]), sc.place(s3, 4, [(2, 2)])
    steps = [(s, None, sc.labels(67, 180 + i)) for i, s in enumerate((s1, s2, s3))]
    sgd_case(5, 10, steps, seed=9, counts=[3, 1, 0])


def state_of(m, opt):
    rows, b = m.get_params()
    return [rows, np.float32(b)] + (list(m.get_opt_state()[:3]) if opt != 'sgd' else [])


@pytest.mark.parametrize("opt", ['sgd', 'adam'])
@pytest.mark.parametrize("rank", [10, 50], ids=['narrow', 'wide'])
def test_unshared_batches_are_bit_identical_to_the_mode_off(built, rank, opt):
    F, B = 6, 300
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes), F, rank, 11)
    argv = ['sgd', LR_SGD] if opt == 'sgd' else ['adam', 1e-2, 1e-8]
    on, off = model(F, rank, B, argv, 1e-2, rows, 0.1, True), model(F, rank, B, argv, 1e-2, rows, 0.1, False)
    for ids, y in batches(sizes, B, 3, 190):
        assert sc.shared_count(ids) == 0
        a, c = on.train_step(ids, y, want_p=True), off.train_step(ids, y, want_p=True)
        assert a['loss'] == c['loss'] and np.array_equal(a['p'].cpu().numpy(), c['p'].cpu().numpy())
        assert on.count_shared_rows() == 0
    for x, z in zip(state_of(on, opt), state_of(off, opt)):
        assert np.array_equal(x, z)
    on.close(), off.close()


def test_toggle_off_returns_to_the_plain_step(built):
    """on -> a shared step -> off; a further unshared step is bit-equal to that step on a handle that was given the same rows and
    bias by set_params and never toggled."""
    F, rank, B = 5, 10, 67
    rows = table(sc.n_rows_of(F, PER), F, rank, 12)
    a = model(F, rank, B, ['sgd', LR_SGD], 1e-2, rows, 0.1, True)
    a.train_step(sc.basic_batch(B, F, PER, 200), sc.labels(B, 201))
    assert a.count_shared_rows() == 3
    a.set_shared_rows(False)
    r1, b1 = a.get_params()                                                  # folds the lazy scale: both handles hold these bits
    c = model(F, rank, B, ['sgd', LR_SGD], 1e-2, r1, b1, False)
    ids, y = sc.background(B, F, PER, 202), sc.labels(B, 203)
    oa, oc = a.train_step(ids, y, want_p=True), c.train_step(ids, y, want_p=True)
    assert oa['loss'] == oc['loss'] and np.array_equal(oa['p'].cpu().numpy(), oc['p'].cpu().numpy())
    (ra, ba), (rc, bc) = a.get_params(), c.get_params()
    assert np.array_equal(ra, rc) and ba == bc and not np.array_equal(ra, r1)
    a.close(), c.close()


def write_yzx(path, n, seed, n_feat=40):
    """Ragged lines: 1 .. 7 features in line order, a feature may repeat across positions of a line."""
    rng = np.random.RandomState(seed)
    w = rng.standard_normal(n_feat)
    with open(path, 'w') as f:
        for _ in range(n):
            feats = list(rng.randint(0, n_feat, size=rng.randint(1, 8)))
            if len(feats) > 2 and rng.uniform() < 0.3:
                feats[-1] = feats[0]                                         # the same feature at two positions
            y = int(rng.uniform() < 1.0 / (1.0 + np.exp(-w[feats].sum())))
            f.write('%d 0 %s\n' % (y, ' '.join('%d:1' % v for v in feats)))


@pytest.mark.parametrize("algo", ['LR', 'FM'])
def test_ipinyou_driver_against_a_float64_replay(built, tmp_path, algo):
    """ipinyou.run, one pass at batch 64 over 300 ragged lines in buffers of 128: the logged eval AUC of every buffer and the
    final table against a NumPy float64 replay of the same schedule (the global RNG seeded alike gives the same buffer order)."""
    train, test, log = str(tmp_path / 'train.yzx'), str(tmp_path / 'test.yzx'), str(tmp_path / 'log')
    write_yzx(train, 300, 1), write_yzx(test, 400, 2)
    np.random.seed(1234)
    res = ipinyou.run(train, test, algo, batch_size=64, buffer=128, eval_size=1000, epochs=1, log_file=log, echo=False)
    m = res['model']
    got, gb = m.get_params()
    m.close()
    # the replay: the same loader calls in the same order
    np.random.seed(1234)
    (d1, f1), (d2, f2) = ipinyou.stat(train), ipinyou.stat(test)
    X_dim, X_feas = max(d1, d2) + 2, max(f1, f2)
    assert (res['X_dim'], res['X_feas']) == (X_dim, X_feas) and X_feas == 7
    rank, lam = (0, 1e-3) if algo == 'LR' else (10, 1e-2)
    seeds = [0x89AB] if algo == 'LR' else [0x3210, 0x7654]
    W = np.random.RandomState(seeds[0]).uniform(-0.001, 0.001, (X_dim, 1))
    V = np.random.RandomState(seeds[-1]).uniform(-0.001, 0.001, (X_dim, rank))
    rows0 = np.concatenate([W, V], axis=1).astype(np.float32).astype(np.float64)
    tr = sc.Trainer(rows0, 0.0, 'sgd', 1e-3, lam, 1)
    aucs, shared = [], 0
    with open(train) as fin:
        while True:
            X_ind, X_val, y = ipinyou.load_ipinyou_data(fin, 128, X_dim - 1, X_feas)
            if X_ind is None:
                break
            ids, wts = ipinyou.to_column_ids(X_ind, X_val)
            assert wts is None
            for lo in range(0, len(y), 64):
                tr.sgd_step(ids[lo:lo + 64], y[lo:lo + 64].astype(np.float64))
                shared += sc.shared_count(ids[lo:lo + 64])
            with open(test) as ft:
                t_ind, t_val, t_y = ipinyou.load_ipinyou_data(ft, 1000, X_dim - 1, X_feas)
                assert ipinyou.load_ipinyou_data(ft, 1000, X_dim - 1, X_feas)[0] is None   # the driver's second read, at EOF
            t_ids, _ = ipinyou.to_column_ids(t_ind, t_val)
            aucs.append(ipinyou.exact_auc(t_y, sc.wr.predict_w(tr.rows, tr.b, t_ids, np.ones(t_ids.shape))))
    assert shared > 20 and len(aucs) == 3 == len(res['log'])
    lines = open(log).read().splitlines()
    assert lines[0] == m.log and len(lines) == 4
    for (step, b_auc, e_auc, loss), want, line, n in zip(res['log'], aucs, lines[1:], (128, 256, 300)):
        assert step == n and abs(e_auc - want) <= 1e-4, (e_auc, want)
        assert line == '%d\t%g\t%g\t%g\t' % (step, b_auc, e_auc, loss) and 0.0 <= b_auc <= 1.0
    change = np.abs(tr.rows - rows0).max() + 1e-12
    assert np.abs(got - tr.rows).max() <= 2e-3 * change + 2e-7
    assert abs(gb - tr.b) <= 2e-3 * abs(tr.b) + 2e-7
