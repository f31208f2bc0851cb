"""FM / LR pre-training on the reference's online schedule (fm_train_online, include/fm_hip.h) on the device, against the
float64 sequential reference of tests/fm_online_cases.py and against the same schedule run as N train_step calls at B = 1.

Parity rule: with err_x = max |x - ref| over the table and b (and, separately, over the predictions),
    err_online <= 2 * err_loop + 2e-7.
Both are f32 evaluations of the same formulas that differ only in the order of their sums, so the online call has no reason to be
worse; the factor two allows for that order and the floor is the absolute term tests/test_gpu_fm.py uses.  On three lines
that file's own bound, 2e-3 * change + 2e-7, applies directly."""
import numpy as np
import pytest

import fm_online_cases as oc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM
from deep_ctr_amd.engine import FNNError

pytestmark = pytest.mark.gpu
SHAPES = [(16, 11), (1, 1), (2, 16), (64, 16), (39, 11), (16, 17), (16, 101), (64, 128)]
LR_SGD = 0.05
INIT = ['uniform', -0.001, 0.001, [1, 2], None]


def model(F, k, rows, lam, shared=False, ptmzr=('sgd', LR_SGD), b=oc.B0, batch=1):
    m = FM(batch, [rows.shape[0], F, k - 1], INIT, list(ptmzr), [lam], 'train', 0, shared_rows=shared)
    m.set_params(rows, b)
    return m


def errs(m, ref_rows, ref_b):
    got, gb = m.get_params()
    return max(np.abs(got - ref_rows).max(), abs(gb - ref_b))


def seed_of(F, k):
    return 100 + F + k


@pytest.mark.parametrize("F,k", SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("lam", [0.0, 1e-2])
def test_online_against_the_reference_and_the_batch_one_loop(built, F, k, weighted, lam):
    import torch
    N = 300
    rows, ids, wts, y, ref_rows, ref_b, ref_p, ref_loss = oc.solved(F, k, N, seed_of(F, k), weighted, LR_SGD, lam)
    on = model(F, k, rows, lam)
    assert on.online_form() == 'plain'
    out = on.train_online(ids, y, wts=wts, want_p=True)
    # the parent's way of running the schedule: a train_step per line (shared_rows: a row may sit twice on a line)
    loop = model(F, k, rows, lam, shared=True)
    ids_d, y_d = loop._dev(ids, torch.int32), loop._dev(y, torch.float32)
    w_d = None if wts is None else loop._dev(wts, torch.float32)
    ps = [loop.train_step(ids_d[n:n + 1], y_d[n:n + 1], want_p=True, want_loss=False, wts=None if w_d is None else w_d[n:n + 1])['p']
          for n in range(N)]
    p_loop = torch.cat(ps).cpu().numpy()
    e_on, e_loop = errs(on, ref_rows, ref_b), errs(loop, ref_rows, ref_b)
    ep_on, ep_loop = np.abs(out['p'].cpu().numpy() - ref_p).max(), np.abs(p_loop - ref_p).max()
    print("F %d k %d: table/b err online %.3g loop %.3g; p err online %.3g loop %.3g" % (F, k, e_on, e_loop, ep_on, ep_loop))
    assert e_on <= 2 * e_loop + 2e-7, "table / b: online %.3g, B = 1 loop %.3g" % (e_on, e_loop)
    assert ep_on <= 2 * ep_loop + 2e-7, "p: online %.3g, B = 1 loop %.3g" % (ep_on, ep_loop)
    assert abs(out['loss'] - ref_loss.sum()) <= 2e-5 * max(1.0, ref_loss.sum())
    assert abs(out['loss_last'] - ref_loss[-1]) <= 2e-5 * max(1.0, ref_loss[-1])
    on.close(), loop.close()


@pytest.mark.parametrize("F,k", SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_three_lines_within_the_batch_steps_bound(built, F, k, weighted):
    lam = 1e-2
    rows, ids, wts, y, ref_rows, ref_b, ref_p, ref_loss = oc.solved(F, k, 3, seed_of(F, k), weighted, LR_SGD, lam)
    on = model(F, k, rows, lam)
    out = on.train_online(ids, y, wts=wts, want_p=True)
    got, gb = on.get_params()
    change = np.abs(ref_rows - rows).max() + 1e-12
    assert np.abs(got - ref_rows).max() <= 2e-3 * change + 2e-7
    assert abs(gb - ref_b) <= 2e-3 * abs(ref_b - oc.B0) + 2e-7
    np.testing.assert_allclose(out['p'].cpu().numpy(), ref_p, rtol=5e-5, atol=1e-6)
    on.close()


@pytest.mark.parametrize("N", [0, 1, 2])
def test_zero_one_and_two_lines(built, N):
    F, k, lam = 16, 11, 1e-2
    rows, ids, wts, y = oc.build(F, k, 3, 5, True)
    ref_rows, ref_b, ref_p, ref_loss = oc.sequential(rows, oc.B0, ids[:N], wts[:N], y[:N], LR_SGD, lam)
    on = model(F, k, rows, lam)
    out = on.train_online(ids[:N], y[:N], wts=wts[:N], want_p=True)
    got, gb = on.get_params()
    assert out['p'].shape == (N,)
    if N == 0:
        assert np.array_equal(got, rows.astype(np.float32)) and gb == np.float32(oc.B0) and out['loss'] == 0.0 and out['loss_last'] == 0.0
    else:
        change = np.abs(ref_rows - rows).max() + 1e-12
        assert np.abs(got - ref_rows).max() <= 2e-3 * change + 2e-7
        assert abs(gb - ref_b) <= 2e-3 * abs(ref_b - oc.B0) + 2e-7
        np.testing.assert_allclose(out['p'].cpu().numpy(), ref_p, rtol=5e-5, atol=1e-6)
        assert abs(out['loss'] - ref_loss.sum()) <= 2e-5 * max(1.0, ref_loss.sum())
        assert abs(out['loss_last'] - ref_loss[-1]) <= 2e-5
    on.close()


@pytest.mark.parametrize("F,k", [(16, 11), (16, 101)])
def test_batch_steps_and_online_calls_interleave(built, F, k):
    lam = 1e-2
    rows, ids, wts, y = oc.build(F, k, 104, 21, True)
    m = model(F, k, rows, lam, shared=True, batch=32)
    w64 = wts.astype(np.float64)
    r, b = rows.copy(), oc.B0
    m.train_step(ids[:32], y[:32], wts=wts[:32])
    b, _, _ = oc.wr.sgd_step_w(r, b, ids[:32], w64[:32], y[:32], LR_SGD, lam, True)
    out = m.train_online(ids[32:72], y[32:72], wts=wts[32:72], want_p=True)
    r, b, p, _ = oc.sequential(r, b, ids[32:72], wts[32:72], y[32:72], LR_SGD, lam)
    m.train_step(ids[72:], y[72:], wts=wts[72:])
    b, _, _ = oc.wr.sgd_step_w(r, b, ids[72:], w64[72:], y[72:], LR_SGD, lam, True)
    got, gb = m.get_params()
    change = np.abs(r - rows).max() + 1e-12
    assert np.abs(got - r).max() <= 2e-3 * change + 2e-7
    assert abs(gb - b) <= 2e-3 * abs(b - oc.B0) + 2e-7
    np.testing.assert_allclose(out['p'].cpu().numpy(), p, rtol=5e-5, atol=1e-6)
    assert m.count_shared_rows() >= 0                             # still the last BATCH step's marks: the call is legal
    m.close()


@pytest.mark.parametrize("F,k", [(16, 11), (64, 128)])
def test_launch_cuts_change_no_bit(built, monkeypatch, F, k):
    """FM_ONLINE_CHUNK=7 cuts 50 lines into eight launches; also: shared_rows on or off is the same call."""
    lam = 1e-2
    rows, ids, wts, y = oc.build(F, k, 50, 31, True)
    res = []
    for chunk, shared in ((None, False), ('7', False), ('1', True)):
        if chunk is None:
            monkeypatch.delenv('FM_ONLINE_CHUNK', raising=False)
        else:
            monkeypatch.setenv('FM_ONLINE_CHUNK', chunk)
        m = model(F, k, rows, lam, shared=shared)
        out = m.train_online(ids, y, wts=wts, want_p=True)
        res.append(m.get_params() + (out['p'].cpu().numpy(), out['loss'], out['loss_last']))
        m.close()
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and res[0][1] == other[1] and np.array_equal(res[0][2], other[2])
        assert res[0][3:] == other[3:]
    assert not np.array_equal(res[0][0], rows.astype(np.float32))


@pytest.mark.parametrize("F,k", [(16, 11), (16, 17)])
def test_the_call_cuts_where_the_scale_folds(built, F, k):
    """lr * lambda = 0.5 halves the scale with every line: in 60 lines it leaves 2^-24 twice, and the call cuts and folds there."""
    rows, ids, wts, y = oc.build(F, k, 60, 41, False)
    ref_rows, ref_b, _, _ = oc.sequential(rows, 0.0, ids, None, y, 0.5, 1.0)
    m = model(F, k, rows, 1.0, ptmzr=('sgd', 0.5), b=0.0)
    m.train_online(ids, y, want_loss=False)
    got, gb = m.get_params()
    np.testing.assert_allclose(got, ref_rows, rtol=2e-3, atol=1e-9)
    np.testing.assert_allclose(gb, ref_b, rtol=2e-3, atol=1e-9)
    m.close()


@pytest.mark.parametrize("ptmzr", [('adam', 0.01, 1e-8), ('ftrl', 0.05)])
def test_adam_and_ftrl_are_refused(built, ptmzr):
    rows, ids, wts, y = oc.build(16, 11, 5, 51, False)
    m = model(16, 11, rows, 1e-2, ptmzr=ptmzr)
    before = m.get_params()
    with pytest.raises(FNNError) as e:
        m.train_online(ids, y)
    assert e.value.code == _capi.FNN_ERR_STATE
    after = m.get_params()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    m.close()


@pytest.mark.parametrize("F,k", [(16, 11), (16, 101)])
def test_an_id_out_of_range_is_masked_and_reported(built, F, k):
    lam = 1e-2
    rows, ids, wts, y = oc.build(F, k, 9, 61, True)
    bad = ids.copy()
    ids[4, 2] = -1
    bad[4, 2] = rows.shape[0]                                     # n_rows itself: one past the table
    ref_rows, ref_b, ref_p, _ = oc.sequential(rows, oc.B0, ids, wts, y, LR_SGD, lam)
    m = model(F, k, rows, lam)
    out = m.train_online(bad, y, wts=wts, want_p=True, want_loss=False)
    assert m.lib.fm_sync(m.h) == _capi.FNN_ERR_RANGE
    assert m.lib.fm_sync(m.h) == _capi.FNN_OK                     # reported once
    got, gb = m.get_params()
    change = np.abs(ref_rows - rows).max() + 1e-12
    assert np.abs(got - ref_rows).max() <= 2e-3 * change + 2e-7
    assert abs(gb - ref_b) <= 2e-3 * abs(ref_b - oc.B0) + 2e-7
    np.testing.assert_allclose(out['p'].cpu().numpy(), ref_p, rtol=5e-5, atol=1e-6)
    m.close()


def write_yzx(path, n, seed, n_feat=40):
    rng = np.random.RandomState(seed)
    w = rng.standard_normal(n_feat)
    with open(path, 'w') as f:
        for _ in range(n):
            feats = list(rng.randint(0, n_feat, size=rng.randint(1, 8)))
            if len(feats) > 2 and rng.uniform() < 0.3:
                feats[-1] = feats[0]
            yy = int(rng.uniform() < 1.0 / (1.0 + np.exp(-w[feats].sum())))
            f.write('%d 0 %s\n' % (yy, ' '.join('%d:1' % v for v in feats)))


def test_the_driver_runs_the_online_schedule(built, tmp_path):
    """ipinyou.run(online=True) on 200 lines in buffers of 80: log and final parameters equal train_online called by hand on the
    same buffers (the global RNG seeded alike gives the same buffer order)."""
    train, test, log = str(tmp_path / 'train.yzx'), str(tmp_path / 'test.yzx'), str(tmp_path / 'log')
    write_yzx(train, 200, 1), write_yzx(test, 150, 2)
    np.random.seed(99)
    res = ipinyou.run(train, test, 'FM', batch_size=4096, buffer=80, eval_size=1000, epochs=1, log_file=log, echo=False, online=True)
    got, gb = res['model'].get_params()
    res['model'].close()
    np.random.seed(99)
    (d1, f1), (d2, f2) = ipinyou.stat(train), ipinyou.stat(test)
    X_dim, X_feas = max(d1, d2) + 2, max(f1, f2)
    m = FM(1, [X_dim, X_feas, 10], ['uniform', -0.001, 0.001, [0x3210, 0x7654], None], ['sgd', 1e-3], [1e-2], 'train', 1000,
           shared_rows=True)
    hand, step = [], 0
    with open(train) as fin:
        while True:
            X_ind, X_val, y = ipinyou.load_ipinyou_data(fin, 80, X_dim - 1, X_feas)
            if X_ind is None:
                break
            ids, wts = ipinyou.to_column_ids(X_ind, X_val)
            out = m.train_online(ids, y, wts=wts, want_p=True)
            step += len(y)
            with open(test) as ft:
                t_ind, t_val, t_y = ipinyou.load_ipinyou_data(ft, 1000, X_dim - 1, X_feas)
                assert ipinyou.load_ipinyou_data(ft, 1000, X_dim - 1, X_feas)[0] is None
            t_ids, t_wts = ipinyou.to_column_ids(t_ind, t_val)
            hand.append((step, ipinyou.exact_auc(y, out['p'].cpu().numpy()), m.evaluate(t_ids, t_y, wts=t_wts)[0], out['loss_last']))
    want, wb = m.get_params()
    m.close()
    assert len(hand) == 3 and res['log'] == hand
    assert np.array_equal(got, want) and gb == wb
    lines = open(log).read().splitlines()
    assert lines[1:] == ['%d\t%g\t%g\t%g\t' % h for h in hand]
