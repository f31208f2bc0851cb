"""Several FM / LR models evaluated on one test feed in one call (fm_predict_multi / fm_eval_multi, FM.predict_many /
FM.evaluate_many, ipinyou.run_many) on the device.  The yardstick throughout is the single-model entry points in the same
process -- `forward` (fm_predict_w in chunks of max_batch) and `evaluate` (fm_eval_w) -- and the comparison is `==` on bits:
model m of a call gives what it gives alone, whatever the other members are, however the call is cut into groups, with a lazy
SGD scale pending, and without a bit of any model changing.  The feeds are tests/fm_online_cases.py's (repeated rows, a row
twice on a line, absent fields, all-absent lines; weights with zeros and negatives)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fm_online_cases as oc
import metrics_ref as mr

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import FM as fm_module
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM, evaluate_many, predict_many, train_online_many
from deep_ctr_amd.LR import LR
from deep_ctr_amd.engine import FNNError

pytestmark = pytest.mark.gpu
INIT = ['uniform', -0.001, 0.001, [1, 2], None]
OK, ARG, STATE, RANGE = _capi.FNN_OK, _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE, _capi.FNN_ERR_RANGE


@functools.lru_cache(maxsize=None)
def feed(F, N, seed, n_rows=1000):
    """(ids, wts, y int32) of N lines; the weights are dropped by the unweighted cases.  Built once and shared: callers do not write to it."""
    _, ids, wts, y = oc.build(F, 4, N, seed, True, n_rows=n_rows)
    return ids, wts, y.astype(np.int32)


def model(F, k, n_rows=1000, seed=1, b=oc.B0, max_batch=512, ptmzr=('sgd', 0.05), lam=1e-2, shared=False):
    m = FM(max_batch, [n_rows, F, k - 1], INIT, list(ptmzr), [lam], 'train', 0, shared_rows=shared)
    assert m.max_batch == max_batch
    m.set_params(oc.build(F, k, 12, seed, False, n_rows=n_rows)[0], b)
    return m


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, 'cpu') else a, dtype=np.float32).view(np.uint32)


def same3(got, want):
    """The three doubles equal as bits (NaN included)."""
    return np.asarray(got, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()


def solo(m, ids, y, wts):
    """(p bits, (auc, rmse, logloss)) of the single-model entry points: `forward`, and fm_eval_w itself, which with one class only
    in y (the one-line case) still writes RMSE and logloss beside a NaN AUC."""
    torch = m._torch
    ids_t, y_t = m._dev(ids, torch.int32), m._dev(y, torch.int32)
    w_t = None if wts is None else m._dev(wts, torch.float32)
    v = [C.c_double() for _ in range(3)]
    torch.cuda.synchronize()
    rc = m.lib.fm_eval_w(m.h, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0],
                         *[C.byref(x) for x in v])
    n_pos = int((y_t != 0).sum())
    assert rc == (OK if 0 < n_pos < ids_t.shape[0] else RANGE), m.lib.fm_last_error(m.h)
    return bits(m.forward(ids_t, wts=w_t)), tuple(x.value for x in v)


def triple(r):
    return r['auc'], r['rmse'], r['logloss']


def check_equal_solo(models, ids, y, wts, what=''):
    ps, rs = predict_many(models, ids, wts=wts), evaluate_many(models, ids, y, wts=wts)
    for i, m in enumerate(models):
        p, want = solo(m, ids, y, wts)
        assert np.array_equal(bits(ps[i]), p), '%s model %d: p' % (what, i)
        assert rs[i]['status'] == OK and same3(triple(rs[i]), want), '%s model %d: %r %r' % (what, i, rs[i], want)
    return ps, rs


# ------------------------------------------------------------------------------------------------ one model, every layout
@pytest.mark.parametrize("F", [1, 16, 17, 39, 64])
@pytest.mark.parametrize("k", [1, 11, 16, 17, 64, 65, 101, 128])
def test_one_model_every_layout(built, k, F):
    """NF / NC = 1..4 and L = 16 | 32; with and without wts; N not a multiple of 16, of 2,048 or of max_batch = 4,096."""
    import torch
    ids, wts, y = feed(F, 10000, 300 + F)
    assert (ids == -1).any() and ids.max() < 1000
    m = model(F, k, max_batch=4096)
    ids_t, w_t, y_t = m._dev(ids, torch.int32), m._dev(wts, torch.float32), m._dev(y, torch.int32)
    for N in (1, 15, 17, 2049, 4097, 10000):
        for w in (None, w_t):
            check_equal_solo([m], ids_t[:N], y_t[:N], None if w is None else w[:N], 'N %d wts %s' % (N, w is not None))
    m.close()


# ------------------------------------------------------------------------------------------------ a mixed group
def mixed_group(F=16):
    return [LR_(F, 1400), model(F, 11, 1000, 2), model(F, 16, 1200, 3, shared=True), model(F, 17, 1100, 4), model(F, 101, 1300, 5)]


def LR_(F, n_rows, seed=6):
    m = LR(512, [n_rows, F], INIT, ['sgd', 0.05], [1e-3], 'train', 0)
    m.set_params(oc.build(F, 1, 12, seed, False, n_rows=n_rows)[0], 0.05)
    return m


@pytest.mark.parametrize("weighted", [False, True])
def test_a_mixed_group_equals_its_solo_calls(built, weighted):
    ids, wts, y = feed(16, 2500, 11)
    wts = wts if weighted else None
    g = mixed_group()
    _, fwd = check_equal_solo(g, ids, y, wts, 'in order')
    _, rev = check_equal_solo(g[::-1], ids, y, wts, 'reversed')
    assert [triple(r) for r in rev[::-1]] == [triple(r) for r in fwd]
    _, dup = check_equal_solo(g + [g[1]], ids, y, wts, 'one handle twice')
    assert triple(dup[5]) == triple(dup[1])
    assert len(set(r['rmse'] for r in fwd)) == 5                    # five different models, not one answer five times
    for m in g:
        m.close()


@pytest.mark.parametrize("F", [1, 39])
def test_a_mixed_group_at_other_field_counts(built, F):
    ids, wts, y = feed(F, 2100, 20 + F)
    g = [LR_(F, 1000), model(F, 11), model(F, 17), model(F, 65)]
    check_equal_solo(g, ids, y, wts)
    for m in g:
        m.close()


# ------------------------------------------------------------------------------------------------ a pending scale; optimisers
def one_column_batch(B=32):
    """Every row under one column of the batch: the batch step is then reproducible bit for bit (include/fm_hip.h)."""
    return (17 * np.arange(16) + np.random.RandomState(3).randint(0, 17, size=(B, 16))).astype(np.int32)


def test_a_pending_scale_is_applied_and_not_folded(built):
    """After online steps with lambda > 0 the tables are `scale * stored` with the scale unfolded; after a batch step too.  The
    group evaluation equals each model's own, and what it leaves behind equals what twins that were only trained hold."""
    ids, wts, y = feed(16, 2500, 31)
    b_ids = one_column_batch()

    def trained():
        g = [model(16, 11, seed=1, lam=1e-2), model(16, 17, seed=2, lam=3e-2), model(16, 1, seed=3, lam=2e-2), model(16, 101, seed=4, lam=1e-2)]
        train_online_many(g, ids[:300], y[:300].astype(np.float32), wts=wts[:300])
        g[1].train_step(b_ids, y[300:332].astype(np.float32), wts=wts[300:332])       # a batch step on top, on one of them
        return g
    g, twins = trained(), trained()
    none = [model(16, 11, seed=1), model(16, 17, seed=2), model(16, 1, seed=3), model(16, 101, seed=4)]
    _, rs = check_equal_solo(g, ids, y, wts)
    _, r0 = check_equal_solo(none, ids, y, wts)
    assert all(triple(a) != triple(b) for a, b in zip(rs, r0))      # the training, scale included, shows in the numbers
    for m, t in zip(g, twins):
        (rows, b), (trows, tb) = m.get_params(), t.get_params()
        assert np.array_equal(bits(rows), bits(trows)) and b == tb
    for m in g + twins + none:
        m.close()


@pytest.mark.parametrize("ptmzr", [('adam', 0.01, 1e-8), ('ftrl', 0.05)])
def test_adam_and_ftrl_handles_predict(built, ptmzr):
    ids, wts, y = feed(16, 2500, 33)
    b_ids = one_column_batch()

    def trained():
        g = [model(16, 11, seed=1, ptmzr=ptmzr), model(16, 17, seed=2, ptmzr=ptmzr), model(16, 11, seed=3)]
        for m in g:
            m.train_step(b_ids, y[:32].astype(np.float32), wts=wts[:32])
        return g
    g, twins = trained(), trained()
    check_equal_solo(g, ids, y, wts)
    for m, t in zip(g, twins):
        (rows, b), (trows, tb) = m.get_params(), t.get_params()
        assert np.array_equal(bits(rows), bits(trows)) and b == tb
    for a, b in zip(g[:2], twins[:2]):
        for u, v in zip(a.get_opt_state()[:3], b.get_opt_state()[:3]):
            assert np.array_equal(bits(u), bits(v))
    for m in g + twins:
        m.close()


# ------------------------------------------------------------------------------------------------ groups; many models
def test_groups_change_no_bit(built, monkeypatch):
    """About 12.5 N bytes a model: at N = 2,049 a cap of 60,000 bytes holds two models, so nine run as five groups."""
    ids, wts, y = feed(16, 2049, 41)
    g = [model(16, (11, 1, 50, 17, 101)[i % 5], seed=60 + i, n_rows=1000 + 10 * i) for i in range(9)]
    monkeypatch.delenv('FM_EVAL_SCRATCH_BYTES', raising=False)
    _, whole = check_equal_solo(g, ids, y, wts, 'one group')
    for cap in ('60000', '1'):                                       # pairs; one model a group
        monkeypatch.setenv('FM_EVAL_SCRATCH_BYTES', cap)
        cut = evaluate_many(g, ids, y, wts=wts)
        assert [triple(r) for r in cut] == [triple(r) for r in whole], cap
    for order in ('model', 'tile'):                                  # the grid order of the predictions changes no bit either
        monkeypatch.setenv('FM_EVAL_ORDER', order)
        check_equal_solo(g, ids, y, wts, 'order ' + order)
    for m in g:
        m.close()


def test_260_tiny_models_more_than_cus(built):
    ids, wts, y = feed(4, 33, 51, n_rows=300)
    g = [model(4, 3, n_rows=300, seed=5 + i % 7, b=0.01 * i, max_batch=8) for i in range(260)]
    _, rs = check_equal_solo(g, ids, y, wts)
    assert len(set(r['logloss'] for r in rs)) > 200
    for m in g:
        m.close()


# ------------------------------------------------------------------------------------------------ the raw call
def raw_eval(models, ids_t, w_t, y_t, N, hs=None, n_models=None, fill=-7.0):
    """fm_eval_multi through ctypes, outputs pre-filled: (rc, auc, rmse, logloss, status) as lists."""
    M = len(models)
    hs = (C.c_void_p * M)(*[m.h.value for m in models]) if hs is None else hs
    out = [(C.c_double * M)(*([fill] * M)) for _ in range(3)]
    status = (C.c_int * M)(*([77] * M))
    models[0]._torch.cuda.synchronize()                           # the tensors were made on another stream than the handles'
    rc = models[0].lib.fm_eval_multi(hs, M if n_models is None else n_models, None if ids_t is None else ids_t.data_ptr(),
                                     None if w_t is None else w_t.data_ptr(), None if y_t is None else y_t.data_ptr(), N,
                                     out[0], out[1], out[2], status)
    return (rc,) + tuple(list(o) for o in out) + (list(status),)


def dev(m, ids, wts, y):
    import torch
    return m._dev(ids, torch.int32), None if wts is None else m._dev(wts, torch.float32), m._dev(y, torch.int32)


def message(m):
    return m.lib.fm_last_error(m.h).decode()


# ------------------------------------------------------------------------------------------------ metric edges, per model
EDGE_ROWS = np.asarray([[1.0], [np.inf], [-np.inf]], np.float32)


def edge_models():
    """One field, rank 0.  Model 0 reproduces the battery's logits (tests/test_gpu_metrics_edges.py: row 0 weighted by z, an
    infinite logit is row 1 or 2 at weight 1); the others have zero rows and a bias alone: every prediction 1.0, 0.5, 0.0."""
    ms = []
    for rows, b in ((EDGE_ROWS, 0.0), (np.zeros((3, 1), np.float32), 40.0), (np.zeros((3, 1), np.float32), 0.0),
                    (np.zeros((3, 1), np.float32), -200.0)):
        m = LR(4096, [3, 1], INIT, ['sgd', 0.05], [0.0], 'train', 0)
        m.set_params(rows, b)
        ms.append(m)
    return ms


def edge_feed(z):
    z = np.asarray(z, np.float32)
    ids, w = np.zeros((len(z), 1), np.int32), z.reshape(-1, 1).copy()
    for row in (1, 2):
        hit = z == EDGE_ROWS[row, 0]
        ids[hit, 0], w[hit, 0] = row, 1.0
    return ids, w


@pytest.mark.parametrize("name", ['saturated', 'all-equal', 'three-values', 'N2049-positives-in-last-block'])
def test_metric_edges_per_model(built, name):
    """Saturated and tied predictions, model by model: equal to fm_eval_w as bits, and against tests/metrics_ref.py on the
    device's own predictions under the bounds of tests/test_gpu_metrics_edges.py (AUC equal, RMSE / logloss 1e-12 relative)."""
    z, y = mr.battery(name)
    ids, w = edge_feed(z)
    y = np.array(y)
    ms = edge_models()
    ps, rs = check_equal_solo(ms, ids, y, w)
    mr.precondition(name, ps[0].cpu().numpy(), y)
    for p, v in zip(ps[1:], (1.0, 0.5, 0.0)):
        assert (p.cpu().numpy() == np.float32(v)).all()
    for i, (p, r) in enumerate(zip(ps, rs)):
        ref = mr.metrics_ref(p.cpu().numpy(), y)
        d = [abs(r[k] - ref[j]) / abs(ref[j]) if ref[j] else abs(r[k]) for j, k in ((1, 'rmse'), (2, 'logloss'))]
        print("[eval-multi edges] %s model %d: auc %.17g (reference %.17g) relative deviation rmse %.2e logloss %.2e" % (name, i, r['auc'], ref[0], d[0], d[1]))
        assert r['auc'] == ref[0] and max(d) <= 1e-12
        if i:
            assert r['auc'] == 0.5                                    # every pair a tie
    for m in ms:
        m.close()


def test_one_diverged_model_among_four(built):
    ids, wts, y = feed(16, 2500, 61)
    g = [model(16, 11, seed=1), model(16, 17, seed=2), model(16, 11, seed=3), model(16, 1, seed=4)]
    rows = oc.build(16, 11, 12, 3, False, n_rows=1000)[0].copy()
    rows[:, 0] = np.nan
    g[2].set_params(rows, oc.B0)
    ids_t, w_t, y_t = dev(g[0], ids, wts, y)
    rc, auc, rmse, ll, status = raw_eval(g, ids_t, w_t, y_t, len(y))
    assert rc == RANGE and status == [OK, OK, RANGE, OK]
    assert np.isnan([auc[2], rmse[2], ll[2]]).all()
    msg = message(g[0])
    assert 'fm_eval_multi' in msg and 'outside [0, 1] in model(s) 2' in msg, msg
    for i in (0, 1, 3):
        assert same3((auc[i], rmse[i], ll[i]), g[i].evaluate(ids, y, wts=wts))
    with pytest.raises(FNNError):
        g[2].evaluate(ids, y, wts=wts)
    rs = evaluate_many(g, ids, y, wts=wts)                           # the Python call does not raise for it
    assert [r['status'] for r in rs] == status and [r['rmse'] for r in rs[:2]] == rmse[:2] and np.isnan(rs[2]['auc'])
    for m in g:
        m.close()


def test_one_class_only(built):
    ids, wts, y = feed(16, 2500, 63)
    g = [model(16, 11, seed=1), model(16, 17, seed=2)]
    ids_t, w_t, _ = dev(g[0], ids, wts, y)
    good = evaluate_many(g, ids, y, wts=wts)
    for y1 in (np.zeros(len(y), np.int32), np.full(len(y), 7, np.int32)):
        y_t = g[0]._dev(y1, g[0]._torch.int32)
        rc, auc, rmse, ll, status = raw_eval(g, ids_t, w_t, y_t, len(y))
        assert rc == RANGE and status == [OK, OK] and np.isnan(auc).all() and 'one class' in message(g[0])
        for i, m in enumerate(g):
            want = C.c_double(), C.c_double(), C.c_double()
            assert m.lib.fm_eval_w(m.h, ids_t.data_ptr(), w_t.data_ptr(), y_t.data_ptr(), len(y), *[C.byref(v) for v in want]) == RANGE
            assert np.isnan(want[0].value) and (rmse[i], ll[i]) == (want[1].value, want[2].value)
        rs = evaluate_many(g, ids, y1, wts=wts)                      # no exception: the AUCs are NaN
        assert all(np.isnan(r['auc']) and r['status'] == OK for r in rs) and [r['rmse'] for r in rs] == rmse
    assert [triple(r) for r in evaluate_many(g, ids, y, wts=wts)] == [triple(r) for r in good]
    for m in g:
        m.close()


def test_an_id_out_of_range_is_per_model(built):
    """The feed's largest id fits model 0's 1,000 rows and not model 1's 900: only model 1 is named, for which the id is absent."""
    ids, wts, y = feed(16, 2500, 65)
    assert 900 <= ids.max() < 1000
    g = [model(16, 11, 1000, seed=1), model(16, 11, 900, seed=2)]
    ids_t, w_t, y_t = dev(g[0], ids, wts, y)
    want = []
    for i, m in enumerate(g):
        v = [C.c_double() for _ in range(3)]
        rc = m.lib.fm_eval_w(m.h, ids_t.data_ptr(), w_t.data_ptr(), y_t.data_ptr(), len(y), *[C.byref(x) for x in v])
        assert rc == (RANGE if i else OK)
        want.append(tuple(x.value for x in v))
    rc, auc, rmse, ll, status = raw_eval(g, ids_t, w_t, y_t, len(y))
    assert rc == RANGE and status == [OK, OK]
    listed = message(g[0]).split('n_rows) in model(s)')[1]
    assert '1' in listed and '0' not in listed, message(g[0])
    for i in range(2):
        assert same3((auc[i], rmse[i], ll[i]), want[i])
    assert [m.lib.fm_sync(m.h) for m in g] == [OK, OK]                # reported once, by the call
    with pytest.raises(FNNError) as e:
        evaluate_many(g, ids, y, wts=wts)
    assert e.value.code == RANGE
    with pytest.raises(FNNError) as e:
        predict_many(g, ids, wts=wts)
    assert e.value.code == RANGE and 'model(s) 1' in str(e.value)
    assert [m.lib.fm_sync(m.h) for m in g] == [OK, OK]
    for m in g:
        m.close()


# ------------------------------------------------------------------------------------------------ streams
def test_the_call_waits_for_work_queued_on_another_handles_stream(built):
    """Sixteen B = 1 train_steps enqueued on model 1's stream (no loss asked for, device tensors: nothing synchronises), then
    the group call at once: its launches run on model 0's stream and must wait for those steps.  A twin that took the same
    steps and was evaluated alone gives the same bits."""
    import torch
    ids, wts, y = feed(16, 2500, 71)
    b_ids = one_column_batch(16)

    def steps(m, t_ids, t_y):
        for n in range(16):
            m.train_step(t_ids[n:n + 1], t_y[n:n + 1], want_loss=False)
    g = [model(16, 11, seed=1), model(16, 17, seed=2), model(16, 1, seed=3)]
    assert len(set(m.stream.cuda_stream for m in g)) == 3
    ids_t, w_t, y_t = dev(g[0], ids, wts, y)
    bi_t, by_t = g[0]._dev(b_ids, torch.int32), g[0]._dev(y[:16], torch.float32)
    before = g[1].evaluate(ids_t, y_t, wts=w_t)
    M = 3
    hs = (C.c_void_p * M)(*[m.h.value for m in g])
    out = [(C.c_double * M)() for _ in range(3)]
    torch.cuda.synchronize()
    steps(g[1], bi_t, by_t)
    assert g[0].lib.fm_eval_multi(hs, M, ids_t.data_ptr(), w_t.data_ptr(), y_t.data_ptr(), len(y), out[0], out[1], out[2], None) == OK
    twin = model(16, 17, seed=2)
    steps(twin, bi_t, by_t)
    want = twin.evaluate(ids_t, y_t, wts=w_t)
    assert want != before and same3((out[0][1], out[1][1], out[2][1]), want)
    for i in (0, 2):
        assert same3((out[0][i], out[1][i], out[2][i]), g[i].evaluate(ids_t, y_t, wts=w_t))
    (rows, b), (trows, tb) = g[1].get_params(), twin.get_params()
    assert np.array_equal(bits(rows), bits(trows)) and b == tb
    for m in g + [twin]:
        m.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(built):
    ids, wts, y = feed(16, 40, 81)
    g = [model(16, 11, seed=1), model(16, 17, seed=2), model(16, 1, seed=3)]
    m0, lib = g[0], g[0].lib
    ids_t, w_t, y_t = dev(m0, ids, wts, y)
    N = len(y)
    other_f = model(15, 11, seed=4)
    bare = FM.__new__(FM)                                          # a handle that never saw fm_set_table
    bare.h, bare.lib = C.c_void_p(), lib
    assert lib.fm_create(16, 11, 1, 0, C.c_void_p(m0.stream.cuda_stream), C.byref(bare.h)) == 0
    one_null = (C.c_void_p * 3)(g[0].h.value, None, g[2].h.value)
    cases = [
        ('n_fields differ', ARG, 2, lambda: raw_eval(g[:2] + [other_f], ids_t, w_t, y_t, N)),
        ('no table', STATE, 1, lambda: raw_eval([g[0], bare, g[2]], ids_t, w_t, y_t, N)),
        ('N = 0', ARG, None, lambda: raw_eval(g, ids_t, w_t, y_t, 0)),
        ('N < 0', ARG, None, lambda: raw_eval(g, ids_t, w_t, y_t, -1)),
        ('N > 2^30', ARG, None, lambda: raw_eval(g, ids_t, w_t, y_t, (1 << 30) + 1)),
        ('null y', ARG, None, lambda: raw_eval(g, ids_t, w_t, None, N)),
        ('null ids', ARG, None, lambda: raw_eval(g, None, w_t, y_t, N)),
        ('null entry', ARG, 1, lambda: raw_eval(g, ids_t, w_t, y_t, N, hs=one_null)),
    ]
    for name, code, index, call in cases:
        rc, auc, rmse, ll, status = call()
        assert rc == code, name
        assert auc == [-7.0] * 3 and rmse == [-7.0] * 3 and ll == [-7.0] * 3 and status == [77] * 3, name
        msg = message(m0)
        assert 'fm_eval_multi' in msg, (name, msg)
        if index is not None:
            assert 'model %d' % index in msg, (name, msg)
    p = [m0._torch.full((N,), -7.0, dtype=m0._torch.float32, device=m0.device) for _ in range(3)]
    p_arr = (C.c_void_p * 3)(*[t.data_ptr() for t in p])
    hs = (C.c_void_p * 3)(*[m.h.value for m in g])
    hs_bare = (C.c_void_p * 3)(g[0].h.value, bare.h.value, g[2].h.value)
    m0._torch.cuda.synchronize()
    assert lib.fm_predict_multi(hs, 3, ids_t.data_ptr(), None, 0, p_arr) == ARG
    assert lib.fm_predict_multi(hs, 3, None, None, N, p_arr) == ARG
    assert lib.fm_predict_multi(hs, 3, ids_t.data_ptr(), None, N, None) == ARG
    assert lib.fm_predict_multi(hs_bare, 3, ids_t.data_ptr(), None, N, p_arr) == STATE and 'fm_predict_multi' in message(m0)
    assert lib.fm_sync(m0.h) == OK and all((t.cpu().numpy() == -7.0).all() for t in p)
    # a null entry of p_out is allowed: that model's predictions are not wanted
    p_arr[1] = None
    assert lib.fm_predict_multi(hs, 3, ids_t.data_ptr(), w_t.data_ptr(), N, p_arr) == OK and lib.fm_sync(m0.h) == OK
    assert (p[1].cpu().numpy() == -7.0).all()
    for i in (0, 2):
        assert np.array_equal(bits(p[i]), bits(g[i].forward(ids_t, wts=w_t)))
    with pytest.raises(ValueError):
        evaluate_many([], ids, y)
    with pytest.raises(ValueError):
        predict_many([g[0], other_f], ids)
    closed = model(16, 11, seed=7)
    closed.close()
    with pytest.raises(FNNError) as e:
        evaluate_many([closed, g[1]], ids, y)
    assert e.value.code == ARG and 'model 0' in str(e.value)
    lib.fm_destroy(bare.h)
    bare.h = None                                                  # or FM.__del__ destroys it a second time
    for m in g + [other_f]:
        m.close()


def test_the_same_call_twice_gives_the_same_bits(built):
    ids, wts, y = feed(16, 2500, 91)
    g = mixed_group()
    a, b = evaluate_many(g, ids, y, wts=wts), evaluate_many(g, ids, y, wts=wts)
    assert [triple(r) for r in a] == [triple(r) for r in b]
    pa, pb = predict_many(g, ids, wts=wts), predict_many(g, ids, wts=wts)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(pa, pb))
    for m in g:
        m.close()


# ------------------------------------------------------------------------------------------------ the driver
def test_the_driver_logs_each_models_own_evaluation(built, golden_dir, tmp_path, monkeypatch):
    """ipinyou.run_many on the demo file: every evaluation of every buffer goes through ONE evaluate_many call, and the AUC it
    logs is the one the model's own `evaluate` gives on the same lines at that moment, formatted as `run` formats it."""
    path = os.path.join(golden_dir, 'demo', 'train.yzx.txt')
    specs = [('FM', 10, 1e-3, 1e-2), ('LR', 0, 1e-3, 1e-3), ('FM', 20, 2e-3, 1e-2)]
    calls = []
    real = fm_module.evaluate_many

    def spy(models, ids, y, wts=None):
        out = real(models, ids, y, wts=wts)
        calls.append(([r['auc'] for r in out], [m.evaluate(ids, y, wts=wts)[0] for m in models]))
        return out
    monkeypatch.setattr(fm_module, 'evaluate_many', spy)
    log = str(tmp_path / 'many.log')
    np.random.seed(123)
    many = ipinyou.run_many(path, path, specs, buffer=500, eval_size=1000, log_file=log, echo=False)
    assert len(calls) == 3                                           # one call per buffer, not one per model
    lines = open(log).read().splitlines()
    assert len(lines) == 3 * 4
    for i in range(3):
        mine = [l.split('\t') for l in lines if l.startswith('%d\t' % i)][1:]
        assert len(mine) == 3 and len(many[i]['log']) == 3
        for (got, want), fields, rec in zip(calls, mine, many[i]['log']):
            assert got[i] == want[i] and rec[2] == want[i] and fields[3] == '%g' % want[i]
        many[i]['model'].close()
