"""Several FM / LR models on the online schedule in one pass (fm_train_online_multi, FM.train_online_many, ipinyou.run_many)
on the device.  The rule throughout: model m of a group call ends BIT FOR BIT as a fresh handle with the same table and b ends
after fm_train_online alone ("solo") -- table, b, p, loss_sum, loss_last -- whatever the other members of the group are.
One group is also held against the float64 sequential reference of tests/fm_online_cases.py under the parity rule of
tests/test_gpu_fm_online.py (err_online <= 2 * err_loop + 2e-7, the loop being the schedule as train_step calls at B = 1).
Handles are created with max_batch = 1, which keeps the many-handle cases light."""
import ctypes as C

import numpy as np
import pytest

import fm_online_cases as oc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM, train_online_many
from deep_ctr_amd.LR import LR
from deep_ctr_amd.engine import FNNError

pytestmark = pytest.mark.gpu
INIT = ['uniform', -0.001, 0.001, [1, 2], None]


class Spec(object):
    """One member of a group: its shape, its own table (seeded), learning rate and L2 weight."""
    def __init__(self, F, k, lr=0.05, lam=1e-2, seed=1, n_rows=oc.N_ROWS, shared=False, b=oc.B0, ptmzr=None):
        self.F, self.k, self.lr, self.lam, self.seed, self.n_rows, self.shared, self.b = F, k, lr, lam, seed, n_rows, shared, b
        self.ptmzr = ptmzr

    def rows(self):
        return oc.build(self.F, self.k, 12, self.seed, False, n_rows=self.n_rows)[0]

    def model(self):
        m = FM(1, [self.n_rows, self.F, self.k - 1], INIT, list(self.ptmzr or ('sgd', self.lr)), [self.lam], 'train', 0,
               shared_rows=self.shared)
        m.set_params(self.rows(), self.b)
        return m


def feed(F, N, seed, weighted, n_rows=oc.N_ROWS):
    """The lines of a group: fm_online_cases' (repeated rows, a row twice on a line, absent lines, ...); the table it builds is not used."""
    _, ids, wts, y = oc.build(F, 4, N, seed, weighted, n_rows=n_rows)
    return ids, wts, y


def result(m, out):
    rows, b = m.get_params()
    p = None if out is None or out['p'] is None else out['p'].cpu().numpy()
    return rows, np.float32(b), p, None if out is None else out['loss'], None if out is None else out['loss_last']


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=''):
    """Equal as bits: table, b, p; equal as numbers (f64 / f32 read back unchanged): the two losses."""
    assert np.array_equal(bits(got[0]), bits(want[0])), what + ': table'
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ': b %r %r' % (got[1], want[1])
    if want[2] is not None and got[2] is not None:
        assert np.array_equal(bits(got[2]), bits(want[2])), what + ': p'
    if want[3] is not None and got[3] is not None:
        assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), what + ': loss_sum %r %r' % (got[3], want[3])
        assert np.float32(got[4]).tobytes() == np.float32(want[4]).tobytes(), what + ': loss_last %r %r' % (got[4], want[4])


def solo(spec, ids, y, wts):
    m = spec.model()
    res = result(m, m.train_online(ids, y, wts=wts, want_p=True))
    m.close()
    return res


def group(specs, ids, y, wts):
    models = [s.model() for s in specs]
    outs = train_online_many(models, ids, y, wts=wts, want_p=True)
    res = [result(m, o) for m, o in zip(models, outs)]
    for m in models:
        m.close()
    return res


def check_group(specs, ids, y, wts):
    got = group(specs, ids, y, wts)
    for i, s in enumerate(specs):
        assert_same(got[i], solo(s, ids, y, wts), 'model %d (F %d k %d)' % (i, s.F, s.k))
    return got


def mixed_ranks(F):
    ks = (1, 11, 16, 17, 101, 128)
    return [Spec(F, k, lr=0.02 + 0.01 * i, lam=(0.0, 1e-2, 3e-2)[i % 3], seed=40 + i, shared=bool(i & 1)) for i, k in enumerate(ks)]


@pytest.mark.parametrize("weighted", [False, True])
def test_ranks_1_to_128_in_one_call_equal_their_solo_runs(built, weighted):
    ids, wts, y = feed(16, 150, 7, weighted)
    got = check_group(mixed_ranks(16), ids, y, wts)
    assert not np.array_equal(got[0][0], mixed_ranks(16)[0].rows().astype(np.float32))        # something was trained


@pytest.mark.parametrize("F", [1, 39, 64])
@pytest.mark.parametrize("weighted", [False, True])
def test_three_models_at_other_field_counts(built, F, weighted):
    ids, wts, y = feed(F, 150, 10 + F, weighted)
    check_group([Spec(F, 1, lr=0.03, lam=1e-2, seed=1), Spec(F, 11, lr=0.05, lam=0.0, seed=2), Spec(F, 17, lr=0.04, lam=2e-2, seed=3)],
                ids, y, wts)


@pytest.mark.parametrize("weighted", [False, True])
def test_nine_models_more_than_one_per_xcd(built, weighted):
    ids, wts, y = feed(16, 150, 21, weighted)
    check_group([Spec(16, (11, 1, 50)[i % 3], lr=0.02 + 0.005 * i, lam=1e-3 * i, seed=60 + i) for i in range(9)], ids, y, wts)


@pytest.mark.parametrize("weighted", [False, True])
def test_260_tiny_models_more_workgroups_than_cus(built, weighted):
    ids, wts, y = feed(4, 50, 31, weighted)
    check_group([Spec(4, 3, lr=0.01 + 0.0005 * i, lam=1e-4 * (i % 7), seed=5) for i in range(260)], ids, y, wts)


def test_a_group_against_the_float64_reference(built):
    """The (16, 11) case of tests/test_gpu_fm_online.py at both of its lambdas, as one group, under that file's parity rule."""
    import torch
    F, k, N, lr = 16, 11, 300, 0.05
    cases = [oc.solved(F, k, N, 100 + F + k, True, lr, lam) for lam in (0.0, 1e-2)]
    rows, ids, wts, y = cases[0][:4]
    assert all(np.array_equal(c[1], ids) for c in cases)                              # one feed: the cases differ in lambda only
    models, loops = [], []
    for lam in (0.0, 1e-2):
        for lst, shared in ((models, False), (loops, True)):
            m = FM(1, [rows.shape[0], F, k - 1], INIT, ['sgd', lr], [lam], 'train', 0, shared_rows=shared)
            m.set_params(rows, oc.B0)
            lst.append(m)
    outs = train_online_many(models, ids, y, wts=wts, want_p=True)
    for m, loop, out, (_, _, _, _, ref_rows, ref_b, ref_p, ref_loss) in zip(models, loops, outs, cases):
        ids_d, y_d, w_d = loop._dev(ids, torch.int32), loop._dev(y, torch.float32), loop._dev(wts, torch.float32)
        p_loop = torch.cat([loop.train_step(ids_d[n:n + 1], y_d[n:n + 1], want_p=True, want_loss=False, wts=w_d[n:n + 1])['p']
                            for n in range(N)]).cpu().numpy()
        err = []
        for mm in (m, loop):
            got, gb = mm.get_params()
            err.append(max(np.abs(got - ref_rows).max(), abs(gb - ref_b)))
        ep_on, ep_loop = np.abs(out['p'].cpu().numpy() - ref_p).max(), np.abs(p_loop - ref_p).max()
        print("table/b err group %.3g loop %.3g; p err group %.3g loop %.3g" % (err[0], err[1], ep_on, ep_loop))
        assert err[0] <= 2 * err[1] + 2e-7
        assert ep_on <= 2 * ep_loop + 2e-7
        assert abs(out['loss'] - ref_loss.sum()) <= 2e-5 * max(1.0, ref_loss.sum())
        assert abs(out['loss_last'] - ref_loss[-1]) <= 2e-5 * max(1.0, ref_loss[-1])
        m.close(), loop.close()


def folding_group():
    """lr * lambda = 0.5 leaves [2^-24, 1] every 24 lines, 0.2 after 75, and lambda = 0 never folds."""
    return [Spec(16, 11, lr=0.5, lam=1.0, seed=71, b=0.0), Spec(16, 17, lr=0.2, lam=1.0, seed=72, b=0.0),
            Spec(16, 11, lr=0.05, lam=0.0, seed=73), Spec(16, 1, lr=0.5, lam=1.0, seed=74, b=0.0)]


def test_cuts_and_folds_change_no_bit(built, monkeypatch):
    ids, wts, y = feed(16, 150, 41, False)
    monkeypatch.delenv('FM_ONLINE_CHUNK', raising=False)
    want = [solo(s, ids, y, None) for s in folding_group()]
    whole = group(folding_group(), ids, y, None)                  # cut only where some member folds
    monkeypatch.setenv('FM_ONLINE_CHUNK', '7')                    # read when a handle is created
    cut = group(folding_group(), ids, y, None)
    for i in range(len(want)):
        assert_same(whole[i], want[i], 'default chunk, model %d' % i)
        assert_same(cut[i], want[i], 'chunk 7, model %d' % i)
    assert np.isfinite(want[0][0]).all() and not np.array_equal(want[0][0], folding_group()[0].rows().astype(np.float32))


@pytest.mark.parametrize("N", [0, 1, 2])
def test_zero_one_and_two_lines(built, N):
    ids, wts, y = feed(16, 3, 5, True)
    specs = [Spec(16, 11, seed=1), Spec(16, 17, lr=0.03, seed=2), Spec(16, 1, lam=0.0, seed=3)]
    got = check_group(specs, ids[:N], y[:N], wts[:N])
    if N == 0:
        for s, g in zip(specs, got):
            assert np.array_equal(g[0], s.rows().astype(np.float32)) and g[1] == np.float32(s.b) and g[3] == 0.0 and g[4] == 0.0
            assert g[2].shape == (0,)


def raw_call(models, ids_t, w_t, y_t, N, p=None, loss=None, last=None, hs=None, lr=None, lam=None, n_models=None):
    """fm_train_online_multi through ctypes, every argument replaceable; p: None or a list of tensors / None per model."""
    M = len(models)
    hs = (C.c_void_p * M)(*[m.h.value for m in models]) if hs is None else hs
    lr = (C.c_float * M)(*[m.lr for m in models]) if lr is None else lr
    lam = (C.c_float * M)(*[m.lam for m in models]) if lam is None else lam
    p_arr = None if p is None else (C.c_void_p * M)(*[None if t is None else t.data_ptr() for t in p])
    models[0]._torch.cuda.synchronize()                           # the tensors were made on another stream than the handles'
    return models[0].lib.fm_train_online_multi(hs or None, M if n_models is None else n_models, None if ids_t is None else ids_t.data_ptr(),
                                               None if w_t is None else w_t.data_ptr(), None if y_t is None else y_t.data_ptr(),
                                               N, lr or None, lam or None, p_arr, loss, last)


def test_nullable_outputs(built):
    import torch
    ids, wts, y = feed(16, 40, 51, True)
    specs = [Spec(16, 11, seed=1), Spec(16, 101, lr=0.03, seed=2), Spec(16, 1, lam=0.0, seed=3)]
    want = [solo(s, ids, y, wts) for s in specs]
    for variant in ('no p array', 'one p entry null', 'no losses', 'nothing'):
        models = [s.model() for s in specs]
        m0 = models[0]
        ids_t, y_t, w_t = m0._dev(ids, torch.int32), m0._dev(y, torch.float32), m0._dev(wts, torch.float32)
        p = [torch.zeros(len(y), dtype=torch.float32, device=m0.device) for _ in models]
        loss, last = (C.c_double * 3)(), (C.c_float * 3)()
        if variant == 'no p array':
            rc = raw_call(models, ids_t, w_t, y_t, len(y), None, loss, last)
            p = [None] * 3
        elif variant == 'one p entry null':
            p[1] = None
            rc = raw_call(models, ids_t, w_t, y_t, len(y), p, loss, None)
        elif variant == 'no losses':
            rc = raw_call(models, ids_t, w_t, y_t, len(y), p, None, None)
        else:
            rc = raw_call(models, ids_t, w_t, y_t, len(y), None, None, None)
            p = [None] * 3
        assert rc == _capi.FNN_OK, variant
        for i, m in enumerate(models):
            assert m.lib.fm_sync(m.h) == _capi.FNN_OK
            rows, b = m.get_params()
            got = (rows, np.float32(b), None if p[i] is None else p[i].cpu().numpy(), None, None)
            assert_same(got, want[i], '%s, model %d' % (variant, i))
            if variant in ('no p array', 'one p entry null'):
                assert loss[i] == want[i][3], variant
            if variant == 'no p array':
                assert np.float32(last[i]) == np.float32(want[i][4])
            m.close()


def test_group_calls_and_batch_steps_interleave(built):
    """Group call, a batch train_step on ONE member, a second group call: the same sequence done solo gives the same bits.
    The batch keeps every row under one column (column f draws from rows 17 f .. 17 f + 16), where the batch step itself is
    reproducible bit for bit (include/fm_hip.h, "Columns and rows")."""
    ids, wts, y = feed(16, 104, 61, True)
    b_ids = (17 * np.arange(16) + np.random.RandomState(3).randint(0, 17, size=(32, 16))).astype(np.int32)
    specs = [Spec(16, 11, seed=1), Spec(16, 17, lr=0.03, seed=2), Spec(16, 1, lam=0.0, seed=3)]

    def make(s):
        m = FM(32, [s.n_rows, s.F, s.k - 1], INIT, ['sgd', s.lr], [s.lam], 'train', 0)
        m.set_params(s.rows(), s.b)
        return m
    models = [make(s) for s in specs]
    o1 = train_online_many(models, ids[:40], y[:40], wts=wts[:40], want_p=True)
    models[1].train_step(b_ids, y[40:72], wts=wts[40:72])
    o2 = train_online_many(models, ids[72:], y[72:], wts=wts[72:], want_p=True)
    for i, s in enumerate(specs):
        m = make(s)
        s1 = m.train_online(ids[:40], y[:40], wts=wts[:40], want_p=True)
        if i == 1:
            m.train_step(b_ids, y[40:72], wts=wts[40:72])
        s2 = m.train_online(ids[72:], y[72:], wts=wts[72:], want_p=True)
        assert np.array_equal(bits(o1[i]['p'].cpu().numpy()), bits(s1['p'].cpu().numpy()))
        assert_same(result(models[i], o2[i]), result(m, s2), 'model %d' % i)
        m.close(), models[i].close()


def test_handles_on_distinct_streams(built):
    """Every FM owns a stream.  set_params, the group call and get_params back to back, twice over, with no synchronisation of
    the test's own: the call is ordered after the first and before the last on every handle."""
    import torch
    ids, wts, y = feed(16, 150, 81, True)
    specs = [Spec(16, (11, 17, 1, 16)[i % 4], lr=0.02 + 0.01 * i, seed=90 + i) for i in range(6)]
    models = [s.model() for s in specs]
    assert len(set(m.stream.cuda_stream for m in models)) == len(models)
    m0 = models[0]
    ids_t, y_t, w_t = m0._dev(ids, torch.int32), m0._dev(y, torch.float32), m0._dev(wts, torch.float32)
    torch.cuda.synchronize()
    want = [solo(s, ids, y, wts) for s in specs]
    for rnd in range(2):
        for m, s in zip(reversed(models), reversed(specs)):
            m.set_params(s.rows(), s.b)
        hs = (C.c_void_p * 6)(*[m.h.value for m in models])
        lr, lam = (C.c_float * 6)(*[m.lr for m in models]), (C.c_float * 6)(*[m.lam for m in models])
        assert m0.lib.fm_train_online_multi(hs, 6, ids_t.data_ptr(), w_t.data_ptr(), y_t.data_ptr(), len(y), lr, lam, None, None,
                                            None) == _capi.FNN_OK
        for i in reversed(range(6)):
            rows, b = models[i].get_params()
            assert_same((rows, np.float32(b), None, None, None), want[i], 'round %d, model %d' % (rnd, i))
    for m in models:
        m.close()


def test_the_call_waits_for_work_queued_on_another_handles_stream(built):
    """Sixteen B = 1 train_steps enqueued on model 2's stream (no loss asked for, so nothing synchronises; device tensors, so
    nothing is copied), then the group call at once: the launches run on model 0's stream and must wait for those steps.  The
    same sequence done solo gives the same bits (a step's rows sit under one column each: it is bit-reproducible)."""
    import torch
    ids, wts, y = feed(16, 150, 83, True)
    b_ids = (17 * np.arange(16) + np.random.RandomState(4).randint(0, 17, size=(16, 16))).astype(np.int32)
    specs = [Spec(16, (11, 17, 11, 1)[i], lr=0.02 + 0.01 * i, seed=30 + i) for i in range(4)]

    def steps(m, t_ids, t_y):
        for n in range(16):
            m.train_step(t_ids[n:n + 1], t_y[n:n + 1], want_loss=False)
    models = [s.model() for s in specs]
    m0 = models[0]
    ids_t, y_t, w_t = m0._dev(ids, torch.int32), m0._dev(y, torch.float32), m0._dev(wts, torch.float32)
    bi_t, by_t = m0._dev(b_ids, torch.int32), m0._dev(y[:16], torch.float32)
    hs = (C.c_void_p * 4)(*[m.h.value for m in models])
    lr, lam = (C.c_float * 4)(*[m.lr for m in models]), (C.c_float * 4)(*[m.lam for m in models])
    torch.cuda.synchronize()
    steps(models[2], bi_t, by_t)
    assert m0.lib.fm_train_online_multi(hs, 4, ids_t.data_ptr(), w_t.data_ptr(), y_t.data_ptr(), len(y), lr, lam, None, None,
                                        None) == _capi.FNN_OK
    for i, s in enumerate(specs):
        m = s.model()
        if i == 2:
            steps(m, bi_t, by_t)
        m.train_online(ids_t, y_t, wts=w_t, want_loss=False)
        assert_same(result(models[i], None), result(m, None), 'model %d' % i)
        m.close(), models[i].close()


def test_refusals_leave_every_member_untouched(built):
    import torch
    ids, wts, y = feed(16, 9, 91, False)
    specs = [Spec(16, 11, seed=1), Spec(16, 17, seed=2), Spec(16, 1, seed=3)]
    models = [s.model() for s in specs]
    m0, lib = models[0], models[0].lib
    before = [m.get_params() for m in models]
    ids_t, y_t = m0._dev(ids, torch.int32), m0._dev(y, torch.float32)
    N = len(y)
    other_f = Spec(15, 11, seed=4).model()
    adam = Spec(16, 11, seed=5, ptmzr=('adam', 0.01, 1e-8)).model()
    ftrl = Spec(16, 11, seed=6, ptmzr=('ftrl', 0.05)).model()
    bare = FM.__new__(FM)                                          # a handle that never saw fm_set_table
    bare.h, bare.lib, bare.lr, bare.lam, bare.stream = C.c_void_p(), lib, 0.05, 0.0, m0.stream
    assert lib.fm_create(16, 11, 1, 0, C.c_void_p(m0.stream.cuda_stream), C.byref(bare.h)) == 0

    def f3(*v):
        return (C.c_float * 3)(*v)
    two_null = (C.c_void_p * 3)(models[0].h.value, None, models[2].h.value)
    twice = (C.c_void_p * 3)(models[0].h.value, models[1].h.value, models[0].h.value)
    ARG, STATE = _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE
    cases = [
        ('null hs', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, N, hs=False, **kw)),
        ('null lr', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, N, lr=False, **kw)),
        ('null lambda', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, N, lam=False, **kw)),
        ('null entry', ARG, 1, lambda kw: raw_call(models, ids_t, None, y_t, N, hs=two_null, **kw)),
        ('no models', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, N, n_models=0, **kw)),
        ('too many models', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, N, n_models=_capi_max() + 1, **kw)),
        ('one handle twice', ARG, 2, lambda kw: raw_call(models, ids_t, None, y_t, N, hs=twice, **kw)),
        ('n_fields differ', ARG, 2, lambda kw: raw_call(models[:2] + [other_f], ids_t, None, y_t, N, **kw)),
        ('N < 0', ARG, None, lambda kw: raw_call(models, ids_t, None, y_t, -1, **kw)),
        ('null ids', ARG, None, lambda kw: raw_call(models, None, None, y_t, N, **kw)),
        ('null y', ARG, None, lambda kw: raw_call(models, ids_t, None, None, N, **kw)),
        ('lr * lambda = 1', ARG, 1, lambda kw: raw_call(models, ids_t, None, y_t, N, lr=f3(0.05, 2.0, 0.05), lam=f3(0.0, 0.5, 0.0), **kw)),
        ('lr * lambda < 0', ARG, 2, lambda kw: raw_call(models, ids_t, None, y_t, N, lr=f3(0.05, 0.05, 0.05), lam=f3(0.0, 0.0, -1.0), **kw)),
        ('lr * lambda NaN', ARG, 0, lambda kw: raw_call(models, ids_t, None, y_t, N, lr=f3(float('nan'), 0.05, 0.05), lam=f3(0.1, 0.0, 0.0), **kw)),
        ('Adam', STATE, 1, lambda kw: raw_call([models[0], adam, models[2]], ids_t, None, y_t, N, **kw)),
        ('FTRL', STATE, 2, lambda kw: raw_call(models[:2] + [ftrl], ids_t, None, y_t, N, **kw)),
        ('no table', STATE, 1, lambda kw: raw_call([models[0], bare, models[2]], ids_t, None, y_t, N, **kw)),
    ]
    extra_before = [m.get_params() for m in (other_f, adam, ftrl)]
    for name, code, index, call in cases:
        loss, last = (C.c_double * 3)(7.0, 7.0, 7.0), (C.c_float * 3)(7.0, 7.0, 7.0)
        assert call({'loss': loss, 'last': last}) == code, name
        assert list(loss) == [7.0] * 3 and list(last) == [7.0] * 3, name
        msg = lib.fm_last_error(None if name == 'null hs' or name in ('no models', 'too many models') else m0.h).decode()
        assert 'fm_train_online_multi' in msg, (name, msg)
        if index is not None:
            assert 'model %d' % index in msg, (name, msg)
        for m, (rows, b) in zip(models + [other_f, adam, ftrl], before + extra_before):
            got, gb = m.get_params()
            assert np.array_equal(bits(got), bits(rows)) and gb == b, name
    with pytest.raises(ValueError):
        train_online_many([], ids, y)
    with pytest.raises(ValueError):
        train_online_many([models[0], other_f], ids, y)
    with pytest.raises(FNNError) as e:
        train_online_many([models[0], models[1], models[0]], ids, y)
    assert e.value.code == ARG
    with pytest.raises(FNNError) as e:
        train_online_many([models[0], adam], ids, y)
    assert e.value.code == STATE
    closed = Spec(16, 11, seed=7).model()
    closed.close()
    with pytest.raises(FNNError) as e:
        train_online_many([closed, models[1]], ids, y)
    assert e.value.code == ARG and 'model 0' in str(e.value)
    lib.fm_destroy(bare.h)
    bare.h = None
    for m in models + [other_f, adam, ftrl]:
        m.close()


def _capi_max():
    return 1024                                                    # FM_ONLINE_MAX_MODELS of include/fm_hip.h


def test_an_id_out_of_range_is_per_model(built):
    """Tables of 300 and 200 rows fed ids up to 299: only model 1 reports, and both equal their solo runs (for which such an
    id is absent).  Without synchronisation each handle's fm_sync reports its own flag."""
    import torch
    ids, wts, y = feed(16, 60, 95, True)
    assert ids.max() >= 200 and ids.max() <= 299
    specs = [Spec(16, 11, seed=1, n_rows=300), Spec(16, 11, seed=2, n_rows=200)]
    want = []
    for s in specs:
        m = s.model()
        out = m.train_online(ids, y, wts=wts, want_p=True, want_loss=False)
        assert m.lib.fm_sync(m.h) == (_capi.FNN_ERR_RANGE if s.n_rows == 200 else _capi.FNN_OK)
        want.append(result(m, out))
        m.close()
    models = [s.model() for s in specs]
    with pytest.raises(FNNError) as e:
        train_online_many(models, ids, y, wts=wts, want_p=True)
    assert e.value.code == _capi.FNN_ERR_RANGE
    listed = str(e.value).split('model(s)')[1]
    assert '1' in listed and '0' not in listed, str(e.value)
    for m, w in zip(models, want):
        assert m.lib.fm_sync(m.h) == _capi.FNN_OK                 # reported once, by the call
        assert_same(result(m, None), w)
        m.close()
    models = [s.model() for s in specs]
    outs = train_online_many(models, ids, y, wts=wts, want_p=True, want_loss=False)
    assert [m.lib.fm_sync(m.h) for m in models] == [_capi.FNN_OK, _capi.FNN_ERR_RANGE]
    for m, o, w in zip(models, outs, want):
        assert_same(result(m, o), w)
        m.close()


def test_the_same_group_twice_gives_the_same_bits(built):
    ids, wts, y = feed(16, 150, 97, True)
    a, b = group(mixed_ranks(16), ids, y, wts), group(mixed_ranks(16), ids, y, wts)
    for i in range(len(a)):
        assert_same(a[i], b[i], 'model %d' % i)


def test_the_driver_trains_every_spec_as_its_own_run_would(built, golden_dir, tmp_path):
    """ipinyou.run_many on the demo file, three specs, against three ipinyou.run(..., online=True) calls with the same buffer.
    `run` shuffles through the global NumPy RNG (collect), in `stat` and for every training and test buffer, and run_many
    reads the files in the same order once: seeded alike, all four see the same lines in the same order."""
    import os
    path = os.path.join(golden_dir, 'demo', 'train.yzx.txt')
    specs = [('FM', 10, 1e-3, 1e-2), ('LR', 0, 1e-3, 1e-3), ('FM', 10, 1e-3, 1e-2)]     # what `run` builds for 'FM' and 'LR'
    log = str(tmp_path / 'many.log')
    np.random.seed(123)
    many = ipinyou.run_many(path, path, specs, buffer=500, eval_size=1000, log_file=log, echo=False)
    assert len(many) == 3 and isinstance(many[1]['model'], LR)
    lines = open(log).read().splitlines()
    for i, (algo, _, _, _) in enumerate(specs):
        one_log = str(tmp_path / ('one%d.log' % i))
        np.random.seed(123)
        one = ipinyou.run(path, path, algo, buffer=500, eval_size=1000, log_file=one_log, echo=False, online=True)
        assert len(one['log']) == 3 and many[i]['log'] == one['log']
        assert (many[i]['X_dim'], many[i]['X_feas']) == (one['X_dim'], one['X_feas'])
        assert_same(result(many[i]['model'], None), result(one['model'], None), 'spec %d' % i)
        assert [l[len('%d\t' % i):] for l in lines if l.startswith('%d\t' % i)] == open(one_log).read().splitlines()
        one['model'].close(), many[i]['model'].close()
    assert len(lines) == 3 * 4
