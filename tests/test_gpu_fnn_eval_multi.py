"""fnn_predict_multi / fnn_eval_multi: the predictions and metrics of several FNN handles on one feed, against solo twins, to the bit.

A twin is a fresh handle with the same parameters that took the same two training steps (so that masters and shadows differ from
the initial ones) and answers solo fnn_eval / fnn_predict (in chunks of its max_batch) on the same device feed.  Compared are the
predictions as uint32 and the float64 metrics with ==; no pair is held at a bound: the group kernel runs the solo kernel's body
on every line, and the metric pass partitions its sums as the solo one does.

Shapes: F = 16, k = 11, about 1,000 rows (synth.field_sizes_tiny), N = 8,229 lines -- no multiple of 16, above every max_batch
used, two feed batches of 4,096 and a third of 37, five metric blocks of 2,048 -- with ids[1, 2] = -1."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, engine, synth
from deep_ctr_amd.engine import FNNEngine, FNNError

from test_gpu_shapes import edge_empties, make_engine, make_problem

pytestmark = pytest.mark.gpu

F_, K, NROWS, N, TB = 16, 11, 1000, 8229, 200
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
DEV = _capi.FNN_MEM_DEVICE
ACTS = ('tanh', 'sigmoid', 'linear')
ARG, STATE, RANGE = _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE, _capi.FNN_ERR_RANGE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.0


class Feed(object):
    """N lines on the device: ids for the NROWS-row table, int32 labels of both classes; its first 2 * TB lines train.  F / K / n:
    the layout and the number of lines (the default: the module's); empties: edge_empties(n, F) as well."""

    def __init__(self, seed=5, F=F_, K=K, n=N, empties=False):
        import torch
        self.dev = torch.device('cuda', 0)
        self.F, self.K, self.seed, self.n = F, K, seed, n
        self.rows, self.fo, ids, y, _, _, _ = make_problem(F, K, 300, 100, n, n_rows=NROWS, seed=seed,
                                                           empty=edge_empties(n, F) if empties else ())
        ids[1, 2] = -1                                                   # an empty field
        self.ids, self.y = ids, y.astype(np.int32)
        assert 0 < self.y.sum() < n
        self.ids_d, self.y_d, self.yf_d = self.put(ids), self.put(self.y), self.put(y.astype(np.float32))

    def put(self, a):
        import torch
        t = torch.as_tensor(np.ascontiguousarray(a)).to(self.dev).contiguous()
        torch.cuda.synchronize()
        return t

    def table(self, n_rows, k=None):
        """The feed's table continued to n_rows rows (rows beyond NROWS are in no line of the feed); another k: its own rows."""
        k = self.K if k is None else k
        rows = self.rows if k == self.K else make_problem(self.F, k, 300, 100, 4, n_rows=NROWS, seed=self.seed)[0]
        if n_rows <= NROWS:
            return rows[:n_rows].copy(), self.fo[:n_rows].copy()
        extra = synth.fm_table(n_rows - NROWS, k, 0.05, 77)
        return np.concatenate([rows, extra]), np.concatenate([self.fo, np.zeros(n_rows - NROWS, np.int32)])


class Spec(object):
    """One model of a group: what make_engine takes and the seed of its initial dense tensors and masks; bag: an FNN_MODE_BAG
    handle of the smallest shape the strip kernel takes bag rows at (h0 = 192, hidden below 64)."""

    def __init__(self, m, prec='bf16', H1=300, H2=100, n_rows=NROWS, max_batch=512, k=K, bag=False, F=F_):
        self.m, self.prec, self.H1, self.H2, self.n_rows, self.max_batch, self.k, self.bag = m, prec, H1, H2, n_rows, max_batch, k, bag
        self.F = F
        self.lr = (0.01, 0.004, 0.02, 0.007, 0.013)[m % 5]
        self.acti = ACTS[m % 3]
        self.p = make_problem(F, k, H1, H2, 4, n_rows=64 if F <= 16 else NROWS, seed=40 + m)[4]     # (the dense tensors do not depend on n_rows)

    def masks(self, s):
        rng = np.random.RandomState(1000 * self.m + s)
        r1, r2 = (rng.uniform(size=self.H1) < 0.5).astype(np.uint8), (rng.uniform(size=self.H2) < 0.5).astype(np.uint8)
        r1[0] = r2[0] = 1
        return r1, r2

    def fresh(self, feed):
        if self.bag:
            from test_gpu_parity import make_snn_engine, make_snn_problem
            ww0, bb0, _, _, p, _, _ = make_snn_problem(8, n_rows=NROWS, h0=192, seed=40 + self.m, n_fields=self.F, h1=self.H1, h2=self.H2)
            return make_snn_engine(ww0, bb0, p, prec=self.prec, lr=self.lr, h0=192, max_batch=self.max_batch, n_fields=self.F, h1=self.H1,
                                   h2=self.H2, acti=self.acti)
        rows, fo = feed.table(self.n_rows, self.k)
        return make_engine(self.F, self.k, self.H1, self.H2, rows, fo, self.p, prec=self.prec, acti=self.acti, max_batch=self.max_batch,
                           lr=self.lr, lam1=(0.02, 0.0, 0.05)[self.m % 3], lamfm=(0.1, 0.3, 0.0, 0.05)[self.m % 4])

    def engine(self, feed, steps=2, tb=TB):
        """A handle that has taken `steps` training steps of tb lines on the head of the feed."""
        eng = self.fresh(feed)
        for s in range(steps):
            r1, r2 = self.masks(s)
            eng.train_step(feed.ids_d[s * tb:(s + 1) * tb], feed.yf_d[s * tb:(s + 1) * tb], r1, r2, want_loss=False)
        eng.sync()
        return eng


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def last_error(eng):
    return (eng.lib.fnn_last_error(eng.h) or b'').decode()


def _arr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def eval_multi(engs, ids_t, y_t, want=None, n=None, tail=0):
    """One raw fnn_eval_multi.  want: per model, whether p_out[m] is given (None: all; 'null': a null p_out).  Returns
    (code, auc, rmse, logloss, status, p per model as numpy or None); every output starts at a sentinel.  tail: that many more
    floats behind each p_out, returned with it."""
    import torch
    M = len(engs)
    n = ids_t.shape[0] if n is None else n
    want = [True] * M if want is None else want
    ps = None if want == 'null' else [torch.full((max(n, 1) + tail,), SENT, dtype=torch.float32, device=ids_t.device) if w else None for w in want]
    torch.cuda.synchronize()
    auc, rmse, ll = ((C.c_double * M)(*([SENT] * M)) for _ in range(3))
    st = (C.c_int * M)(*([77] * M))
    rc = engs[0].lib.fnn_eval_multi(_arr([e.h.value for e in engs]), M, ids_t.data_ptr(), y_t.data_ptr() if y_t is not None else None, n,
                                    auc, rmse, ll, st, None if ps is None else _arr([p.data_ptr() if p is not None else None for p in ps]))
    torch.cuda.synchronize()
    return rc, list(auc), list(rmse), list(ll), list(st), [None] * M if ps is None else [None if p is None else p.cpu().numpy() for p in ps]


def predict_multi(engs, ids_t, n=None, tail=0):
    import torch
    n = ids_t.shape[0] if n is None else n
    ps = [torch.full((max(n, 1) + tail,), SENT, dtype=torch.float32, device=ids_t.device) for _ in engs]
    torch.cuda.synchronize()
    rc = engs[0].lib.fnn_predict_multi(_arr([e.h.value for e in engs]), len(engs), ids_t.data_ptr(), n, _arr([p.data_ptr() for p in ps]))
    torch.cuda.synchronize()
    return rc, [p.cpu().numpy() for p in ps]


def solo_eval(eng, ids_t, y_t, tail=0):
    """The twin's fnn_eval: (code, auc, rmse, logloss, p)."""
    import torch
    p = torch.full((ids_t.shape[0] + tail,), SENT, dtype=torch.float32, device=ids_t.device)
    torch.cuda.synchronize()
    auc, rmse, ll = C.c_double(SENT), C.c_double(SENT), C.c_double(SENT)
    rc = eng.lib.fnn_eval(eng.h, ids_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0], DEV, C.byref(auc), C.byref(rmse), C.byref(ll), p.data_ptr())
    torch.cuda.synchronize()
    return rc, auc.value, rmse.value, ll.value, p.cpu().numpy()


def same_metric(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def assert_equals_twin(got, m, ref, what, with_p=True):
    """got: eval_multi's result, ref: solo_eval's of model m's twin."""
    rc, auc, rmse, ll, st, ps = got
    assert np.isfinite(ref[4]).all() and (ref[4] != SENT).all(), what
    assert auc[m] == ref[1] and rmse[m] == ref[2] and ll[m] == ref[3], '%s: metrics %r against %r' % (what, (auc[m], rmse[m], ll[m]), ref[1:4])
    assert st[m] == 0, what
    if with_p:
        assert np.array_equal(bits(ps[m]), bits(ref[4])), '%s: p, %d of %d differ' % (what, (bits(ps[m]) != bits(ref[4])).sum(), ref[4].size)


def dense_state(e):
    d = e.get_dense()
    return [e.get_table()] + [np.asarray(d[k]) for k in DENSE] + [np.float64(d['b3'])]


def assert_same_state(a, b, what):
    for x, y in zip(dense_state(a), dense_state(b)):
        assert np.array_equal(x, y), what


@pytest.fixture(scope='module')
def feed(built):
    return Feed()


MIXED = [Spec(0, 'bf16', 300, 100, max_batch=512), Spec(1, 'bf16', 290, 90, max_batch=256), Spec(2, 'f32', 300, 100, n_rows=1500),
         Spec(3, 'bf16x3', 40, 20), Spec(4, 'f32', 40, 20)]


@pytest.fixture(scope='module')
def mixed(feed):
    """The five members of several launch classes, their twins, and the twins' solo results (computed once, never changed)."""
    engs, twins = [sp.engine(feed) for sp in MIXED], [sp.engine(feed) for sp in MIXED]
    refs = [solo_eval(t, feed.ids_d, feed.y_d) for t in twins]
    assert all(r[0] == 0 for r in refs)
    yield engs, twins, refs
    for e in engs + twins:
        e.close()


def test_mixed_launch_classes_equal_solo_twins(built, feed, mixed):
    """bf16 300/100 (max_batch 512) with bf16 290/90 (256) in one class, f32 300/100 on 1,500 rows, bf16x3 and f32 at 40/20; the
    three act values.  With every p_out, with a null p_out, with p_out entries partly null, and through fnn_predict_multi."""
    engs, twins, refs = mixed
    got = eval_multi(engs, feed.ids_d, feed.y_d)
    assert got[0] == 0, last_error(engs[0])
    for m in range(len(engs)):
        assert_equals_twin(got, m, refs[m], 'model %d' % m)
    assert len(set(r[1] for r in refs)) == len(refs)                     # five different models
    got = eval_multi(engs, feed.ids_d, feed.y_d, 'null')
    assert got[0] == 0, last_error(engs[0])
    for m in range(len(engs)):
        assert_equals_twin(got, m, refs[m], 'model %d, null p_out' % m, with_p=False)
    want = [True, False, False, True, False]
    got = eval_multi(engs, feed.ids_d, feed.y_d, want)
    assert got[0] == 0, last_error(engs[0])
    for m in range(len(engs)):
        assert_equals_twin(got, m, refs[m], 'model %d, p_out partly null' % m, with_p=want[m])
    rc, ps = predict_multi(engs, feed.ids_d)
    assert rc == 0, last_error(engs[0])
    for m, t in enumerate(twins):
        assert np.array_equal(bits(ps[m]), bits(refs[m][4])), 'fnn_predict_multi, model %d' % m
        assert np.array_equal(bits(ps[m]), bits(t.predict(feed.ids_d).cpu().numpy())), 'fnn_predict in chunks, model %d' % m
    assert [e.lib.fnn_sync(e.h) for e in engs] == [0] * len(engs)


def test_members_off_the_strip_kernel(built, feed):
    """Wide rows (k = 21), hidden 200 / 50 (the layer-by-layer kernels) and a bag-mode handle run their own launches inside the
    call, between two members of the group launch."""
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'bf16', 300, 100, k=21), Spec(2, 'f32', 200, 50, max_batch=256),
             Spec(3, 'f32', 40, 20, bag=True), Spec(4, 'f32', 40, 20)]
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    try:
        got = eval_multi(engs, feed.ids_d, feed.y_d)
        assert got[0] == 0, last_error(engs[0])
        rc, ps = predict_multi(engs, feed.ids_d)
        assert rc == 0, last_error(engs[0])
        for m, t in enumerate(twins):
            ref = solo_eval(t, feed.ids_d, feed.y_d)
            assert ref[0] == 0, last_error(t)
            assert_equals_twin(got, m, ref, 'model %d' % m)
            assert np.array_equal(bits(ps[m]), bits(ref[4])), 'fnn_predict_multi, model %d' % m
    finally:
        for e in engs + twins:
            e.close()


@pytest.mark.parametrize("knob", ['one', 'two', 'model', 'batch', 'feed256'])
def test_scratch_groups_grid_order_and_launch_geometry_change_no_bit(built, feed, mixed, monkeypatch, knob):
    """FNN_EVAL_SCRATCH_BYTES so that one model fits a group, and so that two do (five models: groups of 2, 2, 1);
    FNN_EVAL_ORDER=model; FNN_EVAL_LAUNCH=batch; feed batches of 256 lines."""
    engs, _, refs = mixed
    one = 13 * N + 4096                  # one model's scratch is 12 N (p, keys, their copy) + N / 2 of histograms + 2 KiB: this holds one and not two
    if knob in ('one', 'two'):
        monkeypatch.setenv('FNN_EVAL_SCRATCH_BYTES', str(one if knob == 'one' else 2 * one))
    elif knob == 'model':
        monkeypatch.setenv('FNN_EVAL_ORDER', 'model')
    elif knob == 'batch':
        monkeypatch.setenv('FNN_EVAL_LAUNCH', 'batch')
    else:
        monkeypatch.setenv('FNN_EVAL_FEED_BATCH', '256')
    got = eval_multi(engs, feed.ids_d, feed.y_d)
    assert got[0] == 0, last_error(engs[0])
    rc, ps = predict_multi(engs, feed.ids_d)
    assert rc == 0, last_error(engs[0])
    for m in range(len(engs)):
        assert_equals_twin(got, m, refs[m], 'model %d' % m)
        assert np.array_equal(bits(ps[m]), bits(refs[m][4])), 'fnn_predict_multi, model %d' % m


def test_a_diverged_model_and_one_class(built, feed, mixed):
    """Model 1's w3 is NaN: its status is FNN_ERR_RANGE and its metrics are NaN, the call returns FNN_ERR_RANGE naming it, the
    others equal their twins.  That member is one on the layer-by-layer kernels (hidden 200 / 50), whose output unit passes a
    NaN on; the strip kernel's sigmoid clamps its argument with fmaxf / fminf, which drop a NaN, so a strip member with the same
    w3 (model 3) predicts finite values, solo and here alike, and is held to its solo result like any other.
    An all-zero y: every auc NaN, rmse and logloss the twins'."""
    engs, twins, refs = mixed
    sps = [Spec(7, 'f32', 200, 50, max_batch=256), MIXED[1]]
    bads = [sp.engine(feed) for sp in sps]
    try:
        for sp, bad in zip(sps, bads):
            d = bad.get_dense()
            d['w3'] = np.full(sp.H2, np.nan, np.float32)
            bad.set_dense(d)
        group = [engs[0], bads[0], engs[2], bads[1]]
        got = eval_multi(group, feed.ids_d, feed.y_d)
        assert got[0] == RANGE
        assert last_error(engs[0]) == 'fnn_eval_multi: predictions NaN or outside [0, 1] in model(s) 1'
        assert got[4] == [0, RANGE, 0, 0]
        assert np.isnan([got[1][1], got[2][1], got[3][1]]).all()
        ref = solo_eval(bads[0], feed.ids_d, feed.y_d)
        assert ref[0] == RANGE and np.isnan(ref[1:4]).all() and np.isnan(ref[4]).all()
        assert np.array_equal(bits(got[5][1]), bits(ref[4]))
        ref = solo_eval(bads[1], feed.ids_d, feed.y_d)
        assert ref[0] == 0
        assert_equals_twin(got, 3, ref, 'a strip member with a NaN w3')
        assert_equals_twin(got, 0, refs[0], 'model 0 beside a diverged one')
        assert_equals_twin(got, 2, refs[2], 'model 2 beside a diverged one')
    finally:
        for bad in bads:
            bad.close()
    zero = feed.put(np.zeros(N, np.int32))
    got = eval_multi(engs, feed.ids_d, zero)
    assert got[0] == RANGE
    assert last_error(engs[0]) == 'fnn_eval_multi: only one class present in y (roc_auc_score raises ValueError)'
    assert np.isnan(got[1]).all() and got[4] == [0] * len(engs)
    for m, t in enumerate(twins):
        ref = solo_eval(t, feed.ids_d, zero)
        assert ref[0] == RANGE and np.isnan(ref[1])
        assert got[2][m] == ref[2] and got[3][m] == ref[3], 'model %d' % m
        assert np.array_equal(bits(got[5][m]), bits(ref[4]))


def test_an_id_out_of_range_for_one_model_only(built, feed, mixed):
    """A feed with rows 1,000 and above: absent for the 1,000-row member alone.  fnn_eval_multi names that member and clears its
    flag; fnn_predict_multi leaves the flag to the handle's fnn_sync.  Results equal the twins' on that feed."""
    engs, twins, _ = mixed
    ids = feed.ids.copy()
    ids[5, 3], ids[4100, 0], ids[N - 1, 15] = 1200, 1001, 1499
    ids_d = feed.put(ids)
    group, tw = [engs[2], engs[0]], [twins[2], twins[0]]                 # 1,500 rows, 1,000 rows
    got = eval_multi(group, ids_d, feed.y_d)
    assert got[0] == RANGE
    assert last_error(group[0]) == 'fnn_eval_multi: feature id outside [-1, n_rows) in model(s) 1'
    assert [e.lib.fnn_sync(e.h) for e in group] == [0, 0]                # reported and cleared
    for m, t in enumerate(tw):
        ref = solo_eval(t, ids_d, feed.y_d)
        assert ref[0] == (RANGE if m == 1 else 0)
        assert_equals_twin(got, m, ref, 'model %d' % m)
    rc, ps = predict_multi(group, ids_d)
    assert rc == 0
    assert [e.lib.fnn_sync(e.h) for e in group] == [0, RANGE]
    assert [e.lib.fnn_sync(e.h) for e in group] == [0, 0]


def test_read_only_interleaved_with_steps_and_a_handle_twice(built, feed):
    """The calls change no bit of any member; train_step_many (announcing the next batch) -> evaluate_many -> train_step_many ->
    a solo step -> evaluate_many leaves every model and every result equal to twins that ran solo steps and solo evaluate."""
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'f32', 40, 20), Spec(2, 'bf16', 300, 100)]
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    try:
        before = [dense_state(e) for e in engs]
        got = eval_multi([engs[0], engs[1], engs[0]], feed.ids_d, feed.y_d)
        assert got[0] == 0, last_error(engs[0])
        assert (got[1][0], got[2][0], got[3][0]) == (got[1][2], got[2][2], got[3][2]) and np.array_equal(bits(got[5][0]), bits(got[5][2]))
        assert predict_multi(engs, feed.ids_d)[0] == 0
        for e, b in zip(engs, before):
            for x, y in zip(dense_state(e), b):
                assert np.array_equal(x, y)
        batch = lambda s: (feed.ids_d[s * TB:(s + 1) * TB], feed.yf_d[s * TB:(s + 1) * TB])      # noqa: E731

        def many(s, nxt):
            mk = [sp.masks(s) for sp in specs]
            engine.train_step_many(engs, batch(s)[0], batch(s)[1], [a for a, _ in mk], [b for _, b in mk],
                                   next_ids=batch(nxt)[0] if nxt is not None else None, want_loss=False)
            for t, (a, b) in zip(twins, mk):
                t.train_step(batch(s)[0], batch(s)[1], a, b, want_loss=False)

        def evaluated(what):
            outs = engine.evaluate_many(engs, feed.ids_d, feed.y_d, want_p=True)
            for m, (o, t) in enumerate(zip(outs, twins)):
                ref = t.evaluate(feed.ids_d, feed.y_d, want_p=True)
                assert sorted(o) == sorted(ref) and all(o[k] == ref[k] for k in ('auc', 'rmse', 'logloss')), '%s, model %d' % (what, m)
                assert np.array_equal(bits(o['p'].cpu().numpy()), bits(ref['p'].cpu().numpy())), '%s, model %d' % (what, m)

        many(2, 3)
        evaluated('after the first group step')
        many(3, None)
        a, b = specs[1].masks(4)
        for e in (engs[1], twins[1]):
            e.train_step(batch(4)[0], batch(4)[1], a, b, want_loss=False)
        evaluated('after a solo step')
        for m in range(3):
            assert_same_state(engs[m], twins[m], 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_refusals_name_the_model_and_launch_nothing(built, feed, mixed):
    engs, _, refs = mixed
    others = []
    try:
        rows13, fo13, _, _, p13, _, _ = make_problem(13, K, 300, 100, 4, n_rows=NROWS, seed=5)
        others.append(make_engine(13, K, 300, 100, rows13, fo13, p13, prec='bf16', max_batch=512))
        bare = FNNEngine(F_, K, 300, 100, max_batch=512, precision='bf16')
        bare.set_table(*(feed.table(NROWS) + (-3.0,)))
        others.append(bare)
        begun = MIXED[0].engine(feed)
        others.append(begun)
        r1, r2 = MIXED[0].masks(0)
        begun.step_begin(feed.ids_d[:TB], feed.yf_d[:TB], r1, r2)

        def refused(members, code, text, n=None):
            for _ in range(2):
                got = eval_multi(members, feed.ids_d, feed.y_d, n=n)
                assert got[0] == code
                assert last_error(members[0]) == 'fnn_eval_multi: ' + text
                assert got[1:5] == ([SENT] * len(members),) * 3 + ([77] * len(members),)
                assert all((p == SENT).all() for p in got[5])
                rc, ps = predict_multi(members, feed.ids_d, n=n)
                assert rc == code and last_error(members[0]) == 'fnn_predict_multi: ' + text
                assert all((p == SENT).all() for p in ps)

        refused([engs[0], engs[1], others[0]], ARG, "model 2: n_fields or device differs from model 0's")
        refused([engs[0], bare], STATE, 'model 1: fnn_set_dense has not been called for all three layers')
        refused([engs[0], engs[3], begun], STATE, 'model 2: inside fnn_step_begin / fnn_step_end')
        refused([engs[0], engs[1]], ARG, 'N must be in [1, 2^30]', n=0)
        begun.step_end()
        got = eval_multi(engs[:2], feed.ids_d, feed.y_d)
        assert got[0] == 0
        for m in range(2):
            assert_equals_twin(got, m, refs[m], 'model %d after the refusals' % m)
    finally:
        for e in others:
            e.close()


def test_evaluate_many_and_predict_many(built, feed, mixed):
    engs, twins, refs = mixed
    outs = engine.evaluate_many(engs, feed.ids_d, feed.y_d)
    assert outs == [t.evaluate(feed.ids_d, feed.y_d) for t in twins]
    outs = engine.evaluate_many(engs, feed.ids, feed.y, want_p=True)      # host arrays
    for o, r in zip(outs, refs):
        assert sorted(o) == ['auc', 'logloss', 'p', 'rmse'] and (o['auc'], o['rmse'], o['logloss']) == r[1:4]
        assert np.array_equal(bits(o['p'].cpu().numpy()), bits(r[4]))
    ps = engine.predict_many(engs, feed.ids_d)
    for p, t in zip(ps, twins):
        assert np.array_equal(bits(p.cpu().numpy()), bits(t.predict(feed.ids_d).cpu().numpy()))
    zero = np.zeros(N, np.int32)
    outs = engine.evaluate_many(engs[:2], feed.ids_d, zero)
    assert all(o['status'] == RANGE and 'only one class' in o['error'] and np.isnan(o['auc']) and o['rmse'] > 0 for o in outs)
    with pytest.raises(FNNError):
        twins[0].evaluate(feed.ids_d, zero)


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'deep-ctr_amd', 'FNN.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_many_evaluates_and_predicts_through_the_group_calls(built, tmp_path, monkeypatch):
    """FNN.run_many on tests/golden/demo, two specs, two epochs, first one spec at a time, then both with FNNEngine.evaluate and
    FNNEngine.predict patched to raise: the run completes, and histories and pickles equal the one-spec runs'."""
    from deep_ctr_amd import dl_utils
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('DEEPCTR_DATA_DIR', os.path.join(ROOT, 'tests', 'golden', 'demo'))
    monkeypatch.setenv('DEEPCTR_EPOCHS', '2')
    monkeypatch.delenv('DEEPCTR_PRECISION', raising=False)
    monkeypatch.setattr(dl_utils, 'log_path', str(tmp_path / 'log'))
    mod = _script('fnn_script_eval_many')
    specs = ['1e-3:0.5:0:0.1', '2e-3:0.5:0:0.1']
    load = lambda f: pickle.load(open(str(tmp_path / f), 'rb'))          # noqa: E731
    hist1, pred1 = [], []
    for s in specs:
        one = {}
        hist1 += mod.run_many(['FNN.py', '2997'], [s], one)
        one['engines'][0].close()
        pred1.append([load('mlp3fm_%s_2997_m0.p' % w) for w in ('train', 'test')])

    def never(self, *a, **k):
        raise AssertionError('run_many called a one-engine evaluate / predict')

    monkeypatch.setattr(FNNEngine, 'evaluate', never)
    monkeypatch.setattr(FNNEngine, 'predict', never)
    out = {}
    hists = mod.run_many(['FNN.py', '2997'], specs, out)
    for e in out['engines']:
        e.close()
    assert hists == hist1 and len(hists[0]) == 2 and hists[0] != hists[1]
    for m in range(2):
        for j, w in enumerate(('train', 'test')):
            assert np.array_equal(bits(load('mlp3fm_%s_2997_m%d.p' % (w, m))), bits(pred1[m][j]))
