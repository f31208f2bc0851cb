"""fnn_train_step_multi: one mini-batch step of several FNN handles on one feed, against solo twins, to the bit.

A twin is a fresh handle with the same parameters that takes its own fnn_train_step calls on the same device feed.  Compared
are each step's p and loss, then the table and every dense tensor (fnn_get_dense reads the masters the shadows are refreshed
from; a later step reads the shadows, so a wrong shadow shows in the steps that follow).  No pair is held at a bound: the group
kernels run the solo kernels' bodies on the same records.

Shapes as in test_gpu_fnn_step_plumbing.py: F = 16, k = 11, max_batch 512, about 1,000 rows (synth.field_sizes_tiny) so that
rows repeat inside a strip, three steps, hidden 300 / 100 and 40 / 20 (the two strip shapes).  Every model reads ONE feed; the
feed's ids are drawn for the 1,000-row table, larger tables hold those rows first, so a row keeps its column in every model."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, engine, synth
from deep_ctr_amd.engine import FNNError

from test_gpu_shapes import edge_empties, make_engine, make_problem

pytestmark = pytest.mark.gpu

F_, K, BMAX, B, NROWS, STEPS = 16, 11, 512, 300, 1000, 3
SHAPES = [(300, 100), (40, 20)]
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
DEV = _capi.FNN_MEM_DEVICE
ACTS = ('tanh', 'sigmoid', 'linear')
ARG, STATE, RANGE = _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE, _capi.FNN_ERR_RANGE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Feed(object):
    """Batches of the given lengths on the device: ids for the NROWS-row table, labels.  F / K: the layout (the default: the
    module's); empties: edge_empties in every batch; dup: every batch's last column names one row almost everywhere."""

    def __init__(self, lens, seed=5, F=F_, K=K, empties=False, dup=False):
        import torch
        self.F, self.K, self.seed, self.long = F, K, seed, {}
        self.rows, self.fo, ids, y, _, _, _ = make_problem(F, K, 300, 100, sum(lens), n_rows=NROWS, seed=seed)
        ids[1, 2] = -1                                                   # an empty field
        cut = np.cumsum([0] + list(lens))
        for a, b in zip(cut[:-1], cut[1:]):
            if dup:
                ids[a:b, F - 1] = ids[a, F - 1]
            if empties:
                for t, f in edge_empties(b - a, F):
                    ids[a + t, f] = -1
        self.ids = [np.ascontiguousarray(ids[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        self.y = [np.ascontiguousarray(y[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        self.dev = torch.device('cuda', 0)
        self.d = [(self.put(i), self.put(v)) for i, v in zip(self.ids, self.y)]

    def put(self, a):
        import torch
        t = torch.as_tensor(a).to(self.dev).contiguous()
        torch.cuda.synchronize()
        return t

    def table(self, n_rows, k=None):
        """The feed's table cut to, or continued to, n_rows rows (rows beyond NROWS are in no batch); another k: its own rows
        over the same row ids."""
        k = self.K if k is None else k
        rows = self.rows if k == self.K else make_problem(self.F, k, 300, 100, 4, n_rows=NROWS, seed=self.seed)[0]
        if n_rows <= NROWS:
            return rows[:n_rows].copy(), self.fo[:n_rows].copy()
        if (n_rows, k) not in self.long:                                 # made once: a 2^20-row table is 46 MB
            extra = synth.fm_table(n_rows - NROWS, k, 0.05, 77)
            self.long[(n_rows, k)] = np.concatenate([rows, extra]), np.concatenate([self.fo, np.zeros(n_rows - NROWS, np.int32)])
        return self.long[(n_rows, k)]


class Spec(object):
    """One model of a group: what make_engine takes, the seed of its initial dense tensors and of its masks."""

    def __init__(self, m, prec='bf16', H1=300, H2=100, n_rows=NROWS, max_batch=BMAX, lr=None, F=F_, K=K, reg_all=False, lam1=None):
        self.m, self.prec, self.H1, self.H2, self.n_rows, self.max_batch = m, prec, H1, H2, n_rows, max_batch
        self.F, self.K, self.reg_all = F, K, reg_all
        self.lr = (0.01, 0.004, 0.02, 0.007, 0.013)[m % 5] if lr is None else lr
        self.lam1 = (0.02, 0.0, 0.05)[m % 3] if lam1 is None else lam1
        self.lamfm = (0.1, 0.3, 0.0, 0.05)[m % 4]
        self.acti = ACTS[m % 3]
        self.p = make_problem(F, K, H1, H2, 4, n_rows=64, seed=40 + m)[4]

    def engine(self, feed):
        rows, fo = feed.table(self.n_rows, self.K)
        return make_engine(self.F, self.K, self.H1, self.H2, rows, fo, self.p, prec=self.prec, acti=self.acti, max_batch=self.max_batch,
                           lr=self.lr, lam1=self.lam1, lamfm=self.lamfm, reg_all=self.reg_all)

    def masks(self, feed, s):
        """The dropout rows of step s, on the device."""
        r1, r2 = self.host_masks(s)
        return feed.put(r1), feed.put(r2)

    def host_masks(self, s):
        rng = np.random.RandomState(1000 * self.m + s)
        r1, r2 = (rng.uniform(size=self.H1) < 0.5).astype(np.uint8), (rng.uniform(size=self.H2) < 0.5).astype(np.uint8)
        r1[0] = r2[0] = 1
        return r1, r2


def group_step(engs, ids_t, y_t, masks, nxt=None, want_loss=True, b_size=0):
    """One raw fnn_train_step_multi; returns (code, losses, p per model as numpy)."""
    import torch
    M, n = len(engs), ids_t.shape[0]
    ps = [torch.empty(n, dtype=torch.float32, device=ids_t.device) for _ in engs]
    torch.cuda.synchronize()
    arr = lambda ptrs: (C.c_void_p * M)(*ptrs)                            # noqa: E731
    loss = (C.c_float * M)(*([-1.0] * M))
    rc = engs[0].lib.fnn_train_step_multi(arr([e.h.value for e in engs]), M, ids_t.data_ptr(), y_t.data_ptr(), n,
                                          arr([a.data_ptr() for a, _ in masks]), arr([b.data_ptr() for _, b in masks]), b_size,
                                          nxt.data_ptr() if nxt is not None else None, nxt.shape[0] if nxt is not None else 0,
                                          arr([p.data_ptr() for p in ps]), loss if want_loss else None)
    if rc in (0, RANGE):
        for e in engs:
            torch.cuda.synchronize()
    return rc, list(loss), [p.cpu().numpy() for p in ps]


def solo_step(eng, ids_t, y_t, mask, b_size=0):
    """The twin's step: (code, loss, p)."""
    import torch
    n = ids_t.shape[0]
    p = torch.empty(n, dtype=torch.float32, device=ids_t.device)
    torch.cuda.synchronize()
    loss = C.c_float(-1.0)
    rc = eng.lib.fnn_train_step(eng.h, ids_t.data_ptr(), y_t.data_ptr(), n, mask[0].data_ptr(), mask[1].data_ptr(), b_size, p.data_ptr(),
                                None, DEV, C.byref(loss))
    torch.cuda.synchronize()
    return rc, float(loss.value), p.cpu().numpy()


def last_error(eng):
    return (eng.lib.fnn_last_error(eng.h) or b'').decode()


def assert_same_state(a, b, what):
    ta, tb = a.get_table(), b.get_table()
    assert np.isfinite(ta).all()
    assert np.array_equal(ta, tb), '%s: table, %d of %d floats differ' % (what, (ta != tb).sum(), ta.size)
    da, db = a.get_dense(), b.get_dense()
    for k in DENSE:
        assert np.array_equal(da[k], db[k]), '%s: %s, %d of %d differ' % (what, k, (da[k] != db[k]).sum(), da[k].size)
    assert da['b3'] == db['b3'], '%s: b3' % what


def assert_same_step(got, ref, what):
    assert np.isfinite(got[1]) and np.isfinite(got[2]).all(), what
    assert got[1] == ref[1], '%s: loss %r against %r' % (what, got[1], ref[1])
    assert np.array_equal(got[2], ref[2]), '%s: p, %d of %d differ' % (what, (got[2] != ref[2]).sum(), got[2].size)


def run_against_twins(specs, feed, announce='next', steps=None):
    """The models of `specs` through group steps over the feed's batches, their twins through solo steps; everything compared.
    announce: 'next' (every next batch through next_ids), 'none', or 'miss' (a batch announced that is then not the one given)."""
    steps = range(len(feed.d)) if steps is None else steps
    engs, twins = [], []
    try:
        for sp in specs:
            engs.append(sp.engine(feed))
            twins.append(sp.engine(feed))
        decoy = feed.put(feed.ids[0][::-1].copy())
        for s in steps:
            ids_t, y_t = feed.d[s]
            masks = [sp.masks(feed, s) for sp in specs]
            nxt = None
            if announce == 'next' and s + 1 < len(feed.d):
                nxt = feed.d[s + 1][0]
            elif announce == 'miss':
                nxt = decoy if s % 2 == 0 else feed.d[s][0][:max(1, ids_t.shape[0] - 1)]      # other ids / these ids at another B
            rc, loss, ps = group_step(engs, ids_t, y_t, masks, nxt)
            assert rc == 0, last_error(engs[0])
            for m, (t, sp) in enumerate(zip(twins, specs)):
                ref = solo_step(t, ids_t, y_t, masks[m])
                assert ref[0] == 0, last_error(t)
                assert_same_step((rc, loss[m], ps[m]), ref, 'model %d (%s %dx%d), step %d' % (m, sp.prec, sp.H1, sp.H2, s))
        for m, (e, t) in enumerate(zip(engs, twins)):
            assert not np.array_equal(e.get_table()[:NROWS], feed.rows[:len(e.get_table())][:NROWS])
            assert_same_state(e, t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


@pytest.fixture(scope='module')
def feed3(built):
    return Feed([B] * STEPS)


UNIFORM = [(prec, H1, H2, M) for prec in ('bf16', 'f32', 'bf16x3') for H1, H2 in SHAPES for M in (2, 5)]


@pytest.mark.parametrize("prec,H1,H2,M", UNIFORM, ids=['%s-%dx%d-M%d' % c for c in UNIFORM])
def test_uniform_group_equals_solo_twins(built, feed3, prec, H1, H2, M):
    """M members of one launch class that differ in lr, lambda1, lambda_fm, masks, initial weights and act."""
    run_against_twins([Spec(m, prec, H1, H2) for m in range(M)], feed3)


def test_mixed_group_equals_solo_twins(built, feed3):
    """Several launch classes in one call; 300/100 with 290/90 in one class (both pad to 320/128); two n_rows in one launch class
    (two grouping classes); one table of 2^20 rows, the smallest whose keys (row << 12 | t) need 64 bits (n_rows * 4096 > 2^32 - 1)."""
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'f32', 300, 100), Spec(2, 'bf16', 290, 90), Spec(3, 'bf16x3', 40, 20),
             Spec(4, 'bf16', 40, 20), Spec(5, 'bf16', 300, 100, n_rows=1500), Spec(6, 'bf16', 40, 20, n_rows=1 << 20),
             Spec(7, 'f32', 300, 100), Spec(8, 'bf16', 40, 20)]
    run_against_twins(specs, feed3)


@pytest.fixture(scope='module')
def feed_lens(built):
    return Feed([300, 37, 1, 512], seed=6)


@pytest.mark.parametrize("announce", ['next', 'none', 'miss'])
def test_batch_lengths_with_and_without_the_announcement(built, feed_lens, announce):
    """B = 300, 37, 1 and 512 in one run (ragged and single strips): every next batch announced, none announced, and an
    announced batch that is not the one given -- the announcement is a scheduling hint only."""
    run_against_twins([Spec(0, 'bf16', 300, 100), Spec(1, 'f32', 40, 20), Spec(2, 'bf16', 300, 100), Spec(3, 'f32', 40, 20)], feed_lens, announce)


def test_interleaved_with_solo_steps_and_predict(built, feed3):
    """A group step; a solo step on a member that is not the first; a group step with the list reordered, so that the grouping
    class's first member changes; fnn_predict in between.  The twins take solo steps of the same batches in the same order."""
    specs = [Spec(m, 'bf16', 300, 100) for m in range(3)]
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    try:
        d = feed3.d
        mk = lambda s: [sp.masks(feed3, s) for sp in specs]             # noqa: E731

        def both(order, s, nxt):
            masks = mk(s)
            rc, loss, ps = group_step([engs[m] for m in order], d[s][0], d[s][1], [masks[m] for m in order], nxt)
            assert rc == 0, last_error(engs[order[0]])
            for j, m in enumerate(order):
                assert_same_step((rc, loss[j], ps[j]), solo_step(twins[m], d[s][0], d[s][1], masks[m]), 'model %d, batch %d' % (m, s))

        both([0, 1, 2], 0, d[1][0])                                      # announces batch 1
        masks = mk(2)
        assert_same_step(solo_step(engs[1], d[2][0], d[2][1], masks[1]), solo_step(twins[1], d[2][0], d[2][1], masks[1]), 'solo on member 1')
        pa, pt = engs[2].predict(d[0][0]).cpu().numpy(), twins[2].predict(d[0][0]).cpu().numpy()
        assert np.array_equal(pa, pt)
        both([2, 0, 1], 1, d[2][0])                                      # another first member: its grouping is made now
        pa, pt = engs[0].predict(d[1][0]).cpu().numpy(), twins[0].predict(d[1][0]).cpu().numpy()
        assert np.array_equal(pa, pt)
        both([2, 0, 1], 2, None)                                         # the announced batch, the same first member
        both([1, 2], 0, None)
        for m in range(3):
            assert_same_state(engs[m], twins[m], 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_one_step_at_4096(built):
    """B = 4096, the bound of the three launches, max_batch 4096 (bf16: the LDS weight-gradient form), M = 3."""
    feed = Feed([4096], seed=8)
    run_against_twins([Spec(m, 'bf16', 300, 100, max_batch=4096, lr=0.001) for m in range(3)], feed, 'none')


def test_sixty_four_models(built, feed3):
    """M = 64 at hidden 40 / 20: many models in the grid, one step."""
    run_against_twins([Spec(m, 'bf16', 40, 20) for m in range(64)], feed3, 'none', steps=[0])


def test_one_model_is_the_solo_step(built, feed3):
    run_against_twins([Spec(3, 'f32', 300, 100)], feed3)


@pytest.mark.parametrize("want_loss", [True, False])
def test_an_id_out_of_range_for_one_model_only(built, feed3, want_loss):
    """Model 1's table ends at row 900: the feed's last fields name rows beyond it, which are absent for that model alone.  With
    the losses the call returns FNN_ERR_RANGE naming model 1; without, that handle's fnn_sync reports it.  Model 1 equals a twin
    that took the same feed in solo steps, the others twins that never saw a bad id; later good steps equal the twins'."""
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'bf16', 300, 100, n_rows=900), Spec(2, 'bf16', 300, 100)]
    assert max(int(i.max()) for i in feed3.ids) >= 900
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    try:
        ids_t, y_t = feed3.d[0]
        masks = [sp.masks(feed3, 0) for sp in specs]
        rc, loss, ps = group_step(engs, ids_t, y_t, masks, None, want_loss)
        if want_loss:
            assert rc == RANGE
            assert last_error(engs[0]) == 'fnn_train_step_multi: feature id outside [-1, n_rows) in model(s) 1'
        else:
            assert rc == 0
            assert [e.lib.fnn_sync(e.h) for e in engs] == [0, RANGE, 0]
        assert [e.lib.fnn_sync(e.h) for e in engs] == [0, 0, 0]           # the flags are cleared
        for m, t in enumerate(twins):
            ref = solo_step(t, ids_t, y_t, masks[m])
            assert ref[0] == (RANGE if m == 1 else 0)
            if want_loss:
                assert loss[m] == ref[1]
            assert np.array_equal(ps[m], ref[2]), 'model %d' % m
        # good steps afterwards: ids below 900 only
        good = feed3.ids[1].copy()
        good[good >= 900] = -1
        g_t = feed3.put(good)
        masks = [sp.masks(feed3, 1) for sp in specs]
        rc, loss, ps = group_step(engs, g_t, feed3.d[1][1], masks)
        assert rc == 0, last_error(engs[0])
        for m, t in enumerate(twins):
            assert_same_step((rc, loss[m], ps[m]), solo_step(t, g_t, feed3.d[1][1], masks[m]), 'model %d, good step' % m)
            assert_same_state(engs[m], t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_refusals_name_the_model_and_leave_every_handle_as_it_was(built, feed3):
    """Every refusal that needs a device, twice, with the same code and the same text; then good group steps equal twins' that
    saw no refusal."""
    from test_gpu_parity import make_snn_engine, make_snn_problem
    specs = [Spec(m, 'bf16', 300, 100) for m in range(3)]
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    others = []
    try:
        ids_t, y_t = feed3.d[0]
        masks = [sp.masks(feed3, 0) for sp in specs]
        rows, bb0, _, _, p, _, _ = make_snn_problem(8, n_rows=NROWS, h0=200, seed=3, n_fields=F_, h1=300, h2=100)
        bag = make_snn_engine(rows, bb0, p, prec='bf16', lr=0.01, h0=200, max_batch=BMAX, n_fields=F_, h1=300, h2=100)
        others.append(bag)
        wrows, wfo, _, _, wp, _, _ = make_problem(F_, 20, 300, 100, 4, n_rows=NROWS, seed=5)
        wide = make_engine(F_, 20, 300, 100, wrows, wfo, wp, prec='bf16', max_batch=BMAX)
        others.append(wide)
        dp = specs[1].engine(feed3)
        dp.dp_init_custom(0, 1, lambda view: None, None, sparse='local')
        others.append(dp)
        small = Spec(1, 'bf16', 300, 100, max_batch=256).engine(feed3)
        others.append(small)

        def refused(members, code, text):
            ms = [masks[0]] * len(members)
            for _ in range(2):
                assert engs[0].lib.fnn_sync(engs[0].h) == 0
                rc, loss, _ = group_step(members, ids_t, y_t, ms)
                assert rc == code
                assert last_error(members[0]) == 'fnn_train_step_multi: ' + text
                assert loss == [-1.0] * len(members)                     # untouched

        refused([engs[0], bag, engs[2]], ARG, 'model 1: FNN_MODE_BAG handles take fnn_train_step, one at a time')
        refused([engs[0], engs[1], wide], ARG, 'model 2: wide rows (k >= 17) take fnn_train_step, one at a time')
        refused([engs[0], dp], ARG, 'model 1: a data-parallel handle (fnn_dp_init) takes fnn_train_step')
        refused([engs[0], engs[1], engs[0]], ARG, 'model 2: the same handle twice in one call (two updates would race on one model)')
        refused([engs[0], engs[1], small], ARG, 'model 2: B must be in [1, max_batch]')
        f2 = np.flatnonzero(feed3.fo == 2)
        engs[1].set_shadowed(np.array([(t, 2, int(f2[(t + 1) % len(f2)])) for t in (3, 4, 9)], np.int32))
        refused([engs[0], engs[1], engs[2]], ARG, 'model 1: shadowed features pending (fnn_set_shadowed): such a batch takes fnn_train_step')
        engs[1].set_shadowed(np.zeros((0, 3), np.int32))
        assert engs[2].lib.fnn_step_begin(engs[2].h, ids_t.data_ptr(), y_t.data_ptr(), B, masks[2][0].data_ptr(), masks[2][1].data_ptr(), 0,
                                          None, None, DEV) == 0
        refused([engs[0], engs[1], engs[2]], STATE, 'model 2: inside fnn_step_begin / fnn_step_end')
        assert engs[2].lib.fnn_step_end(engs[2].h, None) == 0
        engs[2].sync()
        assert solo_step(twins[2], ids_t, y_t, masks[2])[0] == 0         # the twin takes the step that fnn_step_begin / _end was
        for s in (1, 2):
            masks = [sp.masks(feed3, s) for sp in specs]
            rc, loss, ps = group_step(engs, feed3.d[s][0], feed3.d[s][1], masks, feed3.d[2][0] if s == 1 else None)
            assert rc == 0, last_error(engs[0])
            for m, t in enumerate(twins):
                assert_same_step((rc, loss[m], ps[m]), solo_step(t, feed3.d[s][0], feed3.d[s][1], masks[m]), 'model %d, step %d' % (m, s))
        for m, t in enumerate(twins):
            assert_same_state(engs[m], t, 'model %d after the refusals' % m)
    finally:
        for e in engs + twins + others:
            e.close()


def test_train_step_many_returns_train_steps_dicts(built, feed3):
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'f32', 40, 20)]
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    try:
        masks = [sp.masks(feed3, 0) for sp in specs]
        outs = engine.train_step_many(engs, feed3.d[0][0], feed3.d[0][1], [a for a, _ in masks], [b for _, b in masks],
                                      next_ids=feed3.d[1][0], want_p=True)
        for o, t, mk in zip(outs, twins, masks):
            ref = t.train_step(feed3.d[0][0], feed3.d[0][1], mk[0], mk[1], want_p=True)
            assert sorted(o) == ['loss', 'p'] and o['loss'] == ref['loss'] and np.array_equal(o['p'].cpu().numpy(), ref['p'].cpu().numpy())
        assert engine.train_step_many(engs, feed3.d[1][0], feed3.d[1][1], [a for a, _ in masks], [b for _, b in masks], want_loss=False) == [{}, {}]
    finally:
        for e in engs + twins:
            e.close()


def test_train_epoch_many_equals_each_engines_train_epoch(built):
    """Seven batches of 100 (the last one short), a `shadowed` array that hits one batch: that batch runs as solo steps."""
    feed = Feed([650], seed=9)
    specs = [Spec(0, 'bf16', 300, 100), Spec(1, 'f32', 40, 20), Spec(2, 'bf16', 300, 100)]
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    try:
        ids_d, y_d = feed.d[0]
        n = 7
        rng = np.random.RandomState(3)
        m1 = [(rng.uniform(size=(n, sp.H1)) < 0.5).astype(np.uint8) for sp in specs]
        m2 = [(rng.uniform(size=(n, sp.H2)) < 0.5).astype(np.uint8) for sp in specs]
        f2 = np.flatnonzero(feed.fo == 2)
        sh = np.array([(t, 2, int(f2[(t + 1) % len(f2)])) for t in (303, 304, 390)], np.int32)      # batch 3
        engine.train_epoch_many(engs, ids_d, y_d, 100, m1, m2, 0, None, sh)
        for m, t in enumerate(twins):
            t.train_epoch(ids_d, y_d, 100, m1[m], m2[m], 0, None, sh)
        for e in engs + twins:
            e.sync()
        for m, t in enumerate(twins):
            assert_same_state(engs[m], t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'deep-ctr_amd', 'FNN.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_many_equals_run_per_spec(built, tmp_path, monkeypatch):
    """FNN.run_many on tests/golden/demo, two specs, two epochs.  The first spec is run()'s own setting for advertiser 2997:
    history and prediction pickles equal run()'s.  A one-spec run_many takes solo steps (n_models == 1 forwards), so each spec
    of the pair is also held against its own one-spec run: histories, pickles and final dense tensors."""
    from deep_ctr_amd import dl_utils
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('DEEPCTR_DATA_DIR', os.path.join(ROOT, 'tests', 'golden', 'demo'))
    monkeypatch.setenv('DEEPCTR_EPOCHS', '2')
    monkeypatch.delenv('DEEPCTR_PRECISION', raising=False)
    monkeypatch.setattr(dl_utils, 'log_path', str(tmp_path / 'log'))
    mod = _script('fnn_script_many')
    specs = ['1e-3:0.5:0:0.1', '2e-3:0.5:0:0.1']
    load = lambda f: pickle.load(open(str(tmp_path / f), 'rb'))          # noqa: E731
    out = {}
    hists = mod.run_many(['FNN.py', '2997'], specs, out)
    assert len(hists) == 2 and all(len(h) == 2 for h in hists) and hists[0] != hists[1]
    dense = [e.get_dense() for e in out['engines']]
    pred = [[load('mlp3fm_%s_2997_m%d.p' % (w, m)) for w in ('train', 'test')] for m in range(2)]
    for e in out['engines']:
        e.close()
    assert mod.run(['FNN.py', '2997']) == hists[0]
    for j, w in enumerate(('train', 'test')):
        assert np.array_equal(load('mlp3fm_%s_2997.p' % w), pred[0][j])
    for m in range(2):
        one = {}
        assert mod.run_many(['FNN.py', '2997'], [specs[m]], one) == [hists[m]]
        d1 = one['engines'][0].get_dense()
        one['engines'][0].close()
        for k in DENSE:
            assert np.array_equal(d1[k], dense[m][k]), 'spec %d: %s' % (m, k)
        assert d1['b3'] == dense[m]['b3']
        for j, w in enumerate(('train', 'test')):
            assert np.array_equal(load('mlp3fm_%s_2997_m0.p' % w), pred[m][j])
    log = open(str(tmp_path / 'log' / 'fm2997_m1.txt')).read()
    assert 'L_r:0.002' in log and 'Test Err:1' in log
