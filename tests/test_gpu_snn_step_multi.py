"""fnn_bag_train_step_multi: one mini-batch step of several FNN_MODE_BAG handles (the SNN fine-tune) on one feed, against solo
twins.  A twin is a fresh handle with equal parameters that takes its own fnn_train_step calls on the same device feed.

Where no row lies under two columns of a batch (layout 'fields': column f draws from field f's own rows) every member is held
to its twin BIT FOR BIT: each step's p and loss, then table, bag bias and the dense tensors.  Where rows are shared between
columns (layout 'active', ingest.MODE_SNN_ACTIVE's) each of a row's columns adds into it with float atomics, in the solo step
as in the group call, so there the rows under at most one column stay bit-equal and the whole table is held to the float64
oracle at the bounds of test_gpu_snn_shapes.check_step -- the twin to the same ones.  The members of equal n_rows share the
first one's grouping WITH its marks of the shared rows: a follower that read its own, stale marks would store one column's sum
over a shared row and fail those bounds.

Shapes: 16 columns, max_batch 512, about 1,000 rows, B = 300, three steps unless a case says otherwise; (h0, H1, H2) =
(200, 300, 100), (300, 300, 100) and (192, 40, 20) are the three strip instances of bag mode."""
import ctypes as C

import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, engine
from deep_ctr_amd.engine import FNNEngine, FNNError

from test_gpu_parity import make_snn_engine, make_snn_problem
from test_gpu_shapes import Bounds
from test_gpu_snn_shapes import edge_empties

pytestmark = pytest.mark.gpu

F_, BMAX, B, NROWS, STEPS = 16, 512, 300, 1000, 3
INSTANCES = [(200, 300, 100), (300, 300, 100), (192, 40, 20)]
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
DEV = _capi.FNN_MEM_DEVICE
ACTS = ('tanh', 'sigmoid', 'linear')
ARG, STATE, RANGE = _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE, _capi.FNN_ERR_RANGE
NAME = 'fnn_bag_train_step_multi: '


class Feed(object):
    """Batches of the given lengths on the device: ids for a table of NROWS rows, labels.  layout as make_snn_problem's;
    empties: edge_empties in every batch; dup: every batch's last column names one row everywhere."""

    def __init__(self, lens, seed=5, F=F_, layout='fields', empties=False, dup=False):
        import torch
        self.F, self.seed, self.tabs = F, seed, {}
        _, _, ids, y, _, _, _ = make_snn_problem(sum(lens), n_rows=NROWS, h0=4, seed=seed, n_fields=F, h1=4, h2=4, layout=layout)
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

    def table(self, n_rows, h0):
        """The bag table [n_rows, h0] and bias [h0] of the feed: tables of one h0 agree in the rows they share."""
        if h0 not in self.tabs:
            rng = np.random.RandomState(self.seed * 1000 + h0)
            self.tabs[h0] = ((rng.standard_normal((2 * NROWS, h0)) * 0.1).astype(np.float32), (rng.standard_normal(h0) * 0.1).astype(np.float32))
        ww0, bb0 = self.tabs[h0]
        assert n_rows <= len(ww0)
        return ww0[:n_rows].copy(), bb0.copy()


class Spec(object):
    """One model of a group: what make_snn_engine takes and the seed of its initial dense tensors and masks."""

    def __init__(self, m, prec='bf16', h0=200, H1=300, H2=100, n_rows=NROWS, max_batch=BMAX, F=F_, lr=None):
        self.m, self.prec, self.h0, self.H1, self.H2, self.n_rows, self.max_batch, self.F = m, prec, h0, H1, H2, n_rows, max_batch, F
        self.lr = (0.01, 0.004, 0.02, 0.007, 0.013)[m % 5] if lr is None else lr
        self.lam1 = (0.02, 0.0, 0.05)[m % 3]
        self.acti = ACTS[m % 3]
        self.p = make_snn_problem(4, n_rows=64, h0=h0, seed=40 + m, n_fields=F, h1=H1, h2=H2, layout='active')[4]

    def engine(self, feed, ww0=None):
        tab, bb0 = feed.table(self.n_rows if ww0 is None else NROWS, self.h0)        # ww0: the member's own table
        return make_snn_engine(tab if ww0 is None else ww0, bb0, self.p, prec=self.prec, lr=self.lr, lam1=self.lam1, h0=self.h0,
                               max_batch=self.max_batch, n_fields=self.F, h1=self.H1, h2=self.H2, acti=self.acti)

    def host_masks(self, s):
        rng = np.random.RandomState(1000 * self.m + s)
        r1, r2 = (rng.uniform(size=self.H1) < 0.7).astype(np.uint8), (rng.uniform(size=self.H2) < 0.7).astype(np.uint8)
        r1[0] = r2[0] = 1
        return r1, r2

    def masks(self, feed, s):
        r1, r2 = self.host_masks(s)
        return feed.put(r1), feed.put(r2)


def group_step(engs, ids_t, y_t, masks, nxt=None, want_loss=True, b_size=0, B=None):
    """One raw fnn_bag_train_step_multi; returns (code, losses, p per model as numpy)."""
    import torch
    M, n = len(engs), ids_t.shape[0] if B is None else B
    ps = [torch.empty(n, dtype=torch.float32, device=ids_t.device) for _ in engs]
    torch.cuda.synchronize()
    arr = lambda ptrs: (C.c_void_p * M)(*ptrs)                            # noqa: E731
    loss = (C.c_float * M)(*([-1.0] * M))
    rc = engs[0].lib.fnn_bag_train_step_multi(arr([e.h.value for e in engs]), M, ids_t.data_ptr(), y_t.data_ptr(), n,
                                              arr([a.data_ptr() for a, _ in masks]), arr([b.data_ptr() for _, b in masks]), b_size,
                                              nxt.data_ptr() if nxt is not None else None, nxt.shape[0] if nxt is not None else 0,
                                              arr([p.data_ptr() for p in ps]), loss if want_loss else None)
    if rc in (0, RANGE):
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


def assert_same_dense(a, b, what):
    ba, bb = a.get_bag_bias(), b.get_bag_bias()
    assert np.array_equal(ba, bb), '%s: bag bias, %d of %d differ' % (what, (ba != bb).sum(), ba.size)
    da, db = a.get_dense(), b.get_dense()
    for k in DENSE:
        assert np.array_equal(da[k], db[k]), '%s: %s, %d of %d differ' % (what, k, (da[k] != db[k]).sum(), da[k].size)
    assert da['b3'] == db['b3'], '%s: b3' % what


def assert_same_state(a, b, what, rows=None):
    ta, tb = a.get_table(), b.get_table()
    assert np.isfinite(ta).all()
    if rows is not None:
        ta, tb = ta[rows], tb[rows]
    assert np.array_equal(ta, tb), '%s: table, %d of %d floats differ' % (what, (ta != tb).sum(), ta.size)
    assert_same_dense(a, b, what)


def assert_same_step(got, ref, what):
    assert np.isfinite(got[1]) and np.isfinite(got[2]).all(), what
    assert got[1] == ref[1], '%s: loss %r against %r' % (what, got[1], ref[1])
    assert np.array_equal(got[2], ref[2]), '%s: p, %d of %d differ' % (what, (got[2] != ref[2]).sum(), got[2].size)


def run_against_twins(specs, feed, announce='next', steps=None):
    """The models of `specs` through group steps over the feed's batches, their twins through solo steps; everything compared
    to the bit.  announce: 'next' (every next batch through next_ids) or 'none'."""
    steps = range(len(feed.d)) if steps is None else steps
    engs, twins = [], []
    try:
        for sp in specs:
            engs.append(sp.engine(feed))
            twins.append(sp.engine(feed))
        for s in steps:
            ids_t, y_t = feed.d[s]
            masks = [sp.masks(feed, s) for sp in specs]
            nxt = feed.d[s + 1][0] if announce == 'next' and s + 1 < len(feed.d) else None
            rc, loss, ps = group_step(engs, ids_t, y_t, masks, nxt)
            assert rc == 0, last_error(engs[0])
            for m, (t, sp) in enumerate(zip(twins, specs)):
                ref = solo_step(t, ids_t, y_t, masks[m])
                assert ref[0] == 0, last_error(t)
                assert_same_step((rc, loss[m], ps[m]), ref, 'model %d (%s h0 %d, %dx%d), step %d' % (m, sp.prec, sp.h0, sp.H1, sp.H2, s))
        for m, (e, t) in enumerate(zip(engs, twins)):
            assert not np.array_equal(e.get_table(), feed.table(specs[m].n_rows, specs[m].h0)[0])      # the steps moved rows
            assert_same_state(e, t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def columns_per_row(ids, n_rows):
    """How many columns of the batch hold each row."""
    n = np.zeros(n_rows, np.int64)
    for f in range(ids.shape[1]):
        r = np.unique(ids[:, f])
        n[r[(r >= 0) & (r < n_rows)]] += 1
    return n


@pytest.fixture(scope='module')
def feed3(built):
    f = Feed([B] * STEPS)
    assert all(columns_per_row(i, NROWS).max() == 1 for i in f.ids)      # 'fields': no row under two columns
    return f


# ------------------------------------------------------------------------------------------------ 1. bit for bit
UNIFORM = [(h0, H1, H2, prec, 8) for (h0, H1, H2) in INSTANCES for prec in ('bf16', 'f32', 'bf16x3')]
UNIFORM += [(h0, H1, H2, prec, 4) for (h0, H1, H2) in INSTANCES[:2] for prec in ('bf16', 'f32', 'bf16x3')]


@pytest.mark.parametrize("h0,H1,H2,prec,waves", UNIFORM, ids=['h%d-%dx%d-%s-nw%d' % c for c in UNIFORM])
def test_uniform_group_equals_solo_twins(built, monkeypatch, feed3, h0, H1, H2, prec, waves):
    """M = 3 members of one launch class that differ in lr, lambda1, act, masks and initial weights, every strip instance in
    every precision, the eight-wave instances also as four waves; with every next batch announced and with none."""
    if waves == 4:
        monkeypatch.setenv('FNN_STEP1_WAVES', '4')              # read by fnn_create
    else:
        monkeypatch.delenv('FNN_STEP1_WAVES', raising=False)
    for announce in ('next', 'none'):
        run_against_twins([Spec(m, prec, h0, H1, H2) for m in range(3)], feed3, announce)


# ------------------------------------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("n", [1, 16, 255, 256, 257])
def test_batch_lengths_at_the_strip_and_tile_edges(built, n):
    run_against_twins([Spec(0, 'f32'), Spec(1, 'f32')], Feed([n], seed=6 + n), 'none')


@pytest.mark.parametrize("F", [2, 17, 64])
def test_column_counts(built, F):
    """The strip sums a line's rows in groups of 16 columns: one group not full, two, four."""
    run_against_twins([Spec(0, 'f32', F=F), Spec(1, 'f32', F=F)], Feed([64], seed=7, F=F), 'none')


@pytest.mark.parametrize("kind", ['empties', 'dup'])
def test_empty_columns_and_one_row_down_a_column(built, kind):
    feed = Feed([B], seed=8, empties=kind == 'empties', dup=kind == 'dup')
    run_against_twins([Spec(0, 'bf16'), Spec(1, 'bf16')], feed, 'none')


# ------------------------------------------------------------------------------------------------ 3. classes
def test_launch_classes_grouping_classes_and_a_bad_id_for_one_model(built, feed3):
    """h0 200 and 300, hidden 300 / 100 and 40 / 20, f32 and bf16 in one call: four launch classes.  Inside model 0's class a
    table of 1,000 rows among tables of 1,500 (two grouping classes) and a follower of model 0.  Step 0 names row 1,200: absent
    for the 1,000-row model alone, which FNN_ERR_RANGE names; every model equals its twin, the flags are cleared, and the good
    steps that follow equal the twins' too."""
    specs = [Spec(0, 'f32', 200, 300, 100, n_rows=1500), Spec(1, 'bf16', 300, 300, 100, n_rows=1500), Spec(2, 'bf16', 192, 40, 20, n_rows=1500),
             Spec(3, 'f32', 200, 300, 100, n_rows=1000), Spec(4, 'f32', 200, 300, 100, n_rows=1500), Spec(5, 'f32', 192, 40, 20, n_rows=1500),
             Spec(6, 'bf16', 300, 300, 100, n_rows=1500)]
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    try:
        bad = feed3.ids[0].copy()
        bad[7, 3] = 1200
        assert columns_per_row(bad, 1500).max() == 1
        bad_t = feed3.put(bad)
        masks = [sp.masks(feed3, 0) for sp in specs]
        rc, loss, ps = group_step(engs, bad_t, feed3.d[0][1], masks, feed3.d[1][0])
        assert rc == RANGE
        assert last_error(engs[0]) == NAME + 'feature id outside [-1, n_rows) in model(s) 3'
        assert [e.lib.fnn_sync(e.h) for e in engs] == [0] * len(engs)      # the flags are cleared
        for m, t in enumerate(twins):
            ref = solo_step(t, bad_t, feed3.d[0][1], masks[m])
            assert ref[0] == (RANGE if m == 3 else 0)
            assert_same_step((0, loss[m], ps[m]), ref, 'model %d, step with the bad id' % m)
        for s in (1, 2):
            masks = [sp.masks(feed3, s) for sp in specs]
            rc, loss, ps = group_step(engs, feed3.d[s][0], feed3.d[s][1], masks, feed3.d[2][0] if s == 1 else None)
            assert rc == 0, last_error(engs[0])
            for m, t in enumerate(twins):
                assert_same_step((rc, loss[m], ps[m]), solo_step(t, feed3.d[s][0], feed3.d[s][1], masks[m]), 'model %d, step %d' % (m, s))
        for m, t in enumerate(twins):
            assert_same_state(engs[m], t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_a_member_with_64bit_sort_keys(built, feed3):
    """A table of 2^20 rows (h0 = 192: 805 MB in f32) makes n_rows * 4096 exceed 2^32 - 1: that member's grouping runs on 64-bit
    keys and it forms a launch class of its own beside a 1,000-row member of the same shape.  Built as test_gpu_snn_shapes
    builds its table; the feed's rows come first, the last row sits in one line."""
    n_rows = 1 << 20
    big = np.random.default_rng(0).standard_normal((n_rows, 192), dtype=np.float32) * np.float32(0.1)
    big[:NROWS] = feed3.table(NROWS, 192)[0]
    feed = Feed([B], seed=5)
    ids = feed.ids[0].copy()
    ids[11, 3] = n_rows - 1                                              # out of range for model 1, whose flag the call reports
    ids_t = feed.put(ids)
    specs = [Spec(0, 'f32', 192, 40, 20, n_rows=n_rows), Spec(1, 'f32', 192, 40, 20)]
    engs, twins = [sp.engine(feed3, w) for sp, w in zip(specs, (big, None))], [sp.engine(feed3, w) for sp, w in zip(specs, (big, None))]
    try:
        assert engs[0].n_rows * 4096 > 2 ** 32 - 1 >= engs[1].n_rows * 4096
        masks = [sp.masks(feed3, 0) for sp in specs]
        rc, loss, ps = group_step(engs, ids_t, feed.d[0][1], masks)
        assert rc == RANGE and last_error(engs[0]) == NAME + 'feature id outside [-1, n_rows) in model(s) 1'
        for m, t in enumerate(twins):
            ref = solo_step(t, ids_t, feed.d[0][1], masks[m])
            assert ref[0] == (RANGE if m == 1 else 0)
            assert_same_step((0, loss[m], ps[m]), ref, 'model %d' % m)
        touched = np.unique(ids[ids >= 0])
        assert np.array_equal(engs[0].get_rows(touched), twins[0].get_rows(touched))
        assert not np.array_equal(engs[0].get_rows(touched[-1:]), big[-1:])            # the last row moved
        assert_same_dense(engs[0], twins[0], 'model 0')
        assert_same_state(engs[1], twins[1], 'model 1')
    finally:
        for e in engs + twins:
            e.close()


# ------------------------------------------------------------------------------------------------ 4. shared rows
def oracle_bounds(bd, eng, acti, got_p, got_loss, ref, ids, state, scale_from):
    """test_gpu_snn_shapes.check_step's f32 bounds on what a group step gives (it returns no gx): p_drop, loss, the whole table,
    bag bias, the six dense tensors, the predictions after the step.  The scale of a tensor's bound is its update since
    `scale_from`, the state the oracle started from (after one step: check_step's own scale)."""
    ww64, bb64, p64 = state
    ww_s, bb_s, p_s = scale_from
    bd.close('p_drop', got_p, ref['p_drop'], 2e-4, 1e-6)
    bd.close('loss', got_loss, ref['loss'], 0.0, 2e-5 * max(1.0, abs(ref['loss'])))
    bd.close('table', eng.get_table(), ww64, 0.0, 1e-3 * (np.abs(ww64 - ww_s).max() + 1e-12) + 2e-7)
    bd.close('bag bias', eng.get_bag_bias(), bb64, 0.0, 1e-3 * (np.abs(bb64 - bb_s).max() + 1e-12) + 2e-7)
    d = eng.get_dense()
    for k in DENSE:
        bd.close(k, d[k], p64[k], 0.0, 1e-3 * (np.abs(p64[k] - p_s[k]).max() + 1e-12) + 1e-7)
    bd.close('b3', d['b3'], p64['b3'], 0.0, 1e-3 * (abs(p64['b3'] - p_s['b3']) + 1e-12) + 1e-7)
    bd.close('predict', eng.predict(ids).cpu().numpy(), orc.snn_predict(p64, ww64, bb64, ids, acti), 3e-4, 1e-6)


def test_rows_under_several_columns(built):
    """layout 'active': a feature's column depends on the line, so rows lie under several columns.  M = 3 of equal n_rows: model
    0 keeps the grouping, models 1 and 2 follow with ITS marks of the shared rows.  After one step p, loss, dense tensors, bag
    bias and the rows under at most one column equal the twin's bit for bit, and every member's WHOLE table -- and the twin's --
    holds check_step's bounds against the float64 oracle; so do two further steps.
    Every handle first takes one SOLO step on a batch without shared rows (twins stay bit-equal): a fresh handle's marks and stamp
    are all zero, which reads as "every row is shared" and would hide a follower that looked at its own marks; after a step of
    its own its stamp has moved on, its marks have not, and with them every shared row would take the plain store."""
    feed = Feed([B] * STEPS, seed=11, layout='active')
    warm = Feed([B], seed=12)
    assert columns_per_row(warm.ids[0], NROWS).max() == 1
    ncol = [columns_per_row(i, NROWS) for i in feed.ids]
    assert all((n > 1).sum() >= 20 for n in ncol), [(n > 1).sum() for n in ncol]
    specs = [Spec(m, 'f32', lr=(0.002, 0.001, 0.003)[m]) for m in range(3)]      # four steps of a batch SUM: rates at which no prediction saturates
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    try:
        start, state = [], []
        for sp in specs:
            ww0, bb0 = feed.table(NROWS, sp.h0)
            p64 = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in sp.p.items()}      # as check_step starts
            state.append((ww0.astype(np.float64), bb0.astype(np.float64), p64))
        for m, sp in enumerate(specs):                                   # the warm-up step, the oracle's too
            mask = sp.masks(feed, 99)
            assert_same_step(solo_step(engs[m], warm.d[0][0], warm.d[0][1], mask), solo_step(twins[m], warm.d[0][0], warm.d[0][1], mask), 'warm-up %d' % m)
            r1, r2 = sp.host_masks(99)
            ww64, bb64, p64 = state[m]
            orc.snn_train_step(p64, ww64, bb64, warm.ids[0], warm.y[0].astype(np.float64), r1.astype(float), r2.astype(float), sp.lr, sp.lam1, sp.acti, vec=True)
            start.append((ww64.copy(), bb64.copy(), {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p64.items()}))
        for s in range(STEPS):
            ids_t, y_t = feed.d[s]
            masks = [sp.masks(feed, s) for sp in specs]
            rc, loss, ps = group_step(engs, ids_t, y_t, masks, feed.d[s + 1][0] if s + 1 < STEPS else None)
            assert rc == 0, last_error(engs[0])
            for m, (t, sp) in enumerate(zip(twins, specs)):
                ref_t = solo_step(t, ids_t, y_t, masks[m])
                assert ref_t[0] == 0
                if s == 0:
                    assert_same_step((rc, loss[m], ps[m]), ref_t, 'model %d' % m)
                    assert_same_state(engs[m], t, 'model %d, rows under at most one column' % m, rows=np.flatnonzero(ncol[0] <= 1))
                r1, r2 = sp.host_masks(s)
                ww64, bb64, p64 = state[m]
                ref = orc.snn_train_step(p64, ww64, bb64, feed.ids[s], feed.y[s].astype(np.float64), r1.astype(float), r2.astype(float),
                                         sp.lr, sp.lam1, sp.acti, vec=True)
                assert np.isfinite(ref['loss']), (m, s)
                for who, e, got in (('group', engs[m], (ps[m], loss[m])), ('twin', t, (ref_t[2], ref_t[1]))):
                    bd = Bounds()
                    oracle_bounds(bd, e, sp.acti, got[0], got[1], ref, feed.ids[s], state[m], start[m])
                    bd.report('shared rows, model %d (%s), step %d, %s' % (m, sp.acti, s, who))
    finally:
        for e in engs + twins:
            e.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_model_and_leave_every_handle_as_it_was(built, monkeypatch, feed3):
    """Every refusal that needs a device, twice, with the same code and the same text; then good group steps equal twins' that
    saw no refusal."""
    from test_gpu_shapes import make_engine, make_problem
    specs = [Spec(m, 'bf16') for m in range(3)]
    engs, twins = [sp.engine(feed3) for sp in specs], [sp.engine(feed3) for sp in specs]
    others = []
    try:
        ids_t, y_t = feed3.d[0]
        masks = [sp.masks(feed3, 0) for sp in specs]
        rows, fo, _, _, p, _, _ = make_problem(F_, 11, 300, 100, 4, n_rows=NROWS, seed=5)
        fm = make_engine(F_, 11, 300, 100, rows, fo, p, prec='bf16', max_batch=BMAX)
        others.append(fm)
        dp = specs[1].engine(feed3)
        dp.dp_init_custom(0, 1, lambda view: None, None, sparse='local')
        others.append(dp)
        small = Spec(1, 'bf16', max_batch=256).engine(feed3)
        others.append(small)
        bare = FNNEngine(F_, 0, 300, 100, max_batch=BMAX, precision='bf16', lambda_fm=0.0, reg_all=True, mode='bag', hidden0=200)
        others.append(bare)
        monkeypatch.setenv('FNN_NO_FUSE', '1')                  # read by fnn_create
        unfused = specs[2].engine(feed3)
        monkeypatch.delenv('FNN_NO_FUSE')
        others.append(unfused)
        import torch
        long_ids = torch.full((4097, F_), -1, dtype=torch.int32, device=ids_t.device)
        long_y = torch.zeros(4097, dtype=torch.float32, device=ids_t.device)
        tabs = [e.get_table() for e in engs]

        def refused(members, code, text, feed=None):
            ms = [masks[0]] * len(members)
            for _ in range(2):
                assert members[0].lib.fnn_sync(members[0].h) == 0
                rc, loss, _ = group_step(members, *(feed or (ids_t, y_t)), ms)
                assert rc == code
                assert last_error(members[0]) == NAME + text
                assert loss == [-1.0] * len(members)                     # untouched

        refused([engs[0], fm, engs[2]], ARG, 'model 1: FNN_MODE_FM handles take fnn_train_step_multi')
        refused([engs[0], dp], ARG, 'model 1: a data-parallel handle (fnn_dp_init) takes fnn_train_step')
        refused([engs[0], engs[1], engs[0]], ARG, 'model 2: the same handle twice in one call (two updates would race on one model)')
        refused([engs[0], engs[1], small], ARG, 'model 2: B must be in [1, max_batch]')
        refused([engs[0], engs[1]], ARG, 'B must be in [1, 4096]', (long_ids, long_y))
        refused([engs[0], bare, engs[1]], STATE, 'model 1: fnn_set_table has not been called')
        refused([engs[0], unfused], ARG, 'model 1: the handle does not run the strip kernel (hidden sizes it is not built for, or FNN_NO_FUSE=1)')
        assert engs[2].lib.fnn_step_begin(engs[2].h, ids_t.data_ptr(), y_t.data_ptr(), B, masks[2][0].data_ptr(), masks[2][1].data_ptr(), 0,
                                          None, None, DEV) == 0
        refused([engs[0], engs[1], engs[2]], STATE, 'model 2: inside fnn_step_begin / fnn_step_end')
        assert engs[2].lib.fnn_step_end(engs[2].h, None) == 0
        engs[2].sync()
        assert solo_step(twins[2], ids_t, y_t, masks[2])[0] == 0         # the twin takes the step that fnn_step_begin / _end was
        for m in (0, 1):
            assert np.array_equal(engs[m].get_table(), tabs[m])          # nothing was written
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


# ------------------------------------------------------------------------------------------------ 6. interleaving
def test_interleaved_with_solo_steps_predict_and_evaluate(built, feed3):
    """A group step; a solo step on a member that is not the first; predict, evaluate and fnn_eval_multi; a group step with the
    list reordered, so that another member keeps the grouping; the announced batch.  The twins take the same batches solo."""
    specs = [Spec(m, 'bf16') for m in range(3)]
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
        assert np.array_equal(engs[2].predict(d[0][0]).cpu().numpy(), twins[2].predict(d[0][0]).cpu().numpy())
        y_i = feed3.put(feed3.y[1].astype(np.int32))
        assert 0 < feed3.y[1].sum() < len(feed3.y[1])
        assert engs[0].evaluate(d[1][0], y_i) == twins[0].evaluate(d[1][0], y_i)
        assert engine.evaluate_many(engs, d[1][0], y_i) == [t.evaluate(d[1][0], y_i) for t in twins]
        both([2, 0, 1], 1, d[2][0])                                      # another first member: its grouping is made now
        both([2, 0, 1], 2, None)                                         # the announced batch, the same first member
        both([1, 2], 0, None)
        for m in range(3):
            assert_same_state(engs[m], twins[m], 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_without_the_losses_a_bad_id_shows_in_that_handles_sync_only(built, feed3):
    specs = [Spec(0, 'bf16', n_rows=1500), Spec(1, 'bf16'), Spec(2, 'bf16', n_rows=1500)]
    engs = [sp.engine(feed3) for sp in specs]
    try:
        bad = feed3.ids[0].copy()
        bad[7, 3] = 1200
        rc, loss, _ = group_step(engs, feed3.put(bad), feed3.d[0][1], [sp.masks(feed3, 0) for sp in specs], None, want_loss=False)
        assert rc == 0 and loss == [-1.0] * 3
        assert [e.lib.fnn_sync(e.h) for e in engs] == [0, RANGE, 0]
        assert [e.lib.fnn_sync(e.h) for e in engs] == [0, 0, 0]
    finally:
        for e in engs:
            e.close()


def test_one_model_is_the_solo_step(built, feed3):
    run_against_twins([Spec(3, 'f32')], feed3)


# ------------------------------------------------------------------------------------------------ 7. engine
def test_train_step_many_returns_train_steps_dicts(built, feed3):
    specs = [Spec(0, 'bf16'), Spec(1, 'f32', 192, 40, 20)]
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
    """Seven batches of 100, the last one short."""
    feed = Feed([650], seed=9)
    specs = [Spec(0, 'bf16'), Spec(1, 'f32', 192, 40, 20), Spec(2, 'bf16')]
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    try:
        ids_d, y_d = feed.d[0]
        n = 7
        rng = np.random.RandomState(3)
        m1 = [(rng.uniform(size=(n, sp.H1)) < 0.7).astype(np.uint8) for sp in specs]
        m2 = [(rng.uniform(size=(n, sp.H2)) < 0.7).astype(np.uint8) for sp in specs]
        engine.train_epoch_many(engs, ids_d, y_d, 100, m1, m2)
        for m, t in enumerate(twins):
            t.train_epoch(ids_d, y_d, 100, m1[m], m2[m])
        for e in engs + twins:
            e.sync()
        for m, t in enumerate(twins):
            assert_same_state(engs[m], t, 'model %d' % m)
    finally:
        for e in engs + twins:
            e.close()


def test_a_mixed_list_gets_fnn_train_step_multis_refusal(built, feed3):
    from test_gpu_shapes import make_engine, make_problem
    rows, fo, _, _, p, _, _ = make_problem(F_, 11, 300, 100, 4, n_rows=NROWS, seed=5)
    fm = make_engine(F_, 11, 300, 100, rows, fo, p, prec='bf16', max_batch=BMAX)
    sp = Spec(0, 'bf16')
    bag = sp.engine(feed3)
    try:
        masks = [sp.masks(feed3, 0)] * 2
        with pytest.raises(FNNError) as ei:
            engine.train_step_many([fm, bag], feed3.d[0][0], feed3.d[0][1], [a for a, _ in masks], [b for _, b in masks])
        assert ei.value.code == ARG
        assert 'fnn_train_step_multi: model 1: FNN_MODE_BAG handles take fnn_train_step, one at a time' in str(ei.value)
    finally:
        fm.close(); bag.close()
