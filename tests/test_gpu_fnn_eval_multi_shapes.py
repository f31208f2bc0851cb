"""fnn_eval_multi / fnn_predict_multi beyond 16 fields x k = 11 and N = 8,229: one prediction launch class whose members differ
in k, hidden size inside a padded shape and max_batch, at 13 and 16 fields; N at the edges of a strip (16 lines), of a metric
block (256) and of a feed batch (4,096, or 256 under FNN_EVAL_FEED_BATCH); members that run their own launches at 12, 17 and 39
fields; a data-parallel, a four-wave and an FNN_NO_FUSE member beside default ones.

Every member is held to its solo twin's fnn_eval on the same device feed, bit for bit: p_out as uint32, auc / rmse / logloss
with ==, the status.  The p of member 0 also goes against orc.predict in float64 on the member's own state (as
test_predict_vs_oracle of test_gpu_shapes.py: rtol 1e-4, atol 1e-6 in f32; the other precisions take check_step's bound on p of
the same file: eight times that in bf16x3, atol 2e-2 in bf16), so that a twin and a group that gather alike wrongly do not pass;
each case prints the worst error as a fraction of that bound.  Every p_out buffer has 64 sentinel floats behind N, which must
stay.

Which case runs which branch of gpredict_sel (deep-ctr_amd/csrc/fnn_api.hip), per element type (continues the table of
tests/test_gpu_fnn_step_multi_shapes.py):

  gpredict_sel                      bf16                          f32                           bf16x3
  big (320 / 128), 8 waves          mixed[F13-bf16], [F16-bf16]   mixed[F13-f32], [F16-f32]     mixed[F13-bf16x3], [F16-bf16x3]
  big, 4 waves (FNN_STEP1_WAVES=4)  test_members_of_other_kinds_at_16_fields: members 2 (bf16), 3 (f32), 4 (bf16x3)
  small (64 / 64), 4 waves          the 63 / 63 and 1 / 1 members of the mixed[..] cases, every type
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401

from test_gpu_shapes import Bounds, f32r
from test_gpu_fnn_eval_multi import (RANGE, SENT, Feed, Spec, bits, eval_multi, last_error, predict_multi, same_metric, solo_eval)

pytestmark = pytest.mark.gpu

TAIL = 64
KNOB_VARS = ('FNN_STEP1_WAVES', 'FNN_NO_FUSE', 'FNN_EVAL_FEED_BATCH', 'FNN_EVAL_ORDER', 'FNN_EVAL_LAUNCH', 'FNN_EVAL_SCRATCH_BYTES')
_feeds = {}


def feed_for(F, n, K=11):
    """One device feed per layout and length, made once and never changed: edge_empties, and both classes in its first two lines."""
    if (F, K, n) not in _feeds:
        fd = Feed(F=F, K=K, n=n, empties=True)
        fd.y[0], fd.y[1] = 1, 0
        fd.y_d, fd.yf_d = fd.put(fd.y), fd.put(fd.y.astype(np.float32))
        _feeds[(F, K, n)] = fd
    return _feeds[(F, K, n)]


def p_bound(bd, prec, got, ref, what):
    if prec == 'bf16':
        bd.close(what, got, ref, 0.0, 2e-2)
    else:
        tol = 8.0 if prec == 'bf16x3' else 1.0
        bd.close(what, got, ref, 1e-4 * tol, 1e-6 * tol)


def oracle_p(eng, sp, ids):
    """orc.predict in float64 on the handle's own table and dense tensors."""
    d = {k: (f32r(v) if isinstance(v, np.ndarray) else v) for k, v in eng.get_dense().items()}
    return orc.predict(d, orc.gather_vec(eng.get_table().astype(np.float64), ids, -3.0), sp.acti)


def assert_member(got, m, ref, n, what):
    """Model m of eval_multi's result against solo_eval's of its twin: p with its sentinels, the metrics, the status."""
    rc, auc, rmse, ll, st, ps = got
    assert ref[0] == 0, what
    assert np.isfinite(ref[4][:n]).all() and (ref[4][:n] != SENT).all(), what
    assert np.array_equal(bits(ps[m][:n]), bits(ref[4][:n])), '%s: p, %d of %d differ' % (what, (bits(ps[m][:n]) != bits(ref[4][:n])).sum(), n)
    assert (ps[m][n:] == SENT).all() and ps[m][n:].size == TAIL, '%s: written behind N' % what
    assert (auc[m], rmse[m], ll[m]) == ref[1:4], '%s: metrics %r against %r' % (what, (auc[m], rmse[m], ll[m]), ref[1:4])
    assert st[m] == 0, what


def group_against_twins(specs, feed, n, label, make=None, tb=64):
    """The members of `specs` (make(m, sp): another way to create member m and its twin) through fnn_eval_multi and
    fnn_predict_multi on the feed's first n lines, against their twins' fnn_eval; member 0 against the oracle."""
    make = make or (lambda m, sp: sp.engine(feed, tb=tb))
    engs, twins = [], []
    try:
        for m, sp in enumerate(specs):
            engs.append(make(m, sp))
            twins.append(make(m, sp))
        ids_t, y_t = feed.ids_d[:n], feed.y_d[:n]
        got = eval_multi(engs, ids_t, y_t, tail=TAIL)
        assert got[0] == 0, last_error(engs[0])
        rc, ps = predict_multi(engs, ids_t, tail=TAIL)
        assert rc == 0, last_error(engs[0])
        for m, t in enumerate(twins):
            what = '%s: model %d (%s %dx%d k=%d)' % (label, m, specs[m].prec, specs[m].H1, specs[m].H2, specs[m].k)
            ref = solo_eval(t, ids_t, y_t, tail=TAIL)
            assert (ref[4][n:] == SENT).all(), what
            assert_member(got, m, ref, n, what)
            assert np.array_equal(bits(ps[m][:n]), bits(ref[4][:n])) and (ps[m][n:] == SENT).all(), what + ', fnn_predict_multi'
        assert [e.lib.fnn_sync(e.h) for e in engs] == [0] * len(engs)
        bd = Bounds()
        p_bound(bd, specs[0].prec, got[5][0][:n], oracle_p(engs[0], specs[0], feed.ids[:n]), 'p')
        bd.report('group ' + label)
    finally:
        for e in engs + twins:
            e.close()


# ------------------------------------------------------------------------------------------------ 2a: mixed members of a class
MIXED = [(F, prec) for F in (13, 16) for prec in ('bf16', 'f32', 'bf16x3')]


@pytest.mark.parametrize("F,prec", MIXED, ids=['F%d-%s' % c for c in MIXED])
def test_one_class_with_mixed_k_hidden_and_max_batch(built, monkeypatch, F, prec):
    """One launch class of k = 1, 5, 11 and 15 at hidden 256 / 64, 300 / 100 and 319 / 127 with max_batch 64, 512 and 4,096
    (member 0: k = 1 at 16 fields, k = 15 at 13), a second one at 63 / 63 and 1 / 1, the two interleaved; N = 4,113: a whole feed
    batch and a ragged second one."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    feed = feed_for(F, 4113)
    ks = (1, 5, 11, 15) if F == 16 else (15, 11, 5, 1)
    lay = [(ks[0], 256, 64, 64), (ks[1], 63, 63, 64), (ks[1], 300, 100, 512), (ks[2], 319, 127, 4096), (ks[3], 1, 1, 512),
           (ks[3], 300, 100, 512)]
    specs = [Spec(m, prec, H1, H2, max_batch=mb, k=k, F=F) for m, (k, H1, H2, mb) in enumerate(lay)]
    group_against_twins(specs, feed, 4113, '2a F%d %s' % (F, prec))


# ------------------------------------------------------------------------------------------------ 2b: N at the edges
EDGE = [Spec(0, 'f32', 300, 100, max_batch=512, k=5), Spec(1, 'bf16', 40, 20, max_batch=64, k=5), Spec(2, 'bf16x3', 319, 127, max_batch=4096, k=5),
        Spec(3, 'bf16', 290, 90, max_batch=256, k=5)]
NS = {'4096': [2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097], '256': [256, 257, 512]}


@pytest.fixture(scope='module')
def edge(built):
    """The four members, their twins, the twins' solo results per N and the oracle's p of member 0, each computed once."""
    import os
    assert not any(v in os.environ for v in KNOB_VARS)
    feed = feed_for(16, 4097, K=5)
    engs, twins = [sp.engine(feed, tb=64) for sp in EDGE], [sp.engine(feed, tb=64) for sp in EDGE]
    refs = {}

    def ref(n):
        if n not in refs:
            refs[n] = [solo_eval(t, feed.ids_d[:n], feed.y_d[:n], tail=TAIL) for t in twins]
        return refs[n]

    yield feed, engs, twins, ref, oracle_p(engs[0], EDGE[0], feed.ids)
    for e in engs + twins:
        e.close()


@pytest.mark.parametrize("order", ['tile', 'model'])
@pytest.mark.parametrize("fb", ['4096', '256'])
def test_n_at_the_edges_of_strip_block_and_feed_batch(built, monkeypatch, edge, fb, order):
    """N = 2, 15, 16, 17, 255, 256, 257, 4,095, 4,096 and 4,097 at the default feed batch; 256, 257 and 512 at feed batches of
    256; each under both grid orders.  Labels hold both classes in every prefix."""
    feed, engs, twins, ref, p64 = edge
    if fb != '4096':
        monkeypatch.setenv('FNN_EVAL_FEED_BATCH', fb)
    monkeypatch.setenv('FNN_EVAL_ORDER', order)
    bd = Bounds()
    for n in NS[fb]:
        ids_t, y_t = feed.ids_d[:n], feed.y_d[:n]
        got = eval_multi(engs, ids_t, y_t, tail=TAIL)
        assert got[0] == 0, last_error(engs[0])
        rc, ps = predict_multi(engs, ids_t, tail=TAIL)
        assert rc == 0, last_error(engs[0])
        for m in range(len(engs)):
            r = ref(n)[m]
            assert_member(got, m, r, n, 'N = %d, model %d' % (n, m))
            assert np.array_equal(bits(ps[m][:n]), bits(r[4][:n])) and (ps[m][n:] == SENT).all(), 'fnn_predict_multi, N = %d, model %d' % (n, m)
        p_bound(bd, EDGE[0].prec, got[5][0][:n], p64[:n], 'p at N = %d' % n)
    bd.report('group 2b feed batch %s, order %s' % (fb, order))


def test_one_line(built, monkeypatch, edge):
    """N = 1 has one class: fnn_predict_multi gives the twins' fnn_predict; fnn_eval_multi returns FNN_ERR_RANGE with every auc
    NaN and rmse and logloss written, as the twins' fnn_eval does."""
    feed, engs, twins, ref, p64 = edge
    ids_t, y_t = feed.ids_d[:1], feed.y_d[:1]
    rc, ps = predict_multi(engs, ids_t, tail=TAIL)
    assert rc == 0, last_error(engs[0])
    got = eval_multi(engs, ids_t, y_t, tail=TAIL)
    assert got[0] == RANGE
    assert last_error(engs[0]) == 'fnn_eval_multi: only one class present in y (roc_auc_score raises ValueError)'
    assert np.isnan(got[1]).all() and got[4] == [0] * len(engs)
    for m, t in enumerate(twins):
        solo = t.predict(ids_t).cpu().numpy()
        assert np.array_equal(bits(ps[m][:1]), bits(solo)) and (ps[m][1:] == SENT).all(), 'model %d' % m
        r = solo_eval(t, ids_t, y_t, tail=TAIL)
        assert r[0] == RANGE and np.isnan(r[1])
        assert np.isfinite([got[2][m], got[3][m]]).all() and same_metric(got[2][m], r[2]) and same_metric(got[3][m], r[3]), 'model %d' % m
        assert np.array_equal(bits(got[5][m][:1]), bits(r[4][:1])) and (got[5][m][1:] == SENT).all(), 'model %d' % m
    bd = Bounds()
    p_bound(bd, EDGE[0].prec, ps[0][:1], p64[:1], 'p at N = 1')
    bd.report('group 2b one line')


# ------------------------------------------------------------------------------------------------ 2c: members off the group launch
@pytest.mark.parametrize("F", [12, 17, 39])
def test_groups_whose_members_run_their_own_launches(built, monkeypatch, F):
    """12, 17 and 39 fields: no member is on the strip kernel, each runs the layer-by-layer kernels in chunks of its max_batch
    inside the call; at 39 fields one member has wide rows (k = 21).  N = 1,043: no multiple of any max_batch or of 16."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    feed = feed_for(F, 1043)
    specs = [Spec(0, 'f32', 300, 100, max_batch=512, k=11, F=F), Spec(1, 'bf16', 200, 50, max_batch=64, k=5, F=F),
             Spec(2, 'bf16x3', 63, 63, max_batch=256, k=15, F=F)]
    if F == 39:
        specs.append(Spec(3, 'bf16', 300, 100, max_batch=512, k=21, F=F))
    group_against_twins(specs, feed, 1043, '2c F%d' % F)


def test_members_of_other_kinds_at_16_fields(built, monkeypatch):
    """A handle after fnn_dp_init_custom with world 1, handles created under FNN_STEP1_WAVES=4 in the three precisions (the
    four-wave prediction instance, launch classes of their own), one created under FNN_NO_FUSE=1 (its own launches) and default
    members of the same shape, in one call."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    feed = feed_for(16, 1043)
    w4, nofuse = {'FNN_STEP1_WAVES': '4'}, {'FNN_NO_FUSE': '1'}
    kinds = [('f32', None), ('bf16', 'dp'), ('bf16', w4), ('f32', w4), ('bf16x3', w4), ('bf16', nofuse), ('bf16', None), ('bf16x3', None)]
    specs = [Spec(m, prec, 300, 100, k=11) for m, (prec, _) in enumerate(kinds)]

    def make(m, sp):
        env = kinds[m][1]
        for k, v in (env.items() if isinstance(env, dict) else ()):
            monkeypatch.setenv(k, v)
        try:
            eng = sp.engine(feed, tb=64)
        finally:
            for v in KNOB_VARS:
                monkeypatch.delenv(v, raising=False)
        if env == 'dp':
            eng.dp_init_custom(0, 1, lambda view: None, None, sparse='local')
        return eng

    group_against_twins(specs, feed, 1043, '2c kinds at 16 fields', make=make)
