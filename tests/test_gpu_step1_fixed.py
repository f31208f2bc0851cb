"""The strip kernel's fixed training form (k_step1<bf16, 5, 2, 4, false, 8, 47>: train = 1 and FNN_WT_STORES = 47 as compile-time
constants, the strip's ids requested ahead of the layer-1 weights) against the generic instance, which reads both at run time.
Nothing but the time of the loads and the waits differs, so two handles in one process -- one created under
FNN_STEP1_FORM=fixed, one under generic, the same table, dense weights, ids, labels and masks -- must agree BIT FOR BIT after
their steps: the table, w1 b1 w2 b2 w3 b3, the loss of every step and grad_bucket().

All cases are bf16 at 16 fields and hidden 300 / 100 (the only shape the fixed instance is built for).  Batches: 16 (one strip),
20 (a strip with padding rows), 272 (over 256: launch 2 runs the LDS weight-gradient form on eight-wave strips), 4096 with Zipf
ids (the benchmark's).  Over them: k = 4, 5, 11, 15 (the w_0 / ones slots in every lane and in two quarters of the row); fields
of 4 and 5 rows (synth.field_sizes_tiny), so rows repeat inside a strip; ids of -1 scattered and as a whole example; an id out
of range (the error rises on both sides, the states stay equal); three steps with and without fnn_prefetch_ids; dropout masks
all ones, all zeros and random.  Prediction, FNN_WT_STORES=0 and FNN_STEP1_WAVES=4 do not run the fixed instance: a `fixed`
handle must equal its `generic` twin there too (a mis-specialised launch would not).  One case holds the fixed form to the
float64 oracle at the bf16 bounds of tests/test_gpu_shapes.py.
"""
import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNEngine, FNNError

from test_gpu_shapes import check_step, make_problem

pytestmark = pytest.mark.gpu

F, H1, H2 = 16, 300, 100
LAM1, LAMFM, W0 = 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
NSTEP = 3

_PROBLEMS = {}


def problem_of(B, K, masks, n_rows=1000):
    """NSTEP batches over one table and one set of weights; computed once per case and never written to."""
    key = (B, K, masks, n_rows)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rows, fo, _, _, p, r1, r2 = make_problem(F, K, H1, H2, B, n_rows=n_rows, seed=B + K)
    sizes = synth.field_sizes_tiny(n_rows, n_fields=F)
    rng = np.random.RandomState(3 * B + K)
    ids = [synth.zipf_ids(B, sizes, 1.1, 50 + B + s) for s in range(NSTEP)]
    for s, i in enumerate(ids):
        for t, f in ((0, 0), (B // 2, 1), (B - 1, F - 1), (B // 3, 5), ((s + 1) % B, 12)):      # scattered empty fields
            i[t, f] = -1
        i[(3 + s) % B, :] = -1                                                              # a whole empty example
    if masks == 'ones':
        r1, r2 = np.ones(H1, np.uint8), np.ones(H2, np.uint8)
    elif masks == 'zeros':
        r1, r2 = np.zeros(H1, np.uint8), np.zeros(H2, np.uint8)
    y = (rng.uniform(size=(NSTEP, B)) < 0.3).astype(np.float32)
    pb = dict(B=B, K=K, rows=rows, fo=fo, ids=ids, y=y, p=p, r1=r1, r2=r2, n_rows=rows.shape[0], lr=0.001 if B >= 4096 else 0.01)
    _PROBLEMS[key] = pb
    return pb


def engine(monkeypatch, form, pb, env=()):
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('FNN_STEP1_FORM', form)                  # read where the handle is created
    eng = FNNEngine(F, pb['K'], H1, H2, max_batch=max(512, pb['B']), precision='bf16', lr=pb['lr'], lambda1=LAM1, lambda_fm=LAMFM)
    eng.set_table(pb['rows'], pb['fo'], W0)
    eng.set_dense(pb['p'])
    return eng


def steps(eng, pb, n, prefetch, ids=None):
    """n training steps -> (losses, error codes, grad_bucket after every step)."""
    import torch
    ids = pb['ids'] if ids is None else ids
    dev = [torch.as_tensor(i).to(eng.device).contiguous() for i in ids[:n]]
    loss, codes, bucket = [], [], []
    for s in range(n):
        if prefetch and s + 1 < n:
            eng.prefetch_ids(dev[s + 1])
        try:
            loss.append(eng.train_step(dev[s], pb['y'][s], pb['r1'], pb['r2'])['loss'])
            codes.append(0)
        except FNNError as e:
            loss.append(None)
            codes.append(e.code)
        bucket.append(eng.grad_bucket().cpu().numpy().copy())
    eng.sync()
    return loss, codes, bucket


def state(eng):
    return eng.get_table(), eng.get_dense()


def assert_same(a, b, sa, sb):
    """a, b: what steps() returned for the two handles; sa, sb: their state()."""
    assert a[1] == b[1], "error codes %r / %r" % (a[1], b[1])
    for s, (la, lb) in enumerate(zip(a[0], b[0])):
        assert la == lb, "loss of step %d: %r / %r" % (s, la, lb)
    for s, (ga, gb) in enumerate(zip(a[2], b[2])):
        assert np.array_equal(ga, gb), "grad_bucket of step %d: %d of %d floats differ" % (s, (ga != gb).sum(), ga.size)
    assert np.array_equal(sa[0], sb[0]), "table: %d of %d floats differ" % ((sa[0] != sb[0]).sum(), sa[0].size)
    for k in DENSE:
        assert np.array_equal(sa[1][k], sb[1][k]), k
    assert sa[1]['b3'] == sb[1]['b3'], "b3"


def both(monkeypatch, pb, n, prefetch, env=(), ids=None):
    """The same steps on a `fixed` and a `generic` handle that live side by side."""
    ef, eg = engine(monkeypatch, 'fixed', pb, env), engine(monkeypatch, 'generic', pb, env)
    try:
        a, b = steps(ef, pb, n, prefetch, ids), steps(eg, pb, n, prefetch, ids)
        sa, sb = state(ef), state(eg)
    finally:
        ef.close()
        eg.close()
    assert_same(a, b, sa, sb)
    return a, sa


# (B, k, masks): every batch, every k, every kind of mask
CASES = [(16, 4, 'ones'), (16, 15, 'random'), (20, 5, 'random'), (20, 11, 'zeros'), (272, 15, 'ones'), (272, 11, 'random'),
         (272, 4, 'zeros')]


@pytest.mark.parametrize("prefetch", [False, True], ids=['plain', 'prefetch'])
@pytest.mark.parametrize("B,K,masks", CASES)
def test_three_steps_are_bit_equal(built, monkeypatch, B, K, masks, prefetch):
    pb = problem_of(B, K, masks)
    a, sa = both(monkeypatch, pb, NSTEP, prefetch)
    assert a[1] == [0] * NSTEP and np.isfinite(a[0]).all()
    assert not np.array_equal(sa[0], pb['rows'])                 # the steps did move the rows


@pytest.mark.parametrize("K", [11, 5])
def test_the_benchmarks_batch_two_steps(built, monkeypatch, K):
    pb = problem_of(4096, K, 'random', n_rows=20000)
    a, sa = both(monkeypatch, pb, 2, True)
    assert a[1] == [0, 0] and np.isfinite(a[0]).all()
    assert not np.array_equal(sa[0], pb['rows'])


@pytest.mark.parametrize("B", [20, 272])
def test_an_id_out_of_range_raises_the_flag_on_both_sides(built, monkeypatch, B):
    pb = problem_of(B, 11, 'random')
    ids = [i.copy() for i in pb['ids']]
    ids[1][B - 2, 7] = pb['n_rows'] + 5                          # step 1 of 3; the steps around it are clean
    a, _ = both(monkeypatch, pb, NSTEP, False, ids=ids)
    assert a[1] == [0, _capi.FNN_ERR_RANGE, 0]


def test_prediction_runs_the_generic_instance(built, monkeypatch):
    pb = problem_of(272, 11, 'random')
    ef, eg = engine(monkeypatch, 'fixed', pb), engine(monkeypatch, 'generic', pb)
    try:
        pf, pg = ef.predict(pb['ids'][0]).cpu().numpy(), eg.predict(pb['ids'][0]).cpu().numpy()
        steps(ef, pb, 1, False)
        steps(eg, pb, 1, False)
        qf, qg = ef.predict(pb['ids'][1]).cpu().numpy(), eg.predict(pb['ids'][1]).cpu().numpy()
    finally:
        ef.close()
        eg.close()
    assert np.isfinite(pf).all() and pf.min() > 0.0 and pf.max() < 1.0
    assert np.array_equal(pf, pg) and np.array_equal(qf, qg)


@pytest.mark.parametrize("env", [('FNN_WT_STORES', '0'), ('FNN_WT_STORES', '15'), ('FNN_STEP1_WAVES', '4')], ids=lambda e: '%s=%s' % e)
@pytest.mark.parametrize("B", [20, 272])
def test_other_store_policies_and_four_waves_fall_back(built, monkeypatch, env, B):
    pb = problem_of(B, 11, 'random')
    a, _ = both(monkeypatch, pb, 2, True, env=(env,))
    assert a[1] == [0, 0]


def test_the_fixed_form_and_the_default_agree(built, monkeypatch):
    """An unset switch is `fixed`."""
    pb = problem_of(272, 11, 'random')
    monkeypatch.delenv('FNN_STEP1_FORM', raising=False)
    ed = FNNEngine(F, pb['K'], H1, H2, max_batch=512, precision='bf16', lr=pb['lr'], lambda1=LAM1, lambda_fm=LAMFM)
    ed.set_table(pb['rows'], pb['fo'], W0)
    ed.set_dense(pb['p'])
    ef = engine(monkeypatch, 'fixed', pb)
    try:
        a, b = steps(ed, pb, 2, True), steps(ef, pb, 2, True)
        sa, sb = state(ed), state(ef)
    finally:
        ed.close()
        ef.close()
    assert_same(a, b, sa, sb)


@pytest.mark.parametrize("B,K", [(272, 11), (20, 4)])
def test_the_fixed_form_within_the_oracles_bounds(built, monkeypatch, B, K):
    """One step against the float64 oracle at the bf16 bounds of test_gpu_shapes.check_step (p, gx', loss, table)."""
    monkeypatch.setenv('FNN_STEP1_FORM', 'fixed')
    prob = make_problem(F, K, H1, H2, B, seed=5, empty=[(0, 0), (B // 2, 1), (B - 1, F - 1)])
    rows, fo, ids, y, p, r1, r2 = prob
    eng = FNNEngine(F, K, H1, H2, max_batch=512, precision='bf16', lr=0.01, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(rows, fo, W0)
        eng.set_dense(p)
        check_step(eng, prob, 0.01, LAM1, LAMFM, prec='bf16', label='step1 fixed B%d k%d' % (B, K))
    finally:
        eng.close()
