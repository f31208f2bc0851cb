"""The head of the strip kernel's fixed training form -- z3's row sums by DPP moves and one 16-byte LDS store, the waves' partial
sums in one LDS trip, the four sigmoids together, the p_out store behind them -- against the generic instance, which keeps the
shuffle sums and the row-by-row head.  Only the way the same values travel differs, so, as in test_gpu_step1_fixed.py, a handle
created under FNN_STEP1_FORM=fixed and one under generic, with the same state, must agree BIT FOR BIT after three steps: every
step's loss, grad_bucket(), the table and the dense layers.

All cases are bf16 at 16 fields and hidden 300 / 100.  Batches: 16 (one strip), 20 (a strip with four live rows in its second
quarter -- one lane group of the head -- and twelve padding rows), 272 (more than one workgroup).  Over them: labels all 0 and
all 1; masks all zeros (z is b3 alone with zeros) and all ones; w3 scaled until |z| passes 30 with both signs (softplus and
sigmoid at saturation; the float64 oracle says which rows); whole examples of -1 ids, the last live row among them.  One case
holds the fixed form to the float64 oracle at the bf16 bounds of tests/test_gpu_shapes.py, and one asks the training step for
its predictions (the C ABI's p_out), which the fixed form stores outside the row loop.
"""
import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine
from oracle import fnn_oracle as orc

from test_gpu_shapes import check_step, make_problem
from test_gpu_step1_fixed import F, H1, H2, LAM1, LAMFM, W0, NSTEP, both, engine

pytestmark = pytest.mark.gpu

K = 11
BATCHES = [16, 20, 272]
ZSAT = 30.0

_PROBLEMS = {}


def problem_of(B, kind):
    """NSTEP batches over one table and one set of weights; computed once per (B, kind) and never written to."""
    key = (B, kind)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rows, fo, _, _, p, r1, r2 = make_problem(F, K, H1, H2, B, seed=7 * B + 1)
    sizes = synth.field_sizes_tiny(1000, n_fields=F)
    rng = np.random.RandomState(11 * B + 5)
    ids = [synth.zipf_ids(B, sizes, 1.1, 90 + B + s) for s in range(NSTEP)]
    y = (rng.uniform(size=(NSTEP, B)) < 0.3).astype(np.float32)
    lr = 0.01
    if kind == 'labels0':
        y[:] = 0.0
    elif kind == 'labels1':
        y[:] = 1.0
    elif kind == 'masks0':
        r1, r2 = np.zeros(H1, np.uint8), np.zeros(H2, np.uint8)
    elif kind == 'masks1':
        r1, r2 = np.ones(H1, np.uint8), np.ones(H2, np.uint8)
    elif kind == 'saturated':
        p = dict(p)
        p['w3'] = (p['w3'] * 400.0).astype(np.float32)
        lr = 0.001
        # the rows' z share a large common part (w_0 and the biases reach every row alike): b3 centres them on the first batch
        z = oracle_z(dict(rows=rows, ids=ids, y=y, p=dict(p, b3=0.0), r1=r1, r2=r2, lr=lr))
        p['b3'] = float(np.float32(-np.median(z)))
    elif kind == 'empty':
        for s, i in enumerate(ids):
            i[B - 1, :] = -1                                     # the last live row of the last strip
            i[(5 + s) % (B - 1), :] = -1
            i[B - 2, F - 1] = -1
    pb = dict(B=B, K=K, rows=rows, fo=fo, ids=ids, y=y, p=p, r1=r1, r2=r2, n_rows=rows.shape[0], lr=lr)
    _PROBLEMS[key] = pb
    return pb


def oracle_z(pb, s=0):
    """z3 of batch s at the initial state, by the float64 oracle (copies: the problem stays as it is)."""
    p64 = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else float(v)) for k, v in pb['p'].items()}
    x = orc.gather(pb['rows'].astype(np.float64), pb['ids'][s], W0)
    d2 = orc.forward_train(p64, x, pb['r1'].astype(np.float64), pb['r2'].astype(np.float64), 'tanh')[3]
    return d2 @ p64['w3'] + p64['b3']


def run(monkeypatch, pb):
    a, sa = both(monkeypatch, pb, NSTEP, False)
    assert a[1] == [0] * NSTEP and np.isfinite(a[0]).all()
    assert np.isfinite(sa[0]).all() and all(np.isfinite(sa[1][k]).all() for k in ('w1', 'b1', 'w2', 'b2', 'w3'))
    return a, sa


@pytest.mark.parametrize("B", BATCHES)
def test_strip_shapes(built, monkeypatch, B):
    pb = problem_of(B, 'plain')
    _, sa = run(monkeypatch, pb)
    assert not np.array_equal(sa[0], pb['rows'])                 # the steps did move the rows


@pytest.mark.parametrize("kind", ['labels0', 'labels1'])
@pytest.mark.parametrize("B", BATCHES)
def test_label_extremes(built, monkeypatch, B, kind):
    run(monkeypatch, problem_of(B, kind))


@pytest.mark.parametrize("kind", ['masks0', 'masks1'])
@pytest.mark.parametrize("B", BATCHES)
def test_mask_extremes(built, monkeypatch, B, kind):
    pb = problem_of(B, kind)
    a, _ = run(monkeypatch, pb)
    if kind == 'masks0':                                        # z = b3 on every row: the loss is B softplus(b3) - b3 sum(y)
        b3 = pb['p']['b3']
        want = B * np.log1p(np.exp(b3)) - b3 * pb['y'][0].sum()
        assert abs(a[0][0] - want) <= 1e-4 * want


@pytest.mark.parametrize("B", BATCHES)
def test_saturated_output_unit(built, monkeypatch, B):
    pb = problem_of(B, 'saturated')
    z = oracle_z(pb)
    assert z.min() < -ZSAT and z.max() > ZSAT, "the case must saturate both ways: z in [%g, %g]" % (z.min(), z.max())
    run(monkeypatch, pb)


@pytest.mark.parametrize("B", BATCHES)
def test_empty_examples_and_the_last_live_row(built, monkeypatch, B):
    run(monkeypatch, problem_of(B, 'empty'))


def test_the_fixed_form_within_the_oracles_bounds(built, monkeypatch):
    """One step against the float64 oracle at the bf16 bounds of test_gpu_shapes.check_step (p, gx', loss, table)."""
    B = 20
    monkeypatch.setenv('FNN_STEP1_FORM', 'fixed')
    prob = make_problem(F, K, H1, H2, B, seed=9, empty=[(0, 0), (B - 1, F - 1)])
    prob[2][B - 1, :] = -1
    rows, fo, ids, y, p, r1, r2 = prob
    eng = FNNEngine(F, K, H1, H2, max_batch=512, precision='bf16', lr=0.01, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        eng.set_table(rows, fo, W0)
        eng.set_dense(p)
        check_step(eng, prob, 0.01, LAM1, LAMFM, prec='bf16', label='step1 head B%d' % B)
    finally:
        eng.close()


@pytest.mark.parametrize("B", [20, 272])
def test_predictions_from_a_training_step(built, monkeypatch, B):
    """want_p: the step's p_out.  Exactly B floats are written (a guard value behind them would not fit the tensor the engine
    allocates, so the check is on the values): bit-equal, inside (0, 1), and what the loss says they are."""
    pb = problem_of(B, 'empty')
    ef, eg = engine(monkeypatch, 'fixed', pb), engine(monkeypatch, 'generic', pb)
    try:
        of = [ef.train_step(pb['ids'][s], pb['y'][s], pb['r1'], pb['r2'], want_p=True) for s in range(NSTEP)]
        og = [eg.train_step(pb['ids'][s], pb['y'][s], pb['r1'], pb['r2'], want_p=True) for s in range(NSTEP)]
        pf, pg = [o['p'].cpu().numpy() for o in of], [o['p'].cpu().numpy() for o in og]
    finally:
        ef.close()
        eg.close()
    for s in range(NSTEP):
        assert of[s]['loss'] == og[s]['loss']
        assert pf[s].shape == (B,) and np.array_equal(pf[s], pg[s]), "p of step %d" % s
        assert np.isfinite(pf[s]).all() and pf[s].min() >= 0.0 and pf[s].max() <= 1.0
    # the first step's predictions come from the initial weights, far from saturation (a 272-example step at this rate drives
    # the later ones to 1.0f on both sides): strictly inside (0, 1), and the loss is their cross-entropy
    assert pf[0].min() > 0.0 and pf[0].max() < 1.0
    yy, q = pb['y'][0].astype(np.float64), pf[0].astype(np.float64)
    xent = -(yy * np.log(q) + (1 - yy) * np.log1p(-q)).sum()
    assert abs(of[0]['loss'] - xent) <= 1e-4 * xent
