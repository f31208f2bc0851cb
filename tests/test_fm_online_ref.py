"""The cases of tests/fm_online_cases.py can catch what they are for: each holds the forwarding hazards, the duplicate columns,
the absent lines and fields and the weights it promises, and on the rows that several lines share the online schedule differs
from ONE batch step over the same lines by far more than the tolerance of the GPU test -- so a kernel that trained a line on
stale rows could not pass there.  CPU only."""
import numpy as np
import pytest

import fm_online_cases as oc
import fm_weighted_ref as wr

SHAPES = [(16, 11), (1, 1), (2, 16), (64, 16), (39, 11), (16, 17), (16, 101), (64, 128)]      # tests/test_gpu_fm_online.py's
LR, N = 0.05, 300


@pytest.mark.parametrize("F,k", SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_cases_hold_what_they_are_for(F, k, weighted):
    rows, ids, wts, y = oc.build(F, k, N, 100 + F + k, weighted)
    assert ids.shape == (N, F) and ids.min() == -1 and ids.max() < oc.N_ROWS
    c = oc.counts(ids, wts)
    if F == 1:                      # one column: a row cannot sit twice on a line, and an absent field is an all-absent line
        del c['row_twice_in_line'], c['absent_fields']
    for name, v in c.items():
        assert v > 0, (name, c)
    for n in (1, 4):                # what the short GPU cases (N = 2, 3) rely on: lines 1 and 2 repeat rows of line 0 / 1
        assert set(ids[n]) & set(ids[n - 1]) - {-1}
    assert set(ids[2]) & set(ids[0]) - {-1}


@pytest.mark.parametrize("F,k", SHAPES)
@pytest.mark.parametrize("lam", [0.0, 1e-2])
def test_the_schedule_is_not_one_batch_step(F, k, lam):
    """Sequential reference against one B = N step (reduce_sum: the same learning rate per line) of the same reference, on the
    rows that more than one line touches: at least 100 times 2e-3 * change + 2e-7, the bound the GPU test applies."""
    rows, ids, wts, y, ref_rows, ref_b, _, _ = oc.solved(F, k, N, 100 + F + k, True, LR, lam)
    batch = rows.copy()
    wr.sgd_step_w(batch, oc.B0, ids, oc.weights_or_ones(ids, wts), y, LR, lam, False)
    sh = oc.shared_rows(ids)
    assert len(sh) >= 8
    tol = 2e-3 * np.abs(ref_rows - rows).max() + 2e-7
    diff = np.abs(ref_rows[sh] - batch[sh]).max()
    assert diff >= 100 * tol, (diff, tol)


def test_sequential_is_the_batch_one_step_repeated():
    rows, ids, wts, y = oc.build(5, 4, 6, 7, True)
    r, b, p, loss = oc.sequential(rows, oc.B0, ids, wts, y, LR, 1e-2)
    r2, b2 = rows.copy(), oc.B0
    for n in range(6):
        assert p[n] == wr.predict_w(r2, b2, ids[n:n + 1], wts[n:n + 1])[0]
        b2, l2, _ = wr.sgd_step_w(r2, b2, ids[n:n + 1], wts[n:n + 1].astype(np.float64), y[n:n + 1], LR, 1e-2, False)   # sum == mean at B = 1
        assert l2 == loss[n]
    assert np.array_equal(r, r2) and b == b2
