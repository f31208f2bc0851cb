"""Seeded cases for FM / LR pre-training on the online schedule (fm_train_online): N lines trained one after another, each on
the parameters the lines before it left.  Shared by tests/test_fm_online_ref.py (which checks that the cases hold what they are
for) and tests/test_gpu_fm_online.py.  Test infrastructure, not a test module.

Every case of three or more lines and two or more fields holds
  - lines that repeat a row of the line before (every line n with n % 3 == 1) and of the line two before (n % 3 == 2): the rows
    a kernel that requested a line's rows too early would read stale;
  - a row twice within one line (n % 7 == 3) and one row under ALL columns of a line (n % 11 == 5);
  - an all-absent line (n % 13 == 6) and absent fields elsewhere (a tenth of the entries; beyond 24 fields, all but 24 or so);
  - with `weighted`, fm_weighted_ref.test_weights: exact zeros, exact ones and negatives.
With one field a row cannot sit twice on a line; everything else holds there too.

Sizes.  The table is N(0, 1) * 0.5 / sqrt(F k), so that yhat is O(1) at every shape (the pair term sums F^2 k products).  A row
under all F columns of a line moves by lr * delta * F (F - 1) times itself -- 200 times at 64 fields -- whatever the data: each
such line has a row of its own at the end of the table, a further factor F smaller.  And lr = 0.05 times the number of features
on a line is the step of the linear part: lines hold about 24 features at most (iPinYou's have 16).  So the run stays a model
being trained, whose predictions do not saturate, at every shape.

The float64 reference of the schedule is fm_weighted_ref.sgd_step_w on one-line slices, N times in order (`sequential`)."""
import functools

import numpy as np

import fm_weighted_ref as wr

N_ROWS = 300
B0 = 0.1


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def build(F, k, N, seed, weighted, n_rows=N_ROWS):
    """(rows [n_rows, k] f64 holding f32 values, ids [N, F] int32, wts [N, F] f32 or None, y [N] f64)."""
    rng = np.random.RandomState(seed)
    n_all = N // 11 + 1                                           # the last rows of the table: one per all-columns line
    rows = rng.standard_normal((n_rows, k)) * (0.5 / np.sqrt(F * k))
    rows[n_rows - n_all:] /= F
    rows = f32r(rows)
    ids = rng.randint(0, n_rows - n_all, size=(N, F))
    hot = rng.uniform(size=(N, F)) < 0.3                          # a few hot rows, as a Zipf feed has: max(8, F) of them
    ids[hot] = rng.randint(0, max(8, F), size=int(hot.sum()))
    ids[rng.uniform(size=(N, F)) < max(0.1, 1.0 - 24.0 / F)] = -1    # absent fields: a tenth, more where a line would pass 24 features
    for n in range(N):
        if ids[n, 0] < 0:
            ids[n, 0] = rng.randint(0, n_rows)
        for back in (1, 2):
            if n >= back and n % 3 == back:
                live = ids[n - back][ids[n - back] >= 0]
                if len(live):
                    ids[n, rng.randint(0, F)] = live[rng.randint(0, len(live))]
        if n % 7 == 3 and F >= 2:
            ids[n, F - 1] = ids[n, 0]                             # one row under two columns of the line
        if n % 11 == 5:
            ids[n, :] = n_rows - 1 - n // 11                      # ... and under all of them
        if n % 13 == 6:
            ids[n, :] = -1                                        # nothing on the line: only b moves
    y = (rng.uniform(size=N) < 0.3).astype(np.float64)
    wts = wr.test_weights(N, F, seed + 1) if weighted else None
    return rows, np.ascontiguousarray(ids, dtype=np.int32), wts, y


def weights_or_ones(ids, wts):
    return np.ones(ids.shape) if wts is None else np.asarray(wts, np.float64)


def sequential(rows, b, ids, wts, y, lr, lam):
    """The online schedule in float64: (rows, b, p [N] before each line's update, losses [N])."""
    r, w = rows.copy(), weights_or_ones(ids, wts)
    p, loss = np.empty(len(y)), np.empty(len(y))
    for n in range(len(y)):
        b, loss[n], pn = wr.sgd_step_w(r, b, ids[n:n + 1], w[n:n + 1], y[n:n + 1], lr, lam, True)
        p[n] = pn[0]
    return r, b, p, loss


@functools.lru_cache(maxsize=None)
def solved(F, k, N, seed, weighted, lr, lam):
    """A case and its sequential reference, computed once: (rows, ids, wts, y, ref_rows, ref_b, ref_p, ref_loss).  Read only."""
    rows, ids, wts, y = build(F, k, N, seed, weighted)
    out = (rows, ids, wts, y) + sequential(rows, B0, ids, wts, y, lr, lam)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def counts(ids, wts):
    """How often a case holds each thing it is for."""
    N, F = ids.shape
    live = [set(int(v) for v in ids[n] if v >= 0) for n in range(N)]
    twice = all_cols = 0
    for n in range(N):
        v = ids[n][ids[n] >= 0]
        twice += len(v) != len(set(v.tolist()))
        all_cols += len(v) == F and len(set(v.tolist())) == 1
    c = {'repeats_line_before': sum(bool(live[n] & live[n - 1]) for n in range(1, N)),
         'repeats_two_before': sum(bool(live[n] & live[n - 2]) for n in range(2, N)),
         'row_twice_in_line': twice, 'row_under_all_columns': all_cols,
         'all_absent_lines': sum(not s for s in live),
         'absent_fields': int(((ids < 0).sum(axis=1) % F != 0).sum())}     # lines with some, not all, fields absent
    if wts is not None:
        w = np.asarray(wts)[ids >= 0]
        c.update(zero_weights=int((w == 0).sum()), negative_weights=int((w < 0).sum()), other_weights=int(((w != 0) & (w != 1)).sum()))
    return c


def shared_rows(ids):
    """Rows that more than one line of the case touches."""
    seen, shared = set(), set()
    for n in range(ids.shape[0]):
        s = set(int(v) for v in ids[n] if v >= 0)
        shared |= s & seen
        seen |= s
    return np.array(sorted(shared), dtype=np.int64)
