"""Inputs of the shared-row tests of FM / LR pre-training (tests/test_fm_shared_ref.py on the CPU, tests/test_gpu_fm_shared.py on
the GPU): batches in which chosen rows sit in chosen (example, column) cells over a ragged background that shares nothing, the
NumPy count of shared rows, and the float64 restatement the GPU results are held to.  Test infrastructure.

The restatement is tests/fm_weighted_ref.py unchanged (TrainerW; weights of 1 where a test has none): its gradient is a sum over
(example, column) entries with np.add.at, which does not care under which column a row sits.  test_fm_shared_ref.py holds it to
float64 autograd of python/FM.py:55-64 on exactly such ids.

Layout of a table: rows 0 .. S_ROWS - 1 are the rows tests place by hand (the smallest ids, so that in the sorted entries of a
column they come first and their segments' positions are known), then `per` rows owned by each column (the background: a row
of column j never shows under another column), then one last row no background uses (the reference's pad row)."""
import numpy as np

import fm_weighted_ref as wr

S_ROWS = 8


def n_rows_of(F, per):
    return S_ROWS + F * per + 1


def background(B, F, per, seed, absent=0.15):
    """ids [B, F] int32: column j draws from its own `per` rows (squared uniform: repeated rows inside a column), a fraction is
    -1, and half of the lines end early (all -1 from a random position on) like lines shorter than the longest one."""
    rng = np.random.RandomState(seed)
    ids = S_ROWS + np.arange(F)[None, :] * per + np.floor(per * rng.uniform(size=(B, F)) ** 2).astype(np.int64)
    ids[rng.uniform(size=(B, F)) < absent] = -1
    for t in range(B):
        if rng.uniform() < 0.5:
            ids[t, rng.randint(1, F + 1):] = -1
    return ids.astype(np.int32)


def place(ids, row, cells):
    """ids[t, j] = row for every (t, j) of cells."""
    for t, j in cells:
        ids[t, j] = row
    return ids


def shared_count(ids):
    """Rows that sit under more than one column of the batch."""
    per_col = [np.unique(c[c >= 0]) for c in np.asarray(ids).T]
    _, cnt = np.unique(np.concatenate(per_col), return_counts=True)
    return int((cnt > 1).sum())


def labels(B, seed):
    return (np.random.RandomState(seed).uniform(size=B) < 0.3).astype(np.float64)


def basic_batch(B, F, per, seed):
    """The narrow case list of the issue in one batch: row 0 under columns 0 and 1 (two, or the only column twice when F = 1
    cannot share: F >= 2 here), row 1 under every column, row 2 twice on line 5, line 6 holding shared rows only, -1 ids."""
    ids = background(B, F, per, seed)
    place(ids, 0, [(0, 0), (1, 0), (2, 1)])
    place(ids, 1, [(10 + i % (B - 10), i % F) for i in range(2 * F)])    # every column, two entries each
    place(ids, 2, [(5, 0), (5, F - 1)])                                  # twice on one line
    ids[6, :] = -1
    place(ids, 0, [(6, 1)])
    place(ids, 1, [(6, 0)])                                              # line 6: shared rows only
    ids[7, :] = -1                                                       # an empty line
    return ids


def hot_batch(B, F, per, seed):
    """Level-1 / level-2 split (B = 300, F >= 4).  Sorted entries of a column start with the hand-placed rows in id order:
    row 0: 40 entries in column 0 -> positions 0 .. 39, several chunks of 16 (narrow) or 32 (wide): a level-2 add; 3 entries in
           column 2 -> positions 0 .. 2, inside a chunk: a level-1 add;
    row 1: 8 entries in column 1 -> positions 0 .. 7, ends on the 8|8 border of chunk 0; one entry in column 3 (position 0);
    row 2: 8 entries in column 1 -> positions 8 .. 15, ends on the chunk border; one entry in column 3 (position 1)."""
    ids = background(B, F, per, seed)
    place(ids, 0, [(t, 0) for t in range(20, 60)] + [(t, 2) for t in (3, 100, 299)])
    place(ids, 1, [(t, 1) for t in range(70, 78)] + [(150, 3)])
    place(ids, 2, [(t, 1) for t in range(80, 88)] + [(151, 3)])
    return ids


def segments(ids, j):
    """{row: (s, e)}: the positions [s, e) a row's entries take among column j's entries sorted by (row, example)."""
    col = np.asarray(ids)[:, j]
    live = np.sort(col[col >= 0], kind='stable')
    out = {}
    for r in np.unique(live):
        w = np.nonzero(live == r)[0]
        out[int(r)] = (int(w[0]), int(w[-1]) + 1)
    return out


def ones_like_ids(ids):
    return np.ones(np.asarray(ids).shape)


class Trainer(wr.TrainerW):
    """fm_weighted_ref.TrainerW with wts=None meaning every value is 1."""

    def sgd_step(self, ids, y, wts=None):
        return wr.TrainerW.sgd_step(self, ids, y, ones_like_ids(ids) if wts is None else wts)

    def step(self, ids, y, wts=None):
        return wr.TrainerW.step(self, ids, y, ones_like_ids(ids) if wts is None else wts)


# Adam / FTRL cases of the GPU test (opt, F, rank, seed): test_fm_shared_ref.py checks on the CPU that the restatement alone
# marks at most 1 % of the touched elements ill for these seeds
OPT_CASES = [('adam', 5, 10, 1), ('ftrl', 5, 10, 2), ('adam', 3, 50, 3), ('ftrl', 3, 50, 4)]
OPT_LRS = {'adam': 1e-2, 'ftrl': 0.05}
OPT_B, OPT_PER, OPT_STEPS = 67, 12, 3


def opt_batches(F, seed):
    return [(basic_batch(OPT_B, F, OPT_PER, 100 * seed + i), labels(OPT_B, 100 * seed + 50 + i)) for i in range(OPT_STEPS)]


def touched(batches, shape):
    m = np.zeros(shape, bool)
    for b in batches:
        ids = b[0]
        m[ids[ids >= 0]] = True
    return m
