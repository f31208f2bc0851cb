"""Reference of the device metrics (fnn::device_metrics behind fnn_eval, fm_eval / fm_eval_w, ipnn_eval / ipnn_eval_w) in plain
NumPy and Python, and the batteries of logits and labels that tests/test_metrics_ref.py (against sklearn, on the CPU) and
tests/test_gpu_metrics_edges.py (against the library) share.

metrics_ref(p32, y) works from float32 predictions as a device returned them; it never models how they were made.
  AUC       exact integers: with the negatives' float32 values sorted, S = sum over the positives of (negatives below) +
            (negatives below or equal), both by binary search, in int64; AUC = float(S) / (2.0 * n_pos * n_neg).  S < 2^53 at
            every size used here, so this is the correctly rounded quotient of the Mann-Whitney statistic with ties at 1/2 --
            what the library forms from its own integer sum -- and can be compared for equality.
  RMSE      sqrt(fsum((y - p)^2) / n) in float64, p64 = p32.astype(float64).
  logloss   -fsum(log(pc) | log(1 - pc)) / n with pc = clip(p64, 2^-52, 1 - 2^-52): sklearn.metrics.log_loss on float64 input.
Positives are y != 0.  ValueError for a single class or any non-finite p, as roc_auc_score / log_loss raise."""
import math

import numpy as np

EPS = 2.0 ** -52


def metrics_ref(p32, y):
    """(auc, rmse, logloss, n_pos) of float32 predictions p32 [n] against labels y [n] (0 / non-zero)."""
    p32, y = np.asarray(p32), np.asarray(y)
    if p32.dtype != np.float32 or p32.ndim != 1 or y.shape != p32.shape:
        raise TypeError("metrics_ref: p32 must be a float32 vector and y its shape")
    if not np.isfinite(p32).all():
        raise ValueError("metrics_ref: %d non-finite predictions" % int((~np.isfinite(p32)).sum()))
    pos = y != 0
    n, n_pos = len(p32), int(pos.sum())
    n_neg = n - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("metrics_ref: only one class present in y")
    neg = np.sort(p32[~pos])
    S = int(np.searchsorted(neg, p32[pos], side='left').astype(np.int64).sum()) + \
        int(np.searchsorted(neg, p32[pos], side='right').astype(np.int64).sum())
    assert S < 2 ** 53
    auc = float(S) / (2.0 * n_pos * n_neg)
    p64 = p32.astype(np.float64)
    rmse = math.sqrt(math.fsum((pos.astype(np.float64) - p64) ** 2) / n)
    pc = np.clip(p64, EPS, 1.0 - EPS)
    logloss = -math.fsum(np.where(pos, np.log(pc), np.log(1.0 - pc))) / n
    return auc, rmse, logloss, n_pos


def sigmoid32(z):
    """1 / (1 + exp(-z)) in NumPy float32: the stand-in for a device's predictions in the CPU test (NaN stays NaN)."""
    z = np.asarray(z, np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-z))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ batteries
# A battery is (z float32 [N], y int32 [N]).  Each pins one y = 1 and one y = 0 example, so both classes are present whatever the
# draw.  precondition(name, p, y) asserts on the PREDICTIONS what the battery is there for, so that a change of the forward (or of
# the stand-in sigmoid) cannot silently turn the case into an easy one.
SAT_Z = (-200.0, -104.0, -90.0, -88.0, -30.0, -17.0, -16.6, -1.0, 0.0, 0.0, 0.5, 1.0, 16.6, 17.0, 30.0, 200.0, np.inf, -np.inf)
LABEL_VALUES = (1, 2, -1, 2 ** 31 - 1, -2 ** 31)
NAN_AT = 17                                              # the example of `saturated` that `saturated-nan` makes NaN
GRID = 2048 * 256                                        # k_metric_auc: at most 2048 blocks of 256 threads, a positive each
N_GRID = 1200000


def _continuous(rng, n):
    return (rng.standard_normal(n) * 2.0).astype(np.float32)


def _bernoulli(rng, n, q):
    y = (rng.uniform(size=n) < q).astype(np.int32)
    y[0], y[1] = 1, 0
    return y


def _saturated(n=9001, seed=11):
    """z from SAT_Z (p exactly 0.0 from about z <= -88.7 or -104 on, exactly 1.0 from about z >= 17 on, in float32), labels
    Bernoulli(0.47) independent of z: every saturated value meets both labels."""
    rng = np.random.RandomState(seed)
    z = np.asarray(SAT_Z, np.float32)[rng.randint(0, len(SAT_Z), size=n)]
    return z, _bernoulli(rng, n, 0.47)


def _saturated_nan():
    z, y = _saturated()
    z[NAN_AT] = np.nan
    return z, y


def _all_equal(n=4097):
    y = _bernoulli(np.random.RandomState(12), n, 0.3)
    return np.zeros(n, np.float32), y


def _three_values(n=100000):
    rng = np.random.RandomState(13)
    z = np.asarray((-1.0, 0.0, 2.0), np.float32)[rng.randint(0, 3, size=n)]
    return z, _bernoulli(rng, n, 0.3)


def _separated(swap, n=5000):
    y = _bernoulli(np.random.RandomState(14), n, 0.3)
    z = np.where((y != 0) != swap, 3.0, -3.0).astype(np.float32)
    return z, y


def _one_below_one_above(n=5000):
    """Negatives and most positives continuous in (-6, 6) or so; positive 0 below every negative (lb = ub = 0), positive 2 above
    every negative (lb = ub = n_neg)."""
    rng = np.random.RandomState(15)
    z, y = _continuous(rng, n), _bernoulli(rng, n, 0.3)
    y[2] = 1
    z[0], z[2] = -12.0, 12.0
    return z, y


def _size(n):
    rng = np.random.RandomState(100 + n)
    z, y = _continuous(rng, n), _bernoulli(rng, n, 0.3)
    return z, y


def _last_block(n=2049):
    """Every positive in examples 2048..: the ragged last block of k_metric_keys (2048 examples a block) holds them all."""
    z = _continuous(np.random.RandomState(16), n)
    y = np.zeros(n, np.int32)
    y[2048:] = 1
    return z, y


def _counted(n, n_pos, seed, sat=0.0):
    """n_pos positives exactly, placed by a seeded permutation; continuous z with a fraction `sat` of it saturated."""
    rng = np.random.RandomState(seed)
    z = _continuous(rng, n)
    if sat:
        hit = rng.uniform(size=n) < sat
        z[hit] = np.asarray((-200.0, -30.0, 30.0, 200.0), np.float32)[rng.randint(0, 4, size=n)][hit]
    y = np.zeros(n, np.int32)
    y[rng.permutation(n)[:n_pos]] = 1
    return z, y


BATTERIES = {
    'saturated': _saturated,
    'all-equal': _all_equal,
    'three-values': _three_values,
    'separated': lambda: _separated(False),
    'separated-swapped': lambda: _separated(True),
    'one-below-one-above': _one_below_one_above,
    'N2': lambda: (np.asarray((0.3, -0.4), np.float32), np.asarray((1, 0), np.int32)),
    'N2047': lambda: _size(2047),
    'N2048': lambda: _size(2048),
    'N2049': lambda: _size(2049),
    'N4097': lambda: _size(4097),
    'N8193': lambda: _size(8193),
    'N2049-positives-in-last-block': _last_block,
    'N5000-npos1': lambda: _counted(5000, 1, 17),
    'N5000-nneg1': lambda: _counted(5000, 4999, 18),
    'grid-npos524288': lambda: _counted(N_GRID, GRID, 19, 0.01),
    'grid-npos524289': lambda: _counted(N_GRID, GRID + 1, 20, 0.01),
    'grid-npos1199999': lambda: _counted(N_GRID, N_GRID - 1, 21, 0.01),
    'grid-npos1': lambda: _counted(N_GRID, 1, 22, 0.01),
}
NONFINITE = {'saturated-nan': _saturated_nan}
EXACT_AUC = {'all-equal': 0.5, 'separated': 1.0, 'separated-swapped': 0.0}

_cache = {}


def battery(name):
    """(z, y) of a battery, built once per process and read-only."""
    if name not in _cache:
        z, y = (BATTERIES.get(name) or NONFINITE[name])()
        z, y = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(y, np.int32)
        z.setflags(write=False)
        y.setflags(write=False)
        _cache[name] = (z, y)
    return _cache[name]


def relabelled(y, seed=23):
    """y with its positives given values from LABEL_VALUES (every one of them used), the zeros kept."""
    rng = np.random.RandomState(seed)
    vals = np.asarray(LABEL_VALUES, np.int64)[rng.randint(0, len(LABEL_VALUES), size=len(y))]
    where = np.flatnonzero(y != 0)
    vals[where[:len(LABEL_VALUES)]] = LABEL_VALUES
    return np.where(y != 0, vals, 0).astype(np.int32)


def precondition(name, p, y):
    """What battery `name` is there for, asserted on predictions p (float32) of its logits."""
    z, y0 = battery(name)
    assert p.dtype == np.float32 and p.shape == z.shape and np.array_equal(y != 0, y0 != 0)
    pos = y != 0
    n_pos = int(pos.sum())
    assert 0 < n_pos < len(y)
    if name in NONFINITE:
        assert np.isnan(p[NAN_AT]) and np.isfinite(np.delete(p, NAN_AT)).all()
        return
    assert np.isfinite(p).all() and p.min() >= 0.0 and p.max() <= 1.0
    if name == 'saturated':
        for cls in (pos, ~pos):                              # exact 0.0 and exact 1.0 under both labels, and the middle
            assert (p[cls] == 0.0).sum() >= 100 and (p[cls] == 1.0).sum() >= 100 and ((p[cls] > 0.25) & (p[cls] < 0.75)).any()
        assert ((p > 0.0) & (p < 1e-6)).any() and ((p < 1.0) & (p > 1.0 - 1e-6)).any()     # just inside the clip too
    elif name == 'all-equal':
        assert (p == p[0]).all()
    elif name == 'three-values':
        assert len(np.unique(p)) == 3 and all(len(np.unique(p[c])) == 3 for c in (pos, ~pos))
    elif name == 'separated':
        assert p[pos].min() > p[~pos].max() and len(np.unique(p)) == 2
    elif name == 'separated-swapped':
        assert p[pos].max() < p[~pos].min() and len(np.unique(p)) == 2
    elif name == 'one-below-one-above':
        assert p[0] < p[~pos].min() and p[2] > p[~pos].max() and n_pos > 1000
    elif name == 'N2049-positives-in-last-block':
        assert len(p) == 2049 and not pos[:2048].any() and pos[2048:].all()
    elif name.startswith('N5000'):
        assert len(p) == 5000 and n_pos == (1 if name.endswith('npos1') else 4999)
    elif name.startswith('grid'):
        assert len(p) == N_GRID and n_pos == int(name[len('grid-npos'):])
        assert (p == 0.0).sum() > 1000 and (p == 1.0).sum() > 1000                         # about 0.25 % each
    else:
        assert len(p) == int(name[1:]) and len(np.unique(p)) > 0.9 * len(p)
