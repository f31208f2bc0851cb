"""tests/metrics_ref.py against sklearn (roc_auc_score, sqrt(mean_squared_error), log_loss(labels=[0, 1])) on the batteries that
tests/test_gpu_metrics_edges.py feeds the library, with a NumPy float32 sigmoid in the device's place.  1e-12 relative: both
sides are float64 sums of the same terms (sklearn's pairwise, the reference's exact fsum), n 2^-53 apart at the worst."""
import numpy as np
import pytest

import metrics_ref as mr

REL = 1e-12


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("name", list(mr.BATTERIES))
def test_metrics_ref_equals_sklearn(name):
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    z, y = mr.battery(name)
    p = mr.sigmoid32(z)
    mr.precondition(name, p, y)
    auc, rmse, ll, n_pos = mr.metrics_ref(p, y)
    p64 = p.astype(np.float64)
    want = (roc_auc_score(y, p64), float(np.sqrt(mean_squared_error(y, p64))), log_loss(y, p64, labels=[0, 1]))
    devs = [rel(g, w) for g, w in zip((auc, rmse, ll), want)]
    print("[metrics-ref] %s: N %d n_pos %d auc %.17g rmse %.17g logloss %.17g; relative deviation from sklearn %.1e %.1e %.1e"
          % ((name, len(y), n_pos, auc, rmse, ll) + tuple(devs)))
    assert n_pos == int((y != 0).sum())
    assert max(devs) <= REL, (devs, (auc, rmse, ll), want)
    if name in mr.EXACT_AUC:
        assert auc == mr.EXACT_AUC[name]


def test_metrics_ref_labels_are_zero_or_not():
    z, y = mr.battery('saturated')
    p = mr.sigmoid32(z)
    y2 = mr.relabelled(y)
    assert set(mr.LABEL_VALUES) <= set(y2.tolist()) and np.array_equal(y2 != 0, y != 0)
    assert mr.metrics_ref(p, y2) == mr.metrics_ref(p, y)


def test_metrics_ref_saturated_penalty():
    """A prediction of exactly 0.0 under y = 1 (or 1.0 under y = 0) costs -log(2^-52) = 36.04 and nothing else does."""
    p = np.asarray([0.0, 1.0, 0.5, 0.5], np.float32)
    _, _, ll, _ = mr.metrics_ref(p, np.asarray([1, 0, 1, 0]))
    assert abs(ll - (2 * 52 * np.log(2.0) + 2 * np.log(2.0)) / 4) <= 1e-14
    _, _, ll, _ = mr.metrics_ref(p, np.asarray([0, 1, 1, 0]))
    assert abs(ll - (2 * -np.log1p(-2.0 ** -52) + 2 * np.log(2.0)) / 4) <= 1e-15


def test_metrics_ref_raises_as_sklearn_does():
    from sklearn.metrics import log_loss, roc_auc_score
    z, y = mr.battery('saturated-nan')
    p = mr.sigmoid32(z)
    mr.precondition('saturated-nan', p, y)
    for fn in (lambda: mr.metrics_ref(p, y), lambda: roc_auc_score(y, p.astype(np.float64)),
               lambda: log_loss(y, p.astype(np.float64), labels=[0, 1])):
        with pytest.raises(ValueError):
            fn()
    good = mr.sigmoid32(mr.battery('saturated')[0])
    for bad in (np.float32(np.inf), np.float32(-np.inf)):
        q = good.copy()
        q[5] = bad
        with pytest.raises(ValueError):
            mr.metrics_ref(q, y)
    for one in (np.zeros_like(y), np.full_like(y, 3)):
        with pytest.raises(ValueError):
            mr.metrics_ref(good, one)            # (sklearn raised here up to 1.6; newer ones warn and return NaN)
