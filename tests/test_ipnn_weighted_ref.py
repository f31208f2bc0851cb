"""The weighted float64 reference (tests/ipnn_weighted_ref.py) against the oracle it extends and against torch autograd, and the
two NumPy feeds (ipnn.criteo_feed, synth.criteo_like).  No GPU."""
import copy

import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.ipnn import criteo_feed

import ipnn_weighted_ref as wr


def _problem(F, K, B, hidden, pairs, seed):
    rng = np.random.RandomState(seed)
    n_rows = 40
    table = rng.standard_normal((n_rows, K)) * 0.3
    ids = rng.randint(0, n_rows, size=(B, F))
    ids[1] = ids[0]                                   # duplicates: the row gradient is a sum
    y = (rng.uniform(size=B) < 0.4).astype(np.float64)
    d = [F * K + (F * (F - 1) // 2 if pairs else 0) + 1] + hidden + [1]
    params = {'b': 0.1, 'W': [rng.uniform(-0.4, 0.4, (d[i], d[i + 1])) for i in range(len(d) - 1)],
              'bias': [rng.uniform(-0.1, 0.1, d[i + 1]) for i in range(len(d) - 1)]}
    masks = [(rng.uniform(size=(B, d[t])) < 0.7).astype(np.float64) for t in range(len(hidden) + 1)]
    return table, ids, y, params, masks


def _same(a, b):
    assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("opt", ['sgd', 'adam', 'ftrl'])
def test_unit_weights_equal_the_oracle_bit_for_bit(opt, pairs):
    """wts all ones: loss, logits, every W, bias, b and the whole table after two steps are the oracle's own, bit for bit."""
    table, ids, y, params, masks = _problem(5, 3, 9, [7, 4], pairs, 3)
    ones = np.ones(ids.shape)
    io.USE_PAIRS = bool(pairs)
    try:
        pa, ta, pb, tb = copy.deepcopy(params), table.copy(), copy.deepcopy(params), table.copy()
        sa = {'sgd': None, 'adam': io.adam_state(pa, ta), 'ftrl': io.ftrl_state(pa, ta)}[opt]
        sb = copy.deepcopy(sa)
        for _ in range(2):
            if opt == 'sgd':
                ra = io.sgd_step(pa, ta, ids, y, 'tanh', 0.05, masks, 0.7)
                rb = wr.sgd_step_w(pb, tb, ids, ones, y, 'tanh', 0.05, masks, 0.7)
            elif opt == 'adam':
                ra = io.adam_step(pa, ta, ids, y, 'tanh', 0.01, sa, masks, 0.7)
                rb = wr.adam_step_w(pb, tb, ids, ones, y, 'tanh', 0.01, sb, masks, 0.7)
            else:
                ra = io.ftrl_step(pa, ta, ids, y, 'tanh', 0.05, sa, masks, 0.7)
                rb = wr.ftrl_step_w(pb, tb, ids, ones, y, 'tanh', 0.05, sb, masks, 0.7)
            assert ra[0] == rb[0]
            _same(ra[1], rb[1])
            _same(ra[2]['e'], rb[2]['e'])
        _same(ta, tb)
        assert pa['b'] == pb['b']
        for t in range(len(pa['W'])):
            _same(pa['W'][t], pb['W'][t])
            _same(pa['bias'][t], pb['bias'][t])
        _same(io.predict(pa, ta, ids, 'tanh'), wr.predict_w(pb, tb, ids, ones, 'tanh'))
        assert io.z1_of.__name__ == 'z1_of' and io.loss_and_grads.__name__ == 'loss_and_grads'       # restored
    finally:
        io.USE_PAIRS = True


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("act", ['tanh', 'sigmoid'])
def test_weighted_gradients_equal_torch_autograd(act, pairs):
    """F = 3, K = 2, B = 5, weights with a 0 and a negative among them: every gradient of the weighted reference equals torch's
    float64 autograd of the same forward (e = wts * table[ids]) to 1e-10 relative."""
    torch = pytest.importorskip("torch")
    F, K, B, hidden = 3, 2, 5, [4, 3]
    table, ids, y, params, masks = _problem(F, K, B, hidden, pairs, 11)
    wts = np.random.RandomState(12).uniform(-0.5, 2.0, size=(B, F))
    wts[0, 0], wts[2, 1], wts[3, 2] = 0.0, -0.75, 1.0
    io.USE_PAIRS = bool(pairs)
    try:
        loss, logits, g = wr.loss_and_grads_w(params, table, ids, wts, y, act, masks, 0.7)
        pr = io.pairs(F)
    finally:
        io.USE_PAIRS = True
    gt = np.zeros_like(table)
    np.add.at(gt, ids, g['e'])

    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)       # noqa: E731
    tt, tb = T(table), T(params['b'])
    tW, tbias = [T(w) for w in params['W']], [T(b) for b in params['bias']]
    e = torch.tensor(wts)[..., None] * tt[torch.tensor(ids, dtype=torch.long)]
    cols = [e.reshape(B, F * K)] + ([torch.stack([(e[:, i] * e[:, j]).sum(dim=1) for (i, j) in pr], dim=1)] if pr else []) + \
           [tb.expand(B, 1)]
    l = torch.cat(cols, dim=1)
    fa = torch.tanh if act == 'tanh' else torch.sigmoid
    for t in range(len(tW)):
        l = (fa(l) * torch.tensor(masks[t]) / 0.7) @ tW[t] + tbias[t]
    lg = l[:, 0]
    tl = torch.nn.functional.binary_cross_entropy_with_logits(lg, torch.tensor(y), reduction='sum')
    tl.backward()

    def close(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), np.abs(a - b).max()
    close(loss, tl.item())
    close(logits, lg.detach().numpy())
    close(gt, tt.grad.numpy())
    close(g['b'], tb.grad.item())
    for t in range(len(tW)):
        close(g['W'][t], tW[t].grad.numpy())
        close(g['bias'][t], tbias[t].grad.numpy())
    assert np.abs(tt.grad.numpy()).max() > 0


def test_criteo_feed_round_trips_the_drivers_split():
    """python/baseline.py:347-349 feeds _vals[:, :13], _cols[:, 13:] - offsets and _vals[:, 13:]: criteo_feed puts them back."""
    rng = np.random.RandomState(2)
    B, n_v, sizes = 7, 13, [3, 10, 1, 50] + [4] * 22
    offsets = n_v + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    cols = np.concatenate([np.tile(np.arange(n_v), (B, 1)), np.stack([o + rng.randint(0, s, B) for o, s in zip(offsets, sizes)], axis=1)], axis=1)
    vals = rng.uniform(0, 3, size=(B, n_v + len(sizes))).astype(np.float32)
    ids, wts = criteo_feed(vals[:, :n_v], cols[:, n_v:] - offsets, vals[:, n_v:], offsets)
    assert ids.dtype == np.int32 and wts.dtype == np.float32 and ids.shape == wts.shape == (B, 39)
    assert np.array_equal(ids, cols) and np.array_equal(wts, vals)
    assert np.array_equal(ids[:, 13:] - offsets, cols[:, n_v:] - offsets) and np.array_equal(ids[:, :13], np.tile(np.arange(13), (B, 1)))
    with pytest.raises(ValueError):
        criteo_feed(vals[:, :n_v], cols[:, n_v:], vals[:, n_v + 1:], offsets)


def test_criteo_like_layout():
    B, n_v, sizes = 4000, 13, synth.field_sizes_tiny(1000, 26)
    ids, wts = synth.criteo_like(B, n_v, sizes, seed=4)
    assert ids.shape == wts.shape == (B, 39) and ids.dtype == np.int32 and wts.dtype == np.float32
    assert np.array_equal(ids[:, :n_v], np.tile(np.arange(n_v), (B, 1)))                    # numeric fields: one constant row each
    v = wts[:, :n_v]
    assert v.min() == 0.0 and v.max() < 2.0 and 0.03 < (v == 0).mean() < 0.07
    assert (wts[:, n_v:] == 1.0).all()
    off = n_v + np.concatenate([[0], np.cumsum(sizes)])
    for j in range(26):
        c = ids[:, n_v + j]
        assert c.min() >= off[j] and c.max() < off[j + 1]
    assert len(np.unique(ids[:, n_v + 3])) < B                                              # zipf: duplicates
    a, b = synth.criteo_like(B, n_v, sizes, seed=4)
    assert np.array_equal(a, ids) and np.array_equal(b, wts)
