"""CPU checks of FM / LR pre-training under Adam and FTRL: the float64 restatement in fm_optim_ref.py against torch
autograd and against TensorFlow's ApplyFtrl formula, and the argument parsing of deep-ctr_amd/FM.py and LR.py."""
import numpy as np
import pytest
import torch

import fm_optim_ref as ref

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import parse_ptmzr, FM
from deep_ctr_amd.LR import LR


def _problem(B, rank, seed):
    rng = np.random.RandomState(seed)
    sizes = synth.field_sizes_tiny(300)
    rows = rng.standard_normal((sum(sizes), rank + 1)) * 0.3
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 1)
    ids[0, 3] = -1
    ids[1, :] = -1
    ids[2, 15] = sum(sizes) - 1                     # the last row
    y = (rng.uniform(size=B) < 0.4).astype(np.float64)
    return rows, 0.3, ids, y


@pytest.mark.parametrize("rank", [0, 1, 10])
@pytest.mark.parametrize("reduce_mean", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 1e-3, 0.05])
def test_dense_grad_equals_autograd(rank, reduce_mean, lam):
    rows, b, ids, y = _problem(97, rank, seed=rank * 7 + reduce_mean)
    g, gb, data, p, _ = ref.dense_grad(rows, b, ids, y, lam, reduce_mean)
    R = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    live = torch.tensor(ids >= 0)
    e = R[torch.tensor(np.where(ids >= 0, ids, 0))] * live[..., None]
    w, v = e[..., 0], e[..., 1:]
    S = v.sum(1)
    z = bt + w.sum(1) + 0.5 * ((S * S).sum(1) - (v * v).sum((1, 2)))
    xent = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor(y), reduction='mean' if reduce_mean else 'sum')
    loss = xent + lam * ((R * R).sum() / 2 + bt * bt / 2)
    loss.backward()
    np.testing.assert_allclose(g, R.grad.numpy(), rtol=1e-10, atol=1e-13)
    assert abs(gb - bt.grad.item()) <= 1e-10 * max(1.0, abs(gb))
    assert abs(data - xent.item()) <= 1e-10 * max(1.0, abs(data))


def test_ftrl_step_equals_tensorflow_apply_ftrl():
    rng = np.random.RandomState(3)
    for lr in (1e-3, 0.05, 1.0):
        w = rng.standard_normal(4000) * 0.2
        accum = 0.1 + rng.exponential(0.5, 4000)
        linear = rng.standard_normal(4000) * 0.1
        g = rng.standard_normal(4000) * np.where(rng.uniform(size=4000) < 0.2, 0.0, 1.0)
        a, l = accum.copy(), linear.copy()
        got = ref.ftrl_update(w, g, a, l, lr)
        tw, ta, tl = ref.apply_ftrl_tf(w, accum, linear, g, lr)
        np.testing.assert_allclose(got, tw, rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(a, ta, rtol=1e-14)
        np.testing.assert_allclose(l, tl, rtol=1e-9, atol=1e-14)


def test_ftrl_zero_gradient_rederives_the_variable():
    """A zero gradient at the first step from the initial state (accum 0.1, linear 0) gives w = 0, whatever w was."""
    w = np.array([0.5, -0.2, 0.0])
    a, l = np.full(3, 0.1), np.zeros(3)
    assert not ref.ftrl_update(w, np.zeros(3), a, l, 0.01).any()


@pytest.mark.parametrize("argv,expect", [
    (['sgd', 0.05], (0, 0.05, 1e-8, 1)),
    (['sgd', 0.05, 'sum'], (0, 0.05, 1e-8, 0)),
    (['adam', 1e-4, 1e-8, 'sum'], (1, 1e-4, 1e-8, 0)),          # python/baseline.py's FM recipe
    (['adam', 1e-3, 1e-6], (1, 1e-3, 1e-6, 1)),
    (['ftrl', 1e-3], (2, 1e-3, 1e-8, 1)),                        # python/baseline.py's LR recipe
    (['ftrl', 1e-3, 'sum'], (2, 1e-3, 1e-8, 0)),
    (['ftrl', 1e-3, 'sum', 'mean'], (2, 1e-3, 1e-8, 1)),          # 'sum' counts only as the last element
])
def test_parse_ptmzr(argv, expect):
    assert parse_ptmzr(argv) == expect


def test_parse_ptmzr_refuses():
    with pytest.raises(NotImplementedError):
        parse_ptmzr(['rmsprop', 1e-3])
    with pytest.raises(ValueError):
        parse_ptmzr(['adam', 1e-3])


def test_fm_and_lr_parse_before_the_device(monkeypatch):
    """The optimiser arguments are checked before any device is touched: an unknown name raises NotImplementedError even
    where no GPU is visible."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    init = ['uniform', -0.01, 0.01, [1, 2], None]
    with pytest.raises(NotImplementedError):
        FM(8, [100, 16, 4], init, ['rmsprop', 0.1], [0.0])
    with pytest.raises(NotImplementedError):
        LR(8, [100, 16], init, ['momentum', 0.1], [0.0])
    from deep_ctr_amd.engine import FNNError
    for cls, rch in ((FM, [100, 16, 4]), (LR, [100, 16])):
        for argv in (['adam', 1e-4, 1e-8, 'sum'], ['ftrl', 1e-3]):
            with pytest.raises(FNNError):                         # parsed, then refused for want of a device
                cls(8, rch, init, argv, [1e-3])
