"""Float64 restatement of FM / LR pre-training WITH per-field value weights (the reference's `sp_wt_hldr`: python/FM.py:24-29 and
:55-64, python/LR.py:23-27 and :53-55), for tests/test_fm_weighted_ref.py and tests/test_gpu_fm_weights.py.  Test infrastructure,
built beside oracle/fm_oracle.py and tests/fm_optim_ref.py without editing them.

The one definition that changes is the embedding: with x = wts[t, f], e_f = x_f * rows[ids[t, f]] (zero at an absent field,
whatever its weight), and

  yhat        = b + sum_f e_f[0] + 1/2 (sum_l (sum_f e_f[l])^2 - sum_f sum_l e_f[l]^2)            l = 1..rank
  d / d w_f   = x_f
  d / d v_f[l] = x_f (S_l - e_f[l]),   S_l = sum_f e_f[l]

(x v)^2 is the reference's v^2 x^2.  Loss, L2 term and optimisers are fm_optim_ref's."""
import numpy as np

import fm_optim_ref as ref


def embed(rows, ids, wts):
    """(e [B, F, K], x [B, F], live [B, F], safe ids): x is 0 at an absent field, so no weight there -- NaN included -- counts."""
    ids = np.asarray(ids)
    wts = np.asarray(wts, dtype=np.float64)
    assert wts.shape == ids.shape, (wts.shape, ids.shape)
    live = ids >= 0
    safe = np.where(live, ids, 0)
    x = np.where(live, wts, 0.0)
    e = np.where(live[..., None], x[..., None] * rows[safe], 0.0)
    return e, x, live, safe


def logits_w(rows, b, ids, wts):
    """rows [D, K] = concat(W, V); returns yhat [B]."""
    e = embed(rows, ids, wts)[0]
    lin, v = e[..., 0], e[..., 1:]
    S = v.sum(axis=1)
    return b + lin.sum(axis=1) + 0.5 * ((S * S).sum(axis=1) - (v * v).sum(axis=(1, 2)))


def predict_w(rows, b, ids, wts):
    return 1.0 / (1.0 + np.exp(-logits_w(rows, b, ids, wts)))


def dense_grad_w(rows, b, ids, wts, y, lam, reduce_mean):
    """fm_optim_ref.dense_grad with weights: (g_rows [D, K], g_b, data loss, p, |g| scale [D, K]).  The scale is the sum of the
    absolute values of every contribution to an element: what the Adam `ill` mask of fm_optim_ref.Trainer needs."""
    B = ids.shape[0]
    e, x, live, safe = embed(rows, ids, wts)
    z = logits_w(rows, b, ids, wts)
    p = 1.0 / (1.0 + np.exp(-z))
    xent = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    delta = (p - y) / (B if reduce_mean else 1.0)
    S = e[..., 1:].sum(axis=1)                                            # [B, rank]
    dx = delta[:, None] * x                                               # [B, F]
    contrib = np.empty(e.shape)
    contrib[..., 0] = dx
    contrib[..., 1:] = dx[..., None] * (S[:, None, :] - e[..., 1:])
    grad = np.zeros_like(rows)
    scale = np.abs(lam * rows)
    np.add.at(grad, safe[live], contrib[live])
    np.add.at(scale, safe[live], np.abs(contrib[live]))
    data = xent.mean() if reduce_mean else xent.sum()
    return grad + lam * rows, delta.sum() + lam * b, data, p, scale


def sgd_step_w(rows, b, ids, wts, y, lr, lam, reduce_mean=True):
    """One SGD step in place on rows, the L2 term dense over the whole table like oracle/fm_oracle.py's sgd_step; returns
    (new b, data loss, p before the update)."""
    g, gb, data, p, _ = dense_grad_w(rows, b, ids, wts, y, lam, reduce_mean)
    rows -= lr * g
    return b - lr * gb, data, p


class TrainerW(ref.Trainer):
    """fm_optim_ref.Trainer whose steps take the batch's weights."""

    def sgd_step(self, ids, y, wts):
        self.b, data, p = sgd_step_w(self.rows, self.b, ids, wts, y, self.lr, self.lam, self.mean)
        return data, p

    def step(self, ids, y, wts):
        g, gb, data, p, scale = dense_grad_w(self.rows, self.b, ids, wts, y, self.lam, self.mean)
        self.t += 1
        if self.opt == 'adam':
            lr_t = ref.adam_lr_t(self.lr, self.t)
            self.ill |= (np.abs(g) <= 1e-5 * scale) & (scale > 0)
            self.ill_b |= abs(gb) <= 1e-5 * (np.abs(p - y).sum() / (len(y) if self.mean else 1) + abs(self.lam * self.b))
            self.lr_sum += lr_t
            self.rows = ref.adam_update(self.rows, g, self.s0, self.s1, lr_t, self.eps)
            self.b = float(ref.adam_update(np.array(self.b), np.array(gb), self.sb0, self.sb1, lr_t, self.eps))
        else:
            self.rows = ref.ftrl_update(self.rows, g, self.s0, self.s1, self.lr)
            self.b = float(ref.ftrl_update(np.array(self.b), np.array(gb), self.sb0, self.sb1, self.lr))
        return data, p


def test_weights(B, F, seed):
    """Uniform in [-0.5, 2), different per example and per field, float32-exact, with about a tenth set to exact 0 and a tenth
    to exact 1 (and one of each in the first example when it has two fields)."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-0.5, 2.0, size=(B, F)).astype(np.float32)
    flat = w.reshape(-1)
    flat[rng.uniform(size=flat.size) < 0.1] = 0.0
    flat[rng.uniform(size=flat.size) < 0.1] = 1.0
    if F > 1:
        flat[0], flat[F - 1] = 0.0, 1.0
    return w


test_weights.__test__ = False
