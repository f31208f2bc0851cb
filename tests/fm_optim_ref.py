"""Float64 restatement of FM / LR pre-training under the reference's Adam and FTRL (python/FM.py, python/LR.py,
python/tf_util.py:15-29), for tests/test_fm_optim.py and tests/test_gpu_fm_optim.py.

  loss        xent (sum | mean) + lambda * (l2_loss(W) + l2_loss(V) + l2_loss(b)), l2_loss(t) = sum(t^2) / 2
  gradient    DENSE: every row gets lambda * theta plus the sum of its examples' gradients
  Adam        tf.train.AdamOptimizer(lr, epsilon=eps), beta1 0.9, beta2 0.999
  FTRL        tf.train.FtrlOptimizer(lr): power -0.5, initial accumulator 0.1, l1 = l2 = 0
The forward is oracle/fm_oracle.py's `logits`; rows [D, K] = concat(W, V), K = rank + 1 (rank 0: LR)."""
import numpy as np

from oracle import fm_oracle as fo

BETA1, BETA2 = 0.9, 0.999


def dense_grad(rows, b, ids, y, lam, reduce_mean):
    """(g_rows [D, K], g_b, data loss, p, |g| scale [D, K]): the gradient of the loss above.  The scale is the sum of the
    absolute values of every contribution to an element (what its f32 rounding error is proportional to)."""
    B = ids.shape[0]
    z = fo.logits(rows, b, ids)
    p = 1.0 / (1.0 + np.exp(-z))
    xent = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    delta = (p - y) / (B if reduce_mean else 1.0)
    live = ids >= 0
    safe = np.where(live, ids, 0)
    g = np.where(live[..., None], rows[safe], 0.0)                       # [B, F, K]
    S = g[..., 1:].sum(axis=1)                                            # [B, rank]
    contrib = np.empty(g.shape)
    contrib[..., 0] = delta[:, None]
    contrib[..., 1:] = delta[:, None, None] * (S[:, None, :] - g[..., 1:])
    grad = np.zeros_like(rows)
    scale = np.abs(lam * rows)
    np.add.at(grad, safe[live], contrib[live])
    np.add.at(scale, safe[live], np.abs(contrib[live]))
    data = xent.mean() if reduce_mean else xent.sum()
    return grad + lam * rows, delta.sum() + lam * b, data, p, scale


def adam_lr_t(lr, t):
    return lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)


def adam_update(w, g, m, v, lr_t, eps):
    """In place on m, v; returns the new w."""
    m *= BETA1
    m += (1.0 - BETA1) * g
    v *= BETA2
    v += (1.0 - BETA2) * g * g
    return w - lr_t * m / (np.sqrt(v) + eps)


def ftrl_update(w, g, accum, linear, lr):
    """In place on accum, linear; returns the new w.  sqrt(accum + g^2) - sqrt(accum) without the cancellation."""
    na = accum + g * g
    sa = np.sqrt(na)
    linear += g - g * g / (sa + np.sqrt(accum)) / lr * w
    accum[...] = na
    return np.where(linear != 0.0, -linear * lr / sa, 0.0)


def apply_ftrl_tf(var, accum, linear, grad, lr, l1=0.0, l2=0.0, lr_power=-0.5):
    """TensorFlow's ApplyFtrl (training_ops.cc) transcribed literally; returns (var, accum, linear), new arrays."""
    new_accum = accum + grad * grad
    linear = linear + grad - (new_accum ** (-lr_power) - accum ** (-lr_power)) / lr * var
    quadratic = 1.0 / (new_accum ** lr_power * lr) + 2.0 * l2
    var = np.where(np.abs(linear) > l1, (np.sign(linear) * l1 - linear) / quadratic, 0.0)
    return var, new_accum, linear


class Trainer(object):
    """The restatement's state: rows, b and the optimiser's state tensors; `step` applies one mini-batch."""

    def __init__(self, rows, b, opt, lr, lam, reduce_mean, eps=1e-8):
        self.rows, self.b = np.array(rows, np.float64), float(b)
        self.opt, self.lr, self.lam, self.mean, self.eps = opt, lr, lam, reduce_mean, eps
        self.reset_state()

    def reset_state(self):
        a0 = 0.1 if self.opt == 'ftrl' else 0.0
        self.s0, self.s1 = np.full_like(self.rows, a0), np.zeros_like(self.rows)
        self.sb0, self.sb1 = np.array(a0), np.array(0.0)
        self.t = 0
        self.ill = np.zeros(self.rows.shape, bool)      # Adam: elements whose gradient was within f32 noise of 0 at some step
        self.ill_b = False
        self.lr_sum = 0.0

    def sgd_step(self, ids, y):
        self.b, data, p = fo.sgd_step(self.rows, self.b, ids, y, self.lr, self.lam, self.mean)
        return data, p

    def step(self, ids, y):
        g, gb, data, p, scale = dense_grad(self.rows, self.b, ids, y, self.lam, self.mean)
        self.t += 1
        if self.opt == 'adam':
            lr_t = adam_lr_t(self.lr, self.t)
            self.ill |= (np.abs(g) <= 1e-5 * scale) & (scale > 0)
            self.ill_b |= abs(gb) <= 1e-5 * (np.abs(p - y).sum() / (len(y) if self.mean else 1) + abs(self.lam * self.b))
            self.lr_sum += lr_t
            self.rows = adam_update(self.rows, g, self.s0, self.s1, lr_t, self.eps)
            self.b = float(adam_update(np.array(self.b), np.array(gb), self.sb0, self.sb1, lr_t, self.eps))
        else:
            self.rows = ftrl_update(self.rows, g, self.s0, self.s1, self.lr)
            self.b = float(ftrl_update(np.array(self.b), np.array(gb), self.sb0, self.sb1, self.lr))
        return data, p
