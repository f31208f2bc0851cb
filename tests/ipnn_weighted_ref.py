"""float64 reference of the inner-product family WITH value weights -- test infrastructure, built on oracle/ipnn_oracle.py without
editing it.  The one definition that changes is the embedding: e[t, f] = wts[t, f] * table[ids[t, f]] (python/FNN_IP_L7.py:103
for the numeric fields, the c_wts of embedding_lookup_sparse for the categorical ones).  Pairs, z1, the stack and the loss follow
from e as they did; dL/de comes out of the oracle's own backward (the pair partner it reads is the weighted e), and the gradient
of a table row is wts[t, f] * dL/de[t, f].

`weighted(wts)` swaps the oracle's z1_of and loss_and_grads for the weighted ones while a step runs, as oracle_pairs swaps
USE_PAIRS; the steps below are the oracle's own sgd_step / adam_step / ftrl_step / predict inside it.  The `g` a step returns holds
g['e'] = wts[..., None] * dL/de: what np.add.at scatters into the table's gradient."""
import contextlib

import numpy as np

from oracle import ipnn_oracle as io


@contextlib.contextmanager
def weighted(wts):
    wts = np.asarray(wts, dtype=np.float64)
    z1_of, lag = io.z1_of, io.loss_and_grads

    def z1_of_w(table, b, ids):
        assert wts.shape == ids.shape, (wts.shape, ids.shape)
        e = wts[..., None] * table[ids]
        B, F, K = e.shape
        p = (np.stack([(e[:, i] * e[:, j]).sum(axis=1) for (i, j) in io.pairs(F)], axis=1) if io.pairs(F) else np.zeros((B, 0)))
        return e, np.concatenate([e.reshape(B, F * K), p, np.full((B, 1), float(b))], axis=1)

    def loss_and_grads_w(*a, **kw):
        loss, logits, g = lag(*a, **kw)
        g['e'] = wts[..., None] * g['e']             # the table gradient: np.add.at(gt, ids, wts[..., None] * dL/de)
        return loss, logits, g
    io.z1_of, io.loss_and_grads = z1_of_w, loss_and_grads_w
    try:
        yield
    finally:
        io.z1_of, io.loss_and_grads = z1_of, lag


def loss_and_grads_w(params, table, ids, wts, y, act_name, masks=None, keep=1.0, reduce='sum'):
    with weighted(wts):
        return io.loss_and_grads(params, table, ids, y, act_name, masks, keep, reduce)


def sgd_step_w(params, table, ids, wts, y, act_name, lr, masks=None, keep=1.0, reduce='sum'):
    with weighted(wts):
        return io.sgd_step(params, table, ids, y, act_name, lr, masks, keep, reduce)


def adam_step_w(params, table, ids, wts, y, act_name, lr, st, masks=None, keep=1.0, **kw):
    with weighted(wts):
        return io.adam_step(params, table, ids, y, act_name, lr, st, masks, keep, **kw)


def ftrl_step_w(params, table, ids, wts, y, act_name, lr, st, masks=None, keep=1.0):
    with weighted(wts):
        return io.ftrl_step(params, table, ids, y, act_name, lr, st, masks, keep)


def predict_w(params, table, ids, wts, act_name):
    with weighted(wts):
        return io.predict(params, table, ids, act_name)


def test_weights(B, F, seed):
    """Uniform in [-0.5, 2), different per example and per field, float32-exact, with exact 0 and exact 1 among them (one of
    each per ten entries, and always in the first example)."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-0.5, 2.0, size=(B, F)).astype(np.float32)
    flat = w.reshape(-1)
    flat[rng.uniform(size=flat.size) < 0.1] = 0.0
    flat[rng.uniform(size=flat.size) < 0.1] = 1.0
    flat[0], flat[F - 1] = 0.0, 1.0
    return w


test_weights.__test__ = False
