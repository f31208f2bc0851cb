"""Float64 NumPy restatement of the mini-batch step of the reference's dA.get_cost_updates
(python/sampling_based_denosing_autoencoder.py:97-113) as da() drives it (:116-232): batch_size = M, cost = T.mean(L), a short last
batch with its own mean, a keep mask on the encoder's input only.  tests/test_dae_batch_ref.py holds it to pretrain_ref.run_dense_da
at M = 1, to torch.autograd and to the input regime of the GPU cases (DAE_BATCH_CASES below, shared with tests/test_gpu_dae_batch.py)."""
import numpy as np

# the GPU parity cases: (row, col, M, N, masked, f64, skip_last).  Every shape, every (M, N) and both keep forms at least once per
# precision, both skip_last values; the thinning keeps the large shapes on short runs.
SHAPES = [(1, 1), (1, 8), (129, 65), (209, 100), (304, 7), (305, 1), (300, 100), (512, 512)]
BATCHES = [(1, 40), (2, 41), (20, 70), (20, 7), (64, 200), (256, 600)]


def _cases():
    out = []
    for f64 in (True, False):
        for si, (row, col) in enumerate(SHAPES):                  # every shape, the (M, N) pairs dealt round
            for t in range(2):
                bi = (2 * si + t + (0 if f64 else 3)) % len(BATCHES)
                if (row, col) == (512, 512) and BATCHES[bi][1] > 200:
                    bi = 2
                M, N = BATCHES[bi]
                out.append((row, col, M, N, (si + t + f64) % 2 == 1, f64, (si + t) % 2))
        for bi, (M, N) in enumerate(BATCHES):                     # every (M, N) at the reference's shape, both keep forms over the list
            c = (300, 100, M, N, bi % 2 == 0, f64, bi % 2)
            if c not in out:
                out.append(c)
    return out


DAE_BATCH_CASES = _cases()


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def keep_mask(N, row, seed):
    """A 0.7-density uint8 keep mask with one example fully corrupted (row 3, where N > 3)."""
    k = (np.random.RandomState(seed).uniform(size=(N, row)) < 0.7).astype(np.uint8)
    if N > 3:
        k[3] = 0
    return k


def batch_grads(W, bh, bv, X, keep):
    """One mini-batch: (cost, gW, gbhid, gbvis, Z)."""
    m = X.shape[0]
    Xt = X if keep is None else X * (keep != 0)
    Y = sigmoid(Xt @ W + bh)
    Z = sigmoid(Y @ W.T + bv)
    L = -np.sum(X * np.log(Z) + (1 - X) * np.log(1 - Z), axis=1)          # against the UNcorrupted X
    D = (Z - X) / m
    dY = (D @ W) * Y * (1 - Y)
    return L.mean(), Xt.T @ dY + D.T @ Y, dY.sum(axis=0), D.sum(axis=0), Z


def run_dense_da_batch(W, bh, bv, X, keep, M, lr, skip_last, z_range=None):
    """One pass over X [N, row] in mini-batches of M (a last batch of N % M with its own mean).  skip_last: the last mini-batch
    only contributes its cost.  Returns (W, bhid, bvis, cost sum over the mini-batches).  z_range (a two-element list, optional)
    receives the smallest and largest reconstruction met."""
    N = X.shape[0]
    cost = 0.0
    for n0 in range(0, N, M):
        k = None if keep is None else keep[n0:n0 + M]
        c, gW, gbh, gbv, Z = batch_grads(W, bh, bv, X[n0:n0 + M], k)
        cost += c
        if z_range is not None:
            z_range[0], z_range[1] = min(z_range[0], Z.min()), max(z_range[1], Z.max())
        if skip_last and n0 + M >= N:
            break
        W, bh, bv = W - lr * gW, bh - lr * gbh, bv - lr * gbv
    return W, bh, bv, cost
