"""Helpers of the RBM / DAE pre-training shape tests (test_pretrain_ref.py on the CPU, test_gpu_rbm_shapes.py and
test_gpu_dae_shapes.py on the GPU) -- TEST INFRASTRUCTURE, no GPU code.

  * the case tables (shapes, seeds, weight costs) and their input sets, so that the CPU tests vouch for exactly the inputs the
    GPU tests run;
  * walks of the float64 oracles (oracle/rbm_oracle.py, oracle/dae_oracle.py) over those inputs;
  * safe_uniforms: the kernels decide `u < hid` in f32 (bf16), the oracle in f64 -- a draw closer to `hid` than the kernel's
    rounding can flip ONE decision and move W by 3e-3 of the whole change.  The draws within `margin` of the oracle's hid are
    moved to hid +- margin on the side they were on: every decision, and with it the trajectory, stays what it was;
  * plain float64 references of the helper kernels with their rounding bounds.
"""
import numpy as np

from oracle import dae_oracle as do
from oracle import rbm_oracle as ro

U32 = 2.0 ** -24                       # unit round-off of f32
RATES = (1e-2, 1e-2, 1e-2)             # 100x the reference's, as test_sparse_minibatch_edge_shapes: updates stand clear of f32 round-off
MOMENTUM = 0.9
TOL = 2e-3                             # the project's bound: error / size of the parameter change
TOL_ERR = 1e-4                         # relative, the summed squared error / cost
MARGIN_F32, MARGIN_BF16 = 1e-3, 2e-2

# ---- case tables: (H, S, N, weightcost); n_rows = 3 * S so that consecutive examples share rows
ONLINE_GENERIC = [(1, 1, 40, 0.05), (7, 5, 120, 0.05), (64, 31, 100, 2e-4), (65, 16, 80, 0.05), (256, 1, 40, 2e-4)]      # k_rbm_sparse
ONLINE_S32 = [(255, 32, 60, 0.05), (256, 32, 60, 0.05), (1, 32, 40, 2e-4)]                                          # k_rbm_sparse32
# (H, S, M, N, weightcost)
BATCH_ATOMIC = [(1, 1, 4, 10, 0.05), (6, 5, 16, 50, 2e-4), (37, 32, 64, 150, 0.05), (255, 32, 20, 60, 2e-4)]
BATCH_MULTI = [(8, 4, 600, 1300, 0.05), (16, 32, 520, 520, 2e-4), (6, 3, 600, 700, 0.05)]      # > 512 examples: several per workgroup
BATCH_LONG_RUNS = (8, 4, 300, 300, 0.05)       # n_rows == S: every row one run of 300 entries
BATCH_REGROUP = (8, 5, 3, 52, 2e-4)            # 18 mini-batches: past the 16 grouped ahead, the last of one example
BATCH_M1 = (8, 5, 1, 60, 0.05)                 # M = 1: the online schedule
# (nvis, nhid, max_n, n of the three steps, weightcost)
DENSE_F32 = [(63, 63, 1, (1, 1, 1), 0.05), (64, 64, 257, (256, 257, 256), 2e-4), (127, 1, 100, (100, 100, 100), 0.05),
             (1, 127, 7, (7, 7, 7), 2e-4), (191, 65, 300, (300, 10, 300), 0.05)]
DENSE_BF16 = [(64, 64, 200, (200, 200, 200), 0.05), (100, 40, 150, (150, 150, 150), 2e-4)]


def r32(a):
    """Round to f32, keep as float64: what the device holds."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16(a):
    """Round-to-nearest-even to bfloat16, kept as float64 (the conversion of the kernels' (bf16_t) casts)."""
    b = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(a))


class Replay(object):
    """Stands in for the oracle's rng: uniform(size=...) hands out the prepared blocks one after another."""

    def __init__(self, blocks):
        self.blocks, self.i = blocks, 0

    def uniform(self, size=None):
        self.i += 1
        return np.asarray(self.blocks[self.i - 1], dtype=np.float64).reshape(size)


def nudge(u, hid, margin):
    """Draws within `margin` of hid -> hid +- margin on the side they were on (rounded to f32, a hair outside the margin).
    Returns (draws, number moved)."""
    u, hid = np.array(u, dtype=np.float64), np.asarray(hid, dtype=np.float64).reshape(np.shape(u))
    near = np.abs(u - hid) < margin
    side = np.where(u < hid, -1.0, 1.0)
    out = r32(hid + side * margin * (1.0 + 2.0 ** -10))        # 2^-10 margin > the f32 rounding of a number below 2
    u[near] = out[near]
    assert not (np.abs(u - hid) < margin).any() and np.array_equal(u < hid, side < 0)
    return u, int(near.sum())


# ------------------------------------------------------------------------------------------ sparse CD-1
def sparse_case(H, S, N, weightcost, M=None, n_rows=None):
    """The input set of one sparse case: S distinct sorted ids out of few rows per example, 0/1 values, parameters and a NON-ZERO
    positional momentum buffer, uniforms -- all pre-rounded to f32."""
    n_rows = 3 * S if n_rows is None else n_rows
    rng = np.random.RandomState(1000 * H + 10 * S + N + (M or 0))
    vid = np.stack([np.sort(rng.choice(n_rows, size=S, replace=False)) for _ in range(N)]).astype(np.int32)
    vval = (rng.uniform(size=(N, S)) < 0.5).astype(np.uint8)
    c = dict(kind='sparse', H=H, S=S, N=N, M=M, n_rows=n_rows, weightcost=weightcost, vid=vid, vval=vval,
             W=r32(rng.uniform(-0.1, 0.1, (n_rows, H))), visbias=r32(rng.uniform(-0.1, 0.1, n_rows)),
             hidbias=r32(rng.uniform(-0.1, 0.1, H)), wstep=r32(rng.uniform(-1e-3, 1e-3, (S, H))),
             unif=r32(rng.uniform(size=(N, H))))
    return c


def _sparse_state(c):
    st = ro.SparseRBMState(c['n_rows'], c['H'], c['S'], np.random.RandomState(0))
    st.W, st.visbias, st.hidbias, st.weightstep = c['W'].copy(), c['visbias'].copy(), c['hidbias'].copy(), c['wstep'].copy()
    return st


def run_sparse(c, unif=None, M='case', weightcost=None, momentum=MOMENTUM, margin=None, n_first=None):
    """Walk the oracle over the case: online (M None) or in mini-batches of M.  margin: nudge the draws on the way (safe_uniforms).
    Returns dict(W, visbias, hidbias, wstep, err, unif, moved)."""
    M = c['M'] if M == 'case' else M
    wc = c['weightcost'] if weightcost is None else weightcost
    unif = np.array(c['unif'] if unif is None else unif, dtype=np.float64)
    st, N, err, moved = _sparse_state(c), (c['N'] if n_first is None else n_first), 0.0, 0
    ex = [(list(c['vid'][n]), c['vval'][n].astype(np.float64)) for n in range(N)]
    kw = dict(weightcost=wc, rates=RATES, momentum=momentum)
    step = 1 if M is None else M
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        if margin is not None:           # hid exactly as the oracle computes it: every example of a mini-batch reads its start state
            for n in range(n0, n1):
                keys, v = ex[n]
                hid = ro._sigmoid(v.reshape(1, -1) @ st.W[keys] + st.hidbias)
                unif[n], k = nudge(unif[n], hid[0], margin)
                moved += k
        rp = Replay(unif[n0:n1])
        if M is None:
            err += ro.sparse_cd1_example(st, ex[n0][0], ex[n0][1], rp, **kw)
        else:
            err += ro.sparse_cd1_minibatch(st, ex[n0:n1], rp, **kw)
    return dict(W=st.W, visbias=st.visbias, hidbias=st.hidbias, wstep=st.weightstep, err=err, unif=unif, moved=moved)


# ------------------------------------------------------------------------------------------ dense CD-1
def dense_case(nvis, nhid, max_n, ns, weightcost):
    rng = np.random.RandomState(100 * nvis + nhid)
    return dict(kind='dense', nvis=nvis, nhid=nhid, max_n=max_n, ns=tuple(ns), weightcost=weightcost,
                W=r32(rng.uniform(-0.1, 0.1, (nvis, nhid))), visbias=r32(rng.uniform(-0.1, 0.1, nvis)),
                hidbias=r32(rng.uniform(-0.1, 0.1, nhid)),
                X=[r32(rng.uniform(0.05, 0.95, (n, nvis))) for n in ns],          # "already sigmoid-ed" inputs (:218)
                unif=[r32(rng.uniform(size=(n, nhid))) for n in ns])


def _dense_state(c):
    st = ro.DenseRBMState(c['nvis'], c['nhid'], np.random.RandomState(0))
    st.W, st.visbias, st.hidbias = c['W'].copy(), c['visbias'].copy(), c['hidbias'].copy()
    st.weightstep = np.zeros_like(st.W)                     # rbm_dense_set zeroes the momentum
    return st


def run_dense(c, unif=None, weightcost=None, momentum=MOMENTUM, margin=None):
    """Three mini-batches of the dense oracle.  Returns dict(W, visbias, hidbias, errs [per step], unif, moved)."""
    wc = c['weightcost'] if weightcost is None else weightcost
    unif = [np.array(u, dtype=np.float64) for u in (c['unif'] if unif is None else unif)]
    st, errs, moved = _dense_state(c), [], 0
    for k, X in enumerate(c['X']):
        if margin is not None:
            unif[k], m = nudge(unif[k], ro._sigmoid(X @ st.W + st.hidbias), margin)
            moved += m
        errs.append(ro.dense_cd1_batch(st, X, Replay([unif[k]]), weightcost=wc, rates=RATES, momentum=momentum))
    return dict(W=st.W, visbias=st.visbias, hidbias=st.hidbias, errs=errs, unif=unif, moved=moved)


def run_dense_bf16(c, unif):
    """dense_cd1_batch as rbm_step<bf16_t> computes it: every operand of a product is bf16 -- the tiled shadows of [W | visbias |
    hidbias] that k_rbm_update writes ((T)w: wf / wtf), the inputs k_rbm_prep casts (Xr / XT), and hid, vis, hid2 as EpiFwd stores
    them for the next GEMM, for k_rbm_binarise, for k_wgrad and for k_rbm_sqerr.  The ones column is exact; accumulation and the
    master parameters [Wp, wsp] are f32 in the kernel and left unrounded here.  Returns run_dense's dict and the sampled states."""
    st, errs, hss = _dense_state(c), [], []
    vis_rate, hid_rate, w_rate = RATES
    for X, u in zip(c['X'], unif):
        n = X.shape[0]
        Wb, vb, hb, Xb = bf16(st.W), bf16(st.visbias), bf16(st.hidbias), bf16(X)
        hid = bf16(ro._sigmoid(Xb @ Wb + hb))
        hs = np.where(np.asarray(u) < hid, 1.0, np.floor(hid))
        vis = bf16(ro._sigmoid(hs @ Wb.T + vb))
        hid2 = bf16(ro._sigmoid(vis @ Wb + hb))
        step = ((Xb.T @ hid - vis.T @ hid2) / n - c['weightcost'] * st.W) * w_rate
        st.weightstep = st.weightstep * MOMENTUM + step
        st.W = st.W + st.weightstep
        st.visbias = st.visbias + (Xb.sum(axis=0) - vis.sum(axis=0)) * (vis_rate / n)
        st.hidbias = st.hidbias + (hid.sum(axis=0) - hid2.sum(axis=0)) * (hid_rate / n)
        errs.append(float(((vis - X) ** 2).sum()))
        hss.append(hs)
    return dict(W=st.W, visbias=st.visbias, hidbias=st.hidbias, errs=errs), hss


def safe_uniforms(c, margin=MARGIN_F32, **kw):
    """The case's uniforms with no draw within `margin` of the oracle's hid, and the share of draws that moved."""
    r = (run_sparse if c['kind'] == 'sparse' else run_dense)(c, margin=margin, **kw)
    total = sum(np.size(u) for u in r['unif']) if c['kind'] == 'dense' else r['unif'][:kw.get('n_first') or c['N']].size
    return r['unif'], r['moved'] / float(total)


# ------------------------------------------------------------------------------------------ the bound
def change_ratios(got, ref, init, names):
    """max |got - ref| / max |ref - init| for every named array."""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / (np.abs(ref[k] - init[k]).max() + 1e-30)) for k in names}


FLOORS = {'W': 0.0, 'visbias': 1e-7, 'hidbias': 1e-7, 'wstep': 1e-8}        # the absolute floors of tests/test_gpu_rbm.py


def within(got, ref, init, names, tol=TOL):
    """The assertion of the shape tests as a predicate: every array within tol of its change (+ floor)."""
    return all(np.abs(np.asarray(got[k], np.float64) - ref[k]).max() <= tol * np.abs(ref[k] - init[k]).max() + FLOORS[k] for k in names)


# ------------------------------------------------------------------------------------------ helper kernels
def bag_sum_ref(W0, b0, ids, n_rows):
    """rbm_bag_sum: sum of the rows of the ids in [0, n_rows) + b0; ids < 0 or >= n_rows contribute nothing.
    Returns (out, bound): 4 * terms * 2^-24 * sum |terms|."""
    n, F = ids.shape
    out, mag = np.zeros((n, W0.shape[1])), np.zeros((n, W0.shape[1]))
    for t in range(n):
        for f in range(F):
            if 0 <= ids[t, f] < n_rows:
                out[t] += W0[ids[t, f]]
                mag[t] += np.abs(W0[ids[t, f]])
    return out + b0, 4.0 * (F + 1) * U32 * (mag + np.abs(b0))


def affine_ref(x, W, bias):
    """rbm_affine: x . W + bias, with 4 * (a + 1) * 2^-24 * (|x| . |W| + |bias|)."""
    return x @ W + bias, 4.0 * (x.shape[1] + 1) * U32 * (np.abs(x) @ np.abs(W) + np.abs(bias))


SIGMOID_OWN = 8.0 * U32      # 1 / (1 + expf(-z)) on an exact z: expf within 2 ulp = 4 * 2^-24 relative, which the map e -> 1 / (1 + e)
#                              damps by e / (1 + e)^2 <= 1/4; the sum and the quotient add 2^-24 and at most 2.5 ulp = 5 * 2^-24: <= 7 * 2^-24 of
#                              a result <= 1


SIGMOID_REL = 10.0 * U32     # the same steps relative to the result: expf's 4 * 2^-24 times e / (1 + e) <= 1, the sum 2^-24, the quotient 5 * 2^-24


def sigmoid_bound(pre_bound):
    """Error of sigmoid(z) when z carries pre_bound: the slope is at most 1/4, plus the evaluation's own rounding."""
    return 0.25 * np.asarray(pre_bound) + SIGMOID_OWN


def cumsum_sigmoid_ref(W0, b0, ids):
    """Layer 0 of da() (dae_oracle.propagate, Q3): sigmoid(cumsum_k(bag) + b0) over ALL ids >= 0.  Returns (out, pre-sigmoid bound):
    unit k sums F * (k + 1) + 1 terms."""
    n, F = ids.shape
    H = W0.shape[1]
    out, bound = np.zeros((n, H)), np.zeros((n, H))
    for t in range(n):
        act = [int(i) for i in ids[t] if i >= 0]
        bag = W0[act].sum(axis=0) if act else np.zeros(H)
        mag = np.abs(W0[act]).sum(axis=0) if act else np.zeros(H)
        out[t] = do.sigmoid(np.cumsum(bag) + b0)
        bound[t] = 4.0 * (F * np.arange(1, H + 1) + 1) * U32 * (np.cumsum(mag) + np.abs(b0))
    if n:
        assert np.array_equal(out[0], do.propagate([W0, b0], [int(i) for i in ids[0] if i >= 0]))
    return out, bound


def sparse_da_example(table, idx, bhid, bvis, x, lr):
    """One example of sparse_da (dae_oracle.sparse_da's loop body): only the biases learn.  Returns (cost, bhid', bvis')."""
    cost, _, dy, d = do.da_grads(table[idx], bhid, bvis, np.asarray(x, np.float64))
    return cost, bhid - lr * dy, bvis - lr * d


def run_sparse_da(table, idx, x, bhid, bvis, lr):
    """N examples in order.  Returns (bhid, bvis, bhid before the last example, cost sum)."""
    cost, prev = 0.0, bhid
    for n in range(idx.shape[0]):
        prev = bhid
        c, bhid, bvis = sparse_da_example(table, idx[n], bhid, bvis, x[n], lr)
        cost += c
    return bhid, bvis, prev, cost


def run_dense_da(W, bh, bv, X, lr, skip_last):
    """da()'s loop (dae_oracle.da): N online steps; skip_last: the last example only contributes its cost."""
    cost = 0.0
    for n in range(X.shape[0]):
        c, gW, dy, d = do.da_grads(W, bh, bv, X[n])
        cost += c
        if skip_last and n == X.shape[0] - 1:
            break
        W, bh, bv = W - lr * gW, bh - lr * dy, bv - lr * d
    return W, bh, bv, cost


# da() shapes of the GPU tests: f32 -- the edges of the register tilings <4,1> <8,2> <19,2> <13,5>, one past each, wide / tall / 1 x 1
DAE_DENSE_F32 = [(1, 1), (64, 64), (65, 64), (64, 65), (128, 128), (129, 128), (304, 128), (305, 128), (304, 129), (208, 320), (209, 320),
                 (208, 321), (7, 1000), (1500, 3)]
# f64 -- the rows-per-wave classes of the split trainer, fewer columns than workgroups, its limit and one past it
DAE_DENSE_F64 = [(128, 64), (129, 65), (208, 512), (209, 100), (304, 7), (305, 1), (512, 512), (1, 8), (513, 512), (512, 513)]


def dae_dense_steps(row, col):
    return 60 if row * col <= 60000 else 40


def dae_dense_case(row, col, N, dtype):
    """da()'s own initialisation range for W, NON-ZERO biases, inputs in (0.05, 0.95); rounded to `dtype`.
    The hidden bias starts at U(-0.1, 0.1) - ln(max(1, col / 128)).  One step moves every reconstruction's pre-activation by
    lr d_i |y|^2; with y near 1/2 in 1,000 hidden units that is 25 d_i, the reconstructions bounce between 1e-8 and 1 - 1e-8, and f32
    has no digits left in 1 - z (logf(1 - z) of the cost is -inf from 6e-8 on) -- an input regime no f32 trainer can be compared in.
    The shift keeps |y|^2 at the 10 to 30 of the reference's 100 to 300 hidden units (tests/test_pretrain_ref.py: every
    reconstruction stays within [1e-4, 1 - 1e-4] at every shape used)."""
    rng = np.random.RandomState(7 * row + col)
    rd = r32 if dtype == np.float32 else (lambda a: np.asarray(a, np.float64))
    b = 4 * np.sqrt(6. / (row + col))
    return dict(W=rd(rng.uniform(-b, b, (row, col))), bh=rd(rng.uniform(-0.1, 0.1, col) - np.log(max(1.0, col / 128.0))),
                bv=rd(rng.uniform(-0.1, 0.1, row)), X=rd(rng.uniform(0.05, 0.95, (N, row))))


def bag_ids(n, F, n_rows, seed):
    """ids [n, F] with -1 entries, duplicates inside a row and one all -1 row (the last)."""
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, n_rows, size=(n, F)).astype(np.int32)
    ids[rng.uniform(size=(n, F)) < 0.25] = -1
    if F > 1:
        ids[0, 0] = ids[0, 1] = 1 % n_rows              # a duplicate
    ids[n - 1] = -1
    return ids
