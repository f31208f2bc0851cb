"""CPU checks of tests/pretrain_ref.py, the helpers of the RBM / DAE shape tests: the margin-safe uniforms leave the oracle's
trajectory bit for bit what it was, at every input set the GPU tests use; the 2e-3 bound of those tests can SEE a wrong
weight-decay or momentum term (the oracle run with weightcost = 0, or momentum 0.89, misses it by 5x or more); the float64
references of the helper kernels agree with the oracles they restate.

Measured here (float64 oracle; largest ratio over W / visbias / hidbias / wstep of |variant - true| to the parameter change):
  weightcost 0.05 -> 0:   online 9.1e-2 .. 1.8e-1, mini-batch 5.6e-2 .. 4.6e-1, dense 2.0e-2 .. 1.5e-1
  momentum 0.9 -> 0.89:   online 8.4e-2 .. 1.4e-1, mini-batch 2.8e-2 .. 1.3e-1, dense 6.7e-3 .. 7.7e-3
against the 2e-3 the GPU tests allow.  The dense trainer starts from zero momentum (rbm_dense_set) and runs three steps, so
momentum weighs on 0.01 s + (0.019 + 0.009) s of a total move of about (1 + 1.9 + 2.71) s: 6.8e-3, which is what is measured --
3.4x the bound rather than 5x; it is asserted at 3x, the sparse trainers (non-zero momentum buffer on entry) at 5x.
Share of draws moved by safe_uniforms: at most 0.63 % at the 1e-3 margin (f32), 4.1 % at 2e-2 (bf16)."""
import numpy as np
import pytest

import pretrain_ref as pr
from oracle import dae_oracle as do
from oracle import rbm_oracle as ro

SP = ('W', 'visbias', 'hidbias', 'wstep')
DN = ('W', 'visbias', 'hidbias')


def sparse_cases():
    out = [pr.sparse_case(H, S, N, wc) for H, S, N, wc in pr.ONLINE_GENERIC + pr.ONLINE_S32]
    out += [pr.sparse_case(H, S, N, wc, M=M) for H, S, M, N, wc in pr.BATCH_ATOMIC + pr.BATCH_MULTI + [pr.BATCH_REGROUP, pr.BATCH_M1]]
    H, S, M, N, wc = pr.BATCH_LONG_RUNS
    return out + [pr.sparse_case(H, S, N, wc, M=M, n_rows=S)]


def dense_cases():
    return [(pr.dense_case(*a), pr.MARGIN_F32) for a in pr.DENSE_F32] + [(pr.dense_case(*a), pr.MARGIN_BF16) for a in pr.DENSE_BF16]


def _id(c):
    return '-'.join(str(c[k]) for k in (('H', 'S', 'M', 'N') if c['kind'] == 'sparse' else ('nvis', 'nhid', 'max_n')))


def _init(c, names):
    return {k: c[k] for k in names}


@pytest.mark.parametrize("c", sparse_cases(), ids=_id)
def test_safe_uniforms_keep_the_sparse_trajectory(c):
    u, share = pr.safe_uniforms(c)
    a, b = pr.run_sparse(c), pr.run_sparse(c, unif=u)
    for k in SP:
        assert np.array_equal(a[k], b[k]), k                        # bit-identical with and without the nudge
    assert a['err'] == b['err']
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)      # still f32 numbers
    again = pr.run_sparse(c, unif=u, margin=pr.MARGIN_F32)          # a second walk finds no draw within the margin
    assert again['moved'] == 0 and np.array_equal(again['unif'], u)
    print("moved share %.4f" % share)
    assert share < 0.05


@pytest.mark.parametrize("c,margin", dense_cases(), ids=lambda v: _id(v) if isinstance(v, dict) else str(v))
def test_safe_uniforms_keep_the_dense_trajectory(c, margin):
    u, share = pr.safe_uniforms(c, margin=margin)
    a, b = pr.run_dense(c), pr.run_dense(c, unif=u)
    for k in DN:
        assert np.array_equal(a[k], b[k]), k
    assert a['errs'] == b['errs']
    again = pr.run_dense(c, unif=u, margin=margin)
    assert again['moved'] == 0
    print("moved share %.4f" % share)
    assert share < 0.05


def test_nudge_moves_only_what_is_close_and_keeps_the_side():
    hid = np.array([0.5, 0.5, 0.5, 0.5, 0.999, 0.0005])
    u = np.array([0.5004, 0.4996, 0.6, 0.5, 0.9995, 0.0001])
    v, moved = pr.nudge(u, hid, 1e-3)
    assert moved == 5 and v[2] == 0.6
    assert np.array_equal(v < hid, u < hid)
    assert (np.abs(v - hid) >= 1e-3).all() and (np.abs(v - hid) < 1.01e-3)[[0, 1, 3, 4, 5]].all()


@pytest.mark.parametrize("c", [c for c in sparse_cases() if c['weightcost'] == 0.05], ids=_id)
def test_the_bound_sees_weightcost_and_momentum_sparse(c):
    u, _ = pr.safe_uniforms(c)
    true = pr.run_sparse(c, unif=u)
    for tag, kw in (('weightcost 0', dict(weightcost=0.0)), ('momentum 0.89', dict(momentum=0.89))):
        var = pr.run_sparse(c, unif=u, **kw)
        r = pr.change_ratios(var, true, _init(c, SP), SP)
        print(tag, {k: '%.1e' % v for k, v in r.items()})
        assert max(r.values()) >= 5 * pr.TOL, (tag, r)
        assert not pr.within(var, true, _init(c, SP), SP)           # the GPU tests' own predicate refuses the variant


@pytest.mark.parametrize("c", [c for c, m in dense_cases() if c['weightcost'] == 0.05 and m == pr.MARGIN_F32], ids=_id)
def test_the_bound_sees_weightcost_and_momentum_dense(c):
    u, _ = pr.safe_uniforms(c)
    true = pr.run_dense(c, unif=u)
    for tag, kw, times in (('weightcost 0', dict(weightcost=0.0), 5), ('momentum 0.89', dict(momentum=0.89), 3)):      # 3x: module docstring
        var = pr.run_dense(c, unif=u, **kw)
        r = pr.change_ratios(var, true, _init(c, DN), DN)
        print(tag, {k: '%.1e' % v for k, v in r.items()})
        assert max(r.values()) >= times * pr.TOL, (tag, r)
        assert not pr.within(var, true, _init(c, DN), DN)


@pytest.mark.parametrize("a", pr.DENSE_BF16, ids=str)
def test_bf16_emulation_follows_the_oracle_decisions(a):
    """The bf16-operand emulation takes the plain oracle's decisions at the 2e-2 margin (so its deviation is rounding, not a
    different sample), stays within 1e-2 of the change, and is the plain oracle when nothing is rounded."""
    c = pr.dense_case(*a)
    u, _ = pr.safe_uniforms(c, margin=pr.MARGIN_BF16)
    plain = pr.run_dense(c, unif=u)
    emu, hss = pr.run_dense_bf16(c, u)
    st = pr._dense_state(c)
    for X, uu, hs in zip(c['X'], u, hss):
        hid = ro._sigmoid(X @ st.W + st.hidbias)
        assert np.array_equal(hs, (uu < hid).astype(np.float64))
        ro.dense_cd1_batch(st, X, pr.Replay([uu]), weightcost=c['weightcost'], rates=pr.RATES, momentum=pr.MOMENTUM)
    r = pr.change_ratios(emu, plain, _init(c, DN), DN)
    print({k: '%.2e' % v for k, v in r.items()})
    assert 1e-5 < max(r.values()) < 1e-2
    keep, pr.bf16 = pr.bf16, (lambda x: np.asarray(x, np.float64))
    try:
        same, _ = pr.run_dense_bf16(c, u)
    finally:
        pr.bf16 = keep
    for k in DN:
        np.testing.assert_allclose(same[k], plain[k], rtol=0, atol=1e-15)


def test_bf16_rounding():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 3 * 2.0 ** -8, -0.1, 0.0, 3.0e-5])
    got = pr.bf16(x)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == 1.0 + 2.0 ** -7 and got[3] == 1.0 + 2.0 ** -6       # ties to even
    assert (np.abs(got - x) <= 2.0 ** -8 * np.abs(x)).all() and got[5] == 0.0          # 8 significant bits: half an ulp is 2^-8
    assert np.array_equal(pr.bf16(got), got)


def test_helper_references_restate_the_oracles():
    rng = np.random.RandomState(3)
    n_rows, H, F = 20, 9, 6
    W0, b0 = rng.uniform(-1, 1, (n_rows, H)), rng.uniform(-1, 1, H)
    ids = pr.bag_ids(5, F, n_rows, 4)
    assert (ids[-1] == -1).all() and ids[0, 0] == ids[0, 1] and (ids == -1).sum() > F
    # rbm_bag_sum + rbm_affine + sigmoid is lower_layers of the RBM oracle (values 1 at the active ids)
    W1, b1 = rng.uniform(-1, 1, (H, 4)), rng.uniform(-1, 1, 4)
    bag, bound = pr.bag_sum_ref(W0, b0, ids, n_rows)
    # a row's duplicates count twice in the kernel's sum (a list of ids), once in the oracle's dict: compare on de-duplicated rows
    uniq = np.full_like(ids, -1)
    for t in range(5):
        s = sorted(set(int(i) for i in ids[t] if i >= 0))
        uniq[t, :len(s)] = s
    bag_u, _ = pr.bag_sum_ref(W0, b0, uniq, n_rows)
    aff, _ = pr.affine_ref(bag_u, W1, b1)
    want = ro.lower_layers([W0, b0, W1, b1], [{int(i): 1 for i in uniq[t] if i >= 0} for t in range(5)])
    np.testing.assert_allclose(ro._sigmoid(aff), want, rtol=0, atol=1e-14)
    assert np.array_equal(bag[-1], b0) and (bound > 0).all()
    # ids >= n_rows are skipped
    big = ids.copy(); big[1, 2] = n_rows; cut = ids.copy(); cut[1, 2] = -1
    assert np.array_equal(pr.bag_sum_ref(W0, b0, big, n_rows)[0], pr.bag_sum_ref(W0, b0, cut, n_rows)[0])
    # the DAE layer 0: the running sum over the hidden units
    out, _ = pr.cumsum_sigmoid_ref(W0, b0, ids)
    for t in range(5):
        np.testing.assert_allclose(out[t], do.propagate([W0, b0], [int(i) for i in ids[t] if i >= 0]), rtol=0, atol=1e-15)
    assert np.array_equal(out[-1], do.sigmoid(b0))


def test_sparse_da_example_is_the_oracle_loop():
    """run_sparse_da against dae_oracle.sparse_da itself (its own table, its RandomState(123) negatives, zero initial biases)."""
    rng = np.random.RandomState(8)
    lines = [(sorted(rng.choice(np.arange(3, 400, 3), size=4, replace=False).tolist()), [1, 1, 1, 1]) for _ in range(12)]
    table, b_pre, info = do.sparse_da(8, 5, lines, sparse_len=400, epochs=1)
    r2 = np.random.RandomState(123)
    r2.randint(2 ** 30)
    for shape, bound in (((8, 5), 5 + 8), ((400, 5), 400 + 8), ((400, 5), 400 + 5), ((8, 5), 8 + 5)):
        r2.uniform(low=-4 * np.sqrt(6. / bound), high=4 * np.sqrt(6. / bound), size=shape)
    idx, x = [], []
    for ids, vals in lines:
        xs, ix = do.sample_negatives(r2, ids, vals)
        idx.append(ix); x.append(xs)
    bh, bv, prev, cost = pr.run_sparse_da(table, np.array(idx), np.array(x, np.float64), np.zeros(5), np.zeros(8), 0.1)
    assert np.array_equal(bh, info['b']) and np.array_equal(bv, info['bvis']) and np.array_equal(prev, b_pre)
    assert abs(cost / 12 - info['costs'][0]) < 1e-12


def test_run_dense_da_is_the_oracle_step():
    c = pr.dae_dense_case(5, 3, 4, np.float64)
    W, bh, bv, cost = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'], 0.1, 0)
    Ws, bhs, bvs, costs = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'], 0.1, 1)
    W3, bh3, bv3, cost3 = pr.run_dense_da(c['W'], c['bh'], c['bv'], c['X'][:3], 0.1, 0)
    assert np.array_equal(Ws, W3) and np.array_equal(bhs, bh3) and np.array_equal(bvs, bv3) and costs == cost      # Q2: the state before the last step
    assert not np.array_equal(W, Ws) and (c['bh'] != 0).all() and (c['bv'] != 0).all()


@pytest.mark.parametrize("row,col", pr.DAE_DENSE_F32 + [(2048, 1024), (100, 100)])
def test_dae_dense_inputs_stay_out_of_saturation(row, col):
    """The f32 trainer is compared where f32 can follow: every reconstruction of every step within [1e-4, 1 - 1e-4] (dae_dense_case)."""
    N = 4 if row == 2048 else pr.dae_dense_steps(row, col)
    c = pr.dae_dense_case(row, col, N, np.float32)
    W, bh, bv = c['W'], c['bh'], c['bv']
    assert (bh != 0).all() and (bv != 0).all()
    for n in range(N):
        cost, gW, dy, d = do.da_grads(W, bh, bv, c['X'][n])
        z = d + c['X'][n]
        assert 1e-4 < z.min() and z.max() < 1 - 1e-4, (n, z.min(), 1 - z.max())
        W, bh, bv = W - 0.1 * gW, bh - 0.1 * dy, bv - 0.1 * d
