"""The RBM pre-training kernels (include/rbm_hip.h) at every shape they accept, against the float64 oracle
(oracle/rbm_oracle.py) walked by tests/pretrain_ref.py: the general-S online trainer (k_rbm_sparse), the S = 32 one at its
edges, the atomic and the sorted mini-batch forms with several examples per workgroup, the padding edges of the dense CD-1
handle in f32 and bf16, and the helper kernels called directly.

Settings of every training case: rates (1e-2, 1e-2, 1e-2), inputs pre-rounded to f32, a non-zero momentum buffer on entry, few
rows (3 S) so that consecutive examples share rows, weightcost 0.05 in at least half of the cases of a group (2e-4 in the rest),
uniforms kept 1e-3 (bf16: 2e-2) clear of the oracle's hid by pretrain_ref.safe_uniforms so that no f32 rounding flips a sample.
Bound: 2e-3 of the parameter change for W, visbias, hidbias, wstep (+ the absolute floors of test_gpu_rbm.py), 1e-4 relative for
the error sum.  Every 0.05 case also runs the oracle with weightcost = 0: the SAME assertions must refuse it
(tests/test_pretrain_ref.py shows the shift is 5x the bound or more).  Each case prints its measured ratios; the largest of
each group, as measured on an MI355X, stand in the tests' docstrings (kernels seen by a kernel trace of this file and
test_gpu_dae_shapes.py: profiles/pretrain_shapes_kernel_stats.csv)."""
import ctypes as C

import numpy as np
import pytest

import pretrain_ref as pr

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

pytestmark = pytest.mark.gpu

SP = ('W', 'visbias', 'hidbias', 'wstep')
DN = ('W', 'visbias', 'hidbias')


def _dev():
    import torch
    dev = torch.device('cuda', 0)
    return torch, dev, torch.cuda.current_stream(dev).cuda_stream


def _t(a, dt=None):
    torch, dev, _ = _dev()
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt or torch.float32).contiguous()


def gpu_sparse(c, unif, M=None, n0=0, n1=None, state=None, want_err=True):
    """rbm_sparse_epoch (M None) or rbm_sparse_batch over examples [n0, n1) from `state` (default: the case's).  Returns the four
    arrays as float32 NumPy, the error sum and (mini-batch) whether dW / dvis came back zero."""
    torch, dev, st = _dev()
    lib = _capi.load()
    n1 = c['N'] if n1 is None else n1
    s = state or c
    W, vb, hb, ws = _t(s['W']), _t(s['visbias']), _t(s['hidbias']), _t(s['wstep'])
    vd, vv, ud = _t(c['vid'][n0:n1], torch.int32), _t(c['vval'][n0:n1], torch.uint8), _t(unif[n0:n1])
    err = C.c_double(-1.0)
    ep = C.byref(err) if want_err else None
    a = (c['weightcost'],) + pr.RATES + (pr.MOMENTUM, ep, st)
    zero = True
    if M is None:
        rc = lib.rbm_sparse_epoch(W.data_ptr(), vb.data_ptr(), hb.data_ptr(), ws.data_ptr(), vd.data_ptr(), vv.data_ptr(), ud.data_ptr(),
                                  n1 - n0, c['H'], c['S'], *a)
    else:
        dW, dvis = torch.zeros_like(W), torch.zeros_like(vb)
        rc = lib.rbm_sparse_batch(W.data_ptr(), dW.data_ptr(), vb.data_ptr(), dvis.data_ptr(), hb.data_ptr(), ws.data_ptr(), vd.data_ptr(),
                                  vv.data_ptr(), ud.data_ptr(), n1 - n0, M, c['H'], c['S'], *a)
        zero = not dW.any().item() and not dvis.any().item()
    assert rc == 0, lib.rbm_last_error()
    torch.cuda.synchronize()
    return dict(W=W.cpu().numpy(), visbias=vb.cpu().numpy(), hidbias=hb.cpu().numpy(), wstep=ws.cpu().numpy(), err=err.value, zero=zero)


def check_sparse(c, got, ref, tag):
    init = {k: c[k] for k in SP}
    r = pr.change_ratios(got, ref, init, SP)
    e = abs(got['err'] - ref['err']) / ref['err'] if got['err'] >= 0 else 0.0
    print("%s H=%d S=%d M=%s N=%d wc=%g: error/change W %.2e visbias %.2e hidbias %.2e wstep %.2e, err sum %.2e"
          % (tag, c['H'], c['S'], c['M'], c['N'], c['weightcost'], r['W'], r['visbias'], r['hidbias'], r['wstep'], e))
    assert pr.within(got, ref, init, SP), r
    assert e <= pr.TOL_ERR
    return r


def refuses_wrong_weightcost(c, got, unif, M):
    """The cross-check: the oracle WITHOUT the weight-decay term (CPU side only) must fail the assertions the true one passes."""
    if c['weightcost'] != 0.05:
        return
    wrong = pr.run_sparse(c, unif=unif, M=M, weightcost=0.0)
    assert not pr.within(got, wrong, {k: c[k] for k in SP}, SP)


def _sparse(c, M, tag, **kw):
    unif, _ = pr.safe_uniforms(c, M=M)
    ref = pr.run_sparse(c, unif=unif, M=M)
    got = gpu_sparse(c, unif, M=M, **kw)
    check_sparse(c, got, ref, tag)
    refuses_wrong_weightcost(c, got, unif, M)
    return unif, ref, got


@pytest.mark.parametrize("H,S,N,wc", pr.ONLINE_GENERIC)
def test_online_general_s(built, H, S, N, wc):
    """k_rbm_sparse (S < 32 is the only way in): H = 1, H not a multiple of 8 or 64, H = 256, S = 1, S = 31.
    Largest measured error/change: W 1.4e-6, visbias 6.4e-7, hidbias 1.7e-5 (H = 256, S = 1), wstep 5.2e-7; error sum 3.5e-8."""
    _sparse(pr.sparse_case(H, S, N, wc), None, 'online')


@pytest.mark.parametrize("H,S,N,wc", pr.ONLINE_S32)
def test_online_s32_edges(built, H, S, N, wc):
    """k_rbm_sparse32 at H = 255 / 256 (the last wave partly idle / full) and H = 1 (255 idle threads shadow column 0).
    Largest measured error/change: W 6.7e-7, visbias 3.5e-7, hidbias 1.4e-6, wstep 4.6e-7; error sum 3.8e-8."""
    _sparse(pr.sparse_case(H, S, N, wc), None, 'online32')


def test_online_without_an_error_sum(built):
    """sq_err_out = NULL: the pass runs and moves the parameters exactly as with it."""
    c = pr.sparse_case(7, 5, 120, 0.05)
    unif, ref, got = _sparse(c, None, 'online')
    blind = gpu_sparse(c, unif, want_err=False)
    for k in SP:
        assert np.array_equal(blind[k], got[k]), k


@pytest.mark.parametrize("H,S,N,N1", [(65, 16, 80, 33), (256, 32, 60, 1)])
def test_online_two_calls_carry_the_momentum_buffer(built, H, S, N, N1):
    """N examples in one call and as N1 + N2 in two calls on fresh copies: bit-identical (wstep, hidbias leave and re-enter through memory)."""
    c = pr.sparse_case(H, S, N, 0.05)
    unif, _ = pr.safe_uniforms(c)
    one = gpu_sparse(c, unif)
    first = gpu_sparse(c, unif, n1=N1)
    second = gpu_sparse(c, unif, n0=N1, state=first)
    for k in SP:
        assert np.array_equal(one[k], second[k]), k
    assert abs(first['err'] + second['err'] - one['err']) <= 1e-12 * one['err']


@pytest.mark.parametrize("H,S,M,N,wc", pr.BATCH_ATOMIC)
def test_minibatch_atomic_form(built, H, S, M, N, wc):
    """k_rbm_batch<false> + k_rbm_apply (H % 4 != 0): the weight decay enters as 2 (ws0 + step) through the atomics; dW / dvis come
    back all zero.  No bit-reproducibility claim (float atomics).
    Largest measured error/change: W 3.6e-7, visbias 3.7e-7, hidbias 7.5e-6 (H = 1), wstep 2.8e-7; error sum 4.1e-8."""
    _, _, got = _sparse(pr.sparse_case(H, S, N, wc, M=M), M, 'atomic')
    assert got['zero']


@pytest.mark.parametrize("H,S,M,N,wc", pr.BATCH_MULTI)
def test_minibatch_several_examples_per_workgroup(built, H, S, M, N, wc):
    """M > 512 workgroups' worth: the `n += gridDim.x` loop with its wsum / hacc / err carried across examples and the tail's sum
    over 512 partials -- k_rbm_batch<true> (two full mini-batches and a short one of 100), k_rbm_batch32, k_rbm_batch<false>.
    Largest measured error/change: W 3.5e-7, visbias 3.4e-7, hidbias 3.3e-6, wstep 3.1e-7; error sum 1.6e-9."""
    c = pr.sparse_case(H, S, N, wc, M=M)
    unif, _, got = _sparse(c, M, 'multi')
    assert got['zero']
    if H % 4 == 0:
        again = gpu_sparse(c, unif, M=M)
        for k in SP:
            assert np.array_equal(got[k], again[k]), k             # the sorted form is bit-reproducible


@pytest.mark.parametrize("case,n_rows", [(pr.BATCH_LONG_RUNS, 4), (pr.BATCH_REGROUP, None)], ids=['runs-of-300', '18-minibatches'])
def test_minibatch_sorted_runs_and_regrouping(built, case, n_rows):
    """n_rows == S: every row one run of 300 sorted entries -- runs that span ten 32-entry chunks, chunks that end one run and start
    the next, keep = 1 - 2 rate_w weightcost 300 = 0.7.  M = 3, N = 52: 18 mini-batches, two groups of the sort, the last of ONE example.
    Largest measured error/change: W 2.8e-7, visbias 2.0e-7, hidbias 1.7e-5, wstep 4.1e-7; error sum 8.3e-10."""
    H, S, M, N, wc = case
    c = pr.sparse_case(H, S, N, wc, M=M, n_rows=n_rows)
    unif, _, got = _sparse(c, M, 'sorted')
    again = gpu_sparse(c, unif, M=M)
    for k in SP:
        assert np.array_equal(got[k], again[k]), k
    assert got['zero']


def test_minibatch_of_one_is_the_online_trainer(built):
    """M = 1 (S < 32): rbm_sparse_batch and rbm_sparse_epoch both within the bound of the SAME online oracle run.
    Measured error/change: W 2.9e-7 / 3.4e-7, hidbias 4.1e-6 both, wstep 2.5e-7 / 2.2e-7; error sum 1.0e-9 / 7.3e-9."""
    H, S, M, N, wc = pr.BATCH_M1
    c = pr.sparse_case(H, S, N, wc, M=M)
    unif, _ = pr.safe_uniforms(c, M=None)
    ref = pr.run_sparse(c, unif=unif, M=None)
    by_one = pr.run_sparse(c, unif=unif, M=1)
    for k in SP:
        np.testing.assert_allclose(by_one[k], ref[k], rtol=0, atol=1e-15)        # the two oracles coincide at M = 1
    for M_, tag in ((None, 'online'), (1, 'batch M=1')):
        got = gpu_sparse(c, unif, M=M_)
        check_sparse(c, got, ref, tag)
        refuses_wrong_weightcost(c, got, unif, None)


# ------------------------------------------------------------------------------------------ dense CD-1
class Dense(object):
    def __init__(self, c, precision):
        self.lib, self.c, self.h = _capi.load(), c, C.c_void_p()
        _, _, st = _dev()
        rc = self.lib.rbm_dense_create(c['nvis'], c['nhid'], c['max_n'], precision, 0, st, C.byref(self.h))
        assert rc == 0, self.lib.rbm_last_error()
        a = [np.ascontiguousarray(c[k], dtype=np.float32) for k in DN]
        assert self.lib.rbm_dense_set(self.h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data) == 0, self.lib.rbm_last_error()

    def step(self, X, unif, want_err=True):
        Xd, ud = _t(X), _t(unif)
        err = C.c_double(-1.0)
        rc = self.lib.rbm_dense_cd1(self.h, Xd.data_ptr(), X.shape[0], ud.data_ptr(), self.c['weightcost'], *pr.RATES, pr.MOMENTUM,
                                    C.byref(err) if want_err else None)
        return rc, err.value

    def get(self):
        c = self.c
        W, vb, hb = np.empty((c['nvis'], c['nhid']), np.float32), np.empty(c['nvis'], np.float32), np.empty(c['nhid'], np.float32)
        assert self.lib.rbm_dense_get(self.h, W.ctypes.data, vb.ctypes.data, hb.ctypes.data) == 0, self.lib.rbm_last_error()
        return dict(W=W, visbias=vb, hidbias=hb)

    def close(self):
        self.lib.rbm_dense_destroy(self.h)


@pytest.mark.parametrize("nvis,nhid,max_n,ns,wc", pr.DENSE_F32)
def test_dense_cd1_padding_edges(built, nvis, nhid, max_n, ns, wc):
    """Kp = rup(nvis + 1, 64), Hp = rup(nhid + 1, 64), Na = rup(n, 256): nvis / nhid of 63 (bias in the last padded column), 64 (bias
    alone in a new tile), 127, 1; n = 1, 256 / 257 / 256 and 300 / 10 / 300 (a handle whose Na shrinks and grows across a 256 boundary:
    rows left over from the longer batch must not reach the correlations).  Three steps: W, visbias, hidbias within 2e-3 of the change,
    each step's squared error within 1e-4; n = max_n + 1 and n = 0 are FNN_ERR_ARG.
    Largest measured error/change: W 5.4e-6, visbias 4.6e-6, hidbias 3.4e-4 (1 x 127, n = 7); squared error 1.2e-7."""
    c = pr.dense_case(nvis, nhid, max_n, ns, wc)
    unif, _ = pr.safe_uniforms(c)
    ref = pr.run_dense(c, unif=unif)
    d = Dense(c, _capi.FNN_PREC_F32)
    try:
        for X, u, e_ref in zip(c['X'], unif, ref['errs']):
            rc, e = d.step(X, u)
            assert rc == 0, d.lib.rbm_last_error()
            print("n=%d sq_err %.6f vs %.6f (%.1e)" % (X.shape[0], e, e_ref, abs(e - e_ref) / e_ref))
            assert abs(e - e_ref) <= pr.TOL_ERR * e_ref
        for n_bad in (max_n + 1, 0):
            Xb, ub = np.zeros((max_n + 1, nvis), np.float32), np.zeros((max_n + 1, nhid), np.float32)
            Xd, ud = _t(Xb), _t(ub)
            rc = d.lib.rbm_dense_cd1(d.h, Xd.data_ptr(), n_bad, ud.data_ptr(), wc, *pr.RATES, pr.MOMENTUM, None)
            assert rc == _capi.FNN_ERR_ARG and b'[1, max_n]' in d.lib.rbm_last_error()
        got = d.get()
    finally:
        d.close()
    init = {k: c[k] for k in DN}
    r = pr.change_ratios(got, ref, init, DN)
    print("dense %dx%d n=%s wc=%g: error/change W %.2e visbias %.2e hidbias %.2e" % (nvis, nhid, ns, wc, r['W'], r['visbias'], r['hidbias']))
    assert pr.within(got, ref, init, DN), r
    if wc == 0.05:
        assert not pr.within(got, pr.run_dense(c, unif=unif, weightcost=0.0), init, DN)


@pytest.mark.parametrize("nvis,nhid,max_n,ns,wc", pr.DENSE_BF16)
def test_dense_cd1_bf16(built, nvis, nhid, max_n, ns, wc):
    """bf16 operands, f32 master weights.  The bound is measured, not chosen: pretrain_ref.run_dense_bf16 rounds to bf16 every operand
    rbm_step<bf16_t> feeds to a product (the shadows of W / visbias / hidbias, X, hid, vis, hid2) and leaves the master weights alone;
    the kernel may be 4x as far from the plain oracle as that emulation is.  On the CPU the emulation deviates by
      64 x 64:  W 2.7e-3, visbias 1.6e-3, hidbias 8.0e-3 of the change, squared error 8.2e-5   -> bounds 1.1e-2, 6.3e-3, 3.2e-2, 3.3e-4
      100 x 40: W 2.1e-3, visbias 1.4e-3, hidbias 5.9e-3 of the change, squared error 7.5e-5   -> bounds 8.6e-3, 5.5e-3, 2.4e-2, 3.0e-4
    (uniforms at the 2e-2 margin: the emulation and the kernel take the oracle's decisions).  Measured on the GPU: the kernel sits ON the
    emulation -- 64 x 64: 2.74e-3, 1.58e-3, 7.98e-3, 8.17e-5; 100 x 40: 2.15e-3, 1.38e-3, 5.89e-3, 7.53e-5."""
    c = pr.dense_case(nvis, nhid, max_n, ns, wc)
    unif, _ = pr.safe_uniforms(c, margin=pr.MARGIN_BF16)
    ref = pr.run_dense(c, unif=unif)
    emu, _ = pr.run_dense_bf16(c, unif)
    init = {k: c[k] for k in DN}
    bound = {k: 4.0 * v for k, v in pr.change_ratios(emu, ref, init, DN).items()}
    bound_e = 4.0 * max(abs(a - b) / b for a, b in zip(emu['errs'], ref['errs']))
    d = Dense(c, _capi.FNN_PREC_BF16)
    try:
        errs = []
        for X, u in zip(c['X'], unif):
            rc, e = d.step(X, u)
            assert rc == 0, d.lib.rbm_last_error()
            errs.append(e)
        got = d.get()
    finally:
        d.close()
    r = pr.change_ratios(got, ref, init, DN)
    re = max(abs(a - b) / b for a, b in zip(errs, ref['errs']))
    print("bf16 %dx%d: error/change W %.2e (bound %.2e) visbias %.2e (%.2e) hidbias %.2e (%.2e), sq_err %.2e (%.2e)"
          % (nvis, nhid, r['W'], bound['W'], r['visbias'], bound['visbias'], r['hidbias'], bound['hidbias'], re, bound_e))
    for k in DN:
        assert r[k] <= bound[k], (k, r[k], bound[k])
    assert re <= bound_e


# ------------------------------------------------------------------------------------------ helper kernels
@pytest.mark.parametrize("H", [1, 257])
@pytest.mark.parametrize("F", [1, 16])
def test_bag_sum(built, H, F):
    """rbm_bag_sum called directly: -1 ids, duplicates, an all -1 row; an id >= n_rows is SKIPPED like a -1 (pinned; rbm_hip.h says so).
    |err| <= 4 (F + 1) 2^-24 sum |terms|; measured: at most 0.125 of that bound."""
    torch, dev, st = _dev()
    lib = _capi.load()
    n, n_rows = 7, 11
    rng = np.random.RandomState(H + F)
    W0, b0 = pr.r32(rng.uniform(-1, 1, (n_rows, H))), pr.r32(rng.uniform(-1, 1, H))
    ids = pr.bag_ids(n, F, n_rows, H * F)
    ids[2, F - 1] = n_rows                    # past the table
    ids[3, 0] = n_rows + 5
    ref, bound = pr.bag_sum_ref(W0, b0, ids, n_rows)
    out = torch.full((n, H), 7.0, dtype=torch.float32, device=dev)
    W0d, b0d, idd = _t(W0), _t(b0), _t(ids, torch.int32)
    assert lib.rbm_bag_sum(W0d.data_ptr(), b0d.data_ptr(), H, n_rows, idd.data_ptr(), n, F, out.data_ptr(), st) == 0, lib.rbm_last_error()
    got = out.cpu().numpy().astype(np.float64)
    print("bag_sum H=%d F=%d: worst error / bound %.3f" % (H, F, (np.abs(got - ref) / bound).max()))
    assert (np.abs(got - ref) <= bound).all()
    assert np.array_equal(got[-1], b0)        # the all -1 row: the bias alone


@pytest.mark.parametrize("n,a,b", [(3, 1, 1), (5, 300, 257)])
def test_affine_and_sigmoid(built, n, a, b):
    """rbm_affine, then rbm_sigmoid in place on its output: 4 (a + 1) 2^-24 sum |products| before the sigmoid, a quarter of it plus the
    evaluation's own 8 * 2^-24 after.  Measured: at most 0.076 of the bound before the sigmoid, 0.096 after."""
    torch, dev, st = _dev()
    lib = _capi.load()
    rng = np.random.RandomState(a + b)
    x, W, bias = pr.r32(rng.uniform(-1, 1, (n, a))), pr.r32(rng.uniform(-1, 1, (a, b))), pr.r32(rng.uniform(-1, 1, b))
    ref, bound = pr.affine_ref(x, W, bias)
    out = torch.full((n, b), 7.0, dtype=torch.float32, device=dev)
    xd, Wd, bd = _t(x), _t(W), _t(bias)
    assert lib.rbm_affine(xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), n, a, b, out.data_ptr(), st) == 0, lib.rbm_last_error()
    got = out.cpu().numpy().astype(np.float64)
    print("affine %dx%dx%d: worst error / bound %.3f" % (n, a, b, (np.abs(got - ref) / bound).max()))
    assert (np.abs(got - ref) <= bound).all()
    assert lib.rbm_sigmoid(out.data_ptr(), n * b, st) == 0, lib.rbm_last_error()
    got = out.cpu().numpy().astype(np.float64)
    sref = 1.0 / (1.0 + np.exp(-ref))
    print("   then sigmoid: worst error / bound %.3f" % (np.abs(got - sref) / pr.sigmoid_bound(bound)).max())
    assert (np.abs(got - sref) <= pr.sigmoid_bound(bound)).all()


@pytest.mark.parametrize("count", [1, 257])
def test_sigmoid(built, count):
    """rbm_sigmoid on exact inputs, +-100 and 0 among them: the evaluation's own rounding only (sigmoid(0) = 1/2 exactly; expf(100)
    overflows to inf and gives 0 where float64 gives 3.7e-44; the element past `count` stays as it was).  Measured: 8.0e-8 at worst."""
    torch, dev, st = _dev()
    lib = _capi.load()
    x = pr.r32(np.random.RandomState(count).uniform(-12, 12, count + 1))
    x[0] = 0.0
    if count > 1:
        x[1], x[2], x[count - 1] = 100.0, -100.0, -30.0
    xd = _t(x)
    assert lib.rbm_sigmoid(xd.data_ptr(), count, st) == 0, lib.rbm_last_error()
    got = xd.cpu().numpy().astype(np.float64)
    with np.errstate(over='ignore'):
        ref = 1.0 / (1.0 + np.exp(-x[:count]))
    print("sigmoid count=%d: worst error %.2e (bound %.2e)" % (count, np.abs(got[:count] - ref).max(), pr.SIGMOID_OWN))
    assert (np.abs(got[:count] - ref) <= np.minimum(pr.SIGMOID_OWN, pr.SIGMOID_REL * ref + 1e-38)).all()
    assert got[0] == 0.5 and got[count] == x[count]
