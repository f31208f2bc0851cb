"""The inner-product step (include/ipnn_hip.h) at the shapes ipnn_create accepts beyond the default layout (16 fields, k = 11):
field counts 2..32, k = 1..16, with and without the pair products, against the float64 oracle (oracle/ipnn_oracle.py).

What depends on F and K is hand-written: k_ip_fwd's 17-float field stride, its pair walk and its slot -> reference map; k_ip_bwd's
closed-form pair index; ref0 (the slot -> reference column map the keep-mask transposition reads for layer 0); the table packing
into 16-float slots and its inverse; the sparse-row update and the dense Adam / FTRL pass over n_rows * 16.  The host picks its
path by the padded widths Dp = [rup(16 F + P + 2, 64), rup(h + 1, 64) .., 64], and every case id starts with the path the
restatement below predicts:
  strip      the strip kernels, f32 (maxD <= 1024: two LDS tiles of 64 KiB)
  strip-duo  the strip kernels with two workgroups per 32-example strip (bf16; at most 4096 examples on 256 CUs)
  gemm       one GEMM launch per product (a hidden layer > 1023, or IPNN_STRIP=0)
then Dp0 and whether k_ip_fwd / k_ip_bwd take more than 64 KiB of dynamic LDS (lds_ip = 16 (17 F + Dp0) 4 bytes: F >= 23 with
pairs, F >= 31 without).

Bounds are those of test_gpu_ipnn: test_ipnn_step_f32_vs_oracle for one f32 step, test_ipnn_bf16_wide_stack_tracks_oracle for
bf16, test_adam_steps_vs_oracle / test_ftrl_steps_vs_oracle for the optimisers, test_ipnn_many_steps_track_oracle for twelve
steps.  Each oracle case prints its worst error as a fraction of its bound.  Batches of 4096 step at lr = 0.001 (the loss is a
sum); hidden sizes stay small where they need not be wide, so that the float64 oracle stays quick.
"""
import contextlib

import numpy as np
import pytest

from oracle import ipnn_oracle as io

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.ipnn import FNN, FNN_IP_L3, IPNNEngine

pytestmark = pytest.mark.gpu

SLOT = 16
N_CU = 256          # MI355X


def rup(a, m):
    return (a + m - 1) // m * m


def npairs(F, pairs):
    return F * (F - 1) // 2 if pairs else 0


def d0_of(F, K, pairs):
    return F * K + npairs(F, pairs) + 1


def padded(F, hidden, pairs):
    """h->Dp of ipnn_create: layer 0 holds F slots of 16, the pair products, b and the ones column."""
    return [rup(SLOT * F + npairs(F, pairs) + 2, 64)] + [rup(h + 1, 64) for h in hidden] + [64]


def lds_ip(F, hidden, pairs):
    """Dynamic LDS of k_ip_fwd (and of k_ip_bwd, launched with the same size): the 17-float embedding tile plus layer 0."""
    return 16 * (F * (SLOT + 1) + padded(F, hidden, pairs)[0]) * 4


def path_of(F, hidden, pairs, prec, B, strip_env=True):
    """ip_run's choice: strip_lds = 2 RT 16 maxD sizeof(T) <= 128 KiB (RT = 2 for bf16), StripDuo for bf16 when both workgroups
    of every strip fit the chip (2 * Ba / 32 <= CUs)."""
    maxD = max(padded(F, hidden, pairs))
    RT, ts = (2, 2) if prec == 'bf16' else (1, 4)
    if not (strip_env and 2 * RT * 16 * maxD * ts <= 128 * 1024):
        return 'gemm'
    return 'strip-duo' if RT == 2 and 2 * (rup(B, 256) // 32) <= N_CU else 'strip'


def case_id(F, K, pairs, hidden, B, prec='f32', *rest, strip_env=True):
    Dp0 = padded(F, hidden, pairs)[0]
    s = '%s-F%d-K%d-%s-Dp0_%d-lds%s-H%s-B%d' % (path_of(F, hidden, pairs, prec, B, strip_env), F, K, 'P' if pairs else 'noP', Dp0,
                                               'GT64K' if lds_ip(F, hidden, pairs) > 64 * 1024 else 'LE64K',
                                               'x'.join(str(h) for h in hidden), B)
    return '-'.join([s] + [str(r) for r in rest if r not in (None, '')])


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def lr_for(B):
    return 0.001 if B >= 4096 else 0.01


@contextlib.contextmanager
def oracle_pairs(pairs):
    """pairs = 0 is the plain FNN class: the oracle's USE_PAIRS switch, restored afterwards."""
    io.USE_PAIRS = bool(pairs)
    try:
        yield
    finally:
        io.USE_PAIRS = True


def problem(F, K, B, hidden, pairs=True, seed=0, n_rows=600, keep_p=0.7):
    """test_gpu_ipnn.problem for any F, K and pairs.  Weights of layer t are uniform in +-min(0.3, 1.5 / sqrt(d_t)), so that
    pre-activations stay O(1) at 1009 inputs as they do at 297."""
    rng = np.random.RandomState(seed)
    sizes = synth.field_sizes_tiny(n_rows, n_fields=F)
    table = f32r(rng.standard_normal((sum(sizes), K)) * 0.2)
    ids = synth.zipf_ids(B, sizes, 1.1, seed + 1)
    y = (rng.uniform(size=B) < 0.3).astype(np.float64)
    y[0] = 1.0
    d = [d0_of(F, K, pairs)] + list(hidden) + [1]
    sc = [min(0.3, 1.5 / np.sqrt(d[i])) for i in range(len(d) - 1)]
    params = {'b': float(np.float32(0.1)), 'W': [f32r(rng.uniform(-sc[i], sc[i], (d[i], d[i + 1]))) for i in range(len(d) - 1)],
              'bias': [f32r(rng.uniform(-0.1, 0.1, d[i + 1])) for i in range(len(d) - 1)]}
    masks = [(rng.uniform(size=(B, d[t])) < keep_p).astype(np.uint8) for t in range(len(hidden) + 1)]
    return table, ids, y, params, masks, d


def copy_params(p):
    return {'b': p['b'], 'W': [w.copy() for w in p['W']], 'bias': [b.copy() for b in p['bias']]}


class Bounds(object):
    """Checks that keep the worst |got - ref| / bound seen (a bound of atol + rtol |ref|, elementwise)."""

    def __init__(self):
        self.worst, self.where = 0.0, ''

    def _keep(self, name, r):
        if not r <= self.worst:
            self.worst, self.where = r, name
        return r

    def close(self, name, got, ref, rtol, atol):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        r = self._keep(name, float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()) if got.size else 0.0)
        assert r <= 1.0, "%s: max error %.3g of its bound (max |d| %.3e)" % (name, r, float(np.abs(got - ref).max()))

    def above(self, name, got, floor, span):
        """got > floor, its fraction of the bound being (1 - got) / span (a cosine with floor 1 - span)."""
        r = self._keep(name, (1.0 - got) / span)
        assert got > floor, "%s: %.5f (floor %.3f)" % (name, got, floor)

    def report(self, label):
        print("\n[ipnn-shapes] %s: worst error %.3f of the bound (%s)" % (label, self.worst, self.where))


def cosine(a, b):
    a, b = a.ravel(), b.ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def check_f32_step(eng, prob, act, lr, drop, keep, pairs, label, bd=None):
    """test_ipnn_step_f32_vs_oracle's checks for any shape: predict before the step (rtol 2e-4), logits (rtol 2e-4, atol 2e-5),
    loss (5e-5 relative), every W, bias and b and every touched row within 2e-3 of its own change; untouched rows bit-unchanged."""
    table, ids, y, params, masks, d = prob
    bd = bd or Bounds()
    with oracle_pairs(pairs):
        bd.close('predict', eng.predict(ids).cpu().numpy(), io.predict(params, table, ids, act), 2e-4, 1e-6)
        out = eng.train_step(ids, y, masks if drop else None, want_logits=True)
        p0, t0 = copy_params(params), table.copy()
        loss, logits, _ = io.sgd_step(params, table, ids, y, act, lr, [m.astype(np.float64) for m in masks] if drop else None, keep)
    bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-4, 2e-5)
    bd.close('loss', out['loss'], loss, 0.0, 5e-5 * max(1.0, abs(loss)))
    b, Ws, bs = eng.get_params()
    for t in range(len(Ws)):
        bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 2e-3 * (np.abs(params['W'][t] - p0['W'][t]).max() + 1e-12) + 2e-7)
        bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 2e-3 * (np.abs(params['bias'][t] - p0['bias'][t]).max() + 1e-12) + 2e-7)
    bd.close('b', b, params['b'], 0.0, 2e-3 * abs(params['b'] - p0['b']) + 2e-7)
    rows = eng.get_rows(np.arange(table.shape[0]))
    touched = np.unique(ids)
    bd.close('table', rows[touched], table[touched], 0.0, 2e-3 * (np.abs(table - t0).max() + 1e-12) + 2e-7)
    untouched = np.setdiff1d(np.arange(table.shape[0]), touched)
    assert np.array_equal(rows[untouched], t0[untouched].astype(np.float32)), "a row no example touched moved"
    bd.report(label)
    return bd


# ------------------------------------------------------------------------------------------------ one f32 step, any shape
# (F, K, pairs, hidden, B, act, drop): F = 22 | 23 straddles lds_ip = 64 KiB with pairs, 30 | 31 without; F = 31 / 32 with pairs
# give Dp0 = 1024, the widest layer 0 the strip kernels take; a layer > 1023 sends F = 2 and F = 32 to the GEMM path
STEP = [
    (2, 1, 1, [40, 24], 17, 'relu', True), (2, 16, 1, [300, 100], 257, 'tanh', False), (2, 5, 1, [1100, 40], 33, 'sigmoid', True),
    (2, 11, 1, [64, 63], 4096, 'relu', True), (3, 2, 1, [30, 20], 257, 'sigmoid', True), (8, 11, 1, [130, 70, 40], 17, 'tanh', True),
    (13, 5, 1, [63], 257, 'relu', False), (17, 16, 1, [200, 100], 1, 'relu', True), (22, 1, 1, [100, 50], 257, 'tanh', True),
    (22, 16, 1, [50, 30, 10], 4096, 'sigmoid', False), (23, 1, 1, [100, 50], 17, 'relu', True),
    (23, 16, 1, [300, 100], 257, 'tanh', True), (24, 2, 1, [40], 257, 'relu', True), (31, 5, 1, [120, 60], 257, 'tanh', True),
    (32, 1, 1, [300, 100], 17, 'relu', True), (32, 16, 1, [100, 50, 25], 257, 'relu', True),
    (32, 16, 1, [1100, 40], 33, 'tanh', True), (32, 11, 1, [64], 4096, 'sigmoid', True), (32, 2, 1, [200], 1, 'tanh', False),
    # pairs = 0: the plain FNN class
    (2, 16, 0, [40, 20], 257, 'tanh', True), (2, 1, 0, [1100, 30], 17, 'relu', True), (30, 16, 0, [100, 50], 257, 'relu', True),
    (31, 16, 0, [100, 50], 257, 'sigmoid', True), (31, 3, 0, [40], 1, 'tanh', False), (32, 16, 0, [300, 100], 4096, 'tanh', True),
    (32, 1, 0, [64, 63], 17, 'relu', False),
]


@pytest.mark.parametrize("F,K,pairs,hidden,B,act,drop", STEP,
                         ids=[case_id(F, K, p, h, B, 'f32', a, 'drop' if dr else 'nodrop') for (F, K, p, h, B, a, dr) in STEP])
def test_ipnn_shape_step_f32_vs_oracle(built, F, K, pairs, hidden, B, act, drop):
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B)
    keep, lr = (0.7 if drop else 1.0), lr_for(B)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=lr, keep_prob=keep, pairs=bool(pairs))
    try:
        assert eng.d == prob[5]
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, act, lr, drop, keep, pairs, case_id(F, K, pairs, hidden, B, 'f32', act))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the in-line GEMM path
ALT = [(2, 1, 1, [40, 24], 257, 'relu'), (2, 16, 0, [100, 30], 300, 'tanh'), (23, 3, 1, [130, 60], 300, 'tanh'),
       (23, 16, 1, [300, 100], 17, 'sigmoid'), (32, 16, 1, [300, 100], 300, 'relu'), (32, 5, 0, [100, 50], 257, 'relu')]


@pytest.mark.parametrize("F,K,pairs,hidden,B,act", ALT,
                         ids=[case_id(F, K, p, h, B, 'f32', a, 'strip0', strip_env=False) for (F, K, p, h, B, a) in ALT])
def test_ipnn_shape_step_without_strips_or_side_stream(built, monkeypatch, F, K, pairs, hidden, B, act):
    """The same step with IPNN_STRIP=0, IPNN_SIDE_STREAM=0 (one GEMM launch per product, everything in line on one stream) and in
    the default form: both against the oracle."""
    for env in ({}, {'IPNN_STRIP': '0', 'IPNN_SIDE_STREAM': '0'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        prob = problem(F, K, B, hidden, pairs, seed=7 * F + K)
        eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=0.01, keep_prob=0.7, pairs=bool(pairs))
        try:
            eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
            check_f32_step(eng, prob, act, 0.01, True, 0.7, pairs, case_id(F, K, pairs, hidden, B, 'f32', act, 'strip0' if env else 'default',
                                                                           strip_env=not env))
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------ StripDuo at maxD = 1024
DUO = [(32, 16, 1), (2, 1, 1), (32, 16, 0)]


@pytest.mark.parametrize("F,K,pairs", DUO, ids=[case_id(F, K, p, [1000, 300], 4096, 'bf16') for (F, K, p) in DUO])
def test_strip_pairs_bit_identical_at_widest_layer0(built, monkeypatch, F, K, pairs):
    """test_strip_pairs_are_bit_identical_to_single_strips at a layer 0 of 1024 (F = 32 with pairs), 576 (F = 32 without) or 64
    (F = 2) padded columns and a stack whose widest layer pads to exactly 1024 (maxD = 1024, the strip kernels' limit): bf16, batch 4096, three steps with
    dropout; logits, every dense tensor, b and the touched rows BIT-equal with and without StripDuo."""
    hidden, B, steps = [1000, 300], 4096, 3
    assert max(padded(F, hidden, pairs)) == 1024 and path_of(F, hidden, pairs, 'bf16', B) == 'strip-duo'
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, pairs, seed=77 + F, n_rows=3000, keep_p=0.5)
    res = []
    for duo in ('1', '0'):
        monkeypatch.setenv('IPNN_STRIP_DUO', duo)
        eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=0.001, keep_prob=0.5, pairs=bool(pairs))
        try:
            eng.set_params(table, params['b'], params['W'], params['bias'])
            logits = []
            for s in range(steps):
                sl = slice(s * B, (s + 1) * B)
                out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
                logits.append(out['logits'].cpu().numpy().copy())
            b, Ws, bs = eng.get_params()
            res.append((np.concatenate(logits), b, Ws, bs, eng.get_rows(np.unique(ids))))
        finally:
            eng.close()
    (la, ba, Wa, bsa, ra), (lb, bb, Wb, bsb, rb) = res
    assert np.isfinite(la).all() and np.abs(la).max() > 0
    assert np.array_equal(la, lb) and ba == bb and np.array_equal(ra, rb)
    for t in range(len(Wa)):
        assert np.array_equal(Wa[t], Wb[t]) and np.array_equal(bsa[t], bsb[t]), t


# ------------------------------------------------------------------------------------------------ one bf16 step
BF16 = [(2, 1, 1, [400, 200]), (2, 16, 1, [400, 200]), (23, 1, 1, [400, 200]), (23, 16, 1, [400, 200]), (32, 1, 1, [400, 200]),
        (32, 16, 1, [400, 200]), (32, 16, 1, [1100, 100]), (31, 16, 0, [400, 200])]


@pytest.mark.parametrize("F,K,pairs,hidden", BF16, ids=[case_id(F, K, p, h, 1024, 'bf16') for (F, K, p, h) in BF16])
def test_ipnn_shape_step_bf16_tracks_oracle(built, F, K, pairs, hidden):
    """test_ipnn_bf16_wide_stack_tracks_oracle's bounds: logits within 5e-2, loss within 2 %, every weight update's cosine with
    the oracle's > 0.99."""
    B = 1024
    table, ids, y, params, masks, d = problem(F, K, B, hidden, pairs, seed=11 + F + K)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='bf16', lr=0.01, keep_prob=0.7, pairs=bool(pairs))
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        out = eng.train_step(ids, y, masks, want_logits=True)
        p0 = [w.copy() for w in params['W']]
        with oracle_pairs(pairs):
            loss, logits, _ = io.sgd_step(params, table, ids, y, 'relu', 0.01, [m.astype(np.float64) for m in masks], 0.7)
        bd = Bounds()
        bd.close('logits', out['logits'].cpu().numpy(), logits, 0.0, 5e-2)
        bd.close('loss', out['loss'], loss, 0.0, 2e-2 * abs(loss))
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.above('cos W%d' % t, cosine(Ws[t] - p0[t], params['W'][t] - p0[t]), 0.99, 0.01)
        bd.report(case_id(F, K, pairs, hidden, B, 'bf16'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ Adam and FTRL, five steps
OPT = [(23, 3, 'adam'), (32, 16, 'adam'), (23, 3, 'ftrl'), (32, 16, 'ftrl')]


@pytest.mark.parametrize("F,K,opt", OPT, ids=[case_id(F, K, 1, [40, 24, 12], 160, 'f32', o) for (F, K, o) in OPT])
def test_ipnn_shape_optimiser_steps_vs_oracle(built, F, K, opt):
    """Five Adam / FTRL steps, each on a batch of its own, so that rows touched by an early step only keep moving through the dense
    pass over n_rows x 16 (Adam: its moments; FTRL: re-derived from the linear term) -- bounds of test_adam_steps_vs_oracle /
    test_ftrl_steps_vs_oracle.  Every row, touched or not, follows the oracle's dense pass; a row no step touched is bit-unchanged
    under Adam and exactly 0 under FTRL."""
    hidden, B, steps = [40, 24, 12], 160, 5
    table, ids, y, params, masks, d = problem(F, K, B * steps, hidden, True, seed=21 + F + K)
    lr = 1e-3 if opt == 'adam' else 1e-2
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=lr, keep_prob=0.7, optimizer=opt, adam_eps=1e-8)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        st = io.adam_state(params, table) if opt == 'adam' else io.ftrl_state(params, table)
        t0, W0 = table.copy(), [w.copy() for w in params['W']]
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            out = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
            m64 = [m[sl].astype(np.float64) for m in masks]
            if opt == 'adam':
                loss, logits, _ = io.adam_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 5e-4, 5e-5)
            else:
                loss, logits, _ = io.ftrl_step(params, table, ids[sl], y[sl], 'relu', lr, st, m64, 0.7)
                bd.close('logits%d' % s, out['logits'].cpu().numpy(), logits, 2e-3, 2e-5)
                bd.close('loss%d' % s, out['loss'], loss, 0.0, 1e-4 * abs(loss))
        b, Ws, bs = eng.get_params()
        rows = eng.get_rows(np.arange(table.shape[0]))
        never = np.setdiff1d(np.arange(table.shape[0]), np.unique(ids))
        early = np.setdiff1d(np.unique(ids[:B]), np.unique(ids[B:]))       # touched by the first step only
        assert len(never) > 0 and len(early) > 0
        if opt == 'adam':
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - W0[t]).max() + 1e-7)
            ct = np.abs(table - t0).max()
            bd.close('table', rows, table, 0.0, 5e-3 * ct + 1e-7)
            bd.close('early rows', rows[early], table[early], 0.0, 5e-3 * ct + 1e-7)
            assert np.abs(table[early] - t0[early]).max() > 0 and np.abs(rows[early] - t0[early]).max() > 0
            assert np.array_equal(rows[never], t0[never].astype(np.float32))
        else:
            for t in range(len(Ws)):
                bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t]).max() + 1e-7)
                bd.close('bias%d' % t, bs[t], params['bias'][t], 0.0, 5e-3 * np.abs(params['bias'][t]).max() + 1e-7)
            bd.close('b', b, params['b'], 0.0, 5e-3 * abs(params['b']) + 1e-7)
            bd.close('table', rows, table, 0.0, 5e-3 * np.abs(table).max() + 1e-7)
            bd.close('early rows', rows[early], table[early], 0.0, 5e-3 * np.abs(table).max() + 1e-7)
            assert not rows[never].any()
        bd.report(case_id(F, K, 1, hidden, B, 'f32', opt))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ twelve steps
def test_ipnn_many_steps_at_32_fields_k5(built):
    """test_ipnn_many_steps_track_oracle at F = 32, K = 5 (Dp0 = 1024, lds_ip > 64 KiB): twelve SGD steps with fresh masks and
    batch lengths; the side-stream work of one step overlaps the next step's start."""
    F, K, hidden = 32, 5, [130, 70, 40]
    table, _, _, params, _, d = problem(F, K, 8, hidden, True, seed=31)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=0.02, keep_prob=0.7)
    bd = Bounds()
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        p0, t0 = [w.copy() for w in params['W']], table.copy()
        rng = np.random.RandomState(77)
        sizes = synth.field_sizes_tiny(600, n_fields=F)
        touched = set()
        for step in range(12):
            B = int(rng.randint(60, 201))
            ids = synth.zipf_ids(B, sizes, 1.1, 100 + step)
            y = (rng.uniform(size=B) < 0.3).astype(np.float64)
            masks = [(rng.uniform(size=(B, d[t])) < 0.7).astype(np.uint8) for t in range(len(hidden) + 1)]
            out = eng.train_step(ids, y, masks, want_logits=(step == 11))
            loss, logits, _ = io.sgd_step(params, table, ids, y, 'relu', 0.02, [m.astype(np.float64) for m in masks], 0.7)
            touched |= set(np.unique(ids).tolist())
        bd.close('logits', out['logits'].cpu().numpy(), logits, 2e-3, 2e-4)
        b, Ws, bs = eng.get_params()
        for t in range(len(Ws)):
            bd.close('W%d' % t, Ws[t], params['W'][t], 0.0, 5e-3 * np.abs(params['W'][t] - p0[t]).max() + 1e-6)
        tr = np.array(sorted(touched))
        bd.close('table', eng.get_rows(tr), table[tr], 0.0, 5e-3 * np.abs(table - t0).max() + 1e-6)
        bd.report(case_id(F, K, 1, hidden, 200, 'f32', '12steps'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ round trips
RT_CASES = [(2, 1, 1), (2, 16, 1), (32, 1, 1), (32, 16, 1), (32, 16, 0)]


@pytest.mark.parametrize("F,K,pairs", RT_CASES, ids=[case_id(F, K, p, [64, 63], 257, 'f32') for (F, K, p) in RT_CASES])
def test_ipnn_set_get_roundtrip_and_zero_lr_bit_exact(built, F, K, pairs):
    """set_params then get_params / get_rows returns every value bit for bit (the packing of a row into its 16-float slot and
    back: at K = 16 the row fills the slot, at K = 1 it is w alone); a step at lr = 0 leaves the table, W, biases and b bit-unchanged."""
    hidden, B = [64, 63], 257
    table, ids, y, params, masks, d = problem(F, K, B, hidden, pairs, seed=5 * F + K)
    eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=B, precision='f32', lr=0.0, keep_prob=0.7, pairs=bool(pairs))
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        t32 = table.astype(np.float32)
        for when in ('set', 'lr0'):
            b, Ws, bs = eng.get_params()
            assert b == np.float32(params['b']), when
            for t in range(len(Ws)):
                assert np.array_equal(Ws[t], params['W'][t].astype(np.float32)), (when, t)
                assert np.array_equal(bs[t], params['bias'][t].astype(np.float32)), (when, t)
            assert np.array_equal(eng.get_rows(np.arange(table.shape[0])), t32), when
            sel = np.array([table.shape[0] - 1, 0, 5, 0, table.shape[0] - 1])        # any order, repeats
            assert np.array_equal(eng.get_rows(sel), t32[sel]), when
            if when == 'set':
                out = eng.train_step(ids, y, masks, want_logits=True)
                assert np.isfinite(out['logits'].cpu().numpy()).all() and np.isfinite(out['loss'])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ predict and evaluate
def test_ipnn_predict_and_eval_vs_sklearn_at_32_fields(built):
    """predict over 2,501 examples at max_batch 1000 (chunks of 1000, 1000 and 501) against the oracle, and ipnn_eval's AUC / RMSE /
    logloss against sklearn on the same float32 predictions at 1e-12 (test_eval_metrics_equal_sklearn_at_39_fields)."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    F, K, hidden, N = 32, 16, [300, 100], 2501
    table, ids, y, params, masks, d = problem(F, K, N, hidden, True, seed=78)
    params['W'][-1] *= 10.0                                 # spread the predictions away from 0.5
    yy = (np.random.RandomState(6).uniform(size=N) < 0.3).astype(np.int32)
    eng = IPNNEngine(F, K, hidden, 'tanh', max_batch=1000, precision='f32', lr=0.01, keep_prob=1.0)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        pp = eng.predict(ids).cpu().numpy()
        bd = Bounds()
        bd.close('predict', pp, io.predict(params, table, ids, 'tanh'), 2e-4, 1e-6)
        bd.report(case_id(F, K, 1, hidden, 1000, 'f32', 'predict-N2501'))
        m = eng.evaluate(ids, yy)
        p64 = pp.astype(np.float64)
        assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
        assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
        assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 64-bit sort keys
def test_ipnn_step_with_64bit_sort_keys_at_32_fields(built):
    """n_rows * 4096 > 2^32 (n_rows >= 1,048,576) makes the id grouping of the sparse-row update sort 64-bit keys (key64).  One
    f32 SGD step at F = 32, K = 5 on 1.1 M rows with Zipf ids (duplicates in every field): the f32 step bounds, every untouched row
    bit-unchanged."""
    F, K, hidden, B = 32, 5, [64, 32], 512
    n_rows = 1100000
    assert n_rows * 4096 > 2 ** 32
    prob = problem(F, K, B, hidden, True, seed=91, n_rows=n_rows)
    ids = prob[1]
    assert ids.max() > 2 ** 20 and len(np.unique(ids)) < ids.size
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=B, precision='f32', lr=0.01, keep_prob=0.7)
    try:
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        check_f32_step(eng, prob, 'relu', 0.01, True, 0.7, True, case_id(F, K, 1, hidden, B, 'f32', 'key64'))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the family classes
@pytest.mark.parametrize("cls", [FNN_IP_L3, FNN], ids=['FNN_IP_L3-F23-K1', 'FNN-F23-K1'])
def test_family_class_at_23_fields_rank_0(built, tmp_path, cls):
    """The reference's constructors at X_feas = 23, rank = 0 (K = 1: every pair product is w_i w_j): the layer widths, one f32
    step against the oracle, and dump()'s shapes (h1_w has d[0] rows)."""
    import pickle
    F, K = 23, 1
    hidden = [40, 24, 12][:cls.N_HIDDEN]
    pairs = cls.PAIRS
    B = 200
    table, ids, y, params, masks, d = problem(F, K, B, hidden, pairs, seed=23)
    m = cls(None, None, B, [table.shape[0], F, 0] + hidden + ['tanh'], ['uniform', -0.01, 0.01, [1, 2, 3, 4, 5], None],
            ['sgd', 0.01, 'sum'], [0.8], 'train', 0, precision='f32')
    try:
        assert m.eng.d == d and m.eng.K == 1
        m.eng.set_params(table, params['b'], params['W'], params['bias'])
        check_f32_step(m.eng, (table, ids, y, params, masks, d), 'tanh', 0.01, True, 0.8, pairs,
                       '%s-%s' % (cls.__name__, case_id(F, K, pairs, hidden, B, 'f32')))
        m.dump(str(tmp_path / 'm.pickle'))
        vm = pickle.load(open(tmp_path / 'm.pickle', 'rb'))
        assert set(vm) == {'W', 'V', 'b'} | {'h%d_%s' % (i, s) for i in range(1, len(d)) for s in 'wb'}
        assert vm['W'].shape == (table.shape[0], 1) and vm['V'].shape == (table.shape[0], 0)
        assert vm['h1_w'].shape == (d[0], hidden[0]) and d[0] == F + (F * (F - 1) // 2 if pairs else 0) + 1
        np.testing.assert_array_equal(vm['W'][:, 0], m.eng.get_rows(np.arange(table.shape[0]))[:, 0])
    finally:
        m.eng.close()
