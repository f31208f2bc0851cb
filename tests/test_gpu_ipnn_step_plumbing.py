"""The host side of the inner-product step (ipnn_api.hip: the per-handle step plan, the kernel selectors, the side-stream scope)
at what the launch-form tests of test_gpu_ipnn.py do not reach: every handle kind (narrow rows, wide rows, many fields) on the
smallest stack that has a wide product AND a tail, with value weights and with the library's drawn masks, held against the knobs
that take the split forms away; the GEMM path and the one-launch-per-product weight gradients against the default form; a refused
call followed by a good one; batch lengths that change on one handle.

The stack: bf16, hidden [300, 70] -- padded widths 320 and 128 (5 and 2 column blocks of 64), so with IPNN_DUO_MIN's default of 5
the cut is 1 < L = 2: product 1 runs as pairs of 32-example strips, products 2 and 3 as the 16-example tail.  B = 300 pads to 512:
16 strips (pairs fit the chip), the last one ragged.  The knobs only regroup launches, never sums, so everything is held to bits;
where sums ARE regrouped (IPNN_STRIP=0, IPNN_GROUP_WGRAD=0: f32 handles) the bound is test_ipnn_alternative_paths_match_oracle's.
"""
import ctypes as C

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import Drawn, IPNNEngine

from test_gpu_ipnn_shapes import problem

pytestmark = pytest.mark.gpu

HIDDEN, B, STEPS = [300, 70], 300, 2
KINDS = {'narrow': (16, 11), 'wide': (4, 20), 'many': (40, 4)}          # (fields, k): k_ip_fwd / k_ip_fwd_w / k_ip_bwd_m
KNOBS = [{'IPNN_TAIL_FUSE': '0'}, {'IPNN_TAIL_SPLIT': '0'}, {'IPNN_STRIP_DUO': '0'}, {'IPNN_SIDE_STREAM': '0'}]


def weights_of(ids, seed):
    """Value weights [B, F]: f32 values around 1, a few exact zeros and ones (numeric fields carry values, categorical ones 1)."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.25, 1.75, ids.shape).astype(np.float32)
    w[rng.uniform(size=ids.shape) < 0.1] = 1.0
    w[rng.uniform(size=ids.shape) < 0.05] = 0.0
    return w


def run(prob, F, K, feed, prec='bf16', opt='sgd', steps=STEPS, lr=0.01, act='relu'):
    """`steps` training steps on slices of the problem, then predict on the last slice's ids: everything a step leaves behind."""
    table, ids, y, params, masks, d = prob
    n = ids.shape[0] // steps
    eng = IPNNEngine(F, K, HIDDEN, act, max_batch=n, precision=prec, lr=lr, keep_prob=0.5, optimizer=opt)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        wts = weights_of(ids, 5) if feed == 'wts' else None
        logits = []
        for s in range(steps):
            sl = slice(s * n, (s + 1) * n)
            m = Drawn(1234, s) if feed == 'drawn' else [mm[sl] for mm in masks]
            out = eng.train_step(ids[sl], y[sl], m, want_logits=True, wts=None if wts is None else wts[sl])
            logits.append(out['logits'].cpu().numpy().copy())
        pr = eng.predict(ids[sl], wts=None if wts is None else wts[sl]).cpu().numpy().copy()
        b, Ws, bs = eng.get_params()
        return {'logits': np.concatenate(logits), 'b': b, 'W': Ws, 'bias': bs, 'rows': eng.get_rows(np.unique(ids)), 'p': pr}
    finally:
        eng.close()


def assert_bits(got, ref, label):
    assert np.isfinite(ref['logits']).all() and np.abs(ref['logits']).max() > 0, label
    assert np.array_equal(got['logits'], ref['logits']), (label, 'logits')
    assert got['b'] == ref['b'], (label, 'b')
    assert np.array_equal(got['rows'], ref['rows']), (label, 'rows')
    assert np.array_equal(got['p'], ref['p']), (label, 'predict')
    for t in range(len(ref['W'])):
        assert np.array_equal(got['W'][t], ref['W'][t]) and np.array_equal(got['bias'][t], ref['bias'][t]), (label, 'layer', t)


_PROB, _DEFAULT = {}, {}


def prob_of(kind, steps=STEPS, n=B):
    key = (kind, steps, n)
    if key not in _PROB:
        F, K = KINDS[kind]
        _PROB[key] = problem(F, K, n * steps, HIDDEN, seed=31 + F, n_rows=900, keep_p=0.5)
    return _PROB[key]


def default_of(kind, feed):
    """The default form's result, computed once per (kind, feed) with no knob set and shared by the knobs' cases."""
    if (kind, feed) not in _DEFAULT:
        F, K = KINDS[kind]
        _DEFAULT[(kind, feed)] = run(prob_of(kind), F, K, feed)
    return _DEFAULT[(kind, feed)]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda e: '-'.join('%s=%s' % kv for kv in e.items()))
@pytest.mark.parametrize("feed", ['wts', 'drawn'])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_split_forms_off_are_bit_identical(built, monkeypatch, kind, feed, knob):
    """Every handle kind, fed value weights beside the caller's masks ('wts': the WV instantiations, k_mask_T) or the library's
    drawn masks ('drawn': k_mask_draw, the plain instantiations): the default form (pairs on product 1, fused tail, side stream)
    against two tail launches, no tail split, one workgroup per strip, and everything in line on one stream."""
    F, K = KINDS[kind]
    ref = default_of(kind, feed)
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    assert_bits(run(prob_of(kind), F, K, feed), ref, (kind, feed, knob))


def assert_close(got, ref, prob, label):
    """test_ipnn_alternative_paths_match_oracle's bound, against the default form instead of the oracle: logits rtol 5e-4 /
    atol 5e-5, every dense weight within 3e-3 of the largest change the steps made to that tensor, plus 3e-7."""
    params = prob[3]
    np.testing.assert_allclose(got['logits'], ref['logits'], rtol=5e-4, atol=5e-5, err_msg=str(label))
    for t in range(len(ref['W'])):
        cw = np.abs(ref['W'][t] - params['W'][t]).max() + 1e-12
        err = np.abs(got['W'][t] - ref['W'][t]).max()
        print('%s W%d: max |d| %.3e, bound %.3e' % (label, t, err, 3e-3 * cw + 3e-7))
        assert err <= 3e-3 * cw + 3e-7, (label, t)


def test_gemm_path_f32_against_the_default_form(built, monkeypatch):
    """f32, the same stack: one GEMM launch per product (IPNN_STRIP=0) against the strip kernels.  Both take their epilogues
    from the same builders; the sums are regrouped."""
    F, K = KINDS['narrow']
    prob = prob_of('narrow')
    ref = run(prob, F, K, 'masks', prec='f32')
    monkeypatch.setenv('IPNN_STRIP', '0')
    assert_close(run(prob, F, K, 'masks', prec='f32'), ref, prob, 'IPNN_STRIP=0')


def test_ungrouped_weight_gradients_adam_against_the_default_form(built, monkeypatch):
    """Adam, two steps: one launch per weight-gradient product (IPNN_GROUP_WGRAD=0, its own split-K) against the grouped launch:
    the slab offsets and the update's arguments come from the same plan."""
    F, K = KINDS['narrow']
    prob = prob_of('narrow')
    ref = run(prob, F, K, 'masks', prec='f32', opt='adam', lr=1e-3)
    monkeypatch.setenv('IPNN_GROUP_WGRAD', '0')
    assert_close(run(prob, F, K, 'masks', prec='f32', opt='adam', lr=1e-3), ref, prob, 'IPNN_GROUP_WGRAD=0')


def state_of(eng, n_rows):
    b, Ws, bs = eng.get_params()
    return {'b': b, 'W': Ws, 'bias': bs, 'table': eng.get_rows(np.arange(n_rows))}


def assert_state_bits(a, b, label):
    assert a['b'] == b['b'] and np.array_equal(a['table'], b['table']), label
    for t in range(len(a['W'])):
        assert np.array_equal(a['W'][t], b['W'][t]) and np.array_equal(a['bias'][t], b['bias'][t]), (label, t)


def fresh(F, K, max_batch, st):
    eng = IPNNEngine(F, K, HIDDEN, 'relu', max_batch=max_batch, precision='bf16', lr=0.01, keep_prob=0.5)
    eng.set_params(st['table'], st['b'], st['W'], st['bias'])
    return eng


@pytest.mark.parametrize("refusal", ['null-mask', 'B-too-long'])
def test_a_refused_step_leaves_the_handle_as_it_was(built, refusal):
    """A training step refused for its arguments (one NULL mask entry; B = max_batch + 1) returns FNN_ERR_ARG before anything is
    enqueued: the next step on that handle equals a fresh handle's first step, bit for bit."""
    import torch
    F, K = KINDS['narrow']
    table, ids, y, params, masks, d = prob_of('narrow', steps=1)
    st0 = {'b': params['b'], 'W': params['W'], 'bias': params['bias'], 'table': table}
    eng, ref = fresh(F, K, B, st0), fresh(F, K, B, st0)
    try:
        if refusal == 'null-mask':
            ids_t = torch.as_tensor(ids).to(eng.device, torch.int32).contiguous()
            y_t = torch.as_tensor(y).to(eng.device, torch.float32).contiguous()
            mts = [torch.as_tensor(m).to(eng.device) for m in masks]
            marr = (C.c_void_p * len(mts))(*[m.data_ptr() for m in mts])
            marr[1] = None
            torch.cuda.synchronize()
            rc = eng.lib.ipnn_train_step(eng.h, ids_t.data_ptr(), y_t.data_ptr(), B, marr, None, None)
            assert rc == _capi.FNN_ERR_ARG and b'null entry' in eng.lib.ipnn_last_error(eng.h)
        else:
            big = np.concatenate([ids, ids[:1]])
            with pytest.raises(FNNError) as ei:
                eng.train_step(big, np.concatenate([y, y[:1]]), [np.concatenate([m, m[:1]]) for m in masks])
            assert ei.value.code == _capi.FNN_ERR_ARG
        got = eng.train_step(ids, y, masks, want_logits=True)
        want = ref.train_step(ids, y, masks, want_logits=True)
        assert np.array_equal(got['logits'].cpu().numpy(), want['logits'].cpu().numpy()) and got['loss'] == want['loss']
        assert_state_bits(state_of(eng, table.shape[0]), state_of(ref, table.shape[0]), refusal)
    finally:
        eng.close(); ref.close()


def test_batch_lengths_change_on_one_handle(built):
    """300, 17, 300 examples on one handle: each step equals a fresh handle's step of that length on a copy of the state -- what
    the handle keeps between calls (the step plan) holds nothing that depends on the batch length."""
    F, K = KINDS['narrow']
    table, ids, y, params, masks, d = prob_of('narrow', steps=3)
    n_rows = table.shape[0]
    st = {'b': params['b'], 'W': params['W'], 'bias': params['bias'], 'table': table}
    eng = fresh(F, K, B, st)
    try:
        lo = 0
        for n in (300, 17, 300):
            sl = slice(lo, lo + n)
            lo += n
            one = fresh(F, K, B, st)
            try:
                want = one.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
                got = eng.train_step(ids[sl], y[sl], [m[sl] for m in masks], want_logits=True)
                assert np.array_equal(got['logits'].cpu().numpy(), want['logits'].cpu().numpy()) and got['loss'] == want['loss'], n
                assert np.array_equal(eng.predict(ids[sl]).cpu().numpy(), one.predict(ids[sl]).cpu().numpy()), n
                st = state_of(eng, n_rows)
                assert_state_bits(st, state_of(one, n_rows), n)
            finally:
                one.close()
    finally:
        eng.close()
