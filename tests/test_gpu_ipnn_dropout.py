"""Drawn keep-masks of the inner-product family on the device (ipnn_train_step_drawn / ipnn_draw_masks, `masks=Drawn(seed, step)`
and IPNNEngine.draw_masks in deep_ctr_amd.ipnn).

1. ipnn_draw_masks equals the NumPy restatement (deep_ctr_amd.dropout.drawn_masks) byte for byte.
2. A drawn step equals, bit for bit, the mask-input step fed the arrays ipnn_draw_masks wrote: two handles from the same
   parameters, steps 5, 6, 7 of seed 99; logits and loss of every step, then every layer, bias, b and table row.  The cases span
   the paths a handle can take (strips, strip pairs, fused tail, GEMM per product, the many-field and wide inner-product kernels,
   both precisions, the optimisers, value weights, the mean loss, the stream / store knobs).
3. One drawn f32 step against the float64 oracle fed drawn_masks(...), under check_f32_step's own bounds.
4. Behaviour: reproducibility, another step, predict / evaluate afterwards, the error codes.

No tolerance anywhere but in 3: everything else is equality of bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, dropout
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import FNN, Drawn, IPNNEngine

import ipnn_weighted_ref as wr
from test_gpu_ipnn_shapes import check_f32_step, lr_for, problem

pytestmark = pytest.mark.gpu

SEED = 99
L7 = [1000, 800, 600, 400, 200, 100, 50]


# ------------------------------------------------------------------------------------------------ 1. the draw itself
# (F, k, pairs, hidden, B, keep)
DRAW = [
    (2, 1, 1, [64], 1, .5), (16, 11, 1, [300, 100], 257, .7), (16, 11, 0, [40], 4095, .5), (39, 11, 1, [60, 30], 17, .5),
    (64, 16, 1, [1100, 40], 4096, .7), (16, 51, 1, [130, 70], 300, .5), (32, 128, 1, [64, 63], 17, 1.0),
]


def _draw_id(c):
    F, K, p, h, B, kp = c
    return 'F%d-K%d-%s-H%s-B%d-keep%g' % (F, K, 'P' if p else 'noP', 'x'.join(map(str, h)), B, kp)


@pytest.mark.parametrize("F,K,pairs,hidden,B,keep", DRAW, ids=[_draw_id(c) for c in DRAW])
def test_draw_masks_equals_the_restatement(built, F, K, pairs, hidden, B, keep):
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=max(256, B), precision='f32', keep_prob=keep, pairs=bool(pairs))
    try:
        for step in (7, (1 << 32) + 7):
            got = [m.cpu().numpy() for m in eng.draw_masks(1234, step, B)]
            want = dropout.drawn_masks(1234, step, B, eng.d[:-1], keep)
            assert len(got) == len(hidden) + 1
            for t, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape == (B, eng.d[t]) and g.dtype == np.uint8
                assert np.array_equal(g, w), "layer %d of step %d: %d bytes differ" % (t, step, int((g != w).sum()))
        if keep < 1.0:
            assert not np.array_equal(got[0], dropout.drawn_masks(1234, 7, B, eng.d[:1], keep)[0]), "step 2^32 + 7 drew step 7's mask"
    finally:
        eng.close()


def test_draw_masks_skips_null_entries_and_leaves_the_rest_alone(built):
    """A NULL entry is skipped; no byte outside [B, d_t] is written (the arrays sit inside larger, poisoned ones)."""
    F, K, hidden, B = 16, 11, [70, 33], 67
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', keep_prob=0.5)
    try:
        n = [B * eng.d[t] for t in range(3)]
        bufs = [torch.full((n[t] + 512,), 0xAB, dtype=torch.uint8, device=eng.device) for t in range(3)]
        marr = (C.c_void_p * 3)(bufs[0].data_ptr() + 256, None, bufs[2].data_ptr() + 256)
        torch.cuda.synchronize()
        eng._ck(eng.lib.ipnn_draw_masks(eng.h, 5, 6, B, marr))
        eng.sync()
        want = dropout.drawn_masks(5, 6, B, eng.d[:-1], 0.5)
        for t in (0, 2):
            b = bufs[t].cpu().numpy()
            assert np.all(b[:256] == 0xAB) and np.all(b[256 + n[t]:] == 0xAB)
            assert np.array_equal(b[256:256 + n[t]].reshape(B, eng.d[t]), want[t])
        assert np.all(bufs[1].cpu().numpy() == 0xAB)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. drawn step == mask-input step
def _engines(F, K, hidden, B, prec, pairs, opt, reduce, keep, act, prob, lr):
    out = []
    for _ in range(2):
        eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision=prec, lr=lr, keep_prob=keep, pairs=bool(pairs),
                         optimizer=opt, reduce=reduce)
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        out.append(eng)
    return out


def _same_state(a, b, n_rows):
    ba, Wa, bsa = a.get_params()
    bb, Wb, bsb = b.get_params()
    assert np.float32(ba).tobytes() == np.float32(bb).tobytes(), "b"
    for t in range(len(Wa)):
        assert np.all(np.isfinite(Wa[t]))
        assert Wa[t].tobytes() == Wb[t].tobytes(), "W of layer %d" % (t + 1)
        assert bsa[t].tobytes() == bsb[t].tobytes(), "bias of layer %d" % (t + 1)
    ra, rb = a.get_rows(np.arange(n_rows)), b.get_rows(np.arange(n_rows))
    assert np.all(np.isfinite(ra))
    assert ra.tobytes() == rb.tobytes(), "table rows"


def twin(monkeypatch, F, K, pairs, hidden, B, prec, opt='sgd', reduce='sum', weighted=False, env=None, keep=0.5, act='relu',
         n_rows=600, ones=False, after=None):
    """Steps 5, 6, 7 of seed 99 on two handles: `Drawn` on one, the arrays of draw_masks (or, `ones`: explicit all-ones masks
    at keep_prob 1) on the other."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    prob = problem(F, K, B, hidden, pairs, seed=100 * F + K + B, n_rows=n_rows)
    table, ids, y = prob[0], prob[1], prob[2]
    wts = wr.test_weights(B, F, 7 * F + K + B) if weighted else None
    lr = {'sgd': lr_for(B), 'adam': 1e-3, 'ftrl': 1e-2}[opt]
    ea, eb = _engines(F, K, hidden, B, prec, pairs, opt, reduce, keep, act, prob, lr)
    try:
        moved = []
        for step in (5, 6, 7):
            if ones:
                masks = [np.ones((B, ea.d[t]), np.uint8) for t in range(len(hidden) + 1)]
            else:
                masks = eb.draw_masks(SEED, step, B)
                assert 0 < int(masks[0].sum()) < masks[0].numel(), "a mask with keep_prob < 1 that keeps all or nothing"
            oa = ea.train_step(ids, y, Drawn(SEED, step), want_logits=True, wts=wts)
            ob = eb.train_step(ids, y, masks, want_logits=True, wts=wts)
            la, lb = oa['logits'].cpu().numpy(), ob['logits'].cpu().numpy()
            assert np.all(np.isfinite(la)) and np.isfinite(oa['loss'])
            assert la.tobytes() == lb.tobytes(), "logits of step %d: %d of %d differ" % (step, int((la != lb).sum()), B)
            assert oa['loss'] == ob['loss'], "loss of step %d" % step
            moved.append(la)
        assert not np.array_equal(moved[0], moved[1]), "two steps with the same logits: nothing was learnt or drawn"
        _same_state(ea, eb, table.shape[0])
        if after:
            after(ea, eb, prob)
    finally:
        ea.close(); eb.close()


H = [300, 100]
# (F, K, pairs, hidden, B, prec, n_rows): strips, strip pairs (bf16) and the fused tail at four batch sizes; a layer above 1023
# units: one GEMM launch per product
BOTH = [(16, 11, 1, H, B, p, 600) for p in ('f32', 'bf16') for B in (1, 17, 257, 4096)] + \
       [(16, 11, 1, [1100, 100], 257, p, 600) for p in ('f32', 'bf16')]
# 39 fields with pairs: 16-example forward, 4-example backward (f16b4); 46: the 8-example forward (f8b4); 64 without pairs;
# wide rows; the plain FNN on wide rows; the reference's FNN_IP_L7 at its batch
F32 = [(39, 11, 1, [60, 30], 257, 'f32', 1500), (46, 16, 1, [50, 30], 257, 'f32', 1500), (64, 16, 0, [50, 20], 257, 'f32', 1500),
       (16, 51, 1, [100, 50], 257, 'f32', 600), (16, 101, 1, [100, 50], 17, 'f32', 600), (8, 101, 0, [64, 30], 257, 'f32', 600),
       (16, 11, 1, L7, 4096, 'f32', 600)]


def _twin_id(c):
    F, K, p, h, B, prec, _ = c
    return 'F%d-K%d-%s-H%s-B%d-%s' % (F, K, 'P' if p else 'noP', 'x'.join(map(str, h)), B, prec)


@pytest.mark.parametrize("F,K,pairs,hidden,B,prec,n_rows", BOTH + F32, ids=[_twin_id(c) for c in BOTH + F32])
def test_drawn_step_equals_mask_input_step(built, monkeypatch, F, K, pairs, hidden, B, prec, n_rows):
    twin(monkeypatch, F, K, pairs, hidden, B, prec, n_rows=n_rows)


@pytest.mark.parametrize("what", ['wts', 'adam', 'ftrl', 'mean'])
def test_drawn_step_equals_mask_input_step_bf16_variants(built, monkeypatch, what):
    kw = {'wts': dict(weighted=True), 'adam': dict(opt='adam'), 'ftrl': dict(opt='ftrl'), 'mean': dict(reduce='mean')}[what]
    twin(monkeypatch, 16, 11, 1, H, 257, 'bf16', **kw)


def test_drawn_step_equals_mask_input_step_f32_weighted_many_fields(built, monkeypatch):
    twin(monkeypatch, 39, 11, 1, [60, 30], 17, 'f32', weighted=True, n_rows=1500)


KNOB_ENVS = [{'IPNN_SIDE_STREAM': '0'}, {'IPNN_WT': '0'}, {'IPNN_MASK_SIDE': '1'}, {'IPNN_STRIP_DUO': '0'}]


@pytest.mark.parametrize("env", KNOB_ENVS, ids=['%s=%s' % next(iter(e.items())) for e in KNOB_ENVS])
def test_drawn_step_equals_mask_input_step_under_knobs(built, monkeypatch, env):
    twin(monkeypatch, 16, 11, 1, H, 257, 'bf16', env=env)


@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_keep_prob_one_drawn_equals_all_ones_masks(built, monkeypatch, prec):
    twin(monkeypatch, 16, 11, 1, H, 257, prec, keep=1.0, ones=True)


# ------------------------------------------------------------------------------------------------ 3. the oracle anchor
class _DrawnSteps(object):
    """An engine whose train_step draws: check_f32_step hands it the arrays it also feeds the oracle; the step itself takes only
    (seed, step)."""

    def __init__(self, eng, seed, step):
        self.eng, self.drawn = eng, Drawn(seed, step)

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def train_step(self, ids, y, masks=None, **kw):
        assert masks is not None
        return self.eng.train_step(ids, y, self.drawn, **kw)


def test_drawn_step_f32_vs_oracle(built):
    F, K, hidden, B, act, keep, step = 16, 11, H, 257, 'tanh', 0.5, 7
    table, ids, y, params, _, d = problem(F, K, B, hidden, True, seed=100 * F + K + B)
    lr = lr_for(B)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max(256, B), precision='f32', lr=lr, keep_prob=keep)
    try:
        assert eng.d == d
        eng.set_params(table, params['b'], params['W'], params['bias'])
        masks = dropout.drawn_masks(SEED, step, B, d[:-1], keep)
        check_f32_step(_DrawnSteps(eng, SEED, step), (table, ids, y, params, masks, d), act, lr, True, keep, True, 'drawn-F16-K11-H300x100-B257')
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. behaviour
def _fresh_run(prob, step, prec='bf16', B=257):
    eng = IPNNEngine(16, 11, H, 'relu', max_batch=256 if B <= 256 else 512, precision=prec, lr=0.01, keep_prob=0.5)
    try:
        eng.set_params(prob[0], prob[3]['b'], prob[3]['W'], prob[3]['bias'])
        out = eng.train_step(prob[1], prob[2], Drawn(SEED, step), want_logits=True)
        return out['logits'].cpu().numpy(), out['loss'], eng.get_params(), eng.get_rows(np.arange(prob[0].shape[0]))
    finally:
        eng.close()


def test_same_seed_and_step_on_fresh_handles_give_the_same_bits(built):
    prob = problem(16, 11, 257, H, True, seed=5)
    a, b, c = _fresh_run(prob, 5), _fresh_run(prob, 5), _fresh_run(prob, 6)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[3].tobytes() == b[3].tobytes()
    for Wa, Wb in zip(a[2][1], b[2][1]):
        assert Wa.tobytes() == Wb.tobytes()
    assert not np.array_equal(a[0], c[0]), "another step drew the same logits"


def test_predict_and_evaluate_after_drawn_steps_equal_the_twin(built, monkeypatch):
    def after(ea, eb, prob):
        ids, yy = prob[1], prob[2].astype(np.int32)
        pa, pb = ea.predict(ids).cpu().numpy(), eb.predict(ids).cpu().numpy()
        assert pa.tobytes() == pb.tobytes()
        assert ea.evaluate(ids, yy) == eb.evaluate(ids, yy)
    twin(monkeypatch, 16, 11, 1, H, 257, 'bf16', after=after)


def test_batch_outside_the_handle_is_refused(built):
    F, K, hidden = 16, 11, [64]
    table, ids, y, params, _, d = problem(F, K, 300, hidden, True, seed=3)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=0.01, keep_prob=0.5)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        ids_t = torch.as_tensor(ids).to(eng.device, torch.int32)
        y_t = torch.as_tensor(y).to(eng.device, torch.float32)
        mk = [torch.zeros((300, d[t]), dtype=torch.uint8, device=eng.device) for t in range(2)]
        marr = (C.c_void_p * 2)(*[m.data_ptr() for m in mk])
        torch.cuda.synchronize()
        for B in (0, -1, 257):
            assert eng.lib.ipnn_train_step_drawn(eng.h, ids_t.data_ptr(), None, y_t.data_ptr(), B, 1, 2, None, None) == _capi.FNN_ERR_ARG
            assert b'max_batch' in eng.lib.ipnn_last_error(eng.h)
            assert eng.lib.ipnn_draw_masks(eng.h, 1, 2, B, marr) == _capi.FNN_ERR_ARG
        assert eng.lib.ipnn_draw_masks(eng.h, 1, 2, 16, None) == _capi.FNN_ERR_ARG
        with pytest.raises(FNNError) as ei:
            eng.draw_masks(1, 2, 257)
        assert ei.value.code == _capi.FNN_ERR_ARG
        out = eng.train_step(ids[:256], y[:256], Drawn(1, 2))
        assert np.isfinite(out['loss'])
        assert all(int(m.sum()) == 0 for m in mk), "a refused ipnn_draw_masks wrote"
    finally:
        eng.close()


@pytest.mark.parametrize("F,K", [(16, 11), (16, 101)], ids=['narrow', 'wide'])
def test_out_of_range_id_in_a_drawn_step_is_reported(built, F, K):
    """An id outside [0, n_rows) in a drawn step is FNN_ERR_RANGE at the step's sync; the handle then steps on."""
    hidden, B = [64], 64
    table, ids, y, params, _, d = problem(F, K, B, hidden, True, seed=2)
    eng = IPNNEngine(F, K, hidden, 'relu', max_batch=256, precision='f32', lr=0.01, keep_prob=0.5)
    try:
        eng.set_params(table, params['b'], params['W'], params['bias'])
        bad = ids.copy()
        bad[5, 3] = table.shape[0] + 7
        with pytest.raises(FNNError) as ei:
            eng.train_step(bad, y, Drawn(SEED, 1))
        assert ei.value.code == _capi.FNN_ERR_RANGE
        out = eng.train_step(ids, y, Drawn(SEED, 2))
        assert np.isfinite(out['loss'])
    finally:
        eng.close()


def test_family_class_takes_drawn(built):
    """_IPFamily.train_step(ids, y, masks=Drawn(...), wts=...) reaches the drawn entry point: the plain FNN class, twice the
    same step from the same seeds gives the same loss, another step another loss."""
    F, rank, B = 8, 4, 64
    sizes = [40] * F
    X_dim = sum(sizes)
    rng = np.random.RandomState(4)
    ids = (rng.randint(0, 40, size=(B, F)) + np.arange(F) * 40).astype(np.int32)
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    wts = rng.uniform(0.5, 1.5, size=(B, F)).astype(np.float32)

    def loss_of(step):
        m = FNN(None, None, B, [X_dim, F, rank, 30, 20, 'relu'], ['uniform', -0.1, 0.1, [1, 2, 3, 4, 5, 6, 7, 8], None],
                ['sgd', 0.01, 'sum'], [0.5], precision='f32')
        try:
            return m.train_step(ids, y, masks=Drawn(SEED, step), wts=wts)['loss']
        finally:
            m.eng.close()
    a, b, c = loss_of(3), loss_of(3), loss_of(4)
    assert np.isfinite(a) and a == b and a != c
