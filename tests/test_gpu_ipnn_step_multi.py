"""ipnn_train_step_multi (include/ipnn_hip.h) through ipnn.train_step_many / ipnn.train_epoch_many: one mini-batch step of several
inner-product models on one feed in one call, against the solo steps of a second set of engines with the same parameters.
Every comparison against the solo engines is exact: np.array_equal on logits, dense tensors and touched rows, == on b and on
the losses.  The problems are test_gpu_ipnn_shapes.problem's, the engines test_gpu_ipnn_eval_multi.make's."""
import ctypes as C

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn
from deep_ctr_amd.engine import FNNError
from deep_ctr_amd.ipnn import Drawn, IPNNEngine

from test_gpu_ipnn_eval_multi import ACTS, close, feed, make, weights
from test_gpu_ipnn_shapes import check_f32_step, problem

pytestmark = pytest.mark.gpu

NAME = 'ipnn_train_step_multi'


def make_lk(F, K, hidden, prec, act, lr, keep, max_batch=256, seed=0, n_rows=600, **kw):
    """make() with a learning rate and a keep probability of the caller's (make fixes both)"""
    table, _, _, params, _, d = problem(F, K, 8, hidden, True, seed=seed, n_rows=n_rows)
    eng = IPNNEngine(F, K, hidden, act, max_batch=max_batch, precision=prec, lr=lr, keep_prob=keep, **kw)
    assert eng.d == d
    eng.set_params(table, params['b'], params['W'], params['bias'])
    return eng


def two_sets(build):
    """the same list of engines twice: one steps solo, one in group calls"""
    return build(), build()


def train_feed(F, B, n_rows=600, seed=77):
    ids, y = feed(F, B, n_rows=n_rows, seed=seed)
    return ids, y.astype(np.float32)


def masks_for(e, B, seed, keep_p=0.7):
    rng = np.random.RandomState(seed)
    return [(rng.uniform(size=(B, e.d[t])) < keep_p).astype(np.uint8) for t in range(len(e.hidden) + 1)]


def state(e, ids):
    b, Ws, bs = e.get_params()
    return b, Ws, bs, e.get_rows(np.unique(ids))


def assert_state_equal(a, g, ids, label):
    sa, sg = state(a, ids), state(g, ids)
    assert sa[0] == sg[0], '%s: b %r against %r' % (label, sg[0], sa[0])
    for t in range(len(sa[1])):
        assert np.array_equal(sa[1][t], sg[1][t]), '%s: W%d' % (label, t + 1)
        assert np.array_equal(sa[2][t], sg[2][t]), '%s: bias%d' % (label, t + 1)
    assert np.array_equal(sa[3], sg[3]), '%s: touched rows' % label


def step_both(solo, group, ids, y, masks=None, wts=None, label='', logits=True):
    """one step of every engine: solo calls on `solo`, one group call on `group`; losses, logits and parameters equal"""
    ref = [e.train_step(ids, y, masks[m] if masks else None, want_logits=logits, wts=wts) for m, e in enumerate(solo)]
    got = ipnn.train_step_many(group, ids, y, masks=masks, wts=wts, want_logits=logits)
    assert len(got) == len(group)
    for m in range(len(solo)):
        print("[ipnn-step-multi] %s model %d of %d, B = %d: loss %.9g (solo %.9g)" % (label, m, len(solo), len(y), got[m]['loss'], ref[m]['loss']))
        assert got[m]['loss'] == ref[m]['loss'], '%s model %d: loss %r against %r' % (label, m, got[m]['loss'], ref[m]['loss'])
        if logits:
            assert np.array_equal(got[m]['logits'].cpu().numpy(), ref[m]['logits'].cpu().numpy()), '%s model %d: logits' % (label, m)
        assert_state_equal(solo[m], group[m], ids, '%s model %d' % (label, m))
    return ref, got


# ------------------------------------------------------------------------------------------------ 1. one f32 class
@pytest.mark.parametrize("B", [10, 100, 256])
def test_one_f32_class(built, B):
    """no dropout, then the caller's masks, then Drawn with a different seed per model; three steps each"""
    solo, group = two_sets(lambda: [make_lk(4, 5, [40, 24], 'f32', ACTS[m], 0.01, 0.7, seed=10 + m) for m in range(3)])
    try:
        ids, y = train_feed(4, B)
        for s in range(3):
            step_both(solo, group, ids, y, None, label='plain step %d' % s)
        for s in range(3):
            step_both(solo, group, ids, y, [masks_for(e, B, 50 + 3 * s + m) for m, e in enumerate(solo)], label='masks step %d' % s)
        for s in range(3):
            step_both(solo, group, ids, y, [Drawn(1000 + m, s) for m in range(3)], label='drawn step %d' % s)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 2. bf16: pairs / tail split solo
@pytest.mark.parametrize("hidden", [[320, 40], [384, 64, 320, 40]], ids=['320x40', '384x64x320x40'])
@pytest.mark.parametrize("B", [100, 300])
def test_bf16_class_against_pairs_and_tail_split(built, B, hidden):
    """The solo step picks pairs, the tail split and the fused tail here (cut < L); the group runs single strips.  B = 300: a
    ragged last strip."""
    solo, group = two_sets(lambda: [make(4, 5, hidden, 'bf16', 'relu', max_batch=512, seed=20 + m) for m in range(4)])
    try:
        ids, y = train_feed(4, B)
        for s in range(2):
            step_both(solo, group, ids, y, [masks_for(e, B, 60 + 4 * s + m) for m, e in enumerate(solo)], label='%r step %d' % (hidden, s))
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 3. 16 fields, k = 11
def test_16_fields_bf16_four_lr_and_keep(built):
    lk = [(0.01, 0.5), (0.003, 0.7), (0.03, 0.9), (0.001, 1.0)]
    solo, group = two_sets(lambda: [make_lk(16, 11, [300, 100], 'bf16', ACTS[m % 3], lr, keep, seed=30 + m) for m, (lr, keep) in enumerate(lk)])
    try:
        ids, y = train_feed(16, 100)
        for s in range(5):
            step_both(solo, group, ids, y, [Drawn(7 + m, 100 + s) for m in range(4)], label='step %d' % s)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 4. a mixed list
def test_mixed_list_of_8_fields_with_weights(built):
    """narrow f32, narrow bf16, bf16 without pairs, wide rows (k = 20), a GEMM-path member (a hidden layer of 1100), a narrow member
    with max_batch = 512: the wide-row and GEMM-path members run their own steps inside the call."""
    def build():
        return [make(8, 5, [40, 24], 'f32', 'relu', seed=40), make(8, 5, [40, 24], 'bf16', 'tanh', seed=41),
                make(8, 5, [40, 24], 'bf16', 'sigmoid', pairs=False, seed=42), make(8, 20, [40, 24], 'f32', 'tanh', seed=43),
                make(8, 5, [1100, 40], 'f32', 'relu', seed=44), make(8, 5, [40, 24], 'f32', 'sigmoid', max_batch=512, seed=45)]
    solo, group = two_sets(build)
    try:
        ids, y = train_feed(8, 200)
        w = weights(ids)
        for s in range(2):
            step_both(solo, group, ids, y, [masks_for(e, 200, 70 + 6 * s + m) for m, e in enumerate(solo)], wts=w, label='weighted step %d' % s)
        step_both(solo, group, ids, y, None, label='unweighted')
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 5. optimisers
def test_sgd_adam_ftrl_in_one_class(built):
    def build():
        return [make(4, 5, [40, 24], 'f32', 'relu', seed=50, optimizer='sgd'), make(4, 5, [40, 24], 'f32', 'tanh', seed=51, optimizer='adam', reduce='mean'),
                make(4, 5, [40, 24], 'f32', 'sigmoid', seed=52, optimizer='ftrl'), make(4, 5, [40, 24], 'f32', 'relu', seed=53, optimizer='adam')]
    solo, group = two_sets(build)
    try:
        ids, y = train_feed(4, 100)
        for s in range(4):                          # the optimiser state shows in the steps that follow
            step_both(solo, group, ids, y, [masks_for(e, 100, 80 + 4 * s + m) for m, e in enumerate(solo)], label='step %d' % s)
    finally:
        close(solo + group)


@pytest.mark.parametrize("B", [100, 300])
def test_adam_and_ftrl_in_a_bf16_class(built, B):
    """The same in bf16, where the solo step runs pairs and the tail split (hidden 320 / 40: cut = 1 < L) and the group single
    strips: Adam, FTRL and SGD members through six steps with drawn masks, equality after every one."""
    opts = ['adam', 'ftrl', 'sgd', 'adam']
    solo, group = two_sets(lambda: [make_lk(4, 5, [320, 40], 'bf16', ACTS[m % 3], 0.01, 0.7, max_batch=512, seed=54 + m, optimizer=o)
                                    for m, o in enumerate(opts)])
    try:
        ids, y = train_feed(4, B)
        for s in range(6):
            step_both(solo, group, ids, y, [Drawn(20 + m, s) for m in range(4)], label='bf16 %s step %d' % ('/'.join(opts), s))
        other, yo = train_feed(4, B, seed=321)
        step_both(solo, group, other, yo, None, label='other ids, no dropout')
    finally:
        close(solo + group)


@pytest.mark.parametrize("prec", ['f32', 'bf16'])
def test_labels_that_are_not_0_or_1(built, prec):
    """y uniform in [0, 1]: the product z y of the loss is no longer exact, so a group kernel that fuses it where the solo kernel
    does not (or the other way round) shows in the loss."""
    solo, group = two_sets(lambda: [make_lk(4, 5, [40, 24], prec, ACTS[m], 0.01, 0.7, seed=64 + m, optimizer=o)
                                    for m, o in enumerate(['sgd', 'adam', 'sgd'])])
    try:
        ids, _ = train_feed(4, 250)
        y = np.random.RandomState(3).uniform(size=250).astype(np.float32)
        for s in range(4):
            step_both(solo, group, ids, y, [Drawn(30 + m, s) for m in range(3)], label='soft labels %s step %d' % (prec, s))
    finally:
        close(solo + group)


def test_device_tensors_of_other_types_are_converted_in_front_of_the_hand_shake(built):
    """y as int64 and as bool, masks as bool, ids as int64, all device tensors made on the caller's stream right before the
    call: their conversions are kernels on that stream, and the engines' streams wait behind them."""
    import torch
    solo, group = two_sets(lambda: [make_lk(4, 5, [40, 24], 'f32', ACTS[m], 0.01, 0.7, seed=57 + m) for m in range(3)])
    try:
        ids, y = train_feed(4, 256)
        dev = group[0].device
        for s in range(3):
            mk = [masks_for(e, 256, 90 + 3 * s + m) for m, e in enumerate(solo)]
            big = torch.randn(4096, 4096, device=dev)
            big = big @ big                                  # work in front of the conversions on the caller's stream
            ids_d = torch.as_tensor(ids).to(dev).to(torch.int64)
            y_d = torch.as_tensor(y).to(dev) > 0.5 if s % 2 else torch.as_tensor(y).to(dev).to(torch.int64)
            mk_d = [[torch.as_tensor(m).to(dev) != 0 for m in ms] for ms in mk]
            ref = [e.train_step(ids, y, mk[m], want_logits=True) for m, e in enumerate(solo)]
            got = ipnn.train_step_many(group, ids_d, y_d, masks=mk_d, want_logits=True)
            for m in range(3):
                assert got[m]['loss'] == ref[m]['loss'], 'step %d model %d: loss' % (s, m)
                assert np.array_equal(got[m]['logits'].cpu().numpy(), ref[m]['logits'].cpu().numpy()), 'step %d model %d: logits' % (s, m)
                assert_state_equal(solo[m], group[m], ids, 'step %d model %d' % (s, m))
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 6. grouping classes
def test_grouping_classes_and_stale_groupings(built):
    """n_rows 600, 600 and 900 on one feed with ids below 600: the two 600-row members share one grouping.  Member 1 was stepped
    solo on OTHER ids just before: a stale grouping or stale owner counts of its own buffers would show."""
    def build():
        return [make(4, 5, [40, 24], 'f32', ACTS[m], seed=60 + m, n_rows=n) for m, n in enumerate([600, 600, 900])]
    solo, group = two_sets(build)
    try:
        ids, y = train_feed(4, 200)
        other, yo = train_feed(4, 150, seed=123)
        for e in (solo[1], group[1], solo[2], group[2]):
            e.train_step(other, yo)
        for s in range(3):
            step_both(solo, group, ids, y, None, label='step %d' % s)
            for e in (solo[1], group[1]):
                e.train_step(other, yo)              # and a solo step between the group steps: the member's own grouping again
            assert_state_equal(solo[1], group[1], np.concatenate([ids, other]), 'after the solo step %d' % s)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 7. interleaving
def test_interleaved_with_solo_steps_and_evaluation(built):
    solo, group = two_sets(lambda: [make(4, 5, [40, 24], 'f32', ACTS[m], seed=70 + m) for m in range(3)])
    try:
        ids, y = train_feed(4, 100)
        yi = y.astype(np.int32)
        step_both(solo, group, ids, y, None, label='first')
        r1, g1 = solo[1].train_step(ids, y), group[1].train_step(ids, y)
        assert r1['loss'] == g1['loss']
        ev = ipnn.evaluate_many(group, ids, yi)
        for m, e in enumerate(solo):
            ref = e.evaluate(ids, yi)
            assert all(ev[m][k] == ref[k] for k in ('auc', 'rmse', 'logloss')), 'evaluate_many, model %d' % m
        step_both(solo[::-1], group[::-1], ids, y, None, label='reversed')
        assert np.array_equal(group[0].predict(ids).cpu().numpy(), solo[0].predict(ids).cpu().numpy())
        step_both(solo, group, ids, y, None, label='last')
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 8. deferred updates
def test_members_with_a_pending_side_update(built, monkeypatch):
    monkeypatch.setenv('IPNN_UPDATE_SIDE', '1')
    solo, group = two_sets(lambda: [make(4, 5, [40, 24], 'f32', ACTS[m], seed=80 + m) for m in range(3)])
    try:
        ids, y = train_feed(4, 100)
        for e in solo + group:
            e.train_step(ids, y, want_loss=False)   # leaves its dense update and sparse rows running on the side stream
        for s in range(2):
            step_both(solo, group, ids, y, None, label='step %d' % s)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 9. one model
def test_one_model_is_the_solo_step(built):
    solo, group = two_sets(lambda: [make_lk(4, 5, [40, 24], 'f32', 'tanh', 0.01, 0.7, seed=90)])
    try:
        ids, y = train_feed(4, 100)
        step_both(solo, group, ids, y, None, label='plain')
        step_both(solo, group, ids, y, [masks_for(solo[0], 100, 91)], label='masks')
        step_both(solo, group, ids, y, [Drawn(5, 6)], label='drawn')
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 10. without the loss
def test_without_loss_then_sync(built):
    solo, group = two_sets(lambda: [make(4, 5, [40, 24], 'f32', ACTS[m], seed=100 + m) for m in range(3)])
    try:
        ids, y = train_feed(4, 100)
        for s in range(2):
            for e in solo:
                e.train_step(ids, y, want_loss=False)
            out = ipnn.train_step_many(group, ids, y, want_loss=False)
            assert all(o['loss'] is None and o['logits'] is None for o in out)
        for e in solo + group:
            e.sync()
        for m in range(3):
            assert_state_equal(solo[m], group[m], ids, 'model %d' % m)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 11. the whole-list grid dimension
def test_64_models_in_one_call(built):
    solo, group = two_sets(lambda: [make(4, 5, [40, 24], 'f32', ACTS[m % 3], seed=200 + m) for m in range(64)])
    try:
        ids, y = train_feed(4, 10)
        ref = [e.train_step(ids, y, want_logits=True) for e in solo]
        got = ipnn.train_step_many(group, ids, y, want_logits=True)
        for m in range(64):
            assert got[m]['loss'] == ref[m]['loss'], 'model %d: loss' % m
            assert np.array_equal(got[m]['logits'].cpu().numpy(), ref[m]['logits'].cpu().numpy()), 'model %d: logits' % m
        for m in (0, 1, 31, 62, 63):
            assert_state_equal(solo[m], group[m], ids, 'model %d' % m)
        b_s = [e.get_params()[0] for e in solo]
        b_g = [e.get_params()[0] for e in group]
        assert b_s == b_g
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 12. refusals
def test_refusals_leave_every_member_untouched(built):
    """Every refusal of the header's list but one: a member whose strip pair gave up earlier (FNN_ERR_STATE) would need a pair
    that fails, which no test provokes."""
    engs =[make(4, 5, [40, 24], 'f32', ACTS[m], seed=300 + m) for m in range(3)]
    other_f = make(5, 5, [40, 24], 'f32', 'relu', seed=303)
    no_table = make(4, 5, [40, 24], 'f32', 'relu', seed=304, set_params=False)
    try:
        e0 = engs[0]
        lib, torch = e0.lib, e0._torch
        ids, y = train_feed(4, 100)
        ids_t, y_t = e0._dev(ids, torch.int32), e0._dev(y, torch.float32)
        big = e0._dev(np.zeros((300, 4), np.int32), torch.int32)
        mk = [e0._dev(m, torch.uint8) for m in masks_for(e0, 100, 1)]
        before = [state(e, ids) for e in engs]

        def hs_of(es):
            return (C.c_void_p * len(es))(*[e.h.value if e is not None else None for e in es])

        def rows_of(ptrs):
            return (C.c_void_p * len(ptrs))(*ptrs)
        full = rows_of([m.data_ptr() for m in mk])
        holed = rows_of([mk[0].data_ptr(), None, mk[2].data_ptr()])
        masks_ok = (C.c_void_p * 3)(C.cast(full, C.c_void_p).value, None, C.cast(full, C.c_void_p).value)
        masks_bad = (C.c_void_p * 3)(C.cast(full, C.c_void_p).value, None, C.cast(holed, C.c_void_p).value)
        u64 = (C.c_uint64 * 3)(1, 2, 3)
        I, Y = ids_t.data_ptr(), y_t.data_ptr()
        ARG, STATE = _capi.FNN_ERR_ARG, _capi.FNN_ERR_STATE
        # (arguments after hs and n_models, expected code, a piece of the message, whose error string)
        cases = [
            ((None, 3, I, None, Y, 100, None, None, None, None, None), ARG, 'null hs', None),
            ((hs_of([engs[0], None, engs[2]]), 3, I, None, Y, 100, None, None, None, None, None), ARG, 'model 1', e0),
            ((hs_of(engs), 0, I, None, Y, 100, None, None, None, None, None), ARG, 'n_models', None),
            ((hs_of(engs), 257, I, None, Y, 100, None, None, None, None, None), ARG, 'n_models', None),
            ((hs_of(engs), 3, None, None, Y, 100, None, None, None, None, None), ARG, 'null ids', e0),
            ((hs_of(engs), 3, I, None, None, 100, None, None, None, None, None), ARG, 'null y', e0),
            ((hs_of(engs), 3, I, None, Y, 0, None, None, None, None, None), ARG, 'B must be', e0),
            ((hs_of(engs), 3, big.data_ptr(), None, Y, 300, None, None, None, None, None), ARG, 'model 0', e0),
            ((hs_of([engs[0], engs[1], other_f]), 3, I, None, Y, 100, None, None, None, None, None), ARG, 'model 2', e0),
            ((hs_of([engs[0], engs[1], engs[0]]), 3, I, None, Y, 100, None, None, None, None, None), ARG, 'model 2', e0),
            ((hs_of(engs), 3, I, None, Y, 100, masks_ok, u64, u64, None, None), ARG, 'masks and seeds', e0),
            ((hs_of(engs), 3, I, None, Y, 100, None, u64, None, None, None), ARG, 'seeds without steps', e0),
            ((hs_of(engs), 3, I, None, Y, 100, None, None, u64, None, None), ARG, 'steps without seeds', e0),
            ((hs_of(engs), 3, I, None, Y, 100, masks_bad, None, None, None, None), ARG, 'model 2', e0),
            ((hs_of([engs[0], no_table, engs[2]]), 3, I, None, Y, 100, None, None, None, None, None), STATE, 'model 1', e0),
        ]
        for args, code, piece, who in cases:
            rc = lib.ipnn_train_step_multi(*args)
            msg = (lib.ipnn_last_error(who.h if who is not None else None) or b'').decode()
            print("[ipnn-step-multi] refusal %d: %s" % (rc, msg))
            assert rc == code, (rc, code, msg)
            assert msg.startswith(NAME + ': '), msg
            assert piece in msg, (piece, msg)
        for e in engs:
            e.sync()
        for m, e in enumerate(engs):
            now = state(e, ids)
            assert now[0] == before[m][0] and np.array_equal(now[3], before[m][3]), 'model %d moved' % m
            assert all(np.array_equal(a, b) for a, b in zip(now[1] + now[2], before[m][1] + before[m][2])), 'model %d moved' % m
        # a larger max_batch in front does not hide a smaller one behind it
        wide0 = make(4, 5, [40, 24], 'f32', 'relu', max_batch=512, seed=305)
        try:
            rc = lib.ipnn_train_step_multi(hs_of([wide0, engs[1]]), 2, big.data_ptr(), None, Y, 300, None, None, None, None, None)
            msg = (lib.ipnn_last_error(wide0.h) or b'').decode()
            assert rc == ARG and msg.startswith(NAME + ': ') and 'model 1' in msg, (rc, msg)
        finally:
            wide0.close()
        with pytest.raises(FNNError):
            ipnn.train_step_many([engs[0], no_table], ids, y)
    finally:
        close(engs + [other_f, no_table])


# ------------------------------------------------------------------------------------------------ 13. an epoch
def test_train_epoch_many_against_the_loops(built):
    lk = [(0.01, 0.6), (0.02, 0.8), (0.005, 1.0)]
    solo, group = two_sets(lambda: [make_lk(4, 5, [40, 24], 'f32', ACTS[m], lr, keep, seed=400 + m) for m, (lr, keep) in enumerate(lk)])
    try:
        ids, y = train_feed(4, 700)
        seeds = [11, 12, 13]
        got = ipnn.train_epoch_many(group, ids, y, 256, seeds=seeds, first_step=40)
        assert len(got) == 3 and all(len(g) == 3 for g in got)
        for s, lo in enumerate(range(0, 700, 256)):
            hi = min(700, lo + 256)
            for m, e in enumerate(solo):
                ref = e.train_step(ids[lo:hi], y[lo:hi], Drawn(seeds[m], 40 + s))
                assert got[s][m] == ref['loss'], 'step %d model %d: %r against %r' % (s, m, got[s][m], ref['loss'])
        for m in range(3):
            assert_state_equal(solo[m], group[m], ids, 'model %d' % m)
    finally:
        close(solo + group)


# ------------------------------------------------------------------------------------------------ 14. against the oracle
class _GroupStepped(object):
    """an engine whose train_step is its place in a group call: what check_f32_step drives"""

    def __init__(self, engs, m, masks_of_others):
        self.engs, self.m, self.others = engs, m, masks_of_others

    def __getattr__(self, name):
        return getattr(self.engs[self.m], name)

    def train_step(self, ids, y, masks=None, want_logits=False):
        mk = None
        if masks is not None:
            mk = list(self.others)
            mk[self.m] = masks
        return ipnn.train_step_many(self.engs, ids, y, masks=mk, want_logits=want_logits)[self.m]


def test_group_step_f32_against_the_oracle(built):
    """Two steps of the first case at B = 100 with masks, held to oracle.ipnn_oracle.sgd_step with check_f32_step's bounds."""
    B, keep, lr = 100, 0.7, 0.01
    probs = [problem(4, 5, B, [40, 24], True, seed=500 + m) for m in range(3)]
    engs = [IPNNEngine(4, 5, [40, 24], ACTS[m], max_batch=256, precision='f32', lr=lr, keep_prob=keep) for m in range(3)]
    try:
        for e, p in zip(engs, probs):
            e.set_params(p[0], p[3]['b'], p[3]['W'], p[3]['bias'])
        ids = probs[1][1]
        others = [masks_for(e, B, 510 + m, keep) for m, e in enumerate(engs)]
        for m in (1,):                                   # the feed is model 1's problem: its ids, its y, its masks
            prob = (probs[m][0], ids, probs[m][2], probs[m][3], probs[m][4], probs[m][5])
            proxy = _GroupStepped(engs, m, others)
            for s in range(2):
                check_f32_step(proxy, prob, ACTS[m], lr, True, keep, True, 'group step %d, model %d' % (s, m))
    finally:
        close(engs)
