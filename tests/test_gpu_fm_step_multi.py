"""One mini-batch step of several FM / LR models in one call (fm_train_step_multi, FM.train_step_many, ipinyou.run_many_batches) on
the device.  The rule throughout: model m of a group call ends BIT FOR BIT as a fresh handle with the same table and b ends after
its own train_step calls ("solo") -- every step's p and loss, then table, b and the Adam / FTRL state -- whatever the other members
of the group are.  The one exception is the solo step's own: rows that really sit under several columns of a batch on a
shared-rows handle take f32 atomics; those cases are held to the float64 restatement fm_shared_cases.Trainer under the bounds of
tests/test_gpu_fm_shared.py (p rtol 5e-5 / atol 1e-6, loss 2e-5 relative, rows 2e-3 * max|change| + 2e-7).
Tables are small (fm_shared_cases.n_rows_of(F, 12) rows) except the one 64-bit-key model."""
import numpy as np
import pytest

import fm_shared_cases as sc
from test_gpu_fm_fields import INIT, table

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM, train_step_many
from deep_ctr_amd.engine import FNNError

pytestmark = pytest.mark.gpu
PER = 12


class Spec(object):
    """One member of a group: its shape, its own table (seeded), optimiser, learning rate and L2 weight."""
    def __init__(self, F, k, lr=0.05, lam=1e-2, seed=1, n_rows=None, shared=False, b=0.1, opt='sgd', mean=1, max_batch=None):
        self.F, self.k, self.lr, self.lam, self.seed, self.shared, self.b, self.opt, self.mean = F, k, lr, lam, seed, shared, b, opt, mean
        self.n_rows, self.max_batch = n_rows or sc.n_rows_of(F, PER), max_batch

    def rows(self):
        return table(self.n_rows, self.F, self.k - 1, self.seed)

    def model(self, B):
        argv = [self.opt, self.lr] + ([1e-8] if self.opt == 'adam' else []) + ([] if self.mean else ['sum'])
        m = FM(self.max_batch or B, [self.n_rows, self.F, self.k - 1], INIT, argv, [self.lam], 'train', 0, shared_rows=self.shared)
        m.set_params(self.rows(), self.b)
        return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def state(m):
    rows, b = m.get_params()
    return [rows, np.float32(b)] + (list(m.get_opt_state()) if m.optimizer else [])


def record(res, m, out):
    res['p'].append(out['p'].cpu().numpy())
    res['loss'].append(out['loss'])
    if m.shared_rows:
        res['count'].append(m.count_shared_rows())


def new_result():
    return {'p': [], 'loss': [], 'count': []}


def solo(spec, steps):
    m = spec.model(max(len(s[2]) for s in steps))
    res = new_result()
    for ids, wts, y in steps:
        record(res, m, m.train_step(ids, y, want_p=True, wts=wts))
    res['state'] = state(m)
    m.close()
    return res


def group(specs, steps):
    B = max(len(s[2]) for s in steps)
    models = [s.model(B) for s in specs]
    res = [new_result() for _ in specs]
    for ids, wts, y in steps:
        for r, m, out in zip(res, models, train_step_many(models, ids, y, wts=wts, want_p=True)):
            record(r, m, out)
    for r, m in zip(res, models):
        r['state'] = state(m)
        m.close()
    return res


def assert_same(got, want, what=''):
    """Equal as bits: every step's p and loss, the shared-row counts, table, b and the optimiser state."""
    assert len(got['p']) == len(want['p'])
    for i, (a, c) in enumerate(zip(got['p'], want['p'])):
        assert np.array_equal(bits(a), bits(c)), '%s: p of step %d' % (what, i)
    for i, (a, c) in enumerate(zip(got['loss'], want['loss'])):
        assert np.float32(a).tobytes() == np.float32(c).tobytes(), '%s: loss of step %d: %r %r' % (what, i, a, c)
    assert got['count'] == want['count'], '%s: shared-row counts %r %r' % (what, got['count'], want['count'])
    assert len(got['state']) == len(want['state'])
    for i, (a, c) in enumerate(zip(got['state'], want['state'])):
        assert np.array_equal(bits(a), bits(c)) if i != 5 else a == c, '%s: state[%d]' % (what, i)


def check_group(specs, steps):
    got = group(specs, steps)
    for i, s in enumerate(specs):
        assert_same(got[i], solo(s, steps), 'model %d (F %d k %d %s)' % (i, s.F, s.k, s.opt))
    return got


def zipf_steps(F, B, n, seed, weighted, per=PER):
    """n consecutive batches over the same small table: background lines (repeated rows inside a column, -1 ids, short lines); a
    row never sits under two columns, so plain and shared-rows handles are both reproducible to the bit."""
    out = []
    for i in range(n):
        ids = sc.background(B, F, per, seed + i)
        wts = sc.wr.test_weights(B, F, seed + 50 + i) if weighted else None
        out.append((ids, wts, sc.labels(B, seed + 100 + i).astype(np.float32)))
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------------
def mixed_ranks(F, mean=None):
    ks = (1, 11, 16, 17, 101, 128)
    return [Spec(F, k, lr=0.02 + 0.01 * i, lam=(0.0, 1e-2, 3e-2)[i % 3], seed=40 + i, shared=bool(i & 1),
                 mean=(i % 2 if mean is None else mean)) for i, k in enumerate(ks)]


@pytest.mark.parametrize("weighted", [False, True])
def test_ranks_1_to_128_in_one_call_equal_their_solo_steps(built, weighted):
    """Three consecutive steps of B = 150 (not a multiple of 16; the later steps read rows the earlier ones wrote), narrow and
    both wide layouts, plain and shared-rows handles, reduce_mean 0 and 1 mixed per model."""
    specs = mixed_ranks(16)
    got = check_group(specs, zipf_steps(16, 150, 3, 7, weighted))
    assert not np.array_equal(got[0]['state'][0], specs[0].rows().astype(np.float32))          # something was trained


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 39, 64])
def test_three_models_at_other_field_counts(built, F):
    check_group([Spec(F, 1, lr=0.03, lam=1e-2, seed=1), Spec(F, 11, lr=0.05, lam=0.0, seed=2, mean=0),
                 Spec(F, 17, lr=0.04, lam=2e-2, seed=3)], zipf_steps(F, 150, 2, 10 + F, F == 39))


# 3 ---------------------------------------------------------------------------------------------------------------------------
def one_column_mask(ids, n_rows):
    """True for the rows that sit under at most one column of the batch."""
    per_col = [np.unique(c[c >= 0]) for c in np.asarray(ids).T]
    rows_, cnt = np.unique(np.concatenate(per_col), return_counts=True)
    mask = np.ones(n_rows, bool)
    mask[rows_[cnt > 1]] = False
    return mask


def level_specs(shared):
    lrs = {'sgd': 0.05, 'adam': 1e-2, 'ftrl': 0.05}
    return [Spec(5, k, lr=lrs[opt], lam=1e-3, seed=3 + j, opt=opt, shared=shared)
            for j, (k, opt) in enumerate((k, opt) for k in (11, 51) for opt in ('sgd', 'adam', 'ftrl'))]


def test_both_update_levels_under_sgd_adam_and_ftrl(built):
    """hot_batch as it is, on shared-rows handles: a 40-entry segment (level 2 on narrow and wide rows), segments ending on chunk
    borders, and three rows under two columns.  p, loss, the count, b, and table and optimiser state of every row under one
    column equal solo as bits; the three shared rows take atomics, solo as well, and are held to solo under the row bound."""
    ids = sc.hot_batch(300, 5, PER, 50)
    steps = [(ids, None, sc.labels(300, 60).astype(np.float32))]
    assert sc.shared_count(ids) == 3 and sc.segments(ids, 0)[0] == (0, 40)
    specs = level_specs(True)
    one = one_column_mask(ids, specs[0].n_rows)
    for i, (s, got) in enumerate(zip(specs, group(specs, steps))):
        want = solo(s, steps)
        assert np.array_equal(bits(got['p'][0]), bits(want['p'][0])) and got['loss'] == want['loss'] and got['count'] == want['count'] == [3], i
        assert np.array_equal(bits(got['state'][1]), bits(want['state'][1])), i
        for j in (0, 2, 3)[:3 if s.opt != 'sgd' else 1]:
            assert np.array_equal(bits(got['state'][j][one]), bits(want['state'][j][one])), (i, j)
        if s.opt != 'sgd':
            assert np.array_equal(bits(got['state'][4]), bits(want['state'][4])) and got['state'][5] == want['state'][5] == 1
        change = np.abs(want['state'][0] - s.rows()).max() + 1e-12
        assert np.abs(got['state'][0] - want['state'][0]).max() <= 2e-3 * change + 2e-7, i


def test_both_update_levels_on_plain_handles(built):
    """The same batches with the three shared rows moved out of each other's way (a plain handle would race on them), two steps:
    everything equals solo as bits, get_opt_state included."""
    steps = []
    for i in range(2):
        ids = sc.hot_batch(300, 5, PER, 50 + i)
        ids[:, 2][ids[:, 2] == 0] = 3                                        # row 0 stays in column 0 only
        ids[:, 3][ids[:, 3] == 1] = 4
        ids[:, 3][ids[:, 3] == 2] = 5
        assert sc.shared_count(ids) == 0 and sc.segments(ids, 0)[0] == (0, 40)
        steps.append((ids, None, sc.labels(300, 60 + i).astype(np.float32)))
    got = check_group(level_specs(False), steps)
    assert len(got[1]['state']) == 6 and got[1]['state'][5] == 2                                # Adam: state compared, two steps


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 17, 4096])
def test_batch_length_edges(built, B):
    """B = 4096 on the small table: every row is a long segment."""
    check_group([Spec(5, 11, lr=0.05, seed=1), Spec(5, 51, lr=0.03, lam=0.0, seed=2, mean=0)], zipf_steps(5, B, 2, 300 + B, False))


@pytest.mark.parametrize("k,shared", [(11, True), (51, False)])
def test_a_group_of_one(built, k, shared):
    """n_models == 1 is served by the solo step; same contract, and the range error still names model 0."""
    spec = Spec(5, k, lr=0.04, seed=7, shared=shared)
    check_group([spec], zipf_steps(5, 67, 2, 800, False))
    m = spec.model(67)
    ids, wts, y = zipf_steps(5, 67, 1, 810, False)[0]
    ids[3, 2] = spec.n_rows
    with pytest.raises(FNNError) as e:
        train_step_many([m], ids, y)
    assert e.value.code == _capi.FNN_ERR_RANGE and 'fm_train_step_multi' in str(e.value) and 'model(s) 0' in str(e.value)
    assert _capi.load().fm_sync(m.h) == 0
    m.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
BIG = 1100000


def big_steps(top):
    """basic_batch without its shared rows; top: the background moved to the top of the BIG table (test_64bit_sort_keys' move)."""
    steps = []
    for i in range(2):
        ids = sc.background(67, 5, PER, 150 + i)
        if top:
            ids = np.where(ids >= sc.S_ROWS, ids + (BIG - sc.n_rows_of(5, PER)), ids).astype(np.int32)
            sc.place(ids, 3, [(1, 0), (2, 0)])                               # a row every model has
        steps.append((ids, None, sc.labels(67, 160 + i).astype(np.float32)))
    return steps


def test_two_grouping_classes_64_and_32_bit_keys(built):
    assert BIG * 4096 > 2 ** 32
    specs = [Spec(5, 11, lr=0.04, seed=1), Spec(5, 4, lr=0.05, seed=8, n_rows=BIG), Spec(5, 17, lr=0.03, seed=2, n_rows=200),
             Spec(5, 11, lr=0.02, seed=3, shared=True)]
    check_group(specs, big_steps(False))
    check_group(specs[1:2] + specs[:1], big_steps(False))                    # the 64-bit class in front: its merge rides in launch 2


def test_an_id_out_of_range_for_the_small_models_only(built):
    steps = big_steps(True)
    assert max(s[0].max() for s in steps) >= BIG - PER - 1
    specs = [Spec(5, 4, lr=0.05, seed=8, n_rows=BIG), Spec(5, 11, lr=0.04, seed=1), Spec(5, 17, lr=0.03, seed=2, n_rows=200)]
    lib = _capi.load()
    # without the losses: nothing raises, every handle's fm_sync reports its own flag
    models = [s.model(67) for s in specs]
    for ids, wts, y in steps:
        train_step_many(models, ids, y, want_p=True, want_loss=False)
        assert [lib.fm_sync(m.h) for m in models] == [0, _capi.FNN_ERR_RANGE, _capi.FNN_ERR_RANGE]
        assert [lib.fm_sync(m.h) for m in models] == [0, 0, 0]
    got = [state(m) for m in models]
    # with the losses: FNN_ERR_RANGE lists the small models and clears their flags
    again = [s.model(67) for s in specs]
    with pytest.raises(FNNError) as e:
        train_step_many(again, steps[0][0], steps[0][2])
    assert e.value.code == _capi.FNN_ERR_RANGE and 'model(s) 1, 2' in str(e.value)
    assert [lib.fm_sync(m.h) for m in again] == [0, 0, 0]
    for m in models + again:
        m.close()
    # solo: the same ids are absent for the small models, and the large model never hears of their flags
    for i, s in enumerate(specs):
        m = s.model(67)
        for ids, wts, y in steps:
            m.train_step(ids, y, want_loss=False)
            assert lib.fm_sync(m.h) == (0 if i == 0 else _capi.FNN_ERR_RANGE)
        for a, c in zip(got[i], state(m)):
            assert np.array_equal(bits(a), bits(c)), 'model %d' % i
        m.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def trainer_of(spec):
    return sc.Trainer(spec.rows(), spec.b, 'sgd', spec.lr, spec.lam, spec.mean)


def hold_to_trainer(spec, steps, res, counts):
    """test_gpu_fm_shared.sgd_case's checks on a member of a group."""
    tr = trainer_of(spec)
    for i, (ids, wts, y) in enumerate(steps):
        data, p = tr.sgd_step(ids, y.astype(np.float64), wts)
        np.testing.assert_allclose(res['p'][i], p, rtol=5e-5, atol=1e-6)
        assert abs(res['loss'][i] - data) <= 2e-5 * max(1.0, abs(data))
        assert res['count'][i] == sc.shared_count(ids) == counts[i], (i, res['count'][i])
    change = np.abs(tr.rows - spec.rows()).max() + 1e-12
    err = np.abs(res['state'][0] - tr.rows).max()
    print("[fm-step-multi] F %d k %d: max row error %.3g of bound %.3g" % (spec.F, spec.k, err, 2e-3 * change + 2e-7))
    assert err <= 2e-3 * change + 2e-7
    assert abs(res['state'][1] - tr.b) <= 2e-3 * abs(tr.b - spec.b) + 2e-7


def shared_specs():
    return [Spec(5, 11, lr=0.05, seed=1, shared=True), Spec(5, 11, lr=0.05, seed=1, shared=False), Spec(5, 51, lr=0.04, seed=5, shared=True),
            Spec(5, 1, lr=0.03, lam=0.0, seed=6, shared=True, mean=0), Spec(5, 51, lr=0.04, seed=5, shared=False)]


def test_rows_shared_between_columns(built):
    """basic_batch: a row under two columns, under all five, twice on a line.  Shared-rows and plain handles in one call: every
    model's p and loss of the first step and, after it, every row under ONE column equal solo as bits (the plain handles race on
    the shared rows, solo as well: nothing else is asked of them); the shared-rows members' whole run is held to the float64
    restatement, and their counts to the NumPy count."""
    steps = [(sc.basic_batch(67, 5, PER, 10 + i), None, sc.labels(67, 20 + i).astype(np.float32)) for i in range(3)]
    specs = shared_specs()
    first = group(specs, steps[:1])
    one_col = one_column_mask(steps[0][0], specs[0].n_rows)
    assert (~one_col).sum() == 3
    for i, s in enumerate(specs):
        want = solo(s, steps[:1])
        assert np.array_equal(bits(first[i]['p'][0]), bits(want['p'][0])) and first[i]['loss'] == want['loss'], i
        assert first[i]['count'] == want['count'] == ([3] if s.shared else [])
        assert np.array_equal(bits(first[i]['state'][0][one_col]), bits(want['state'][0][one_col])), i
        assert np.array_equal(bits(first[i]['state'][1]), bits(want['state'][1])), i
    whole = group(specs, steps)
    for i, s in enumerate(specs):
        if s.shared:
            hold_to_trainer(s, steps, whole[i], [3, 3, 3])


def test_feeds_that_share_nothing_leave_shared_handles_equal_to_plain_ones(built):
    steps = zipf_steps(5, 67, 3, 400, False)
    specs = shared_specs()
    got = check_group(specs, steps)
    for a, c in ((0, 1), (2, 4)):                                            # the same model with the mode on and off
        for x, z in zip(got[a]['state'], got[c]['state']):
            assert np.array_equal(bits(x), bits(z))
        assert all(np.array_equal(bits(x), bits(z)) for x, z in zip(got[a]['p'], got[c]['p']))
    assert all(r['count'] == [0, 0, 0] for r, s in zip(got, specs) if s.shared)


def test_stale_marks_do_not_outlive_their_step(built):
    """test_gpu_fm_shared.py's three batches through the group call: rows shared in step 1 sit under one column in step 2, step 3
    shares nothing.  Two members share a grouping class, so the second one's counts come from the copied marks."""
    s1 = sc.basic_batch(67, 5, PER, 170)
    s2 = sc.background(67, 5, PER, 171)
    sc.place(s2, 0, [(1, 0), (2, 0)]), sc.place(s2, 1, [(3, 4)]), sc.place(s2, 2, [(4, 2), (5, 2), (6, 2)])
    sc.place(s2, 4, [(7, 1), (8, 3)])                                        # another row is shared now
    s3 = sc.background(67, 5, PER, 172)
    sc.place(s3, 0, [(1, 1)]), sc.place(s3, 4, [(2, 2)])
    steps = [(s, None, sc.labels(67, 180 + i).astype(np.float32)) for i, s in enumerate((s1, s2, s3))]
    specs = [Spec(5, 11, lr=0.05, seed=9, shared=True), Spec(5, 11, lr=0.03, lam=0.0, seed=10, shared=True),
             Spec(5, 51, lr=0.04, seed=11, shared=True)]
    got = group(specs, steps)
    for s, r in zip(specs, got):
        hold_to_trainer(s, steps, r, [3, 1, 0])


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_scale_folds_at_different_steps(built):
    """lr * lambda of 0.9, 0.8, 0.5 and 0.0: the lazy scale (1 - lr lambda)^n drops below 2^-24 and folds after step 8 (0.1^8),
    after step 11 (0.2^11), not within these twelve steps (0.5^24 = 2^-24), never.  Every step's p and loss equal solo as bits
    (they read the scale as the step before left it), then the tables."""
    steps = zipf_steps(5, 67, 12, 500, False)
    specs = [Spec(5, 11, lr=0.05, lam=18.0, seed=1), Spec(5, 11, lr=0.05, lam=10.0, seed=2), Spec(5, 11, lr=0.05, lam=0.0, seed=3),
             Spec(5, 51, lr=0.05, lam=18.0, seed=4), Spec(5, 11, lr=0.05, lam=16.0, seed=5)]
    dec = [1.0 - float(np.float32(s.lr)) * float(np.float32(s.lam)) for s in specs]
    assert [min([n for n in range(1, 13) if d ** n < 5.96e-8] or [0]) for d in dec] == [8, 0, 0, 8, 11]
    check_group(specs, steps)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_multi_solo_and_online_calls_interleave(built):
    steps = zipf_steps(5, 67, 4, 600, False)
    specs = [Spec(5, 11, lr=0.05, seed=1), Spec(5, 51, lr=0.03, seed=2), Spec(5, 1, lr=0.04, seed=3, shared=True)]

    def run(many):
        models = [s.model(67) for s in specs]

        def all_step(ids, wts, y):
            if many:
                return [o['p'].cpu().numpy() for o in train_step_many(models, ids, y, want_p=True)]
            return [m.train_step(ids, y, want_p=True)['p'].cpu().numpy() for m in models]
        ps = all_step(*steps[0])
        ps.append(models[0].train_step(steps[1][0], steps[1][2], want_p=True)['p'].cpu().numpy())
        ps.append(models[1].train_online(steps[2][0], steps[2][2], want_p=True)['p'].cpu().numpy())
        ps += all_step(*steps[3])
        out = ps + [x for m in models for x in state(m)]
        for m in models:
            m.close()
        return out
    for i, (a, c) in enumerate(zip(run(True), run(False))):
        assert np.array_equal(bits(a), bits(c)), i


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_260_tiny_models_more_models_than_cus(built):
    check_group([Spec(4, 3, lr=0.01 + 0.0005 * i, lam=1e-4 * (i % 7), seed=5 + i % 3) for i in range(260)], zipf_steps(4, 50, 2, 31, False))


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_no_bit_of_any_model(built):
    ids, wts, y = zipf_steps(5, 67, 1, 700, False)[0]
    specs = [Spec(5, 11, lr=0.05, seed=1), Spec(5, 51, lr=0.03, seed=2, shared=True), Spec(5, 11, lr=0.01, seed=3, opt='adam')]
    models = [s.model(67) for s in specs]
    train_step_many(models, ids, y)                                           # a pending scale, a step count and marks to lose
    before = [state(m) for m in models]
    counts = models[1].count_shared_rows()

    def refused(ms, code, what, ids=ids, y=y):
        with pytest.raises(FNNError) as e:
            train_step_many(ms, ids, y)
        assert e.value.code == code and 'fm_train_step_multi' in str(e.value) and what in str(e.value), str(e.value)

    refused(models + [models[0]], _capi.FNN_ERR_ARG, 'model 3')                  # a handle twice
    other = Spec(5, 11, seed=4, max_batch=32).model(32)
    refused(models + [other], _capi.FNN_ERR_ARG, 'model 3')                      # B above the smallest max_batch
    other.close()
    bare = FM(67, [sc.n_rows_of(5, PER), 5, 10], INIT, ['sgd', 0.05], [1e-2], 'train', 0)
    lib = _capi.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.fm_create(5, 11, 67, 0, None, C.byref(h)) == 0                   # a handle without a table
    keep, bare.h = bare.h, h
    refused(models + [bare], _capi.FNN_ERR_STATE, 'model 3')
    bare.h = keep
    lib.fm_destroy(h)
    bare.close()
    hot = Spec(5, 11, lr=0.5, lam=2.0, seed=5).model(67)                        # lr * lambda >= 1 on an SGD member
    refused(models + [hot], _capi.FNN_ERR_ARG, 'model 3')
    hot.close()
    six = Spec(6, 11, seed=6).model(67)                                         # differing n_fields, under the Python check
    hs = (C.c_void_p * 4)(*[m.h.value for m in models + [six]])
    lr, lam = (C.c_float * 4)(0.05, 0.05, 0.05, 0.05), (C.c_float * 4)(0, 0, 0, 0)
    loss = (C.c_float * 4)(7, 7, 7, 7)
    import torch
    ids_t, y_t = models[0]._dev(ids, torch.int32), models[0]._dev(y, torch.float32)
    assert lib.fm_train_step_multi(hs, 4, ids_t.data_ptr(), None, y_t.data_ptr(), 67, lr, lam, None, None, loss) == _capi.FNN_ERR_ARG
    assert list(loss) == [7, 7, 7, 7] and b'model 3' in lib.fm_last_error(models[0].h)
    six.close()
    with pytest.raises(ValueError):
        train_step_many([], ids, y)
    assert models[1].count_shared_rows() == counts
    for i, m in enumerate(models):
        for a, c in zip(before[i], state(m)):
            assert np.array_equal(bits(a), bits(c)) if not isinstance(a, int) else a == c, i
        m.close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def write_yzx(path, n, seed, n_feat=40, disjoint=False):
    """test_gpu_fm_shared.write_yzx: ragged lines of 1 .. 7 features in line order, a feature may repeat across positions of a
    line.  disjoint: position j draws from its own features, so that no row sits under two columns of a batch."""
    rng = np.random.RandomState(seed)
    w = rng.standard_normal(n_feat if not disjoint else 7 * 8)
    with open(path, 'w') as f:
        for _ in range(n):
            if disjoint:
                feats = [8 * j + int(rng.randint(0, 8)) for j in range(rng.randint(1, 8))]
            else:
                feats = list(rng.randint(0, n_feat, size=rng.randint(1, 8)))
                if len(feats) > 2 and rng.uniform() < 0.3:
                    feats[-1] = feats[0]                                     # the same feature at two positions
            y = int(rng.uniform() < 1.0 / (1.0 + np.exp(-w[feats].sum())))
            f.write('%d 0 %s\n' % (y, ' '.join('%d:1' % v for v in feats)))


@pytest.mark.parametrize("disjoint", [True, False], ids=['no-shared-rows', 'shared-rows'])
def test_driver_against_run_per_spec(built, tmp_path, disjoint):
    """run_many_batches at batch 64 over 300 lines in buffers of 128 against ipinyou.run per spec, numpy.random seeded alike.  A
    feed that shares no rows: the logs and the final tables are equal as bits.  One that does: within the rounding bounds."""
    train, test = str(tmp_path / 'train.yzx'), str(tmp_path / 'test.yzx')
    write_yzx(train, 300, 1, disjoint=disjoint), write_yzx(test, 400, 2, disjoint=disjoint)
    specs = [('FM', 10, 1e-3, 1e-2), ('LR', 0, 1e-3, 1e-3), ('FM', 10, 1e-3, 1e-2)]
    log = str(tmp_path / 'log')
    np.random.seed(1234)
    res = ipinyou.run_many_batches(train, test, specs, batch_size=64, buffer=128, eval_size=1000, log_file=log, echo=False)
    lines = open(log).read().splitlines()
    assert len(res) == 3 and len(lines) == 3 + 3 * 3
    for i, (algo, rank, lr, lam) in enumerate(specs):
        slog = str(tmp_path / ('log%d' % i))
        np.random.seed(1234)
        one = ipinyou.run(train, test, algo, batch_size=64, buffer=128, eval_size=1000, log_file=slog, echo=False)
        (got, gb), (want, wb) = res[i]['model'].get_params(), one['model'].get_params()
        mine = [ln[len('%d\t' % i):] for ln in lines if ln.startswith('%d\t' % i)]
        assert [h[0] for h in res[i]['log']] == [128, 256, 300] == [h[0] for h in one['log']]
        if disjoint:
            assert mine == open(slog).read().splitlines()
            assert res[i]['log'] == one['log']
            assert np.array_equal(bits(got), bits(want)) and gb == wb
        else:
            r0 = one['model'].X_dim
            assert mine[0] == open(slog).read().splitlines()[0] and got.shape[0] == r0
            for a, c in zip(res[i]['log'], one['log']):
                # both AUCs: test_gpu_fm_shared.py's 1e-4 for a logged AUC (a flipped pair of ~2e4 moves it by 5e-5)
                assert abs(a[1] - c[1]) <= 1e-4 and abs(a[2] - c[2]) <= 1e-4 and abs(a[3] - c[3]) <= 2e-5 * max(1.0, abs(c[3]))
            seeds = [0x89AB] if algo == 'LR' else [0x3210, 0x7654]
            W = np.random.RandomState(seeds[0]).uniform(-0.001, 0.001, (r0, 1))
            V = np.random.RandomState(seeds[-1]).uniform(-0.001, 0.001, (r0, rank if algo == 'FM' else 0))
            change = np.abs(want - np.concatenate([W, V], axis=1).astype(np.float32)).max() + 1e-12
            assert np.abs(got - want).max() <= 2e-3 * change + 2e-7
            assert abs(gb - wb) <= 2e-3 * abs(wb) + 2e-7
        one['model'].close()
    for r in res:
        r['model'].close()
