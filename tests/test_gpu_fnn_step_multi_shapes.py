"""fnn_train_step_multi beyond 16 fields x k = 11 and the default knobs: 13..16 fields, k = 1..15, hidden sizes at the edges of the
two padded shapes, per-model settings the header says may differ, every kernel the group selectors can return, and the refusals.

Two references for every step case.  (1) Each member against a solo twin that takes fnn_train_step on the same feed: p and the
loss of every step, then the table and the six dense tensors, bit for bit (include/fnn_hip.h promises that).  (2) Member 0 (or the
member a case names) against the float64 oracle after the first step, at check_step's bounds for its precision without the gx
bound (the group call returns no gx): a twin and a group that are wrong in the same way -- the w_0 slot, a pad column -- pass (1)
and miss (2).  Every case prints its worst oracle error as a fraction of its bound.

Inputs are small: about 1,000 table rows (rows repeat inside a strip), max_batch 512, batches of 300 / 257 / 17 / 1 lines, three
steps with the next batch announced, edge_empties in every batch and a duplicate-heavy last column in every other case.

Which case runs which branch of the group selectors of deep-ctr_amd/csrc/fnn_api.hip.  `grid` stands for the test_shape_grid
cases of that precision and hidden size, knob[x] for test_knob[x], rows[x] for test_rows_2_20[x], max_batch for
test_max_batch_differs_inside_a_launch_class:

  gstep1_sel                                        bf16                       f32                       bf16x3
  big (320 / 128), 8 waves, fixed form (WTF 47)     grid, big hidden           -- (bf16 only)            -- (bf16 only)
  big, 8 waves, generic                             knob[generic-bf16],        grid, big hidden          grid, big hidden
                                                    knob[wt0-bf16]
  big, 4 waves                                      knob[waves4-bf16]          knob[waves4-f32]          knob[waves4-bf16x3]
  small (64 / 64: 1 / 1 .. 63 / 63), 4 waves        grid, small hidden         grid, small hidden        grid, small hidden
  (10 instances.  The fixed form's F <= 32 test is true at every field count of the strip kernel, 13..16: its other arm cannot
   be reached.  FNN_STEP1_WAVES=4 at a small shape returns the small instance, which has four waves anyway:
   knob[waves4-small-bf16].)

  gstep2_sel (key width, sort runs, wgrad form)     bf16                       f32 / bf16x3 (4-byte elements: direct only)
  32-bit keys, 4 runs, lds                          grid (max_batch 512)       --
  32-bit keys, 4 runs, direct                       knob[direct-bf16],         grid
                                                    max_batch (its member 4)
  32-bit keys, 16 runs, lds                         knob[sort16-bf16]          --
  32-bit keys, 16 runs, direct                      knob[sort16+direct-bf16]   knob[sort16-f32], knob[sort16-bf16x3]
  64-bit keys, 4 runs, lds                          rows[bf16] member 0        --
  64-bit keys, 4 runs, direct                       rows[bf16] member 1        rows[f32+bf16x3] members 0 / 2
  64-bit keys, 16 runs, lds                         rows[bf16] member 2        --
  64-bit keys, 16 runs, direct                      rows[bf16] member 3        rows[f32+bf16x3] members 1 / 3
  (8 + 4 + 4 instances.  The lds form where the plan would not choose it: knob[lds-mb256-bf16], max_batch 256, and
   knob[lds-slot-bf16], the slot-per-lane scatter.  test_setters_between_group_calls[rows2^20] moves a member from the first row
   to the fifth between two calls.)

  gstep3_sel (key width, sort runs)                 every type: the cases of gstep2_sel's rows of that key width and run count
  (4 instances per type)

  gpredict_sel: tests/test_gpu_fnn_eval_multi_shapes.py carries its rows.

A LaunchClass also compares split-K, the two scatter forms, FNN_SCAT2_WGS and the store policy: knob[splitk2-*], knob[splitk16-*]
(in bf16 sixteen slices mean eight: make_plan), knob[slot-*], knob[quarter-*], knob[block-*], knob[wgs16-*], knob[wt0-bf16];
test_mixed_knobs_in_one_call puts members that differ in one of them each into one call.
"""
import ctypes as C

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

from test_gpu_shapes import Bounds, compare_step, make_engine, make_problem, oracle_step
from test_gpu_fnn_step_multi import (ARG, NROWS, Feed, Spec, assert_same_state, assert_same_step, group_step, last_error,
                                     solo_step)

pytestmark = pytest.mark.gpu

PAIRS = [(300, 100), (256, 64), (319, 127), (63, 63), (1, 1), (40, 20)]
PRECS = ['bf16', 'f32', 'bf16x3']
LENS = [300, 257, 17, 1]
KNOB_VARS = ('FNN_STEP1_WAVES', 'FNN_STEP1_FORM', 'FNN_WT_STORES', 'FNN_SORT_RUNS', 'FNN_WGRAD_FORM', 'FNN_SPLITK', 'FNN_SCAT1_FORM',
             'FNN_SCAT2_FORM', 'FNN_SCAT2_WGS', 'FNN_NO_FUSE', 'FNN_ROLE_OFF')

_feeds = {}


def feed_for(F, K, lens, dup=False, seed=5):
    """One device feed per layout and batch lengths, made once and never changed."""
    key = (F, K, tuple(lens), dup, seed)
    if key not in _feeds:
        _feeds[key] = Feed(list(lens), seed=seed, F=F, K=K, empties=True, dup=dup)
    return _feeds[key]


def create(sp, feed, monkeypatch, env=None):
    """sp's handle, created with the variables of `env` set; they are deleted again before the next handle."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return sp.engine(feed)
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)


def oracle_first_step(sp, feed, b_size=0):
    """The float64 oracle's first step of model sp on the feed's first batch: what compare_step takes, and the table before it.
    A table longer than the feed's reaches the oracle cut to NROWS rows: the rows beyond are in no batch."""
    rows = feed.table(min(sp.n_rows, NROWS), sp.K)[0]
    rows64 = rows.astype(np.float64).copy()
    p64 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sp.p.items()}
    r1, r2 = sp.host_masks(0)
    gx, loss, p_drop, g = oracle_step(rows64, p64, feed.ids[0], feed.y[0], r1, r2, sp.lr, sp.lam1, sp.lamfm, sp.acti,
                                      b_size=b_size if b_size > 0 else None, reg_all=sp.reg_all)
    return rows, (rows64, p64, gx, loss, p_drop, g)


def run_case(specs, feed, monkeypatch, label, envs=None, oracle_on=0, b_sizes=None, between=None, invariant=None, twin_envs=None):
    """The models of `specs` through three group steps over the feed's batches, the next batch announced; their twins through
    solo steps.  envs[m]: the variables model m AND its twin are created under.  Compared: (1) and (2) of the module docstring.
    b_sizes[s]: the b_size of step s.  between(s, engs, twins): what happens to both after step s.  invariant: indices of members
    that are also held, bit for bit, to a second twin created under twin_envs[m] (a knob that is promised to change no bit)."""
    M = len(specs)
    envs = envs or [None] * M
    b_sizes = b_sizes or [0] * len(feed.d)
    engs, twins, plain = [], [], {}
    try:
        for m, sp in enumerate(specs):
            engs.append(create(sp, feed, monkeypatch, envs[m]))
            twins.append(create(sp, feed, monkeypatch, envs[m]))
        for m in (invariant or []):
            plain[m] = create(specs[m], feed, monkeypatch, (twin_envs or {}).get(m))
        for s in range(len(feed.d)):
            ids_t, y_t = feed.d[s]
            masks = [sp.masks(feed, s) for sp in specs]
            nxt = feed.d[s + 1][0] if s + 1 < len(feed.d) else None
            rc, loss, ps = group_step(engs, ids_t, y_t, masks, nxt, b_size=b_sizes[s])
            assert rc == 0, last_error(engs[0])
            for m, (t, sp) in enumerate(zip(twins, specs)):
                what = '%s: model %d (%s %dx%d k=%d), step %d' % (label, m, sp.prec, sp.H1, sp.H2, sp.K, s)
                ref = solo_step(t, ids_t, y_t, masks[m], b_size=b_sizes[s])
                assert ref[0] == 0, last_error(t)
                assert_same_step((rc, loss[m], ps[m]), ref, what)
                if m in plain:
                    ref = solo_step(plain[m], ids_t, y_t, masks[m], b_size=b_sizes[s])
                    assert ref[0] == 0, last_error(plain[m])
                    assert_same_step((rc, loss[m], ps[m]), ref, what + ', against the twin without the knob')
            if s == 0 and oracle_on is not None:
                sp, e = specs[oracle_on], engs[oracle_on]
                rows, ref = oracle_first_step(sp, feed, b_sizes[0])
                bd = Bounds()
                compare_step(bd, sp.prec, rows, sp.lr, ps[oracle_on], loss[oracle_on], e.get_table()[:NROWS], e.get_dense(), ref)
                bd.report('group ' + label)
            if between is not None:
                between(s, engs, twins)
        for m, (e, t) in enumerate(zip(engs, twins)):
            assert_same_state(e, t, '%s: model %d' % (label, m))
            if m in plain:
                assert_same_state(e, plain[m], '%s: model %d against the twin without the knob' % (label, m))
    finally:
        for e in engs + twins + list(plain.values()):
            e.close()


# ------------------------------------------------------------------------------------------------ 1a: the shape grid
# every pair of F in 13..16 and k in {1, 2, 4, 5, 12, 15} once; hidden pair, precision and batch length rotate so that every hidden
# pair meets every precision, every precision every batch length and every k four hidden pairs
GRID = []
for _fi, _F in enumerate((13, 14, 15, 16)):
    for _ki, _K in enumerate((1, 2, 4, 5, 12, 15)):
        _i = 6 * _fi + _ki
        GRID.append((_F, _K) + PAIRS[(_fi + _ki) % 6] + (PRECS[_ki % 3], LENS[(2 * _fi + _ki) % 4], _i % 2 == 1))
assert len({(c[2], c[3], c[4]) for c in GRID}) == 18 and len({(c[4], c[5]) for c in GRID}) == 12


def grid_id(c):
    return 'F%d-K%d-H%dx%d-%s-B%d%s' % (c[:6] + ('-dup' if c[6] else '',))


@pytest.mark.parametrize("F,K,H1,H2,prec,B,dup", GRID, ids=[grid_id(c) for c in GRID])
def test_shape_grid(built, monkeypatch, F, K, H1, H2, prec, B, dup):
    """Three members of one launch class that differ in lr, lambda1, lambda_fm, act, masks and initial weights."""
    feed = feed_for(F, K, [B] * 3, dup)
    run_case([Spec(m, prec, H1, H2, F=F, K=K) for m in range(3)], feed, monkeypatch, '1a ' + grid_id((F, K, H1, H2, prec, B, dup)))


# ------------------------------------------------------------------------------------------------ 1b: several k in one call
@pytest.mark.parametrize("F,precs", [(16, ('bf16', 'f32')), (13, ('bf16x3', 'bf16'))], ids=['F16', 'F13'])
def test_several_k_in_one_call(built, monkeypatch, F, precs):
    """k = 5, 15, 1, 5, 11, 15, 1, 11 in call order, each k with its own table over the same row ids: four launch classes of two
    members each, none adjacent in the call, the two of a class at different hidden sizes of one padded shape."""
    a, b = precs
    feed = feed_for(F, 11, [300, 257, 17], dup=(F == 13))
    lay = [(5, a, 300, 100), (15, a, 40, 20), (1, a, 319, 127), (5, a, 256, 64), (11, b, 63, 63), (15, a, 1, 1), (1, a, 300, 100),
           (11, b, 40, 20)]
    specs = [Spec(m, prec, H1, H2, F=F, K=k) for m, (k, prec, H1, H2) in enumerate(lay)]
    run_case(specs, feed, monkeypatch, '1b F%d' % F)


# ------------------------------------------------------------------------------------------------ 1c: per-model settings
def test_reg_all_differs_inside_a_launch_class(built, monkeypatch):
    """reg_all 1, 0, 1, 0 in one f32 launch class; the oracle check is on member 0: reg_all = 1 at lambda1 = 0.5, where the
    term on w1 / b1 / w2 / b2 (lr 2 lambda1 w, about 1e-3 at |w| = 0.1) is a hundred times the bound on those tensors."""
    feed = feed_for(16, 11, [300, 257, 17])
    specs = [Spec(m, 'f32', 300, 100, reg_all=(m % 2 == 0), lam1=(0.5 if m == 0 else None)) for m in range(4)]
    assert specs[2].lam1 > 0
    run_case(specs, feed, monkeypatch, '1c reg_all')


def test_max_batch_differs_inside_a_launch_class(built, monkeypatch):
    """bf16 at B = 256 with max_batch 300, 512, 768 and 4,096 -- one launch class whose members differ in ldT -- and a max_batch
    256 member, which the plan gives the direct weight-gradient form and split-K 8: another class."""
    feed = feed_for(15, 4, [256, 256, 256], dup=True)
    specs = [Spec(m, 'bf16', 300, 100, max_batch=mb, F=15, K=4) for m, mb in enumerate((300, 512, 768, 4096, 256))]
    run_case(specs, feed, monkeypatch, '1c max_batch')


@pytest.mark.parametrize("order", [(0, 1, 4), (4, 1, 0)], ids=['0-B-4B', '4B-B-0'])
def test_b_size_zero_B_and_4B(built, monkeypatch, order):
    """b_size 0, B and 4 B on successive calls (a data-parallel search passes the global length); in the other order the oracle's
    step is the 4 B one."""
    B = 300
    feed = feed_for(14, 12, [B] * 3)
    specs = [Spec(0, 'f32', 300, 100, F=14, K=12), Spec(1, 'bf16', 300, 100, F=14, K=12), Spec(2, 'bf16x3', 40, 20, F=14, K=12),
             Spec(3, 'f32', 300, 100, F=14, K=12)]
    run_case(specs, feed, monkeypatch, '1c b_size ' + '-'.join(str(o) for o in order), b_sizes=[o * B for o in order])


@pytest.mark.parametrize("new_rows", [1500, 1 << 20], ids=['rows1500', 'rows2^20'])
def test_setters_between_group_calls(built, monkeypatch, new_rows):
    """Four bf16 members of one grouping class.  After the first call, which announced the second batch: fnn_set_table on the
    class's first member, to 1,500 rows (another grouping class) or to 2^20 rows (64-bit keys: another launch class), and
    fnn_set_hparams on member 1; after the second call fnn_set_dense on member 2.  The twins get the same."""
    feed = feed_for(16, 11, [300, 257, 17])
    specs = [Spec(m, 'bf16', 300, 100) for m in range(4)]
    table = feed.table(new_rows)
    dense = make_problem(16, 11, 300, 100, 4, n_rows=64, seed=91)[4]

    def between(s, engs, twins):
        for group in (engs, twins):
            if s == 0:
                group[0].set_table(table[0], table[1], -2.5)
                group[1].set_hparams(0.003, 0.04, 0.2)
            elif s == 1:
                group[2].set_dense(dense)

    run_case(specs, feed, monkeypatch, '1c setters ' + str(new_rows), between=between)


# ------------------------------------------------------------------------------------------------ 1d: knobs
SLOT_TWIN = {'FNN_SPLITK': '4', 'FNN_WGRAD_FORM': 'direct'}      # what FNN_SCAT1_FORM=slot moves besides the scatter body (make_plan)
# (id, env, precisions, hidden, max_batch, the environment of a twin that must give the same bits or None)
KNOBS = [
    ('waves4', {'FNN_STEP1_WAVES': '4'}, PRECS, (300, 100), 512, None),
    ('waves4-small', {'FNN_STEP1_WAVES': '4'}, ['bf16'], (40, 20), 512, None),
    ('generic', {'FNN_STEP1_FORM': 'generic'}, ['bf16'], (300, 100), 512, None),
    ('wt0', {'FNN_WT_STORES': '0'}, ['bf16'], (300, 100), 512, None),
    ('sort16', {'FNN_SORT_RUNS': '16'}, PRECS, (300, 100), 512, {}),
    ('sort16+direct', {'FNN_SORT_RUNS': '16', 'FNN_WGRAD_FORM': 'direct'}, ['bf16'], (40, 20), 512, {'FNN_WGRAD_FORM': 'direct'}),
    ('direct', {'FNN_WGRAD_FORM': 'direct'}, ['bf16'], (300, 100), 512, None),
    ('lds-mb256', {'FNN_WGRAD_FORM': 'lds'}, ['bf16'], (300, 100), 256, None),
    ('lds-slot', {'FNN_WGRAD_FORM': 'lds', 'FNN_SCAT1_FORM': 'slot'}, ['bf16'], (40, 20), 512, None),
    ('splitk2', {'FNN_SPLITK': '2'}, ['bf16', 'f32'], (300, 100), 512, None),
    ('splitk16', {'FNN_SPLITK': '16'}, ['bf16', 'f32'], (300, 100), 512, None),
    ('slot', {'FNN_SCAT1_FORM': 'slot'}, PRECS, (300, 100), 512, SLOT_TWIN),
    ('quarter', {'FNN_SCAT1_FORM': 'quarter'}, ['bf16', 'f32'], (40, 20), 512, {}),
    ('block', {'FNN_SCAT2_FORM': 'block'}, ['bf16', 'f32'], (300, 100), 512, {}),
    ('wgs16', {'FNN_SCAT2_WGS': '16'}, ['bf16', 'f32'], (300, 100), 512, None),
]
KNOB_CASES = [(k[0], k[1], prec, k[3], k[4], k[5]) for k in KNOBS for prec in k[2]]


@pytest.mark.parametrize("name,env,prec,hidden,max_batch,same_as", KNOB_CASES, ids=['%s-%s' % (c[0], c[2]) for c in KNOB_CASES])
def test_knob(built, monkeypatch, name, env, prec, hidden, max_batch, same_as):
    """A uniform group of three, every handle and twin created under the knob.  The scatter forms and the sort runs change no
    bit: there member 0 also equals a twin created without the knob."""
    lens = [256, 17, 1] if max_batch == 256 else [300, 257, 17]
    feed = feed_for(14, 5, lens, dup=True)
    specs = [Spec(m, prec, hidden[0], hidden[1], max_batch=max_batch, F=14, K=5) for m in range(3)]
    run_case(specs, feed, monkeypatch, '1d %s %s' % (name, prec), envs=[env] * 3, invariant=[0] if same_as is not None else None,
             twin_envs={0: same_as})


def test_mixed_knobs_in_one_call(built, monkeypatch):
    """Twelve bf16 and f32 members of one shape, each created under another knob value, default-knob members among them: members
    that differ only in split-K, a scatter form, FNN_SCAT2_WGS, the store policy, the sort runs or the waves per strip must not
    share a launch class, and default members after them must not inherit their arguments."""
    feed = feed_for(14, 5, [300, 257, 17], dup=True)
    envs = [None, {'FNN_SPLITK': '2'}, {'FNN_SCAT1_FORM': 'quarter'}, None, {'FNN_SCAT2_FORM': 'block'}, {'FNN_SCAT2_WGS': '16'},
            {'FNN_WT_STORES': '0'}, {'FNN_SORT_RUNS': '16'}, {'FNN_STEP1_WAVES': '4'}, {'FNN_SCAT1_FORM': 'slot'}, {'FNN_SPLITK': '16'}, None]
    precs = ['bf16'] * 9 + ['f32'] * 3
    specs = [Spec(m, precs[m], 300, 100, F=14, K=5) for m in range(len(envs))]
    run_case(specs, feed, monkeypatch, '1d mixed', envs=envs, invariant=[2, 4, 7], twin_envs={2: {}, 4: {}, 7: {}})


@pytest.mark.parametrize("precs", [('bf16',) * 4, ('f32', 'f32', 'bf16x3', 'bf16x3')], ids=['bf16', 'f32+bf16x3'])
def test_rows_2_20(built, monkeypatch, precs):
    """Tables of 2^20 rows: 64-bit sort keys with both merge forms (and, in bf16, both weight-gradient forms)."""
    feed = feed_for(16, 11, [300, 257, 17])
    s16 = {'FNN_SORT_RUNS': '16'}
    if precs[0] == 'bf16':
        envs = [None, {'FNN_WGRAD_FORM': 'direct'}, s16, dict(s16, FNN_WGRAD_FORM='direct')]
    else:
        envs = [None, s16, None, s16]
    specs = [Spec(m, precs[m], (300, 40)[m % 2], (100, 20)[m % 2], n_rows=1 << 20) for m in range(4)]
    run_case(specs, feed, monkeypatch, '1d rows2^20 ' + '+'.join(sorted(set(precs))), envs=envs)


def test_splitk_16_in_bf16_keeps_the_weight_gradient_of_a_short_batch(built, monkeypatch):
    """A batch of up to 256 lines is padded to 256; a bf16 product walks the batch 32 lines at a time, so sixteen slices of such
    a batch would hold no step at all and the dense tensors would not move.  The dense tensors of one solo bf16 step at B = 17
    under FNN_SPLITK=16 against the oracle's, each within 5e-2 of the largest move of that tensor -- the share check_step allows
    the bf16 table update of its largest move."""
    feed = feed_for(14, 5, [17, 17, 17], dup=True)
    sp = Spec(0, 'bf16', 300, 100, F=14, K=5)
    eng = create(sp, feed, monkeypatch, {'FNN_SPLITK': '16'})
    try:
        ref = solo_step(eng, feed.d[0][0], feed.d[0][1], sp.masks(feed, 0))
        assert ref[0] == 0, last_error(eng)
        rows, (rows64, p64, gx, loss, p_drop, g) = oracle_first_step(sp, feed)
        d = eng.get_dense()
        bd = Bounds()
        for k in ('w1', 'b1', 'w2', 'b2', 'w3'):
            bd.close(k, d[k], p64[k], 0.0, 5e-2 * np.abs(p64[k] - sp.p[k]).max() + 1e-6)
        bd.report('solo bf16 FNN_SPLITK=16 B=17')
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 1e: refusals
class _Null(object):
    """A null entry of hs, mask1 or mask2 for group_step."""
    h = C.c_void_p(None)

    @staticmethod
    def data_ptr():
        return None


def test_refusals_off_the_strip_kernel_other_field_counts_next_B_and_null_entries(built, monkeypatch):
    """The refusals test_gpu_fnn_step_multi.py leaves out, twice each with the header's code, the exact message with the member's
    index and the loss array untouched; then good group steps equal twins that saw no refusal."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    feed = feed_for(16, 11, [300, 257, 17])
    specs = [Spec(m, 'bf16', 300, 100) for m in range(3)]
    engs, twins = [sp.engine(feed) for sp in specs], [sp.engine(feed) for sp in specs]
    others = []
    strip = 'the handle does not run the strip kernel (hidden sizes it is not built for, or FNN_NO_FUSE=1)'
    try:
        ids_t, y_t = feed.d[0]
        masks = [sp.masks(feed, 0) for sp in specs]

        def other(F, K, H1, H2, env=None, max_batch=512):
            rows, fo, _, _, p, _, _ = make_problem(F, K, H1, H2, 4, n_rows=NROWS, seed=5)
            for k, v in (env or {}).items():
                monkeypatch.setenv(k, v)
            e = make_engine(F, K, H1, H2, rows, fo, p, prec='bf16', max_batch=max_batch)
            for k in (env or {}):
                monkeypatch.delenv(k)
            others.append(e)
            return e

        def refused(members, text, ids=ids_t, nxt=None, ms=None):
            ms = [masks[0]] * len(members) if ms is None else ms
            for _ in range(2):
                assert engs[0].lib.fnn_sync(engs[0].h) == 0
                rc, loss, _ = group_step(members, ids, y_t, ms, nxt)
                assert rc == ARG
                assert last_error(members[0]) == 'fnn_train_step_multi: ' + text
                assert loss == [-1.0] * len(members)                     # untouched

        f12 = [other(12, 11, 300, 100), other(12, 11, 300, 100)]
        ids12 = feed.put(make_problem(12, 11, 300, 100, 300, n_rows=NROWS, seed=5)[2])
        refused(f12, 'model 0: ' + strip, ids=ids12)
        refused([engs[0], other(16, 11, 200, 50)], 'model 1: ' + strip)
        refused([engs[0], engs[1], other(16, 11, 300, 100, {'FNN_NO_FUSE': '1'})], 'model 2: ' + strip)
        refused([engs[0], other(13, 11, 300, 100), engs[1]], "model 1: n_fields or device differs from model 0's")
        long_next = feed.put(np.concatenate([feed.ids[0], feed.ids[1]])[:400])
        refused([engs[0], other(16, 11, 300, 100, max_batch=300), engs[1]], 'model 1: next_B must be in [1, max_batch]', nxt=long_next)
        refused([engs[0], _Null, engs[2]], 'model 1: null handle')
        refused(engs, 'model 2: null mask1 or mask2', ms=[masks[0], masks[1], (_Null, masks[2][1])])
        refused(engs, 'model 1: null mask1 or mask2', ms=[masks[0], (masks[1][0], _Null), masks[2]])
        for s in range(3):
            masks = [sp.masks(feed, s) for sp in specs]
            rc, loss, ps = group_step(engs, feed.d[s][0], feed.d[s][1], masks, feed.d[s + 1][0] if s < 2 else None)
            assert rc == 0, last_error(engs[0])
            for m, t in enumerate(twins):
                assert_same_step((rc, loss[m], ps[m]), solo_step(t, feed.d[s][0], feed.d[s][1], masks[m]), 'model %d, step %d' % (m, s))
        for m, t in enumerate(twins):
            assert_same_state(engs[m], t, 'model %d after the refusals' % m)
    finally:
        for e in engs + twins + others:
            e.close()
