"""The decayed update of wide FM rows (k_scatdw1 / k_scatdw2: scatw1_form<true> / scatw2_form<true> of csrc/sparse_rows.hip.h,
FNN_MODE_FM at k = 17..128) on the hand-built layouts of tests/wide_layouts.py, up to 16384 keys per field, held to ONE float32
unit in the last place.

The reference is the reference's own sequential loop (orc.scatter_sgd / orc.scatter_sgd_feats, python/FNN_wnzh.py:299-306) in
float64 on the DEVICE's gradients: fnn_train_step's gx_out (k_gx_ref) is a verbatim copy of the float32 gx' the update reads,
whatever the precision of the GEMMs, so the network does not enter.  lr and lambda_fm are the float32 values the handle holds and
c = 1 - 2 lambda_fm lr / b_size is formed in double as update_cpow does.  The kernel forms row c^(e-s) - lr sum g c^(e-1-pos) in
f64 and rounds once; the loop rounds in f64 at every visit: they differ by about n 2^-53 relative, far inside half a float32
ulp, so after rounding to float32 they differ by at most one ulp -- a derived bound, not a measured one.  Rows that no id names
come back bit-equal.  Each case prints how many elements differ at all.

Sensitivity, asserted on the device's gx: the median of lr |gx| over the live (example, field, lane) entries is at least 100
ulp of the row element the entry lands in, so an entry dropped, doubled or weighted with the wrong power of c cannot hide inside
the bound; and b_size is chosen so that c^B lies in 0.05..0.5: the decay of a row hit by the whole batch is large, yet its first
entries still weigh in.
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError

import wide_layouts as wl
from test_gpu_shapes import DENSE, make_engine, make_problem

pytestmark = pytest.mark.gpu

H1, H2 = 64, 63
LAMFM = 5.0
W0 = -3.0


def lr_of(B):
    """As float32 holds it.  The loss is a sum over the batch and one row sits in every example: at 0.001 (test_gpu_shapes.lr_for)
    a step of 4096 examples and more drives the hidden units into saturation, and the NEXT step's gx is zero to the last bit
    in most entries, which would leave nothing to test.  The sensitivity condition holds at 0.0001 with room to spare."""
    return float(np.float32(0.0001 if B >= 4096 else 0.01))


def bsize_of(B, lr):
    """b_size with c^B = exp(-2 lambda_fm lr B / b_size) near 0.3."""
    return max(1, int(round(2 * LAMFM * lr * B / 1.2)))


def ordered(a):
    """float32 -> integers in the order of the floats (+0 and -0 both 0): a difference of 1 is one ulp."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def ulps(a, b):
    return np.abs(ordered(a) - ordered(b))


def problem(K, sizes, seed):
    F = len(sizes)
    _, _, _, _, p, r1, r2 = make_problem(F, K, H1, H2, 8, seed=seed)
    return synth.fm_table(sum(sizes), K, 0.05, seed), synth.field_of_row(sizes), p, r1, r2


def sensitivity(ids_by_field, gx, ref32, K, lr):
    """Median over the live (example, field, lane) entries of lr |gx| in ulps of the element of the reference it lands in.
    ids_by_field: [(field, examples, rows)]."""
    ratio = []
    for f, t, r in ids_by_field:
        if len(t):
            ratio.append((lr * np.abs(gx[t, 1 + f * K:1 + (f + 1) * K]) / np.spacing(np.abs(ref32[r]))).ravel().astype(np.float32))
    return float(np.median(np.concatenate(ratio)))


def check_table(label, got, before, ref64, touched, sens):
    """The 1-ulp bound, the untouched rows, the sensitivity condition; prints the count of differing elements."""
    ref32 = ref64.astype(np.float32)
    u = ulps(got, ref32)
    mask = np.zeros(len(before), bool)
    mask[touched] = True
    print("\n[wide exact] %s: %d of %d elements differ from the float32-rounded reference (worst %d ulp); %d rows touched, "
          "median lr |gx| = %.0f ulp" % (label, int((u > 0).sum()), u.size, int(u.max()), int(mask.sum()), sens))
    assert mask.sum() > 0 and (~mask).sum() > 0
    assert np.array_equal(got[~mask], before[~mask]), "%s: an untouched row changed" % label
    assert not np.array_equal(got[mask], before[mask])
    assert sens >= 100.0, "%s: median lr |gx| is %.1f ulp of the rows" % (label, sens)
    bad = np.argwhere(u > 1)
    assert len(bad) == 0, "%s: %d elements beyond 1 ulp, first (row, lane) %s: got %r ref %r" % (
        label, len(bad), bad[0], got[tuple(bad[0])], ref32[tuple(bad[0])])


def exact_step(eng, label, K, ids, y, r1, r2, lr, bs, oracle_gx=False):
    """One step on `eng`, the table against the sequential loop on the device's gx.  oracle_gx: also the device's gx against
    the float64 network on the device's state before the step, at test_gpu_shapes.check_step's f32 bound."""
    before = eng.get_table()
    dense = eng.get_dense() if oracle_gx else None
    out = eng.train_step(ids, y, r1, r2, b_size=bs, want_gx=True)
    assert np.isfinite(out['loss']), label
    gx = out['gx'].cpu().numpy().astype(np.float64)
    got = eng.get_table()
    c = 1.0 - 2.0 * LAMFM * lr / bs
    assert 0.05 < c ** len(ids) < 0.5
    ref = orc.scatter_sgd(before.astype(np.float64), ids, gx, lr, LAMFM, bs)
    by_field = [(f, np.flatnonzero(ids[:, f] >= 0), ids[ids[:, f] >= 0, f]) for f in range(ids.shape[1])]
    sens = sensitivity(by_field, gx, ref.astype(np.float32), K, lr)
    check_table(label, got, before, ref, np.unique(ids[ids >= 0]), sens)
    if oracle_gx:
        p64 = {k: np.asarray(v, np.float64) if isinstance(v, np.ndarray) else float(v) for k, v in dense.items()}
        x = orc.gather_vec(before.astype(np.float64), ids, W0)
        g64 = orc.train_call(p64, x, y.astype(np.float64), r1.astype(np.float64), r2.astype(np.float64), lr, 0.0, 'tanh')[0]
        np.testing.assert_allclose(gx, g64, rtol=2e-3, atol=2e-5 * np.abs(g64).max() + 1e-9, err_msg=label)


@pytest.mark.parametrize("case", wl.EXACT, ids=[wl.exact_id(c) for c in wl.EXACT])
def test_decayed_update_is_exact_on_hand_built_segments(built, case):
    """What each layout and shape reaches: tests/wide_layouts.py and tests/test_wide_layouts.py.  Two steps: the second batch
    holds the same runs on other examples and starts from the rows the first wrote; its gx is also held to the float64 network
    on the device's state (check_step's f32 bound), where a pad lane or the w_0 / ones column that took a gradient would show."""
    K, B, mb, codes, prec, steps = case
    lr = lr_of(B)
    bs = bsize_of(B, lr)
    ids0, sizes = wl.build(codes, B, 11)
    rows, fo, p, r1, r2 = problem(K, sizes, seed=K + B)
    rng = np.random.RandomState(B + K)
    eng = make_engine(len(codes), K, H1, H2, rows, fo, p, prec=prec, max_batch=mb, lr=lr, lam1=0.0, lamfm=LAMFM, w0=W0)
    try:
        for s in range(steps):
            ids = ids0 if s == 0 else wl.build(codes, B, 11 + s)[0]
            y = (rng.uniform(size=B) < 0.3).astype(np.float32)
            exact_step(eng, '%s step %d' % (wl.exact_id(case), s), K, ids, y, r1, r2, lr, bs, oracle_gx=s > 0)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ shadowed features
def feature_lists(B, sizes, rng, p_single):
    """The lines of test_gpu_fnn_wide.test_wide_shadowed_features_vs_oracle: 0..3 features per field (one with probability
    p_single), drawn from the first five rows of the field, a feature listed twice now and then, the line's features shuffled;
    line 0 also holds a row that only ever appears shadowed.  Feature id == row id."""
    F = len(sizes)
    offs = np.cumsum([0] + list(sizes[:-1]))
    feats = []
    for t in range(B):
        ft = []
        for f in range(F):
            n = 1 if rng.uniform() < p_single else int(rng.randint(0, 4))
            pick = list(offs[f] + rng.randint(0, min(sizes[f], 5), size=n))
            if n == 3 and rng.uniform() < 0.5:
                pick[2] = pick[0]
            ft += pick
        rng.shuffle(ft)
        feats.append([int(v) for v in ft])
    fbig = int(np.argmax(sizes))
    rare = int(offs[fbig] + sizes[fbig] - 1)
    feats[0] = [rare] + feats[0] + [int(offs[fbig])]
    return feats


def shadow_of(feats, fo):
    """(ids [B, F] with the LAST feature of a field, the (t, field, row) list of the features it shadows), as the reference's
    gather keeps and its update loop still visits."""
    F = int(fo.max()) + 1
    ids = np.full((len(feats), F), -1, np.int32)
    shadow = []
    for t, ft in enumerate(feats):
        seen = {}
        for feat in ft:
            f = int(fo[feat])
            if f in seen:
                shadow.append((t, f, seen[f]))
            seen[f] = feat
            ids[t, f] = feat
    return ids, np.asarray(shadow, np.int32).reshape(-1, 3)


def shadowed_step(eng, label, K, feats, fo, y, r1, r2, lr):
    """One step with the shadowed list set, against orc.scatter_sgd_feats on the device's gx: 1 ulp."""
    ids, shadow = shadow_of(feats, fo)
    B = len(feats)
    bs = bsize_of(B, lr)
    before = eng.get_table()
    eng.set_shadowed(shadow)
    out = eng.train_step(ids, y, r1, r2, b_size=bs, want_gx=True)
    assert np.isfinite(out['loss']), label
    gx = out['gx'].cpu().numpy().astype(np.float64)
    got = eng.get_table()
    ident = {int(r): int(r) for r in range(len(fo))}
    field_of = {int(r): int(fo[r]) for r in range(len(fo))}
    ref = orc.scatter_sgd_feats(before.astype(np.float64), feats, ident, field_of, gx, lr, LAMFM, bs)
    visits = np.array([(t, fo[feat], feat) for t, ft in enumerate(feats) for feat in ft])
    by_field = [(f, visits[visits[:, 1] == f, 0], visits[visits[:, 1] == f, 2]) for f in range(ids.shape[1])]
    sens = sensitivity(by_field, gx, ref.astype(np.float32), K, lr)
    check_table(label, got, before, ref, np.unique(visits[:, 2]), sens)
    main_rows = set(int(v) for v in ids[ids >= 0])
    only_shadow = sorted(set(int(r) for r in shadow[:, 2]) - main_rows)
    assert len(only_shadow) > 0 and np.all(np.abs(got[only_shadow] - before[only_shadow]).max(axis=1) > 0)
    return ids, shadow


def to_exactly(feats, fo, total):
    """Trim the lines and repeat line 1's first feature so that lines + shadowed entries == total."""
    n_sh = np.cumsum([len(ft) - len(set(int(fo[v]) for v in ft)) for ft in feats])
    B = int(np.flatnonzero(np.arange(1, len(feats) + 1) + n_sh <= total)[-1]) + 1
    feats = [list(ft) for ft in feats[:B]]
    feats[1] = feats[1] + [feats[1][0]] * (total - B - int(n_sh[B - 1]))
    return feats


SIZES4 = [7, 24, 20, 300]


def test_shadowed_features_regrow_the_global_slot_on_a_wide_handle(built):
    """max_batch 4096 (the handle's slots: N2 = 4096, a decay table of 4097 powers), B = 4000 and more than 96 shadowed entries:
    B + n lies in 4097..8192, so the grouping takes the regrown global slot at N2 = 8192 and the decay table is regrown to
    8193 powers (ensure_global_ws), a row hit by up to a fifth of the batch.  Then a plain step on the same handle, back on its
    own slot, checked the same way."""
    K, B = 18, 4000
    lr = lr_of(4096)
    rng = np.random.RandomState(B)
    rows, fo, p, r1, r2 = problem(K, SIZES4, seed=B)
    feats = feature_lists(B, SIZES4, rng, 0.8)
    eng = make_engine(4, K, H1, H2, rows, fo, p, max_batch=4096, lr=lr, lam1=0.0, lamfm=LAMFM, w0=W0)
    try:
        y = (rng.uniform(size=B) < 0.3).astype(np.float32)
        ids, shadow = shadowed_step(eng, 'shadowed 4000 + n on max_batch 4096', K, feats, fo, y, r1, r2, lr)
        assert len(shadow) > 96 and 4096 < B + len(shadow) <= 8192
        exact_step(eng, 'plain step after the shadowed one (max_batch 4096)', K, ids, y, r1, r2, lr, bsize_of(B, lr), oracle_gx=True)
    finally:
        eng.close()


def test_shadowed_features_fill_16384_keys_and_one_more_is_refused(built):
    """max_batch 16384 with B + n = 16384 exactly (no padding key in the global slot), a plain step behind it, then
    B + n = 16385: FNN_ERR_ARG, and no bit of the table or of the dense tensors changes."""
    K, total = 20, 16384
    lr = lr_of(total)
    rng = np.random.RandomState(total)
    rows, fo, p, r1, r2 = problem(K, SIZES4, seed=total)
    feats = to_exactly(feature_lists(16200, SIZES4, rng, 0.99), fo, total)
    B = len(feats)
    eng = make_engine(4, K, H1, H2, rows, fo, p, max_batch=16384, lr=lr, lam1=0.0, lamfm=LAMFM, w0=W0)
    try:
        y = (rng.uniform(size=B) < 0.3).astype(np.float32)
        ids, shadow = shadowed_step(eng, 'shadowed B + n = 16384 on max_batch 16384', K, feats, fo, y, r1, r2, lr)
        assert B + len(shadow) == total and len(shadow) > 96
        exact_step(eng, 'plain step after the shadowed one (max_batch 16384)', K, ids, y, r1, r2, lr, bsize_of(B, lr), oracle_gx=True)
        table, dense = eng.get_table(), eng.get_dense()
        eng.set_shadowed(np.concatenate([shadow, shadow[:1]]))
        with pytest.raises(FNNError) as ei:
            eng.train_step(ids, y, r1, r2, b_size=bsize_of(B, lr), want_gx=True)
        assert ei.value.code == _capi.FNN_ERR_ARG and '16384' in str(ei.value)
        eng.sync()
        assert np.array_equal(eng.get_table(), table)
        after = eng.get_dense()
        assert all(np.array_equal(after[k], dense[k]) for k in DENSE) and after['b3'] == dense['b3']
    finally:
        eng.close()
