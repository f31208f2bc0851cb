"""The NATIVE data-parallel step (fnn_dp_init / fnn_dp_init_custom, include/fnn_hip.h) beyond the one layout every other
two-rank test uses (16 fields, k = 11, hidden 300 / 100; bag mode: 16 columns, h0 = 200).  Everything the step moves between
ranks is a count or an offset make_plan (fnn_api.hip) derives from the shape; `plan` below restates it, and every multi-rank
case asserts the element count of each collective it sees against it before it looks at a number.

  K1p = rup(16 F, 64) (wide rows, k >= 17: rup(F rup(k, 4) + 2, 64); bag: rup(h0 + 1, 64)), H1p = rup(H1 + 1, 64), H2p = rup(H2 + 1, 64)
  nw12 = K1p H1p + H1p H2p, nw = nw12 + H2p, nbag = K1p in bag mode (else 0), ldT = rup(max_batch, 256)
  slabs all-reduce   splitk * nslab floats, nslab = nw12 + 64 H2p + 64 nbag, splitk 8 or 4: k_reduce / the launch-3 tail take
                     column 0 of the 64-wide w3 slab at nw12 + (i - nw12) * 64 and the bag-bias block at nw12 + 64 H2p
  bucket all-reduce  nw + nbag floats: launch_update reads the bag bias at bucket + nw; k_p2p_update splits its grid into
                     nw12 / 4 float4 items and nw - nw12 + nbag scalars and rebuilds (row, column) from K1p / H1p / H2p
  EXCHANGE           two all-gathers per step: ldT * F ids (k_pad_ids pads with -1) and ldT * K1p floats of gx' per rank, then
                     scatter_global_impl over world * ldT examples (bag mode: the shards one after the other)

Shapes (F, k, H1, H2) -> K1p / H1p / H2p: nslab, nw + nbag, and the family that runs them:
  strip, three launches (families 1, 3, 4, 5, 7)
    (13 | 14 | 16, k, 256..319, 64..127)   256 / 320 / 128: nslab 131,072, bucket 123,008   k = 1, 4, 12, 15: the w_0 / ones slot
    (13 | 16, k, 63 | 8, 63 | 8)           256 /  64 /  64: nslab  24,576, bucket  20,544   of gx' in every lane and quarter
  layer by layer (families 2, 7): its own K1p / H1p / H2p size slabs and bucket
    (2, 1, 300, 100)      64 /  320 / 128: nslab    69,632, bucket    61,568   one 64-column block of x'
    (3, 15, 65, 64)       64 /  128 / 128: nslab    32,768, bucket    24,704   H1 + 1 and H2 + 1 just past a multiple of 64
    (39, 11, 500, 255)   640 /  512 / 256: nslab   475,136, bucket   459,008   the reference's 39 columns, H2 + 1 = 256 exactly
    (64, 15, 300, 100)  1024 /  320 / 128: nslab   376,832, bucket   368,768   the widest x'
    (12, 4, 1, 1)        192 /   64 /  64: nslab    20,480, bucket    16,448   one live unit per layer
    (16, 11, 4095, 1)    256 / 4096 /  64: nslab 1,314,816, bucket 1,310,784   the longest bucket and slabs
    (16, 51, 300, 100)   896 /  320 / 128: nslab   335,872, bucket   327,808   wide rows (rw = 52), test_gpu_fnn_wide.py's shape
  bag mode (F, h0, H1, H2), the instances of test_gpu_snn_shapes.py (families 6, 7): nbag = K1p
    (39, 300, 300, 100), (2, 316, 319, 127)   320 / 320 / 128: nslab 172,032, bucket 143,808   cx5: the bias block behind 320 columns
    (16, 192, 256, 64)                        256 / 320 / 128: nslab 147,456, bucket 123,264
    (64, 252, 63, 63)                         256 /  64 /  64: nslab  40,960, bucket  20,800   the bias block larger than w2's
  ldT: max_batch 256 -> 256 (a shard of 256 fills it, one of 1 or 100 or 150 does not), 300 -> 512 (a shard of 300 fits neither
  256 nor 512), 512 -> 512, 4096 -> 4096.

Families:
  1  two ranks, LOCAL, strip shapes, slabs and bucket; then prefetch on / off, bit for bit        nslab, nw, the w3 column
  2  two ranks, LOCAL, every rank on the layer-by-layer kernels (asserted), slabs and bucket      K1p / H1p / H2p of that path
  3  three ranks, LOCAL, shards 256 + 1 + 100 on handles of max_batch 256                         the sum over more than two views
  4  FM EXCHANGE, three steps, two and three ranks                                                ldT * F, ldT * K1p, world * ldT
  5  exact mode through the portable API (fnn_sparse_grad / fnn_step_scatter_global)              the slot layout of gx' at k = 1, 15
  6  bag mode, LOCAL and EXCHANGE, `fields` and `active` layouts                                  off_bag, nbag, bucket + nw
  7  world size 1, bucket through RCCL and P2P, bit for bit against a plain engine                k_p2p_update's item split

References.  A: the float64 oracle stepping the GLOBAL batch (oracle_step; orc.snn_train_step in bag mode) at the bounds of
test_gpu_shapes.check_step (f32: tol 1; bf16x3: tol 8, table 40; bf16: loss and table -- check_step holds no dense tensor to
the oracle in bf16, so neither does this file) and, in bag mode, of test_gpu_snn_shapes.check_step; the sum of the ranks'
losses against the oracle's at check_step's loss bound.  B: ONE engine stepping the global batch at test_gpu_dp._dense_close's
bound -- |d - ref| <= tol * max|ref - initial| + 1e-7 per tensor (b3: + 1e-6), tol 3e-4 on the three launches and 5e-4 on
the layer-by-layer path -- written here through Bounds.close(rtol 0, atol tol * scale + 1e-7), the same inequality, so that
the fraction of the bound is kept.  LOCAL tables as test_two_virtual_ranks_local_sparse: rows one rank alone touched meet the
oracle (b_size = the global length) and the single engine on that rank, and keep their initial bits on the others.  The
multi-step EXCHANGE cases use the bounds of test_gpu_shapes.test_multi_step_sequence_with_prefetch (loss 1e-4, table and
dense rtol 1e-4 / atol 1e-6, predictions rtol 2e-4 / atol 1e-6) at lr = 0.001, the reference's default: the loss is a SUM
over the batch, so their 406..450 examples move the weights per step as that test's 200 do at 0.002 (at 0.002 the second
loss triples: a saturated step no run takes, test_gpu_shapes.lr_for); every one-step case steps at lr_for(G) = 0.01.  Every problem has empty entries in field 0, field 1 and the last field, a duplicate-heavy column
that moves from case to case, and lambda1 = 0.05 (an L2 term summed over the ranks would leave B's bound by orders).
Bit-exact: the ranks' dense tensors in every form, FM EXCHANGE tables, prefetch on / off, world-1 bucket and P2P against a
plain engine, rows no rank touched.  Each case prints its worst error as a fraction of its bound.

Two or more ranks of one process never meet on the P2P collective here (dp_rehearsal_worker.py says why): P2P is family 7 only.
"""
import functools

import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd.engine import FNNEngine

from test_gpu_dp import VirtualRanks, _p2p_same_process
from test_gpu_parity import make_snn_engine, make_snn_problem
from test_gpu_shapes import DENSE, Bounds, _kw, case_id, edge_empties, lr_for, make_engine, make_problem, oracle_step, path_of

pytestmark = pytest.mark.gpu

LAM1, LAMFM = 0.05, 0.1
WIDE = (16, 51, 300, 100)                                      # test_gpu_fnn_wide.py's data-parallel shape


def rup(a, m):
    return (a + m - 1) // m * m


def plan(F, K, H1, H2, h0=0, max_batch=4096):
    """make_plan of fnn_api.hip: what the collectives carry (h0 > 0: bag mode)."""
    K1p = rup(h0 + 1, 64) if h0 else rup(F * rup(K, 4) + 2, 64) if K >= 17 else rup(16 * F, 64)
    H1p, H2p = rup(H1 + 1, 64), rup(H2 + 1, 64)
    nw12 = K1p * H1p + H1p * H2p
    nbag = K1p if h0 else 0
    return dict(K1p=K1p, nslab=nw12 + 64 * H2p + 64 * nbag, bucket=nw12 + H2p + nbag, ldT=rup(max_batch, 256))


def dp_path(F, K, H1, H2):
    """path_of, and strip_shape_ok's first line: wide rows never take the strip kernel."""
    return 'layer' if K >= 17 else path_of(F, H1, H2)


def cid(F, K, H1, H2, *rest):
    """case_id with the path a wide handle really takes."""
    s = case_id(F, K, H1, H2, *rest)
    return 'layer-wide' + s[len('strip'):] if K >= 17 else s


def copy_p(p):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def batch_empties(G, F, steps, extra=()):
    """edge_empties in every batch of the feed."""
    return sorted({(s * G + t, f) for s in range(steps) for (t, f) in list(edge_empties(G, F)) + list(extra)})


@functools.lru_cache(maxsize=None)
def fm_problem(F, K, H1, H2, G, steps, kind, i):
    """The feed of one case (steps * G examples) -- shared by the cases of a shape and never written to."""
    kw = _kw(kind, G, F)
    return make_problem(F, K, H1, H2, steps * G, seed=100 * F + K + i, dup_col=kw.get('dup_col', (2 + 5 * i) % F),
                        empty=batch_empties(G, F, steps, kw.get('empty', ())))


@functools.lru_cache(maxsize=None)
def fm_oracle(F, K, H1, H2, G, steps, kind, i, lr):
    """Reference A: `steps` oracle steps of the global batches -> (rows64, p64, grads of the last step, losses)."""
    rows, fo, ids, y, p, r1, r2 = fm_problem(F, K, H1, H2, G, steps, kind, i)
    rows64, p64, losses, g = rows.astype(np.float64), copy_p(p), [], None
    for s in range(steps):
        sl = slice(s * G, (s + 1) * G)
        _, loss, _, g = oracle_step(rows64, p64, ids[sl], y[sl], r1, r2, lr, LAM1, LAMFM, b_size=G)
        losses.append(loss)
    return rows64, p64, g, losses


@functools.lru_cache(maxsize=None)
def fm_single(F, K, H1, H2, G, steps, kind, i, lr, prec):
    """Reference B: one engine stepping the global batches -> (dense, table)."""
    rows, fo, ids, y, p, r1, r2 = fm_problem(F, K, H1, H2, G, steps, kind, i)
    eng = make_engine(F, K, H1, H2, rows, fo, p, prec=prec, lr=lr, lam1=LAM1, lamfm=LAMFM)
    try:
        for s in range(steps):
            eng.train_step(ids[s * G:(s + 1) * G], y[s * G:(s + 1) * G], r1, r2, want_loss=False)
        return eng.get_dense(), eng.get_table()
    finally:
        eng.close()


def cuts_of(shards):
    edges = np.cumsum([0] + list(shards))
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def rotating_cuts(shards, steps):
    """Step s deals the shard lengths rotated by s: a rank's shard shrinks from one step to the next, so its gx' buffer holds
    the longer step's rows behind the shorter one's -- rows only the -1 padding of the gathered ids keeps out of the table."""
    return [cuts_of(list(shards[s % len(shards):]) + list(shards[:s % len(shards)])) for s in range(steps)]


def run_native(mk, world, sparse, payload, ids, y, r1, r2, G, cuts, steps=1, prefetch=False):
    """`steps` native steps on `world` virtual ranks (VirtualRanks.run: one host thread per engine, barrier abort, bounded
    join); cuts: the ranks' slices of a global batch, or one such list per step.  Returns per rank (dense, table, bag bias
    or None), per rank the per-step losses, the collective counts and the element counts rank 0's collectives carried:
    floats per all-reduce, bytes per rank per all-gather."""
    import torch
    ranks = [mk() for _ in range(world)]
    vr = VirtualRanks(world)
    sizes = {'allreduce': [], 'allgather': []}

    def counted(r):
        ar, ag = vr.allreduce_for(r), vr.allgather_for(r)

        def ar0(view):
            sizes['allreduce'].append(view.numel())
            ar(view)

        def ag0(send, recv):
            assert recv.numel() == world * send.numel()
            sizes['allgather'].append(send.numel())
            ag(send, recv)
        return (ar0, ag0) if r == 0 else (ar, ag)
    for r, e in enumerate(ranks):
        ar, ag = counted(r)
        e.dp_init_custom(r, world, ar, ag, sparse=sparse)
        e.dp_set_payload(payload)
        assert e.dp_config()['payload'] == payload and e.dp_config()['collective'] == 'callback'
    by_step = cuts if isinstance(cuts[0], list) else [cuts] * steps
    dev = [[torch.as_tensor(np.ascontiguousarray(ids[s * G:(s + 1) * G][by_step[s][r]])).cuda() for s in range(steps)]
           for r in range(world)]
    losses = [[] for _ in ranks]

    def rank_fn(r):
        def go():
            for s in range(steps):
                if prefetch and s + 1 < steps:
                    ranks[r].prefetch_ids(dev[r][s + 1])
                out = ranks[r].train_step(dev[r][s], y[s * G:(s + 1) * G][by_step[s][r]], r1, r2, b_size=G)
                losses[r].append(out['loss'])
        return go
    vr.run([rank_fn(r) for r in range(world)])
    states = [(e.get_dense(), e.get_table(), e.get_bag_bias() if e.bag else None) for e in ranks]
    for e in ranks:
        e.close()
    return states, losses, dict(vr.calls), sizes


def check_counts(calls, sizes, pl, payload, sparse, steps, F):
    """What the collectives carried, against make_plan's restatement."""
    assert calls['allreduce'] == steps and calls['allgather'] == (2 * steps if sparse == 'exchange' else 0), calls
    for n in sizes['allreduce']:
        if payload == 'bucket':
            assert n == pl['bucket'], (n, pl)
        else:
            assert n in (4 * pl['nslab'], 8 * pl['nslab']), (n, pl)
    if sparse == 'exchange':
        assert sizes['allgather'] == [4 * pl['ldT'] * F, 4 * pl['ldT'] * pl['K1p']] * steps, (sizes, pl)


def assert_same_dense(states):
    """Every rank forms the same sum and applies the same update: bit-identical dense tensors."""
    for d, _, bb in states[1:]:
        for k in states[0][0]:
            assert np.array_equal(states[0][0][k], d[k]), k
        if bb is not None:
            assert np.array_equal(states[0][2], bb)


def dense_b(bd, tag, d, ref, p, tol, which='B'):
    """test_gpu_dp._dense_close's bound against `ref` (reference B unless `which` names another)."""
    for k in DENSE:
        scale = np.abs(ref[k] - np.asarray(p[k], np.float32)).max() + 1e-12
        bd.close('%s %s %s' % (tag, which, k), d[k], ref[k], 0.0, tol * scale + 1e-7)
    bd.close('%s %s b3' % (tag, which), d['b3'], ref['b3'], 0.0, tol * abs(ref['b3'] - float(p['b3'])) + 1e-6)


def dense_a(bd, tag, d, p64, g, lr, prec):
    """Reference A at check_step's bounds for the dense tensors and b3 (bf16: check_step has none)."""
    if prec == 'bf16':
        return
    tol = 8.0 if prec == 'bf16x3' else 1.0
    for k in DENSE:
        bd.close('%s A %s' % (tag, k), d[k], p64[k], 1e-5 * tol, 1e-3 * lr * np.abs(g[k]).max() * tol + 1e-7)
    bd.close('%s A b3' % tag, d['b3'], p64['b3'], 0.0, 1e-5 * tol)


def table_a(bd, name, got, ref64, change, prec):
    """check_step's table bound; `change` = max |rows64 - rows| of the whole step (bf16)."""
    if prec == 'bf16':
        bd.close(name, got, ref64, 0.0, 5e-2 * change + 1e-6)
    else:
        tt = 40.0 if prec == 'bf16x3' else 1.0
        bd.close(name, got, ref64, 1e-5 * tt, 2e-7 * tt)


def loss_a(bd, got, ref, prec):
    if prec == 'bf16':
        bd.close('A loss', got, ref, 0.0, 2e-2 * ref)
    else:
        bd.close('A loss', got, ref, 0.0, 2e-5 * (8.0 if prec == 'bf16x3' else 1.0) * max(1.0, abs(ref)))


def alone(ids_g, cuts):
    """(per rank the rows it alone touched, the rows any rank touched)."""
    t = [set(int(v) for v in np.unique(ids_g[c])) - {-1} for c in cuts]
    own = [t[r] - set().union(*(t[q] for q in range(len(t)) if q != r)) for r in range(len(t))]
    return [np.array(sorted(o), np.int64) for o in own], np.array(sorted(set().union(*t)), np.int64)


def check_local_fm(case, shards, prec, payload, label, max_batch=4096):
    """One LOCAL step of len(shards) ranks against A and B; returns nothing, prints the worst fraction."""
    F, K, H1, H2, G, steps, kind, i = case
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    lr, cuts, world = lr_for(G), cuts_of(shards), len(shards)
    assert sum(shards) == G
    rows64, p64, g, ref_losses = _oracle_one(case, lr)
    ref_dense, ref_rows = _first_step_single(case, lr, prec)
    states, losses, calls, sizes = run_native(
        lambda: make_engine(F, K, H1, H2, rows, fo, p, prec=prec, max_batch=max_batch, lr=lr, lam1=LAM1, lamfm=LAMFM),
        world, 'local', payload, ids, y, r1, r2, G, cuts)
    check_counts(calls, sizes, plan(F, K, H1, H2, max_batch=max_batch), payload, 'local', 1, F)
    bd = Bounds()
    loss_a(bd, sum(l[0] for l in losses), ref_losses[0], prec)
    tolb = 3e-4 if dp_path(F, K, H1, H2) == 'strip' else 5e-4
    own, touched = alone(ids[:G], cuts)
    untouched = np.setdiff1d(np.arange(rows.shape[0]), touched)
    change64 = np.abs(rows64 - rows).max()
    change = np.abs(ref_rows - rows.astype(np.float32)).max()
    assert len(untouched) and len(own[int(np.argmax(shards))])
    for r, (d, tab, _) in enumerate(states):
        dense_a(bd, 'rank%d' % r, d, p64, g, lr, prec)
        dense_b(bd, 'rank%d' % r, d, ref_dense, p, tolb)
        if len(own[r]):
            table_a(bd, 'rank%d A own rows' % r, tab[own[r]], rows64[own[r]], change64, prec)
            bd.close('rank%d B own rows' % r, tab[own[r]], ref_rows[own[r]], 0.0, 3e-4 * change + 1e-7)
        for q in range(world):
            if q != r:
                assert np.array_equal(tab[own[q]], rows[own[q]]), (r, q)
        assert np.array_equal(tab[untouched], rows[untouched]), r
    assert_same_dense(states)
    bd.report(label)


@functools.lru_cache(maxsize=None)
def _oracle_one(case, lr):
    """Reference A of the FIRST batch of a case's feed (the prefetch cases step on from it)."""
    F, K, H1, H2, G, steps, kind, i = case
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    rows64, p64 = rows.astype(np.float64), copy_p(p)
    _, loss, _, g = oracle_step(rows64, p64, ids[:G], y[:G], r1, r2, lr, LAM1, LAMFM, b_size=G)
    return rows64, p64, g, [loss]


@functools.lru_cache(maxsize=None)
def _first_step_single(case, lr, prec):
    """Reference B of the first batch."""
    F, K, H1, H2, G, steps, kind, i = case
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    eng = make_engine(F, K, H1, H2, rows, fo, p, prec=prec, lr=lr, lam1=LAM1, lamfm=LAMFM)
    try:
        eng.train_step(ids[:G], y[:G], r1, r2, want_loss=False)
        return eng.get_dense(), eng.get_table()
    finally:
        eng.close()


KINDS = ('empty', 'dup', '')

# ------------------------------------------------------------------------------------------------ 1: two ranks, LOCAL, strip
# (F, K, H1, H2, precision, shards)
STRIP = [(13, 1, 256, 64, 'f32', (257, 243)), (13, 15, 319, 127, 'f32', (257, 243)), (16, 4, 63, 63, 'f32', (257, 243)),
         (16, 15, 8, 8, 'f32', (257, 243)), (14, 12, 300, 100, 'f32', (257, 243)), (14, 12, 300, 100, 'f32', (1, 511)),
         (13, 15, 319, 127, 'bf16', (257, 243)), (13, 15, 319, 127, 'bf16x3', (257, 243)),
         (16, 4, 63, 63, 'bf16', (257, 243)), (16, 4, 63, 63, 'bf16x3', (257, 243))]


def _sid(c):
    return case_id(c[0], c[1], c[2], c[3], sum(c[5]), c[4], '+'.join(str(s) for s in c[5]))


@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
@pytest.mark.parametrize("F,K,H1,H2,prec,shards", STRIP, ids=[_sid(c) for c in STRIP])
def test_two_ranks_local_strip_shapes(built, monkeypatch, F, K, H1, H2, prec, shards, payload):
    """One LOCAL step on two virtual ranks at a strip shape against A and B (257 + 243, and 1 + 511: a rank whose whole shard
    is one example); then three steps with the next batch announced (fnn_prefetch_ids) and three without: losses, dense
    tensors and tables bit for bit per rank, as test_two_virtual_ranks_local_sparse_prefetch_changes_nothing."""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    assert dp_path(F, K, H1, H2) == 'strip'
    i = [c[:4] for c in STRIP].index((F, K, H1, H2))
    G, steps = sum(shards), 3
    case = (F, K, H1, H2, G, steps, KINDS[i % 3], i)
    check_local_fm(case, shards, prec, payload, _sid((F, K, H1, H2, prec, shards)) + '-' + payload)
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    lr, cuts = lr_for(G), cuts_of(shards)

    def mk():
        return make_engine(F, K, H1, H2, rows, fo, p, prec=prec, lr=lr, lam1=LAM1, lamfm=LAMFM)
    a, la, _, _ = run_native(mk, 2, 'local', payload, ids, y, r1, r2, G, cuts, steps, prefetch=False)
    b, lb, _, _ = run_native(mk, 2, 'local', payload, ids, y, r1, r2, G, cuts, steps, prefetch=True)
    assert la == lb
    for (da, ta, _), (db, tb, _) in zip(a, b):
        assert np.array_equal(ta, tb)
        for k in da:
            assert np.array_equal(da[k], db[k]), k
    assert_same_dense(a)
    assert not np.array_equal(a[0][1], a[1][1])                 # LOCAL: each replica holds its own shard's row updates


# ------------------------------------------------------------------------------------------------ 2: two ranks, LOCAL, layer
LAYER = [(2, 1, 300, 100, 'f32'), (3, 15, 65, 64, 'f32'), (39, 11, 500, 255, 'f32'), (64, 15, 300, 100, 'f32'),
         (12, 4, 1, 1, 'f32'), (16, 11, 4095, 1, 'f32'), WIDE + ('f32',), (39, 11, 500, 255, 'bf16')]


@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
@pytest.mark.parametrize("F,K,H1,H2,prec", LAYER, ids=[cid(*c[:4], 500, c[4]) for c in LAYER])
def test_two_ranks_local_layer_shapes(built, monkeypatch, F, K, H1, H2, prec, payload):
    """One LOCAL step with BOTH ranks on the layer-by-layer kernels (k_wgrad's slabs and k_reduce's bucket sized by this
    shape's own K1p / H1p / H2p; bucket payload: dp_finish_bucket from fnn_step_end's place) against A and B, 257 + 243."""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    assert dp_path(F, K, H1, H2) == 'layer'
    i = [c[:4] for c in LAYER].index((F, K, H1, H2))
    case = (F, K, H1, H2, 500, 1, KINDS[(i + 1) % 3], i)
    check_local_fm(case, (257, 243), prec, payload, cid(F, K, H1, H2, 500, prec, payload))


# ------------------------------------------------------------------------------------------------ 3: three ranks
@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
def test_three_ranks_local(built, monkeypatch, payload):
    """VirtualRanks(3) at 13 fields, k = 15 on handles of max_batch 256 (ldT = 256): shards 256 + 1 + 100 -- one fills ldT,
    one is a single example.  The collective sums three views; a count that drops a tensor's tail shows in all of them."""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    F, K, H1, H2 = 13, 15, 300, 100
    check_local_fm((F, K, H1, H2, 357, 1, 'dup', 3), (256, 1, 100), 'f32', payload,
                   case_id(F, K, H1, H2, 357, '256+1+100', payload), max_batch=256)


# ------------------------------------------------------------------------------------------------ 4: FM EXCHANGE
MS_LR = 0.001         # the loss is a sum over the batch: ~400 examples at 0.001 move what test_multi_step's 200 move at 0.002
# (F, K, H1, H2, max_batch, shards, precision)
EXCH = [(13, 1, 300, 100, 256, (256, 150), 'f32'), (13, 15, 256, 64, 256, (256, 150), 'f32'),
        (16, 4, 63, 63, 256, (256, 150), 'f32'), (16, 12, 319, 127, 300, (300, 150), 'f32'),
        (13, 15, 300, 100, 256, (256, 1, 100), 'f32'), (13, 15, 319, 127, 256, (256, 150), 'bf16'),
        (13, 15, 319, 127, 300, (300, 150), 'bf16')]


def _xid(c):
    return case_id(c[0], c[1], c[2], c[3], sum(c[5]), c[6], 'mb%d' % c[4], '+'.join(str(s) for s in c[5]))


@pytest.mark.parametrize("F,K,H1,H2,max_batch,shards,prec", EXCH, ids=[_xid(c) for c in EXCH])
def test_fm_exchange_three_steps(built, monkeypatch, F, K, H1, H2, max_batch, shards, prec):
    """FNN_DP_SPARSE_EXCHANGE for three steps: slot k of field 0 / field 1 in gx' carries the gradient of w_0 / of the ones
    column, never a row's; the ids of a shard shorter than ldT are padded with -1.  Either leaking into a row, or into the
    table's pad slot, shows in a later step's loss, the table or the predictions.  f32: A step by step at the multi-step
    bounds, B at test_two_virtual_ranks_exchange_keeps_replicas_identical's (tables 3e-4 of the change, dense 5e-4 -- three
    steps, not one); bf16: B only.  Every rank's WHOLE table is checked, and all tables are bit-identical.  The shard lengths
    rotate over the steps (rotating_cuts): at ldT = 512 the 150-example shard that follows a 300-example one leaves that
    step's rows 256..299 in the gx' it sends (the strip kernel rewrites rup(B, 256) rows), beside ids that must be -1.  (A
    scratch library whose k_pad_ids repeats the shard's last id fails every case here.  At max_batch 256 no rows are left
    over: the repeated ids carry zero gradients and only decay that example's rows by (ldT - B) * 2 lambda_fm lr / G = 5e-5
    of their value, which leaves the bounds by a factor of 1.04 (bf16, B) to 1.5 (f32, A; three ranks: 4.6); with rows left
    over, at max_batch 300, the factor is 10 to 400 -- hence the second bf16 case.)"""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    assert dp_path(F, K, H1, H2) == 'strip'
    i = EXCH.index((F, K, H1, H2, max_batch, shards, prec))
    G, steps, world = sum(shards), 3, len(shards)
    cuts = rotating_cuts(shards, steps)
    case = (F, K, H1, H2, G, steps, KINDS[i % 3], 20 + i)
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    ref_dense, ref_rows = fm_single(F, K, H1, H2, G, steps, case[6], case[7], MS_LR, prec)
    states, losses, calls, sizes = run_native(
        lambda: make_engine(F, K, H1, H2, rows, fo, p, prec=prec, max_batch=max_batch, lr=MS_LR, lam1=LAM1, lamfm=LAMFM),
        world, 'exchange', 'slabs', ids, y, r1, r2, G, cuts, steps)
    check_counts(calls, sizes, plan(F, K, H1, H2, max_batch=max_batch), 'slabs', 'exchange', steps, F)
    bd = Bounds()
    touched = np.unique(ids[ids >= 0])
    untouched = np.setdiff1d(np.arange(rows.shape[0]), touched)
    change = np.abs(ref_rows[touched] - rows[touched].astype(np.float32)).max()
    assert len(untouched)
    if prec == 'f32':
        rows64, p64, _, ref_losses = fm_oracle(F, K, H1, H2, G, steps, case[6], case[7], MS_LR)
        for s in range(steps):
            bd.close('A loss of step %d' % s, sum(l[s] for l in losses), ref_losses[s], 1e-4, 0.0)
    for r, (d, tab, _) in enumerate(states):
        if prec == 'f32':
            bd.close('rank%d A table' % r, tab, rows64, 1e-4, 1e-6)
            for k in DENSE:
                bd.close('rank%d A %s' % (r, k), d[k], p64[k], 1e-4, 1e-6)
        bd.close('rank%d B table' % r, tab[touched], ref_rows[touched], 0.0, 3e-4 * change + 1e-7)
        dense_b(bd, 'rank%d' % r, d, ref_dense, p, 5e-4)
        assert np.array_equal(tab[untouched], rows[untouched]), r
        assert np.array_equal(tab, states[0][1]), r             # replicas stay identical
    assert_same_dense(states)
    if prec == 'f32':           # the final state's predictions on the whole feed (set / get round-trip bit for bit: test_gpu_shapes)
        d, tab, _ = states[0]
        eng = make_engine(F, K, H1, H2, tab, fo, d, max_batch=max_batch, lr=MS_LR, lam1=LAM1, lamfm=LAMFM)
        try:
            pr = eng.predict(ids).cpu().numpy()
        finally:
            eng.close()
        bd.close('A predictions', pr, orc.predict(p64, orc.gather_vec(rows64, ids, -3.0)), 2e-4, 1e-6)
    bd.report(_xid((F, K, H1, H2, max_batch, shards, prec)))


# ------------------------------------------------------------------------------------------------ 5: exact mode, portable API
@pytest.mark.parametrize("F,K,H1,H2", [(13, 1, 300, 100), (16, 15, 63, 63)], ids=lambda v: str(v))
def test_exact_mode_through_the_portable_api(built, monkeypatch, F, K, H1, H2):
    """fnn_step_begin, fnn_sparse_grad, a host-side concatenation (the shorter shard padded with -1 ids) and
    fnn_step_scatter_global on both engines, the buckets summed as test_gpu_shapes' data-parallel test does: two steps at
    k = 1 and k = 15; both tables equal the single engine's at the bound of
    test_virtual_two_rank_exchange_mode_equals_single_gpu_tables and are bit-identical to each other."""
    import torch
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    G, steps, cut = 500, 2, [slice(0, 256), slice(256, 500)]
    case = (F, K, H1, H2, G, steps, 'empty', 40 + K)
    rows, fo, ids, y, p, r1, r2 = fm_problem(*case)
    kw = dict(lr=0.01, lam1=LAM1, lamfm=LAMFM)
    ref_dense, ref_rows = fm_single(F, K, H1, H2, G, steps, case[6], case[7], 0.01, 'f32')
    ranks = [make_engine(F, K, H1, H2, rows, fo, p, **kw) for _ in range(2)]
    try:
        for s in range(steps):
            ids_s, y_s = ids[s * G:(s + 1) * G], y[s * G:(s + 1) * G]
            buckets = [e.step_begin(ids_s[h], y_s[h], r1, r2, b_size=G) for e, h in zip(ranks, cut)]
            assert buckets[0].numel() == plan(F, K, H1, H2)['bucket']
            dev = buckets[0].device
            ids_g = torch.full((512, F), -1, dtype=torch.int32, device=dev)
            gx_g = None
            for r, (e, h) in enumerate(zip(ranks, cut)):
                e.sync()
                n = h.stop - h.start
                sg = e.sparse_grad(n)
                if gx_g is None:
                    assert sg.shape[1] == plan(F, K, H1, H2)['K1p']
                    gx_g = torch.zeros((512, sg.shape[1]), dtype=torch.float32, device=dev)
                ids_g[256 * r:256 * r + n] = torch.as_tensor(ids_s[h]).to(dev)
                gx_g[256 * r:256 * r + n] = sg
            tot = buckets[0] + buckets[1]
            torch.cuda.synchronize()
            for b in buckets:
                b.copy_(tot)
            torch.cuda.synchronize()
            for e in ranks:
                e.step_scatter_global(ids_g, gx_g)
                e.step_end()
                e.sync()
        bd = Bounds()
        touched = np.unique(ids[ids >= 0])
        untouched = np.setdiff1d(np.arange(rows.shape[0]), touched)
        change = np.abs(ref_rows[touched] - rows[touched].astype(np.float32)).max()
        tabs = [e.get_table() for e in ranks]
        for r, e in enumerate(ranks):
            bd.close('rank%d B table' % r, tabs[r][touched], ref_rows[touched], 0.0, 2e-4 * change + 1e-7)
            assert np.array_equal(tabs[r][untouched], ref_rows[untouched])
            dense_b(bd, 'rank%d' % r, e.get_dense(), ref_dense, p, 5e-4)
        assert np.array_equal(tabs[0], tabs[1])
        bd.report(case_id(F, K, H1, H2, G, 'portable-exact'))
    finally:
        for e in ranks:
            e.close()


# ------------------------------------------------------------------------------------------------ 6: bag mode
BAG = [(39, 300, 300, 100), (16, 192, 256, 64), (64, 252, 63, 63), (2, 316, 319, 127)]
BAG_LR = 0.01


def bag_id(F, h0, H1, H2, *rest):
    return '-'.join(['bag-F%d-h%d-H%dx%d' % (F, h0, H1, H2)] + [str(r) for r in rest])


@functools.lru_cache(maxsize=None)
def bag_problem(F, h0, H1, H2, G, steps, layout, n_rows):
    kw = dict(dup_col=(F // 3) or (F - 1), empty=batch_empties(G, F, steps)) if layout == 'fields' else {}
    prob = make_snn_problem(steps * G, n_rows=n_rows, h0=h0, seed=F + h0, n_fields=F, h1=H1, h2=H2, layout=layout, **kw)
    prob[5][0] = prob[6][0] = 1                                 # one-unit layers stay live
    return prob


def bag_engine(prob, F, h0, H1, H2, max_batch=4096):
    return make_snn_engine(prob[0], prob[1], prob[4], lr=BAG_LR, lam1=LAM1, h0=h0, max_batch=max_batch, n_fields=F, h1=H1, h2=H2)


@functools.lru_cache(maxsize=None)
def bag_refs(F, h0, H1, H2, G, steps, layout, n_rows):
    """A: orc.snn_train_step over the global batches; B: one engine stepping them."""
    prob = bag_problem(F, h0, H1, H2, G, steps, layout, n_rows)
    ww0, bb0, ids, y, p, r1, r2 = prob
    ww64, bb64, p64, losses = ww0.astype(np.float64), bb0.astype(np.float64), copy_p(p), []
    for s in range(steps):
        sl = slice(s * G, (s + 1) * G)
        losses.append(orc.snn_train_step(p64, ww64, bb64, ids[sl], y[sl].astype(np.float64), r1.astype(float), r2.astype(float),
                                         BAG_LR, LAM1, vec=True)['loss'])
    eng = bag_engine(prob, F, h0, H1, H2)
    try:
        for s in range(steps):
            eng.train_step(ids[s * G:(s + 1) * G], y[s * G:(s + 1) * G], r1, r2, want_loss=False)
        single = (eng.get_dense(), eng.get_table(), eng.get_bag_bias())
    finally:
        eng.close()
    return (ww64, bb64, p64, losses), single


def bag_dense_a(bd, tag, d, bias, p64, bb64, p, bb0):
    """test_gpu_snn_shapes.check_step's f32 bounds for the six dense tensors and the bag bias."""
    for k in DENSE:
        bd.close('%s A %s' % (tag, k), d[k], p64[k], 0.0, 1e-3 * (np.abs(p64[k] - p[k]).max() + 1e-12) + 1e-7)
    bd.close('%s A b3' % tag, d['b3'], p64['b3'], 0.0, 1e-3 * (abs(p64['b3'] - p['b3']) + 1e-12) + 1e-7)
    bd.close('%s A bag bias' % tag, bias, bb64, 0.0, 1e-3 * (np.abs(bb64 - bb0).max() + 1e-12) + 2e-7)


def bag_dense_b(bd, tag, d, bias, ref_dense, ref_bb, p, bb0, tol=5e-4):
    """test_two_virtual_ranks_bag_mode_native's bounds against the single engine (5e-4 of the change)."""
    dense_b(bd, tag, d, ref_dense, p, tol)
    bd.close('%s B bag bias' % tag, bias, ref_bb, 0.0, tol * np.abs(ref_bb - bb0).max() + 1e-7)


@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
@pytest.mark.parametrize("F,h0,H1,H2", BAG, ids=[bag_id(*c) for c in BAG])
def test_two_ranks_bag_mode_local(built, monkeypatch, F, h0, H1, H2, payload):
    """FNN_MODE_BAG, one LOCAL step, 257 + 243: the slabs carry the bag-bias block behind the 64-wide w3 slab (off_bag), the
    bucket carries the bias behind nw.  Dense tensors and the bag bias against A and B; rows one rank alone touched as
    test_two_virtual_ranks_bag_mode_native checks them (rtol 1e-5 / atol 2e-7 against the single engine) and against A."""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    monkeypatch.delenv('FNN_STEP1_WAVES', raising=False)
    G, cuts = 500, cuts_of((257, 243))
    key = (F, h0, H1, H2, G, 1, 'fields', 1000)
    prob = bag_problem(*key)
    ww0, bb0, ids, y, p, r1, r2 = prob
    (ww64, bb64, p64, ref_losses), (ref_dense, ref_rows, ref_bb) = bag_refs(*key)
    states, losses, calls, sizes = run_native(lambda: bag_engine(prob, F, h0, H1, H2), 2, 'local', payload, ids, y, r1, r2, G, cuts)
    check_counts(calls, sizes, plan(F, 0, H1, H2, h0=h0), payload, 'local', 1, F)
    bd = Bounds()
    bd.close('A loss', losses[0][0] + losses[1][0], ref_losses[0], 0.0, 2e-5 * max(1.0, abs(ref_losses[0])))
    own, touched = alone(ids, cuts)
    untouched = np.setdiff1d(np.arange(ww0.shape[0]), touched)
    upd = np.abs(ww64 - ww0).max() + 1e-12
    assert all(len(o) for o in own)
    for r, (d, tab, bias) in enumerate(states):
        bag_dense_a(bd, 'rank%d' % r, d, bias, p64, bb64, p, bb0)
        bag_dense_b(bd, 'rank%d' % r, d, bias, ref_dense, ref_bb, p, bb0)
        bd.close('rank%d A own rows' % r, tab[own[r]], ww64[own[r]], 0.0, 1e-3 * upd + 2e-7)
        bd.close('rank%d B own rows' % r, tab[own[r]], ref_rows[own[r]], 1e-5, 2e-7)
        assert np.array_equal(tab[own[1 - r]], ww0[own[1 - r]]) and np.array_equal(tab[untouched], ww0[untouched]), r
    assert_same_dense(states)
    bd.report(bag_id(F, h0, H1, H2, 'local', payload))


BAGX = [(16, 192, 256, 64, 'fields', 1000), (39, 300, 300, 100, 'active', 600)]


@pytest.mark.parametrize("F,h0,H1,H2,layout,n_rows", BAGX, ids=[bag_id(*c[:5]) for c in BAGX])
def test_two_ranks_bag_mode_exchange(built, monkeypatch, F, h0, H1, H2, layout, n_rows):
    """FNN_MODE_BAG under EXCHANGE for two steps on handles of max_batch 512, shards 330 + 170, then 170 + 330 (neither fills
    ldT, and rank 0's second shard leaves rows 256..329 of the first step's deltas in the buffer it sends, beside ids that
    must be -1): the gathered shards replay one after the other.  Tables, bag bias and dense tensors against A and B at
    test_two_virtual_ranks_bag_mode_exchange's bounds (tables 3e-4 of the change, dense and bias 5e-4).  `fields`: no row
    sits in two columns, every sum has a fixed order, and the replicas are bit-identical.  `active` (the reference's own
    feed, at the cx5 strip instance): most touched rows sit in several columns and take the float-atomic branch, whose order
    is not fixed -- the replicas are held to each other at the same bound as to the references, not bit for bit."""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    monkeypatch.delenv('FNN_STEP1_WAVES', raising=False)
    G, steps = 500, 2
    cuts = rotating_cuts((330, 170), steps)
    key = (F, h0, H1, H2, G, steps, layout, n_rows)
    prob = bag_problem(*key)
    ww0, bb0, ids, y, p, r1, r2 = prob
    if layout == 'active':
        from test_gpu_snn_shapes import shared_rows
        for s in range(steps):
            for c in cuts[s]:
                assert shared_rows(ids[s * G:(s + 1) * G][c])[0] > 20
    (ww64, bb64, p64, ref_losses), (ref_dense, ref_rows, ref_bb) = bag_refs(*key)
    states, losses, calls, sizes = run_native(lambda: bag_engine(prob, F, h0, H1, H2, max_batch=512), 2, 'exchange', 'slabs',
                                              ids, y, r1, r2, G, cuts, steps)
    check_counts(calls, sizes, plan(F, 0, H1, H2, h0=h0, max_batch=512), 'slabs', 'exchange', steps, F)
    bd = Bounds()
    touched = np.unique(ids[ids >= 0])
    untouched = np.setdiff1d(np.arange(ww0.shape[0]), touched)
    change = np.abs(ref_rows[touched] - ww0[touched]).max()
    bch = np.abs(ref_bb - bb0).max()
    for s in range(steps):
        bd.close('A loss of step %d' % s, losses[0][s] + losses[1][s], ref_losses[s], 0.0, 5e-5 * max(1.0, abs(ref_losses[s])))
    for r, (d, tab, bias) in enumerate(states):
        bd.close('rank%d A table' % r, tab[touched], ww64[touched], 0.0, 3e-4 * change + 1e-7)
        bd.close('rank%d B table' % r, tab[touched], ref_rows[touched], 0.0, 3e-4 * change + 1e-7)
        assert np.array_equal(tab[untouched], ww0[untouched]), r
        dense_b(bd, 'rank%d' % r, d, ref_dense, p, 5e-4)
        dense_b(bd, 'rank%d' % r, d, p64, p, 5e-4, which='A')
        bd.close('rank%d B bag bias' % r, bias, ref_bb, 0.0, 5e-4 * bch + 1e-7)
        bd.close('rank%d A bag bias' % r, bias, bb64, 0.0, 5e-4 * bch + 1e-7)
    (d0, t0, b0), (d1, t1, b1) = states
    if layout == 'fields':
        assert np.array_equal(t0, t1) and np.array_equal(b0, b1)
        assert_same_dense(states)
    else:
        bd.close('rank1 table to rank0', t1[touched], t0[touched], 0.0, 3e-4 * change + 1e-7)
        bd.close('rank1 bag bias to rank0', b1, b0, 0.0, 5e-4 * bch + 1e-7)
        dense_b(bd, 'rank1 to rank0', d1, d0, p, 5e-4)
        print("\n[dp shapes] active layout: replicas' tables bit-identical this run: %s" % np.array_equal(t0, t1))
    bd.report(bag_id(F, h0, H1, H2, layout, 'exchange'))


# ------------------------------------------------------------------------------------------------ 7: world size 1, bit for bit
WORLD1 = [('fm', 13, 15, 63, 63, 'f32'), ('fm', 16, 4, 319, 127, 'bf16'), ('fm', 39, 11, 500, 255, 'f32'),
          ('fm',) + WIDE + ('f32',), ('bag', 39, 300, 300, 100, 'f32')]


@pytest.mark.parametrize("mode,F,K,H1,H2,prec", WORLD1,
                         ids=[(bag_id(*c[1:5]) if c[0] == 'bag' else cid(*c[1:5], None, c[5])) for c in WORLD1])
def test_world_one_bucket_and_p2p_are_the_plain_step(built, monkeypatch, mode, F, K, H1, H2, prec):
    """test_world_one_bucket_payload_and_p2p_are_the_single_gpu_step at other shapes: the bucket payload through real RCCL
    (launch 3 without its update or, on the layer-by-layer path, k_reduce; the all-reduce of nw + nbag floats; k_update) and
    the P2P collective over the one region (k_p2p_update: nw12 / 4 float4 items, then nw - nw12 + nbag scalars, (row, column)
    rebuilt from K1p / H1p / H2p for the w1 / w1t / w2 / w2t shadows) leave, after three steps, the bits of a plain engine:
    losses, dense tensors, table, bag bias.  (K is h0 in the bag case.)"""
    monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    B, steps = 300, 3
    if mode == 'bag':
        prob = bag_problem(F, K, H1, H2, B, steps, 'fields', 1000)   # no row in two columns: every sum of the step has a fixed order

        def mk():
            return bag_engine(prob, F, K, H1, H2)
    else:
        prob = fm_problem(F, K, H1, H2, B, steps, 'empty', 60)

        def mk():
            return make_engine(F, K, H1, H2, prob[0], prob[1], prob[4], prec=prec, lr=0.01, lam1=LAM1, lamfm=LAMFM)
    _, _, ids, y, _, r1, r2 = prob
    plain, bk, pp = mk(), mk(), mk()
    try:
        bk.dp_init(0, 1, FNNEngine.dp_unique_id())
        bk.dp_set_payload('bucket')
        pp.dp_init(0, 1, FNNEngine.dp_unique_id())
        _p2p_same_process([pp])                                 # ONE engine: no second rank of this process on the P2P collective
        assert bk.dp_config()['payload'] == 'bucket' and pp.dp_config()['collective'] == 'p2p'
        for e in (bk, pp):
            e.prof_enable(True)
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            a = plain.train_step(ids[sl], y[sl], r1, r2)
            for e in (bk, pp):
                assert e.train_step(ids[sl], y[sl], r1, r2, b_size=B)['loss'] == a['loss'], s
        assert bk.prof_get('allreduce')[1] == steps and pp.prof_get('allreduce')[1] == 0 and pp.prof_get('p2p_update')[1] == steps
        da, ta = plain.get_dense(), plain.get_table()
        assert not np.array_equal(da['w1'], np.asarray(prob[4]['w1'], np.float32))
        for e in (bk, pp):
            db = e.get_dense()
            for k in da:
                assert np.array_equal(da[k], db[k]), k
            assert np.array_equal(ta, e.get_table())
            if mode == 'bag':
                assert np.array_equal(plain.get_bag_bias(), e.get_bag_bias())
    finally:
        for e in (plain, bk, pp):
            e.close()
