"""In bf16 on FM rows the strip kernel writes its transposed activations (x'^T, d1^T, d2^T, delta2^T, delta1^T) either 8 bytes
per lane (a lane's 4 examples of a column) or, with bit 32 of FNN_WT_STORES (the default, 47), 16 bytes per lane after a
v_permlane16_swap between 16-lane rows.  The bytes and their addresses are the same, so everything a step computes must agree bit
for bit: 15 against 47 (written through) and 0 against 32 (plain stores), after two steps, on the table, the six dense tensors,
the loss and the gx' the step returns.  (The 8-byte arms are the stores the rest of the suite holds to the float64 oracle.)
Bag mode (x'^T from the LDS tile, delta_x^T) keeps the 8-byte stores -- the 16-byte form was level there and is not in the code --
so its cases check that the bit changes nothing; their ids keep every row in one column: rows shared by several columns take
float atomics, whose order no store form decides.

Shapes: the k_step1<5, 2, ..> instances at hidden 300 / 100 with eight waves (runs of 3 and 1 tiles per wave: pairs, an unpaired
last tile, clipped runs) and with FNN_STEP1_WAVES=4 (runs of 5, 2 and 4), <1, 1, ..> at hidden 40 / 20 (single tiles; 13 fields:
the gather's last group of 16 pieces is half full), bag mode at h0 = 200 (CX = 4) and 300 (CX = 5).  Batches of 16 (one strip), 40 (a partial last strip: the rows past B stay
zero in both halves of a slot -- the weight gradients read them), 100 and 272 (strips in both halves of a 32-example fragment).
"""
import numpy as np
import pytest

from oracle import fnn_oracle as orc

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.engine import FNNEngine

gpu = pytest.mark.gpu

LR, LAM1, LAMFM, W0 = 0.01, 0.02, 0.1, -3.0
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
BS = [16, 40, 100, 272]
NSTEP = 6
# name -> (F, K, H1, H2, bag h0 or 0, FNN_STEP1_WAVES)
SHAPES = {'c5x2-nw8': (16, 11, 300, 100, 0, 8), 'c5x2-nw4': (16, 11, 300, 100, 0, 4), 'c1x1': (13, 11, 40, 20, 0, 8),
          'bag-cx4-c1x1': (13, 0, 40, 20, 200, 8), 'bag-cx5-c5x2-nw8': (17, 0, 300, 100, 300, 8), 'bag-cx4-c5x2-nw4': (13, 0, 300, 100, 200, 4)}


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


_PROBLEMS = {}


def problem_of(shape, B):
    """NSTEP batches of ids / labels and one set of weights; computed once per (shape, B)."""
    if (shape, B) in _PROBLEMS:
        return _PROBLEMS[(shape, B)]
    F, K_, H1, H2, h0, _ = SHAPES[shape]
    rng = np.random.RandomState(B + 7)
    if h0:
        from test_gpu_parity import make_snn_problem
        ww0, bb0, _, _, p, r1, r2 = make_snn_problem(B, n_rows=600, h0=h0, seed=3, n_fields=F, h1=H1, h2=H2, layout='fields')
        ids = [make_snn_problem(B, n_rows=600, h0=h0, seed=10 + s, n_fields=F, h1=H1, h2=H2, layout='fields')[2] for s in range(NSTEP)]
        pb = dict(rows=ww0, bb0=bb0, p=p)
    else:
        sizes = synth.field_sizes_tiny(1000, n_fields=F)
        p = orc.init_fnn_weights(1 + F * K_, H1, H2, 'tanh', seed=1234)
        p['w3'] = rng.uniform(-0.2, 0.2, H2)
        p['b1'] = rng.uniform(-0.1, 0.1, H1)
        p['b2'] = rng.uniform(-0.1, 0.1, H2)
        p['b3'] = 0.05
        p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
        r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
        r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
        ids = [synth.zipf_ids(B, sizes, 1.1, 20 + s) for s in range(NSTEP)]
        for i in ids:
            i[B // 2, 1] = -1                                    # an empty field
        pb = dict(rows=synth.fm_table(sum(sizes), K_, 0.05, 5), fo=synth.field_of_row(sizes), p=p)
    r1[0] = r2[0] = 1
    pb.update(shape=shape, B=B, ids=ids, y=(rng.uniform(size=(NSTEP, B)) < 0.3).astype(np.float32), r1=r1, r2=r2)
    _PROBLEMS[(shape, B)] = pb
    return pb


def run(monkeypatch, pb, stores, prec='bf16', steps=2, prefetch=False):
    """`steps` training steps under FNN_WT_STORES=`stores` -> (table, dense tensors, losses, gx' of every step[, bag bias])."""
    import torch
    F, K_, H1, H2, h0, waves = SHAPES[pb['shape']]
    monkeypatch.setenv('FNN_WT_STORES', str(stores))
    monkeypatch.setenv('FNN_STEP1_WAVES', str(waves))
    if h0:
        eng = FNNEngine(F, 0, H1, H2, max_batch=512, precision=prec, lr=LR, lambda1=0.001, lambda_fm=0.0, reg_all=True, mode='bag',
                        hidden0=h0)
    else:
        eng = FNNEngine(F, K_, H1, H2, max_batch=512, precision=prec, lr=LR, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        if h0:
            eng.set_table(pb['rows'], np.zeros(pb['rows'].shape[0], np.int32), 0.0)
            eng.set_bag_bias(pb['bb0'])
        else:
            eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids'][:steps]]
        loss, gx = [], []
        for s in range(steps):
            if prefetch and s + 1 < steps:
                eng.prefetch_ids(dev_ids[s + 1])
            out = eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_gx=True)
            loss.append(out['loss'])
            gx.append(out['gx'].cpu().numpy())
        eng.sync()
        return eng.get_table(), eng.get_dense(), loss, gx, (eng.get_bag_bias() if h0 else None)
    finally:
        eng.close()


def assert_same_bits(a, b):
    assert np.array_equal(a[0], b[0]), "table: %d of %d floats differ" % ((a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[1]['b3'] == b[1]['b3']
    assert a[2] == b[2], "loss"
    for s in range(len(a[3])):
        assert np.array_equal(a[3][s], b[3][s]), "gx' of step %d" % s
    if a[4] is not None:
        assert np.array_equal(a[4], b[4]), "bag bias"


@gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_16_byte_stores_are_bit_identical(built, monkeypatch, shape, B):
    pb = problem_of(shape, B)
    for old, new in ((15, 47), (0, 32)):
        a = run(monkeypatch, pb, old)
        b = run(monkeypatch, pb, new)
        assert not np.array_equal(b[0], pb['rows'])               # the steps did move the rows
        assert np.isfinite(b[2]).all()
        assert_same_bits(a, b)


@gpu
@pytest.mark.parametrize("prec", ['f32', 'bf16x3'])
def test_bit_32_changes_nothing_in_the_4_byte_modes(built, monkeypatch, prec):
    pb = problem_of('c5x2-nw8', 100)
    assert_same_bits(run(monkeypatch, pb, 15, prec=prec), run(monkeypatch, pb, 47, prec=prec))


@gpu
@pytest.mark.parametrize("shape", ['c5x2-nw8', 'bag-cx4-c1x1'])
def test_six_back_to_back_steps_with_prefetch(built, monkeypatch, shape):
    """Every launch follows the one before it at once: a 16-byte write-through store that the weight gradients of launch 2 (or
    the next step) missed would show here."""
    pb = problem_of(shape, 272)
    a = run(monkeypatch, pb, 15, steps=NSTEP, prefetch=True)
    b = run(monkeypatch, pb, 47, steps=NSTEP, prefetch=True)
    assert_same_bits(a, b)
