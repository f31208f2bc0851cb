"""The bf16 weight-gradient products (wgrad_tile) have two forms: `direct` (every wave loads its A fragment and the block's four B
fragments from global memory) and `lds` (the workgroup stages the slice's fragments through LDS, a stage of four k-steps at a
time in two buffers; FNN_WGRAD_FORM, read by fnn_create).  Both issue the same MFMAs into the same accumulators in the same
k order, so everything a step leaves behind must agree bit for bit: two handles with the same state, one per form, take three
training steps on the same batches, and the six dense tensors, the gradient bucket and the table rows of the last batch are
compared with np.array_equal.

What the staging can get wrong depends on the k-steps per slice, nkt = rup(B, 256) / split-K / 32 in bf16, against the stage of 4
and the two buffers (8 k-steps requested ahead):
  B = 16    one strip; nkt = 1 (split-K 8) or 2 (4): a slice shorter than a stage, most slices all padding;
  B = 48    nkt as at 16, slices of unequal use;
  B = 520   rup = 768: nkt = 3 (a ragged single stage) or 6 (a whole stage and a ragged one); the last strip is half empty, so
            the batch padding reaches the operands;
  B = 2600  rup = 2816: nkt = 11 (4 + 4 + 3: a buffer requested again, and a ragged last stage) or 22;
  B = 4096  nkt = 16 or 32: whole stages only, every buffer requested again.
Fields and k: 16 fields (the three-launch step, k_step2) and 4 fields (K1p = 64: the layer-by-layer kernels, k_wgrad) at
k = 10; 16 fields at k = 1 and k = 15, the ends of what 16-float rows take.  Hidden 300 / 100, and 40 / 20, the smallest pair of
padded sizes the strip kernel is built for (64 / 64: the products have 3, 2 and 1 live column fragments of the four loaded).
Every batch has an id of -1.  Also: FNN_NO_FUSE=1 (k_wgrad at 16 fields), steps without fnn_prefetch_ids, a bf16 bag-mode handle
(the SNN step: a fourth product, the bias gradient), and an f32 and a bf16x3 handle, which keep their register ring under `lds`.
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
NSTEP = 3


def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


_PROBLEMS = {}


def problem_of(B, F=16, K=10, H1=300, H2=100, h0=0):
    """NSTEP batches of ids / labels and one set of weights; computed once per shape."""
    key = (B, F, K, H1, H2, h0)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rng = np.random.RandomState(B + 7)
    if h0:
        from test_gpu_parity import make_snn_problem
        ww0, bb0, _, _, p, r1, r2 = make_snn_problem(B, n_rows=600, h0=h0, seed=3, n_fields=F, h1=H1, h2=H2, layout='fields')
        ids = [make_snn_problem(B, n_rows=600, h0=h0, seed=10 + s, n_fields=F, h1=H1, h2=H2, layout='fields')[2] for s in range(NSTEP)]
        pb = dict(rows=ww0, bb0=bb0, p=p)
    else:
        sizes = synth.field_sizes_tiny(1000, n_fields=F)
        p = orc.init_fnn_weights(1 + F * K, H1, H2, 'tanh', seed=1234)
        p['w3'] = rng.uniform(-0.2, 0.2, H2)
        p['b1'] = rng.uniform(-0.1, 0.1, H1)
        p['b2'] = rng.uniform(-0.1, 0.1, H2)
        p['b3'] = 0.05
        p = {k: (f32r(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
        r1 = (rng.uniform(size=H1) < 0.5).astype(np.uint8)
        r2 = (rng.uniform(size=H2) < 0.5).astype(np.uint8)
        ids = [synth.zipf_ids(B, sizes, 1.1, 20 + s) for s in range(NSTEP)]
        pb = dict(rows=synth.fm_table(sum(sizes), K, 0.05, 5), fo=synth.field_of_row(sizes), p=p)
    for i in ids:
        i[B // 2, 1] = -1                                        # an absent field
    r1[0] = r2[0] = 1
    pb.update(B=B, F=F, K=K, H1=H1, H2=H2, h0=h0, ids=ids, y=(rng.uniform(size=(NSTEP, B)) < 0.3).astype(np.float32), r1=r1, r2=r2)
    _PROBLEMS[key] = pb
    return pb


def run(monkeypatch, pb, form, prec='bf16', splitk=None, prefetch=True, no_fuse=False):
    """NSTEP training steps under FNN_WGRAD_FORM=`form` (None: unset) -> (dense tensors, gradient bucket, rows of the last batch[, bag bias])."""
    import torch
    if form is None:
        monkeypatch.delenv('FNN_WGRAD_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_WGRAD_FORM', form)
    if splitk is None:
        monkeypatch.delenv('FNN_SPLITK', raising=False)
    else:
        monkeypatch.setenv('FNN_SPLITK', str(splitk))
    if no_fuse:
        monkeypatch.setenv('FNN_NO_FUSE', '1')
    else:
        monkeypatch.delenv('FNN_NO_FUSE', raising=False)
    h0 = pb['h0']
    lr = 0.001 if pb['B'] >= 2048 else LR
    if h0:
        eng = FNNEngine(pb['F'], 0, pb['H1'], pb['H2'], max_batch=4096, precision=prec, lr=lr, lambda1=0.001, lambda_fm=0.0,
                        reg_all=True, mode='bag', hidden0=h0)
    else:
        eng = FNNEngine(pb['F'], pb['K'], pb['H1'], pb['H2'], max_batch=4096, precision=prec, lr=lr, lambda1=LAM1, lambda_fm=LAMFM)
    try:
        if h0:
            eng.set_table(pb['rows'], np.zeros(pb['rows'].shape[0], np.int32), 0.0)
            eng.set_bag_bias(pb['bb0'])
        else:
            eng.set_table(pb['rows'], pb['fo'], W0)
        eng.set_dense(pb['p'])
        dev_ids = [torch.as_tensor(i).to(eng.device).contiguous() for i in pb['ids']]
        for s in range(NSTEP):
            if prefetch and s + 1 < NSTEP:
                eng.prefetch_ids(dev_ids[s + 1])
            eng.train_step(dev_ids[s], pb['y'][s], pb['r1'], pb['r2'], want_loss=False)
        eng.sync()
        last = pb['ids'][-1]
        rows = eng.get_rows(np.unique(last[last >= 0]))
        return eng.get_dense(), eng.grad_bucket().cpu().numpy().copy(), rows, (eng.get_bag_bias() if h0 else None)
    finally:
        eng.close()


def assert_same_bits(a, b, pb):
    for k in DENSE:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert a[0]['b3'] == b[0]['b3']
    assert np.array_equal(a[1], b[1]), "gradient bucket: %d of %d floats differ" % ((a[1] != b[1]).sum(), a[1].size)
    assert np.array_equal(a[2], b[2]), "rows of the last batch"
    if a[3] is not None:
        assert np.array_equal(a[3], b[3]), "bag bias"
    # the steps did something: the gradients are not all zero and the first layer moved
    assert np.any(a[1] != 0) and not np.array_equal(a[0]['w1'], np.asarray(pb['p']['w1'], np.float32))


def both(monkeypatch, pb, **kw):
    d = run(monkeypatch, pb, 'direct', **kw)
    l = run(monkeypatch, pb, 'lds', **kw)
    assert_same_bits(d, l, pb)


@gpu
@pytest.mark.parametrize("splitk", [4, 8])
@pytest.mark.parametrize("B", [16, 48, 520, 2600, 4096])
def test_forms_are_bit_identical_three_launch_step(built, monkeypatch, B, splitk):
    both(monkeypatch, problem_of(B), splitk=splitk)


@gpu
@pytest.mark.parametrize("splitk", [4, 8])
@pytest.mark.parametrize("B", [16, 520])
def test_forms_are_bit_identical_smallest_hidden_pair(built, monkeypatch, B, splitk):
    both(monkeypatch, problem_of(B, H1=40, H2=20), splitk=splitk)


@gpu
@pytest.mark.parametrize("F,K", [(4, 10), (16, 1), (16, 15)])
@pytest.mark.parametrize("B", [48, 520])
def test_forms_are_bit_identical_fields_and_ranks(built, monkeypatch, B, F, K):
    both(monkeypatch, problem_of(B, F=F, K=K), splitk=8)


@gpu
@pytest.mark.parametrize("B,splitk", [(48, 8), (520, 4), (4096, None)])
def test_forms_are_bit_identical_layer_by_layer(built, monkeypatch, B, splitk):
    """FNN_NO_FUSE=1: the stand-alone k_wgrad (split-K 4 unless told otherwise)."""
    both(monkeypatch, problem_of(B), splitk=splitk, no_fuse=True)


@gpu
@pytest.mark.parametrize("B,splitk", [(48, 4), (520, 8), (4096, 8)])
def test_forms_are_bit_identical_without_prefetch(built, monkeypatch, B, splitk):
    """No fnn_prefetch_ids: launch 2 carries no sort role, every step groups its own batch first."""
    both(monkeypatch, problem_of(B), splitk=splitk, prefetch=False)


@gpu
@pytest.mark.parametrize("B", [100, 520])
def test_forms_are_bit_identical_bag_mode(built, monkeypatch, B):
    """The SNN step in bf16 (h0 = 200, 13 columns, hidden 40 / 20, a table of 600 rows): four products, the last one the bias
    gradient against the ones matrix.  Every row stays in one column (rows shared by columns take float atomics)."""
    both(monkeypatch, problem_of(B, F=13, K=0, H1=40, H2=20, h0=200))


@gpu
@pytest.mark.parametrize("prec", ['f32', 'bf16x3'])
def test_other_precisions_do_not_take_the_lds_form(built, monkeypatch, prec):
    both(monkeypatch, problem_of(520), prec=prec)


@gpu
def test_default_of_a_bf16_three_launch_handle_is_lds_at_split_k_4(built, monkeypatch):
    """With nothing set, a bf16 handle on FM rows with max_batch > 256 whose steps take the three launches runs the LDS form
    with four K slices; FNN_WGRAD_FORM=direct alone runs eight, as before the LDS form existed."""
    pb = problem_of(520)
    dflt = run(monkeypatch, pb, None)
    assert_same_bits(dflt, run(monkeypatch, pb, 'lds', splitk=4), pb)
    direct = run(monkeypatch, pb, 'direct')
    assert_same_bits(direct, run(monkeypatch, pb, 'direct', splitk=8), pb)
    assert not np.array_equal(dflt[1], direct[1])                # four slices and eight round differently
