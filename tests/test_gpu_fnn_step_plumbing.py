"""The host side of the FNN step (fnn_api.hip): the ways into one step that must leave the same bits, and the refusals.

What the neighbouring modules hold against oracles or replay twins -- the fixed and generic strip forms (test_gpu_step1_fixed.py),
replay twins with shadowed features and prefetch (test_gpu_lifecycle.py), the virtual ranks (test_gpu_dp.py, test_gpu_parity.py) --
is not repeated.  Here two or three handles of ONE process take the same inputs through different entry points:

  fnn_train_step           against fnn_step_begin + fnn_step_scatter + fnn_step_end and against fnn_step_begin + fnn_step_end
                           (scatter implied): bf16, f32 and bf16x3 at both strip shapes, and the bag handle (h0 = 200);
  world 1 data parallelism fnn_dp_init_custom with an identity all-reduce, slabs and bucket payload, against the plain step: the
                           four tails of run_step_fast (single, split API, slabs collective, bucket collective) without a second GPU;
  host pointers            FNN_MEM_HOST against device pointers, p_out and gx_out requested;
  refusals                 each refused twice with the same code, an id out of range that rises at the sync, then good steps equal
                           to a twin's that saw no refusal;
  the 4,096 boundary       B = 300, B = 4097 (the smallest batch that leaves the three launches), B = 300 announced by
                           fnn_prefetch_ids, against a replay twin loaded after the second step (test_gpu_lifecycle.py's idiom);
  FNN_ROLE_OFF=0           equals unset.

F = 16, k = 11, max_batch 512, B = 300: pads to 512 (a ragged last strip), and over 256, so that a bf16 handle takes the LDS
weight-gradient form at split-K 4.  Hidden 300 / 100 and 40 / 20 are the two strip shapes.  About 1,000 rows
(synth.field_sizes_tiny), so that rows repeat inside a strip.  Three steps per run.

Every comparison is to the bit: the table, every dense tensor, the bag bias, each step's loss, p, gx where asked for, and the
dense-gradient bucket (every path leaves the step's data term there).  The library built from the commit before the host-side
refactor passes this file unchanged, every pair bit-equal: no pair is held at a bound."""
import ctypes as C

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, synth
from deep_ctr_amd.engine import FNNError

from test_gpu_parity import make_snn_engine, make_snn_problem
from test_gpu_shapes import make_engine, make_problem

pytestmark = pytest.mark.gpu

F_, K, BMAX, B, NROWS, STEPS = 16, 11, 512, 300, 1000, 3
SHAPES = [(300, 100), (40, 20)]
DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
DEV, HOST = _capi.FNN_MEM_DEVICE, _capi.FNN_MEM_HOST


class Problem(object):
    """Parameters and STEPS batches of `b` examples (or the lengths in `lens`), on the host and on the device."""

    def __init__(self, H1, H2, prec, h0=0, lens=None, max_batch=BMAX, lr=0.01, seed=5):
        import torch
        lens = lens or [B] * STEPS
        self.H1, self.H2, self.prec, self.h0, self.max_batch, self.lr = H1, H2, prec, h0, max_batch, lr
        if h0:
            self.rows, self.bb0, ids, y, self.p, r1, r2 = make_snn_problem(sum(lens), n_rows=NROWS, h0=h0, seed=seed, n_fields=F_, h1=H1, h2=H2)
            self.fo = np.zeros(len(self.rows), np.int32)
            self.xdim = h0
        else:
            self.rows, self.fo, ids, y, self.p, r1, r2 = make_problem(F_, K, H1, H2, sum(lens), n_rows=NROWS, seed=seed)
            self.bb0, self.xdim = None, 1 + F_ * K
        ids[1, 2] = -1                                                   # an empty field
        cut = np.cumsum([0] + lens)
        self.ids = [np.ascontiguousarray(ids[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        self.y = [np.ascontiguousarray(y[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        assert all(min(len(np.unique(i[:16, f])) for f in range(F_)) < 16 for i in self.ids)     # rows repeat inside a strip
        rng = np.random.RandomState(seed + 9)
        self.r1 = [(rng.uniform(size=H1) < 0.5).astype(np.uint8) for _ in lens]
        self.r2 = [(rng.uniform(size=H2) < 0.5).astype(np.uint8) for _ in lens]
        for r in self.r1 + self.r2:
            r[0] = 1
        dev = torch.device('cuda', 0)
        self.d = [tuple(torch.as_tensor(a).to(dev).contiguous() for a in it) for it in zip(self.ids, self.y, self.r1, self.r2)]
        torch.cuda.synchronize()

    def engine(self):
        if self.h0:
            return make_snn_engine(self.rows, self.bb0, self.p, prec=self.prec, lr=self.lr, h0=self.h0, max_batch=self.max_batch, n_fields=F_,
                                   h1=self.H1, h2=self.H2)
        return make_engine(F_, K, self.H1, self.H2, self.rows, self.fo, self.p, prec=self.prec, max_batch=self.max_batch, lr=self.lr)


def ck(eng, rc):
    if rc != 0:
        raise FNNError(rc, (eng.lib.fnn_last_error(eng.h) or b'').decode())


def step(eng, pb, s, how='train', mem=DEV):
    """Step s of the problem through one entry point; returns (loss, p, gx, the bucket after the step)."""
    import torch
    n = len(pb.ids[s])
    loss = C.c_float(0.0)
    if mem == HOST:
        ids, y, r1, r2 = (a.ctypes.data for a in (pb.ids[s], pb.y[s], pb.r1[s], pb.r2[s]))
        p, gx = np.empty(n, np.float32), np.empty((n, pb.xdim), np.float32)
        pp, gp = p.ctypes.data, gx.ctypes.data
    else:
        ids, y, r1, r2 = (t.data_ptr() for t in pb.d[s])
        p, gx = torch.empty(n, dtype=torch.float32, device=eng.device), torch.empty((n, pb.xdim), dtype=torch.float32, device=eng.device)
        torch.cuda.synchronize()
        pp, gp = p.data_ptr(), gx.data_ptr()
    if how == 'train':
        ck(eng, eng.lib.fnn_train_step(eng.h, ids, y, n, r1, r2, 0, pp, gp, mem, C.byref(loss)))
    else:
        ck(eng, eng.lib.fnn_step_begin(eng.h, ids, y, n, r1, r2, 0, pp, gp, mem))
        if how == 'split':
            ck(eng, eng.lib.fnn_step_scatter(eng.h))
        else:
            assert how == 'split-implied', how
        ck(eng, eng.lib.fnn_step_end(eng.h, C.byref(loss)))
    eng.sync()
    bucket = eng.grad_bucket().cpu().numpy().copy()
    if mem == DEV:
        p, gx = p.cpu().numpy(), gx.cpu().numpy()
    return float(loss.value), p, gx, bucket


def read(eng, bag):
    return eng.get_table(), eng.get_dense(), (eng.get_bag_bias() if bag else None)


def assert_state_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: table, %d of %d floats differ" % (what, (a[0] != b[0]).sum(), a[0].size)
    for k in DENSE:
        assert np.array_equal(a[1][k], b[1][k]), '%s: %s, %d of %d differ' % (what, k, (a[1][k] != b[1][k]).sum(), a[1][k].size)
    assert a[1]['b3'] == b[1]['b3'], '%s: b3' % what
    if a[2] is not None:
        assert np.array_equal(a[2], b[2]), '%s: bag bias' % what


def assert_step_bits(a, b, what):
    assert np.isfinite(a[1]).all() and np.isfinite(a[0])
    assert a[0] == b[0], '%s: loss %r against %r' % (what, a[0], b[0])
    for name, x, z in (('p', a[1], b[1]), ('gx', a[2], b[2]), ('bucket', a[3], b[3])):
        assert np.array_equal(x, z), '%s: %s, %d of %d differ' % (what, name, (x != z).sum(), x.size)


def run_pair(pb, ways, steps=STEPS):
    """One fresh handle per entry in `ways` -- (name, set-up, how, memory kind) --, all taking the problem's steps; everything is
    held against the first."""
    engs = []
    try:
        for name, setup, how, mem in ways:
            e = pb.engine()
            setup(e)
            engs.append(e)
        rows0 = pb.rows.copy()
        for s in range(steps):
            outs = [step(e, pb, s, how, mem) for e, (name, setup, how, mem) in zip(engs, ways)]
            for o, w in zip(outs[1:], ways[1:]):
                assert_step_bits(outs[0], o, '%s against %s, step %d' % (ways[0][0], w[0], s))
        st = [read(e, bool(pb.h0)) for e in engs]
        assert not np.array_equal(st[0][0], rows0)
        for x, w in zip(st[1:], ways[1:]):
            assert_state_bits(st[0], x, '%s against %s' % (ways[0][0], w[0]))
    finally:
        for e in engs:
            e.close()


def nothing(e):
    pass


SPLIT_CASES = [('%s-%dx%d' % (prec, H1, H2), prec, H1, H2, 0) for prec in ('bf16', 'f32', 'bf16x3') for H1, H2 in SHAPES] + \
              [('bf16-bag-h0_200', 'bf16', 300, 100, 200), ('f32-bag-h0_200', 'f32', 300, 100, 200)]


@pytest.mark.parametrize("name,prec,H1,H2,h0", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_train_step_equals_the_split_api_both_ways(built, name, prec, H1, H2, h0):
    """fnn_train_step == fnn_step_begin + fnn_step_scatter + fnn_step_end == fnn_step_begin + fnn_step_end, bit for bit."""
    pb = Problem(H1, H2, prec, h0=h0)
    run_pair(pb, [('fnn_train_step', nothing, 'train', DEV), ('begin + scatter + end', nothing, 'split', DEV),
                  ('begin + end', nothing, 'split-implied', DEV)])


@pytest.mark.parametrize("payload", ['slabs', 'bucket'])
@pytest.mark.parametrize("H1,H2", SHAPES)
@pytest.mark.parametrize("prec", ['bf16', 'f32'])
def test_world_one_custom_collective_equals_the_plain_step(built, prec, H1, H2, payload):
    """fnn_dp_init_custom at world 1 with an all-reduce that does nothing: the slabs collective between launches 2 and 3 and the
    bucket collective behind launch 3 (with k_update as a fourth launch) leave the plain step's bits."""
    def dp(e):
        e.dp_init_custom(0, 1, lambda view: None, None, sparse='local')
        e.dp_set_payload(payload)
        assert e.dp_config()['payload'] == payload

    run_pair(Problem(H1, H2, prec), [('plain', nothing, 'train', DEV), ('world 1, %s' % payload, dp, 'train', DEV)])


@pytest.mark.parametrize("H1,H2", SHAPES)
@pytest.mark.parametrize("prec", ['bf16', 'f32'])
def test_host_pointers_equal_device_pointers(built, prec, H1, H2):
    """FNN_MEM_HOST goes through the staging buffers: ids, y and the masks up, p and gx back."""
    run_pair(Problem(H1, H2, prec), [('device pointers', nothing, 'train', DEV), ('host pointers', nothing, 'train', HOST)])


def test_refusals_leave_the_handle_as_it_was(built):
    """Every refusal twice, with the same code both times; an id out of range is seen at the sync and consumes the shadowed
    features and the step; afterwards the handle steps like a twin that saw none of it."""
    pb = Problem(300, 100, 'bf16')
    A, T = pb.engine(), pb.engine()
    try:
        lib, h = A.lib, A.h
        ids, y, r1, r2 = (t.data_ptr() for t in pb.d[0])
        big = np.zeros((BMAX + 1, F_), np.int32)
        for _ in range(2):
            assert lib.fnn_train_step(h, big.ctypes.data, y, BMAX + 1, r1, r2, 0, None, None, HOST, None) == _capi.FNN_ERR_ARG
            assert lib.fnn_train_step(h, None, y, B, r1, r2, 0, None, None, DEV, None) == _capi.FNN_ERR_ARG
            assert lib.fnn_step_end(h, None) == _capi.FNN_ERR_STATE          # no step begun
        assert lib.fnn_step_begin(h, ids, y, B, r1, r2, 0, None, None, DEV) == 0
        for _ in range(2):
            assert lib.fnn_step_begin(h, ids, y, B, r1, r2, 0, None, None, DEV) == _capi.FNN_ERR_STATE
        assert lib.fnn_step_end(h, None) == 0
        assert lib.fnn_step_end(h, None) == _capi.FNN_ERR_STATE
        A.sync()
        ck(T, T.lib.fnn_step_begin(T.h, ids, y, B, r1, r2, 0, None, None, DEV))
        ck(T, T.lib.fnn_step_end(T.h, None))
        T.sync()
        assert_state_bits(read(A, False), read(T, False), 'after the refused calls')
        # an id out of range in a step with shadowed features: the step returns, the error rises at the sync, once
        f2 = np.flatnonzero(pb.fo == 2)
        A.set_shadowed(np.array([(t, 2, int(f2[(t + 1) % len(f2)])) for t in (3, 4, 9)], np.int32))
        bad = pb.ids[1].copy()
        bad[7, 3] = len(pb.rows)
        assert lib.fnn_train_step(h, bad.ctypes.data, pb.y[1].ctypes.data, B, pb.r1[1].ctypes.data, pb.r2[1].ctypes.data, 0, None, None, HOST, None) == 0
        assert lib.fnn_sync(h) == _capi.FNN_ERR_RANGE
        assert lib.fnn_sync(h) == 0
        assert lib.fnn_step_end(h, None) == _capi.FNN_ERR_STATE              # the step was consumed
        # both handles from the same parameters again: what the bad step left in the HANDLE (shadowed features, step state, a
        # grouping, the error word) would show in the steps that follow
        for e in (A, T):
            e.set_table(pb.rows, pb.fo, -3.0)
            e.set_dense(pb.p)
        for s in (1, 2):
            assert_step_bits(step(A, pb, s), step(T, pb, s), 'step %d after the refusals' % s)
        assert_state_bits(read(A, False), read(T, False), 'after the good steps')
    finally:
        A.close()
        T.close()


@pytest.mark.parametrize("H1,H2", SHAPES)
def test_across_the_three_launch_boundary(built, H1, H2):
    """max_batch 8192: B = 300 (three launches), B = 4097 (the smallest batch on the layer-by-layer kernels), then B = 300
    announced by fnn_prefetch_ids before the long step, against a fresh twin loaded with the state after the second step."""
    pb = Problem(H1, H2, 'bf16', lens=[300, 4097, 300], max_batch=8192, lr=0.001)
    A, T = pb.engine(), pb.engine()
    try:
        step(A, pb, 0)
        ck(A, A.lib.fnn_prefetch_ids(A.h, pb.d[2][0].data_ptr(), 300))
        step(A, pb, 1)
        mid = read(A, False)
        assert np.isfinite(mid[0]).all() and not np.array_equal(mid[0], pb.rows)
        T.set_table(mid[0], pb.fo, -3.0)
        T.set_dense(mid[1])
        assert_state_bits(read(T, False), mid, 'set / get round trip')
        assert_step_bits(step(A, pb, 2), step(T, pb, 2), 'the step after B = 4097')
        assert_state_bits(read(A, False), read(T, False), 'after the last step')
    finally:
        A.close()
        T.close()


def test_role_off_zero_equals_unset(built, monkeypatch):
    """FNN_ROLE_OFF=0, set explicitly, masks no role.  (Nonzero values are timing experiments: wrong results by construction.)"""
    pb = Problem(300, 100, 'bf16')
    engs = []
    try:
        monkeypatch.delenv('FNN_ROLE_OFF', raising=False)
        engs.append(pb.engine())
        monkeypatch.setenv('FNN_ROLE_OFF', '0')
        engs.append(pb.engine())
        monkeypatch.delenv('FNN_ROLE_OFF')
        for s in range(STEPS):
            assert_step_bits(step(engs[0], pb, s), step(engs[1], pb, s), 'unset against FNN_ROLE_OFF=0, step %d' % s)
        assert_state_bits(read(engs[0], False), read(engs[1], False), 'unset against FNN_ROLE_OFF=0')
    finally:
        for e in engs:
            e.close()
