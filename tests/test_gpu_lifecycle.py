"""One handle across many calls of different kinds and lengths: what the libraries keep between calls (workspaces sized for
max_batch whose pad rows every epilogue must re-zero, keep-mask buffers and the embedding copy that only training steps write,
the dense update left pending on the side stream, the strip-pair flags' epoch, optimiser moments and step counts, FM's lazy
decay scale) against

  A  the float64 oracles playing the same schedule (tests/lifecycle_ref.py), f32 handles: logits / predictions and the loss at
     every item, every parameter at the end, rows no item touched and rows only the first step touched on their own;
  B  a replay twin, bit for bit: handle A plays all but the last step, a fresh handle T is given A's parameters (set / get is
     bit-exact) and both run the last step -- any stale workspace, mask, flag or pending update shows as a bit difference, in
     bf16 as in f32.  SGD only (optimiser state cannot be set from outside); ids from synth.zipf_ids, every row under one field;
  C  parameters set again on a handle that has stepped: ipnn_set_table / fm_set_table restart the optimiser, with the same and
     with another number of rows.

Bounds are the ones the neighbouring modules carry and are not re-derived:
  inner-product SGD   first step: test_ipnn_step_f32_vs_oracle (logits rtol 2e-4 + 2e-5, loss 5e-5 max(1, |loss|)); later steps:
                      test_ipnn_many_steps_at_32_fields_k5 (logits rtol 2e-3 + 2e-4), the loss at 1e-4 max(1, |loss|): the
                      one-step form at the 1e-4 of the five-step FTRL test; parameters within 5e-3 of the oracle's own total
                      change + 1e-6; one step after ipnn_set_table: the one-step bounds, parameters 2e-3 of the change + 2e-7
  Adam / FTRL         the five-step test of test_gpu_ipnn_shapes.py (Adam: logits 5e-4 + 5e-5, parameters 5e-3 of the change
                      + 1e-7, the loss -- which that test leaves out -- as under SGD; FTRL: logits 2e-3 + 2e-5, loss 1e-4 |loss|,
                      parameters 5e-3 max |parameter| + 1e-7)
  predictions         p = sigmoid(z), so |dp| <= p (1 - p) |dz| with |dz| the logits bound in force, + 1e-6 (the predict check
                      of test_gpu_ipnn_shapes.check_f32_step)
  FM                  test_gpu_fm_wide.py: SGD p rtol 5e-5 + 1e-6, loss 2e-5 max(1, |loss|), rows 2e-3 of the change + 2e-7;
                      Adam / FTRL p and loss 5e-5 at the first step and 2e-3 later, check_state for rows, bias and state
Every oracle case prints its worst error as a fraction of its bound."""
import numpy as np
import pytest

from oracle import fm_oracle as fo

import fm_weighted_ref as fw
import lifecycle_ref as L

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import FM
from deep_ctr_amd.ipnn import Drawn, IPNNEngine

from test_gpu_fm_optim import np_metrics
from test_gpu_fm_wide import check_state as fm_check_state
from test_gpu_ipnn_shapes import Bounds as _Bounds
from test_gpu_parity import make_snn_engine, make_snn_problem
from test_gpu_shapes import make_engine as fnn_engine, make_problem as fnn_problem

pytestmark = pytest.mark.gpu

F = 16
INIT = ['uniform', -0.001, 0.001, [1, 2], None]


class Bounds(_Bounds):
    def report(self, label):
        print("\n[lifecycle] %s: worst error %.3f of the bound (%s)" % (label, self.worst, self.where))


# ================================================================================================ inner-product family
IP_LR = {'sgd': 0.001, 'adam': 1e-3, 'ftrl': 1e-2}          # the loss is a sum: 4096 examples step at 0.001 (test_gpu_ipnn_shapes.lr_for)
IP_HIDDEN = [40, 24, 12]


def ip_logit_bound(opt, first):
    if opt == 'sgd':
        return (2e-4, 2e-5) if first else (2e-3, 2e-4)
    return (5e-4, 5e-5) if opt == 'adam' else (2e-3, 2e-5)


def ip_loss_bound(opt, first, loss):
    if opt == 'ftrl':
        return 1e-4 * abs(loss)
    return (5e-5 if opt == 'sgd' and first else 1e-4) * max(1.0, abs(loss))


def ip_engine(F_, K, hidden, opt='sgd', prec='f32', max_batch=4096, pairs=True, lr=None):
    return IPNNEngine(F_, K, hidden, 'relu', max_batch=max_batch, precision=prec, lr=IP_LR[opt] if lr is None else lr, keep_prob=0.7,
                      pairs=pairs, optimizer=opt, adam_eps=1e-8)


def ip_set(eng, table, params):
    eng.set_params(table, params['b'], params['W'], params['bias'])


def ip_train(eng, it, want_logits=True):
    out = eng.train_step(it['ids'], it['y'], it['masks'], want_logits=want_logits, wts=it['wts'])
    return out['loss'], (out['logits'].cpu().numpy() if want_logits else None)


def ip_read(eng, n_rows):
    b, Ws, bs = eng.get_params()
    return {'b': b, 'W': Ws, 'bias': bs, 'table': eng.get_rows(np.arange(n_rows))}


def assert_ip_bits(a, b, what):
    assert a['b'] == b['b'], '%s: b' % what
    for t in range(len(a['W'])):
        assert np.array_equal(a['W'][t], b['W'][t]), '%s: W%d, %d of %d floats differ' % (what, t, (a['W'][t] != b['W'][t]).sum(), a['W'][t].size)
        assert np.array_equal(a['bias'][t], b['bias'][t]), '%s: bias%d' % (what, t)
    assert np.array_equal(a['table'], b['table']), '%s: table, %d rows differ' % (what, (a['table'] != b['table']).any(axis=1).sum())


def ip_check_params(bd, got, pl, p0, t0, opt, tag='', one_step=False):
    """Every dense tensor, b and the whole table against the player: within 5e-3 of the oracle's own total change (FTRL: of the
    largest parameter, as its five-step test has it); one SGD step: 2e-3 of it + 2e-7 (test_ipnn_step_f32_vs_oracle)."""
    atol = (2e-7 if one_step else 1e-6) if opt == 'sgd' else 1e-7
    frac = 2e-3 if opt == 'sgd' and one_step else 5e-3

    def tol(new, old):
        return frac * (np.abs(new).max() if opt == 'ftrl' else np.abs(np.asarray(new) - np.asarray(old)).max()) + atol
    for t in range(len(got['W'])):
        bd.close(tag + 'W%d' % t, got['W'][t], pl.params['W'][t], 0.0, tol(pl.params['W'][t], p0['W'][t]))
        bd.close(tag + 'bias%d' % t, got['bias'][t], pl.params['bias'][t], 0.0, tol(pl.params['bias'][t], p0['bias'][t]))
    bd.close(tag + 'b', got['b'], pl.params['b'], 0.0, tol(pl.params['b'], p0['b']))
    bd.close(tag + 'table', got['table'], pl.table, 0.0, tol(pl.table, t0))
    return tol(pl.table, t0)


@pytest.mark.parametrize("opt", ['sgd', 'adam', 'ftrl'])
def test_ipnn_schedule_vs_oracle(built, opt):
    """A at 16 fields, k = 11, with pairs: 4096 with masks -> predict 37 -> 17 without dropout -> 257 with drawn masks ->
    evaluate 8195 -> 255 with masks and value weights -> 1 -> 4096 with masks, on one handle of max_batch 4096."""
    from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
    K = 11
    table, params, d, sizes = L.ip_problem(F, K, IP_HIDDEN, seed=3)
    sch = L.ip_schedule(sizes, d)
    never, first_only = L.row_sets(sch, len(table))
    assert len(never) > 0 and len(first_only) > 0
    pl = L.IpPlayer(table, params, d, opt, IP_LR[opt])
    eng = ip_engine(F, K, IP_HIDDEN, opt)
    bd = Bounds()
    try:
        assert eng.d == d
        ip_set(eng, table, params)
        after_first, n_train = None, 0
        for i, it in enumerate(sch):
            name = '%s%d-B%d ' % (it['kind'], i, len(it['ids']))
            rtol, atol = ip_logit_bound(opt, n_train <= 1)             # predictions after the first step: that step's bound
            if it['kind'] == 'train':
                rtol, atol = ip_logit_bound(opt, n_train == 0)
                loss, logits = ip_train(eng, it)
                rloss, rlogits = pl.train(it)
                bd.close(name + 'logits', logits, rlogits, rtol, atol)
                bd.close(name + 'loss', loss, rloss, 0.0, ip_loss_bound(opt, n_train == 0, rloss))
                n_train += 1
                if n_train == 1:
                    after_first = eng.get_rows(first_only)
                continue
            z = pl.logits(it)
            p = 1.0 / (1.0 + np.exp(-z))
            got = eng.predict(it['ids']).cpu().numpy()
            bd.close(name + 'p', got, p, 0.0, p * (1 - p) * (atol + rtol * np.abs(z)) + 1e-6)
            if it['kind'] == 'eval':                                    # test_ipnn_predict_and_eval_vs_sklearn_at_32_fields
                yy = (it['y'] != 0).astype(np.int32)
                m = eng.evaluate(it['ids'], yy)
                p64 = got.astype(np.float64)
                assert abs(m['auc'] - roc_auc_score(yy, p64)) < 1e-12
                assert abs(m['rmse'] - np.sqrt(mean_squared_error(yy, p64))) < 1e-12
                assert abs(m['logloss'] - log_loss(yy, p64, labels=[0, 1])) < 1e-12
        got = ip_read(eng, len(table))
        tol_t = ip_check_params(bd, got, pl, params, table, opt)
        rows = got['table']
        bd.close('rows of the first step only', rows[first_only], pl.table[first_only], 0.0, tol_t)
        assert np.abs(rows[first_only] - table[first_only]).max() > 0
        if opt == 'sgd':                    # nothing after the first step may reach them; rows no item touched never move
            assert np.array_equal(rows[first_only], after_first), "a row only the first step touched moved later"
            assert np.array_equal(rows[never], table[never].astype(np.float32)), "a row no example touched moved"
        elif opt == 'adam':                 # their moments keep them moving; zero gradient and zero moments move nothing
            assert not np.array_equal(rows[first_only], after_first)
            assert np.array_equal(rows[never], table[never].astype(np.float32)), "a row no example touched moved"
        else:                               # re-derived from a zero linear term
            assert not rows[never].any()
        bd.report('ipnn schedule %s' % opt)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ B: the replay twin
# (id, F, K, hidden, precision, pairs, long batch, environment)
IP_TWIN = [('f32-16x11', 16, 11, [130, 70], 'f32', True, 4096, {}),
           ('bf16-16x11', 16, 11, [130, 70], 'bf16', True, 4096, {}),
           ('f32-39x11-many-fields', 39, 11, IP_HIDDEN, 'f32', True, 4096, {}),
           ('bf16-39x11-many-fields', 39, 11, IP_HIDDEN, 'bf16', True, 4096, {}),
           ('f32-16x51-wide', 16, 51, IP_HIDDEN, 'f32', True, 4096, {}),
           ('bf16-16x51-wide', 16, 51, IP_HIDDEN, 'bf16', True, 4096, {}),
           ('bf16-400x200-strip-pairs', 16, 11, [400, 200], 'bf16', True, 2048, {}),
           ('bf16-400x200-one-stream', 16, 11, [400, 200], 'bf16', True, 2048, {'IPNN_SIDE_STREAM': '0'})]


@pytest.mark.parametrize("last", [17, 255])
@pytest.mark.parametrize("name,F_,K,hidden,prec,pairs,big,env", IP_TWIN, ids=[c[0] for c in IP_TWIN])
def test_ipnn_replay_twin_bit_for_bit(built, monkeypatch, name, F_, K, hidden, prec, pairs, big, env, last):
    """B: a step at 257 with drawn masks, a predict at 37, the long masked step and an evaluation on handle A; then the last step
    (17 or 255 examples, masks), right after the long one, on A and on a fresh handle holding A's parameters."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    table, params, d, sizes = L.ip_problem(F_, K, hidden, pairs, n_rows=2000, seed=7 + F_ + K)
    pre = [dict(L.ip_batch(sizes, d, 257, 42, masked=False), masks=Drawn(5, 9)),
           dict(L.ip_batch(sizes, d, 37, 41, masked=False), kind='predict'), L.ip_batch(sizes, d, big, 40),
           dict(L.ip_batch(sizes, d, big + 3, 43, masked=False), kind='eval')]
    it = L.ip_batch(sizes, d, last, 44)
    lr = 0.001
    A = ip_engine(F_, K, hidden, 'sgd', prec, big, pairs, lr)
    T = ip_engine(F_, K, hidden, 'sgd', prec, big, pairs, lr)
    try:
        ip_set(A, table, params)
        for s in pre:
            if s['kind'] == 'train':
                ip_train(A, s, want_logits=False)
            elif s['kind'] == 'predict':
                A.predict(s['ids'])
            else:
                A.evaluate(s['ids'], (s['y'] != 0).astype(np.int32))
        mid = ip_read(A, len(table))
        assert not np.array_equal(mid['table'], table.astype(np.float32)) and np.isfinite(mid['table']).all()
        ip_set(T, mid['table'], mid)
        assert_ip_bits(ip_read(T, len(table)), mid, 'set / get round trip')
        la, za = ip_train(A, it)
        lt, zt = ip_train(T, it)
        assert np.isfinite(za).all() and np.abs(za).max() > 0
        assert np.array_equal(za, zt), "logits: %d of %d differ, max %.3e" % ((za != zt).sum(), za.size, np.abs(za - zt).max())
        assert la == lt, "loss %r on the used handle, %r on the fresh one" % (la, lt)
        assert_ip_bits(ip_read(A, len(table)), ip_read(T, len(table)), 'after the last step')
    finally:
        A.close()
        T.close()


# ------------------------------------------------------------------------------------------------ C: parameters set again
def ip_two_steps(eng, pl, its, opt, bd, tag):
    for s, it in enumerate(its):
        loss, logits = ip_train(eng, it)
        if pl is not None:
            rloss, rlogits = pl.train(it)
            bd.close('%slogits%d' % (tag, s), logits, rlogits, *ip_logit_bound(opt, False))
            bd.close('%sloss%d' % (tag, s), loss, rloss, 0.0, ip_loss_bound(opt, False, rloss))
        yield loss, logits


@pytest.mark.parametrize("opt", ['adam', 'ftrl'])
def test_ipnn_set_params_restarts_the_optimiser(built, opt):
    """C: three steps, IPNNEngine.set_params with the first parameters, two steps.  ipnn_set_table restarts the optimiser (the
    table's, every dense layer's and b's state, the step count; FTRL accumulators back to 0.1), so a fresh handle given the same
    two steps matches bit for bit, and both follow the oracle started from fresh state."""
    K, B = 11, 160
    table, params, d, sizes = L.ip_problem(F, K, IP_HIDDEN, n_rows=600, seed=11)
    its = [L.ip_batch(sizes, d, B, 60 + s) for s in range(5)]
    used, fresh = ip_engine(F, K, IP_HIDDEN, opt, max_batch=256), ip_engine(F, K, IP_HIDDEN, opt, max_batch=256)
    bd = Bounds()
    try:
        ip_set(used, table, params)
        for it in its[:3]:
            ip_train(used, it, want_logits=False)
        ip_set(used, table, params)
        ip_set(fresh, table, params)
        pl = L.IpPlayer(table, params, d, opt, IP_LR[opt])
        ru = list(ip_two_steps(used, pl, its[3:], opt, bd, 'used '))
        rf = list(ip_two_steps(fresh, None, its[3:], opt, bd, 'fresh '))
        gu, gf = ip_read(used, len(table)), ip_read(fresh, len(table))
        ip_check_params(bd, gu, pl, params, table, opt, 'used ')
        ip_check_params(bd, gf, pl, params, table, opt, 'fresh ')
        bd.report('ipnn set_params after three %s steps' % opt)
        for s, ((lu, zu), (lf, zf)) in enumerate(zip(ru, rf)):
            assert np.array_equal(zu, zf), "step %d: logits differ by up to %.3e" % (s, np.abs(zu - zf).max())
            assert lu == lf, "step %d: loss %r on the used handle, %r on the fresh one" % (s, lu, lf)
        assert_ip_bits(gu, gf, 'used against fresh')
    finally:
        used.close()
        fresh.close()


# (id, K, optimiser, row counts one after another): 1.1 M rows sort 64-bit keys (key64), K = 51 is the wide layout (noshare)
IP_RESIZE = [('narrow-sgd-key64', 11, 'sgd', (600, 1100000, 300)), ('narrow-adam', 11, 'adam', (600, 1500, 300)),
             ('wide-sgd', 51, 'sgd', (600, 1500, 300)), ('wide-ftrl', 51, 'ftrl', (600, 1500, 300))]


@pytest.mark.parametrize("name,K,opt,counts", IP_RESIZE, ids=[c[0] for c in IP_RESIZE])
def test_ipnn_set_table_with_another_row_count(built, name, K, opt, counts):
    """C: a table of more and then of fewer rows on a handle that has stepped (rows, noshare, the state tables and the 64-bit
    key choice are re-made), each followed by one step against the oracle started fresh.  The batch reaches the new table's last
    row."""
    B = 257
    eng = ip_engine(F, K, IP_HIDDEN, opt, max_batch=512)
    bd = Bounds()
    try:
        for j, n in enumerate(counts):
            table, params, d, sizes = L.ip_problem(F, K, IP_HIDDEN, n_rows=n, seed=20 + j)
            assert len(table) == n
            it = L.ip_batch(sizes, d, B, 80 + j)
            it['ids'][B - 1, F - 1] = n - 1
            ip_set(eng, table, params)
            pl = L.IpPlayer(table, params, d, opt, IP_LR[opt])
            loss, logits = ip_train(eng, it)
            rloss, rlogits = pl.train(it)
            tag = 'n%d ' % n
            bd.close(tag + 'logits', logits, rlogits, *ip_logit_bound(opt, True))
            bd.close(tag + 'loss', loss, rloss, 0.0, ip_loss_bound(opt, True, rloss))
            got = ip_read(eng, n)
            ip_check_params(bd, got, pl, params, table, opt, tag, one_step=True)
            untouched = np.setdiff1d(np.arange(n), np.unique(it['ids']))
            if opt == 'ftrl':
                assert not got['table'][untouched].any()
            else:
                assert np.array_equal(got['table'][untouched], table[untouched].astype(np.float32)), "a row no example touched moved"
        bd.report('ipnn set_table %s' % name)
    finally:
        eng.close()


# ================================================================================================ FM pre-training
FM_LR = {'sgd': (0.05, 0.02), 'adam': (1e-2, 5e-3), 'ftrl': (0.05, 0.02)}      # before and after the 'hparams' item
FM_LAM = (1e-2, 1e-3)


def fm_make(opt, rank, rows, b, lr, lam, max_batch=4096):
    argv = [opt, lr] + ([1e-8] if opt == 'adam' else [])                # reduce_mean, the driver's setting
    m = FM(max_batch, [rows.shape[0], F, rank], INIT, argv, [lam], 'train', 0)
    m.set_params(rows, b)
    return m


def fm_step(m, it, want_p=True):
    out = m.train_step(it['ids'], it['y'], want_p=want_p, wts=it['wts'])
    return out['loss'], (out['p'].cpu().numpy() if want_p else None)


def fm_tol(opt, first):
    return 5e-5 if opt == 'sgd' or first else 2e-3


@pytest.mark.parametrize("rank", [10, 50])
@pytest.mark.parametrize("opt", ['sgd', 'adam', 'ftrl'])
def test_fm_schedule_vs_oracle(built, opt, rank):
    """A for the FM class at 16 fields, narrow (rank 10) and wide (rank 50) rows, lambda > 0 so that the lazy scale is live:
    4096 -> forward 37 -> 17 -> 257 -> evaluate 8195 -> 255 with value weights -> lr and lambda change -> 1 -> 4096."""
    sizes = synth.field_sizes_tiny(L.FM_ROWS)
    rows = L.fm_table(sum(sizes) + L.FM_GAP, rank, 4)
    sch = L.fm_schedule(sizes)
    never, first_only = L.row_sets(sch, len(rows))
    assert len(never) >= L.FM_GAP and len(first_only) > 0
    m = fm_make(opt, rank, rows, 0.1, FM_LR[opt][0], FM_LAM[0])
    tr = fw.TrainerW(rows, 0.1, opt, FM_LR[opt][0], FM_LAM[0], 1)
    tr.rows0 = rows.copy()
    bd = Bounds()
    try:
        n_train = 0
        for i, it in enumerate(sch):
            name = '%s%d-B%d ' % (it['kind'], i, len(it['ids']))
            if it['kind'] == 'hparams':
                m.lr, m.lam = FM_LR[opt][1], FM_LAM[1]
                tr.lr, tr.lam = FM_LR[opt][1], FM_LAM[1]
            elif it['kind'] == 'train':
                tol = fm_tol(opt, n_train == 0)
                loss, p = fm_step(m, it)
                data, rp = L.fm_train(tr, it)
                bd.close(name + 'p', p, rp, tol, 1e-6)
                bd.close(name + 'loss', loss, data, 0.0, (2e-5 if opt == 'sgd' else tol) * max(1.0, abs(data)))
                n_train += 1
            else:
                got = m.forward(it['ids']).cpu().numpy()
                bd.close(name + 'p', got, fo.predict(tr.rows, tr.b, it['ids']), fm_tol(opt, n_train <= 1), 1e-6)
                if it['kind'] == 'eval':                                # test_fm_eval_vs_numpy
                    yy = (it['y'] != 0).astype(np.int32)
                    auc, rmse, ll = m.evaluate(it['ids'], yy)
                    ea, er, el = np_metrics(got.astype(np.float64), yy)
                    assert abs(auc - ea) <= 1e-12 and abs(rmse - er) <= 1e-9 * er and abs(ll - el) <= 1e-9 * el
        got, gb = m.get_params()
        if opt == 'sgd':
            tol = 2e-3 * (np.abs(tr.rows - rows).max() + 1e-12) + 2e-7
            bd.close('rows', got, tr.rows, 0.0, tol)
            bd.close('b', gb, tr.b, 0.0, 2e-3 * abs(tr.b - 0.1) + 2e-7)
        else:
            fm_check_state(m, tr)
            tol = 5e-3 * (np.abs(tr.rows).max() if opt == 'ftrl' else np.abs(tr.rows - rows).max()) + 1e-7
        # rows no batch touched follow the dense L2 gradient alone; rows of the first step keep their share of it
        ok = ~tr.ill if opt == 'adam' else np.ones(rows.shape, bool)
        for label, sel in (('rows no item touched', never), ('rows of the first step only', first_only)):
            bd.close(label, got[sel][ok[sel]], tr.rows[sel][ok[sel]], 0.0, tol)
            assert np.abs(got[sel] - rows[sel]).max() > 0            # lambda > 0: every row moves
        bd.report('fm schedule %s rank %d' % (opt, rank))
    finally:
        m.close()


@pytest.mark.parametrize("rank", [10, 50])
def test_fm_optimiser_switches_mid_life(built, rank):
    """fm_set_optimizer on a handle that has stepped: SGD steps that leave a decay scale pending (lr * lambda = 0.1), then Adam;
    Adam steps, then SGD again.  The restatement folds the decay (its rows are always folded) and starts each optimiser from zero
    state, as include/fm_hip.h says.  After the Adam phase: test_gpu_fm_wide.check_state.  After the second SGD phase the rows may
    be off by the Adam phase's bound plus the SGD bound on the change of that phase (2e-3 of it + 2e-7)."""
    sizes = synth.field_sizes_tiny(400)
    rows = L.fm_table(sum(sizes) + L.FM_GAP, rank, 5)
    its = [L.fm_batch(sizes, B, 300 + 7 * s) for s, B in enumerate((4096, 17, 257, 255, 1, 4096, 17, 255))]
    m = fm_make('sgd', rank, rows, 0.05, 0.1, 1.0)
    tr = fw.TrainerW(rows, 0.05, 'sgd', 0.1, 1.0, 1)
    bd = Bounds()
    try:
        for it in its[:3]:
            fm_step(m, it, want_p=False)
            L.fm_train(tr, it)
        assert m.lib.fm_set_optimizer(m.h, 1, 0.9, 0.999, 1e-8) == 0          # FM_OPT_ADAM
        m.lr, m.lam = 1e-2, 1e-3
        tr.opt, tr.lr, tr.lam, tr.eps = 'adam', 1e-2, 1e-3, 1e-8
        tr.reset_state()
        tr.rows0 = tr.rows.copy()
        for it in its[3:6]:
            fm_step(m, it, want_p=False)
            L.fm_train(tr, it)
        fm_check_state(m, tr)
        adam_tol = 5e-3 * np.abs(tr.rows - tr.rows0).max() + 1e-7
        adam_b_tol = (2 * tr.lr_sum if tr.ill_b else 5e-3 * tr.lr_sum) + 1e-7
        ill = tr.ill.copy()
        assert m.lib.fm_set_optimizer(m.h, 0, 0.0, 0.0, 0.0) == 0             # FM_OPT_SGD
        m.lr, m.lam = 0.05, 1e-2
        tr.opt, tr.lr, tr.lam = 'sgd', 0.05, 1e-2
        r1, b1 = tr.rows.copy(), tr.b
        for s, it in enumerate(its[6:]):
            loss, p = fm_step(m, it)
            data, rp = L.fm_train(tr, it)
            bd.close('sgd again %d p' % s, p, rp, 2e-3, 1e-6)                  # the Adam steps' own bound on p carries over
        got, gb = m.get_params()
        bd.close('rows', got[~ill], tr.rows[~ill], 0.0, adam_tol + 2e-3 * np.abs(tr.rows - r1).max() + 2e-7)
        bd.close('b', gb, tr.b, 0.0, adam_b_tol + 2e-3 * abs(tr.b - b1) + 2e-7)
        bd.report('fm sgd -> adam -> sgd rank %d' % rank)
    finally:
        m.close()


@pytest.mark.parametrize("last", [17, 255])
@pytest.mark.parametrize("rank", [10, 50])
def test_fm_replay_twin_bit_for_bit(built, rank, last):
    """B for FM under SGD with lambda > 0: a weighted step at 257, a forward at 37, a step at 4096 and an evaluation on A, then
    the last step on both.  Reading A's rows folds its pending decay scale; T receives the folded rows."""
    sizes = synth.field_sizes_tiny(2000)
    rows = L.fm_table(sum(sizes) + L.FM_GAP, rank, 6)
    A, T = fm_make('sgd', rank, rows, 0.1, 0.05, 1e-2), fm_make('sgd', rank, rows, 0.1, 0.05, 1e-2)
    try:
        fm_step(A, dict(L.fm_batch(sizes, 257, 52), wts=fw.test_weights(257, F, 53)), want_p=False)
        A.forward(L.fm_batch(sizes, 37, 51)['ids'])
        fm_step(A, L.fm_batch(sizes, 4096, 50), want_p=False)
        ev = L.fm_batch(sizes, 4099, 54)
        A.evaluate(ev['ids'], (ev['y'] != 0).astype(np.int32))
        mid, mb = A.get_params()
        assert not np.array_equal(mid, rows.astype(np.float32))
        T.set_params(mid, mb)
        back, bb = T.get_params()
        assert np.array_equal(back, mid) and bb == mb
        it = L.fm_batch(sizes, last, 55)
        la, pa = fm_step(A, it)
        lt, pt = fm_step(T, it)
        assert np.array_equal(pa, pt), "p: %d of %d differ" % ((pa != pt).sum(), pa.size)
        assert la == lt, "loss %r on the used handle, %r on the fresh one" % (la, lt)
        (ra, ba), (rt, bt) = A.get_params(), T.get_params()
        assert np.array_equal(ra, rt), "%d rows differ" % (ra != rt).any(axis=1).sum()
        assert ba == bt
    finally:
        A.close()
        T.close()


@pytest.mark.parametrize("rank", [10, 50])
def test_fm_set_table_equals_a_fresh_handle(built, rank):
    """C for FM: after Adam steps fm_set_table leaves the handle as a fresh one -- rows, bias, both state tensors, the bias's
    state sb and the step count t (fm_get_opt_state), right after the call and after two more steps."""
    sizes = synth.field_sizes_tiny(600)
    rows = L.fm_table(sum(sizes) + L.FM_GAP, rank, 7)
    its = [L.fm_batch(sizes, B, 400 + 7 * s) for s, B in enumerate((700, 17, 257, 255, 700))]
    used, fresh = fm_make('adam', rank, rows, 0.1, 1e-2, 1e-3), fm_make('adam', rank, rows, 0.1, 1e-2, 1e-3)
    try:
        for it in its[:3]:
            fm_step(used, it, want_p=False)
        assert used.get_opt_state()[3] == 3 and used.get_opt_state()[2].any()
        used.set_params(rows, 0.1)
        for when in ('set', 'stepped'):
            (ru, bu), (rf, bf) = used.get_params(), fresh.get_params()
            assert np.array_equal(ru, rf) and bu == bf, when
            su, sf = used.get_opt_state(), fresh.get_opt_state()
            assert su[3] == sf[3] == (0 if when == 'set' else 2), when
            for a, b in zip(su[:3], sf[:3]):
                assert np.array_equal(a, b), when
            if when == 'set':
                assert not su[0].any() and not su[1].any() and not su[2].any()
                for it in its[3:]:
                    (lu, pu), (lf, pf) = fm_step(used, it), fm_step(fresh, it)
                    assert np.array_equal(pu, pf) and lu == lf
    finally:
        used.close()
        fresh.close()


@pytest.mark.parametrize("rank", [10, 50])
@pytest.mark.parametrize("opt", ['sgd', 'adam'])
def test_fm_set_table_with_another_row_count(built, opt, rank):
    """C for FM: more and then fewer rows on a handle that has stepped, each followed by one step against the restatement
    started fresh; the batch reaches the new table's last row."""
    lr, lam = FM_LR[opt][0], 1e-3
    m = None
    bd = Bounds()
    try:
        for j, n in enumerate((600, 1500, 300)):
            sizes = synth.field_sizes_tiny(n - L.FM_GAP)
            rows = L.fm_table(n, rank, 30 + j)
            assert sum(sizes) + L.FM_GAP == n
            if m is None:
                m = fm_make(opt, rank, rows, 0.1, lr, lam, max_batch=512)
            else:
                m.set_params(rows, 0.1)
            tr = fw.TrainerW(rows, 0.1, opt, lr, lam, 1)
            tr.rows0 = rows.copy()
            it = L.fm_batch(sizes, 257, 500 + j)
            assert it['ids'].max() == n - 1
            loss, p = fm_step(m, it)
            data, rp = L.fm_train(tr, it)
            bd.close('n%d p' % n, p, rp, 5e-5, 1e-6)
            bd.close('n%d loss' % n, loss, data, 0.0, (2e-5 if opt == 'sgd' else 5e-5) * max(1.0, abs(data)))
            if opt == 'sgd':
                got, gb = m.get_params()
                assert got.shape == rows.shape
                bd.close('n%d rows' % n, got, tr.rows, 0.0, 2e-3 * (np.abs(tr.rows - rows).max() + 1e-12) + 2e-7)
                bd.close('n%d b' % n, gb, tr.b, 0.0, 2e-3 * abs(tr.b - 0.1) + 2e-7)
            else:
                fm_check_state(m, tr)
        bd.report('fm set_table %s rank %d' % (opt, rank))
    finally:
        if m is not None:
            m.close()


# ================================================================================================ FNN engine
FNN_DENSE = ('w1', 'b1', 'w2', 'b2', 'w3')
# (id, F, K, precision, bag h0 or 0, what happens between the long step and the last one)
FNN_TWIN = [('f32-16x11', 16, 11, 'f32', 0, 'plain'), ('bf16-16x11', 16, 11, 'bf16', 0, 'plain'), ('bf16x3-16x11', 16, 11, 'bf16x3', 0, 'plain'),
            ('f32-16x51-wide', 16, 51, 'f32', 0, 'plain'), ('bf16-16x51-wide', 16, 51, 'bf16', 0, 'plain'),
            ('f32-bag-h0_300', 16, 0, 'f32', 300, 'plain'), ('bf16-bag-h0_300', 16, 0, 'bf16', 300, 'plain'),
            ('f32-16x11-shadowed', 16, 11, 'f32', 0, 'shadowed'), ('bf16-16x11-prefetch', 16, 11, 'bf16', 0, 'prefetch')]


def fnn_read(eng, bag):
    return eng.get_table(), eng.get_dense(), (eng.get_bag_bias() if bag else None)


def assert_fnn_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: table, %d of %d floats differ" % (what, (a[0] != b[0]).sum(), a[0].size)
    for k in FNN_DENSE:
        assert np.array_equal(a[1][k], b[1][k]), '%s: %s' % (what, k)
    assert a[1]['b3'] == b[1]['b3'], '%s: b3' % what
    if a[2] is not None:
        assert np.array_equal(a[2], b[2]), '%s: bag bias' % what


@pytest.mark.parametrize("last", [17, 255])
@pytest.mark.parametrize("name,F_,K,prec,h0,between", FNN_TWIN, ids=[c[0] for c in FNN_TWIN])
def test_fnn_replay_twin_bit_for_bit(built, name, F_, K, prec, h0, between, last):
    """B for FNNEngine at 300 x 100: a step at 257, a predict, a step at 4096 (plain, or with fnn_set_shadowed, which takes the
    layer-by-layer kernels between two fused steps, or with fnn_prefetch_ids announcing the last batch before it) on handle A;
    then the last step on A and on a fresh handle holding A's table and dense tensors: p, gx, the loss, the table, every dense
    tensor and the bag bias bit for bit."""
    import torch
    H1, H2, n_rows, lr = 300, 100, 2000, 0.001
    lens = (257, 37, 4096, last)
    if h0:
        ww0, bb0, _, _, p, _, _ = make_snn_problem(8, n_rows=n_rows, h0=h0, seed=3, n_fields=F_)
        sizes = synth.field_sizes_tiny(n_rows, n_fields=F_)
        fo_row = np.zeros(len(ww0), np.int32)
        rows = ww0

        def make():
            return make_snn_engine(ww0, bb0, p, prec=prec, lr=lr, h0=h0, max_batch=4096, n_fields=F_)
    else:
        rows, fo_row, _, _, p, _, _ = fnn_problem(F_, K, H1, H2, 8, n_rows=n_rows, seed=9)
        sizes = synth.field_sizes_tiny(n_rows, n_fields=F_)

        def make():
            return fnn_engine(F_, K, H1, H2, rows, fo_row, p, prec=prec, lr=lr)
    rng = np.random.RandomState(17)
    ids = [synth.zipf_ids(B, sizes, 1.1, 70 + s) for s, B in enumerate(lens)]
    ids[0][5, 1] = -1                                                    # an empty field
    ys = [L.labels(rng, B).astype(np.float32) for B in lens]
    r1 = [(rng.uniform(size=H1) < 0.5).astype(np.uint8) for _ in lens]
    r2 = [(rng.uniform(size=H2) < 0.5).astype(np.uint8) for _ in lens]
    A, T = make(), make()
    try:
        dev = [torch.as_tensor(i).to(A.device).contiguous() for i in ids]
        A.train_step(dev[0], ys[0], r1[0], r2[0], want_loss=False)
        A.predict(dev[1])
        if between == 'shadowed':                                        # rows of field 2, shadowed in examples 3, 4 and 9
            f2 = np.flatnonzero(fo_row == 2)
            A.set_shadowed(np.array([(t, 2, int(f2[(t + 1) % len(f2)])) for t in (3, 4, 9)], np.int32))
        if between == 'prefetch':
            A.prefetch_ids(dev[3])
        A.train_step(dev[2], ys[2], r1[2], r2[2], want_loss=False)
        mid = fnn_read(A, bool(h0))
        assert not np.array_equal(mid[0], rows) and np.isfinite(mid[0]).all()
        T.set_table(mid[0], fo_row, 0.0 if h0 else -3.0)
        T.set_dense(mid[1])
        if h0:
            T.set_bag_bias(mid[2])
        assert_fnn_bits(fnn_read(T, bool(h0)), mid, 'set / get round trip')
        oa = A.train_step(dev[3], ys[3], r1[3], r2[3], want_p=True, want_gx=True)
        ot = T.train_step(dev[3], ys[3], r1[3], r2[3], want_p=True, want_gx=True)
        pa, pt = oa['p'].cpu().numpy(), ot['p'].cpu().numpy()
        assert np.isfinite(pa).all()
        assert np.array_equal(pa, pt), "p: %d of %d differ" % ((pa != pt).sum(), pa.size)
        assert np.array_equal(oa['gx'].cpu().numpy(), ot['gx'].cpu().numpy()), "gx"
        assert oa['loss'] == ot['loss'], "loss %r on the used handle, %r on the fresh one" % (oa['loss'], ot['loss'])
        assert_fnn_bits(fnn_read(A, bool(h0)), fnn_read(T, bool(h0)), 'after the last step')
    finally:
        A.close()
        T.close()
