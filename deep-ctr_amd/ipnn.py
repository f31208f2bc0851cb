"""Inner-product FNN family on MI355X: the arithmetic of the reference's TensorFlow classes
`FNN_IP_L3` / `FNN_IP_L5` / `FNN_IP_L7` (python/FNN_IP_L7.py:5-133) behind include/ipnn_hip.h.
`IPNNEngine` is the PyTorch-ROCm plumbing; the three class names of the reference are kept as
constructors with its `_rch_argv` layout (X_dim, X_feas, rank, h1..hN, act_func), its `forward`
role (`train_step` / `predict`) and its `dump` keys (`W`, `V`, `b`, `h{i}_w`, `h{i}_b`).
One id per field and, optionally, one value weight per (example, field) -- `wts`, e_f = wts * row: the reference's Criteo
feed of 13 numeric and 26 weighted categorical fields, see `criteo_feed` -- at X_feas = 2..64 for rank <= 15 (the reference's own
39 columns included) and 2..32 above; optimiser 'sgd', 'adam' or 'ftrl' (python/tf_util.py:15-29).  rank 0..127
(k = rank + 1 up to 128, either precision): an FM50 / FM100 pickle from FM.dump seeds FNN_IP_L3_50 / FNN100 through
_init_argv."""
import ctypes as C
import pickle

import numpy as np

from . import _capi
from .dropout import _u64
from .engine import FNNError


class Drawn(object):
    """`masks=Drawn(seed, step)`: the library draws the step's keep-masks itself (ipnn_train_step_drawn; dropout.drawn_masks
    restates the draw).  seed and step are integers in uint64; the pair names the masks of one step."""
    __slots__ = ('seed', 'step')

    def __init__(self, seed, step):
        object.__setattr__(self, 'seed', _u64('seed', seed))
        object.__setattr__(self, 'step', _u64('step', step))

    def __setattr__(self, name, value):
        raise AttributeError("Drawn is a value: make another one")

    def __eq__(self, other):
        return isinstance(other, Drawn) and (self.seed, self.step) == (other.seed, other.step)

    def __hash__(self):
        return hash((self.seed, self.step))

    def __repr__(self):
        return "Drawn(seed=%d, step=%d)" % (self.seed, self.step)


def criteo_feed(v_wts, c_ids, c_wts, offsets):
    """The reference's three feeds (python/baseline.py:347-349: `_vals[:, :13]`, `_cols[:, 13:] - offsets`, `_vals[:, 13:]`) as
    one (ids int32 [B, n_v + n_c], wts float32 [B, n_v + n_c]) pair: numeric field i is row i of the table weighted by its value
    (python/FNN_IP_L7.py:103), categorical field j is row c_ids[:, j] + offsets[j] weighted by c_wts[:, j].  Pure NumPy."""
    v_wts, c_ids, c_wts = np.asarray(v_wts), np.asarray(c_ids), np.asarray(c_wts)
    B, n_v = v_wts.shape
    if c_ids.shape != c_wts.shape or c_ids.shape[0] != B:
        raise ValueError("criteo_feed: v_wts %r, c_ids %r, c_wts %r" % (v_wts.shape, c_ids.shape, c_wts.shape))
    off = np.broadcast_to(np.asarray(offsets, dtype=np.int64), (c_ids.shape[1],))
    ids = np.empty((B, n_v + c_ids.shape[1]), dtype=np.int32)
    ids[:, :n_v] = np.arange(n_v, dtype=np.int32)
    ids[:, n_v:] = c_ids.astype(np.int64) + off
    return ids, np.concatenate([v_wts, c_wts], axis=1).astype(np.float32)


def _cfg(n_fields, k, hidden, act, pairs, max_batch, precision, lr, keep_prob, optimizer, adam_betas, adam_eps, device, stream):
    hidden = list(hidden)
    hid = (C.c_int32 * 8)(*(hidden + [0] * (8 - len(hidden))))
    return _capi.ipnn_cfg(n_fields, k, len(hidden), hid, _capi.IPNN_ACTS[act], 1 if pairs else 0, max_batch,
                          1 if precision == 'bf16' else 0, lr, keep_prob, {'sgd': 0, 'adam': 1, 'ftrl': 2}[optimizer], adam_betas[0],
                          adam_betas[1], adam_eps, device, stream)


def plan_query(n_fields, k, hidden, precision='bf16', pairs=True, act='relu', max_batch=4096, optimizer='sgd'):
    """What an IPNNEngine of this shape would choose under the environment's IPNN_* knobs (ipnn_plan_query): needs the library
    but no device.  A dict: 'strips' (the strip kernels run the deep stack; False: one GEMM launch per product), 'pairs', 'cut',
    'rows_fwd' / 'rows_bwd' ('narrow', 'wide' or 'many'), 'shares_step' / 'shares_eval' (the engine shares the launches of
    train_step_many / of evaluate_many and predict_many), 'padded' (the layers' padded widths), 'lds_max', and per strip launch
    -- 'stack_fwd', 'stack_bwd', 'wide_fwd', 'wide_bwd', 'tail_fwd', 'tail_bwd', 'tail_fused' -- a dict of 'cap_a', 'cap_b' (the
    two LDS tiles' widths in columns) and 'lds_bytes'; all zero for a launch the engine never issues."""
    lib = _capi.load()
    cfg = _cfg(n_fields, k, hidden, act, pairs, max_batch, precision, 1e-4, 0.5, optimizer, (0.9, 0.999), 1e-8, 0, None)
    info = _capi.ipnn_plan_info()
    rc = lib.ipnn_plan_query(C.byref(cfg), C.byref(info))
    if rc != 0:
        raise FNNError(rc, (lib.ipnn_last_error(None) or b'').decode())
    out = {name: bool(getattr(info, name)) for name in ('strips', 'pairs', 'shares_step', 'shares_eval')}
    out.update(cut=info.cut, rows_fwd=_capi.IPNN_ROWS[info.rows_fwd], rows_bwd=_capi.IPNN_ROWS[info.rows_bwd],
               padded=list(info.padded[:info.n_layers]), lds_max=int(info.lds_max))
    for name in _capi.IPNN_PLAN_LAUNCHES:
        t = getattr(info, name)
        out[name] = {'cap_a': t.cap_a, 'cap_b': t.cap_b, 'lds_bytes': int(t.lds_bytes)}
    return out


class IPNNEngine(object):
    def __init__(self, n_fields, k, hidden, act='relu', max_batch=4096, precision='bf16', lr=1e-4, keep_prob=0.5, device=0,
                 pairs=True, optimizer='sgd', adam_eps=1e-8, adam_betas=(0.9, 0.999), reduce='sum', stream=None):
        """stream: a torch.cuda.Stream the engine enqueues on (several engines may share one); None: a stream of its own."""
        import torch
        if not torch.cuda.is_available():
            raise FNNError(_capi.FNN_ERR_HIP, "no HIP device visible to PyTorch-ROCm; no CPU fallback")
        self._torch, self.lib = torch, _capi.load()
        self.device = torch.device('cuda', device)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        self.F, self.K, self.hidden = n_fields, k, list(hidden)
        self.max_batch = max_batch
        self.d = [n_fields * k + (n_fields * (n_fields - 1) // 2 if pairs else 0) + 1] + self.hidden + [1]
        self._shape = dict(precision='bf16' if precision == 'bf16' else 'f32', pairs=bool(pairs), act=act, max_batch=max_batch, optimizer=optimizer)
        cfg = _cfg(n_fields, k, self.hidden, act, pairs, max_batch, precision, lr, keep_prob, optimizer, adam_betas, adam_eps, device,
                   C.c_void_p(self.stream.cuda_stream))
        h = C.c_void_p()
        rc = self.lib.ipnn_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise FNNError(rc, (self.lib.ipnn_last_error(None) or b'').decode())
        self.h = h
        self.reduce = reduce                      # 'sum' or 'mean' (python/FNN_IP_L7.py:83-86: anything but 'sum' is the mean)
        self._ck(self.lib.ipnn_set_loss_mean(self.h, 0 if reduce == 'sum' else 1))

    def _ck(self, rc):
        if rc != 0:
            raise FNNError(rc, (self.lib.ipnn_last_error(self.h) or b'').decode())

    @property
    def plan(self):
        """plan_query of this engine's shape, under the knobs as the environment holds them now (the engine read them when it was made)."""
        return plan_query(self.F, self.K, self.hidden, **self._shape)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.ipnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, table, b, Ws, biases):
        t = np.ascontiguousarray(table, dtype=np.float32)
        self._ck(self.lib.ipnn_set_table(self.h, t.ctypes.data, t.shape[0]))
        self._ck(self.lib.ipnn_set_b(self.h, float(b)))
        for i, (W, bias) in enumerate(zip(Ws, biases), start=1):
            W = np.ascontiguousarray(W, dtype=np.float32).reshape(self.d[i - 1], self.d[i])
            bias = np.ascontiguousarray(np.atleast_1d(bias), dtype=np.float32)
            self._ck(self.lib.ipnn_set_layer(self.h, i, W.ctypes.data, bias.ctypes.data))

    def get_params(self):
        Ws, bs = [], []
        for i in range(1, len(self.d)):
            W = np.empty((self.d[i - 1], self.d[i]), np.float32)
            b = np.empty(self.d[i], np.float32)
            self._ck(self.lib.ipnn_get_layer(self.h, i, W.ctypes.data, b.ctypes.data))
            Ws.append(W); bs.append(b)
        bb = C.c_float()
        self._ck(self.lib.ipnn_get_b(self.h, C.byref(bb)))
        return float(bb.value), Ws, bs

    def get_rows(self, row_ids):
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        out = np.empty((len(ids), self.K), np.float32)
        self._ck(self.lib.ipnn_get_rows(self.h, ids.ctypes.data, len(ids), out.ctypes.data))
        return out

    def _dev(self, a, dtype):
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _wts(self, wts, ids_t):
        """Value weights on the device (f32, the shape of ids), or None: every weight 1, the call without weights."""
        if wts is None:
            return None
        if tuple(wts.shape) != tuple(ids_t.shape):
            raise ValueError("wts has shape %r, ids %r" % (tuple(wts.shape), tuple(ids_t.shape)))
        return self._dev(wts, self._torch.float32)

    def train_step(self, ids, y, masks=None, want_logits=False, want_loss=True, wts=None):
        """masks: list of len(hidden)+1 uint8 arrays [B, d_t] (keep-masks for z1 and every hidden layer), or Drawn(seed, step):
        the library draws them on the device (ipnn_train_step_drawn), or None: no dropout.
        wts: value weights [B, F] (e_f = wts * row), None = all ones."""
        torch = self._torch
        ids_t, y_t = self._dev(ids, torch.int32), self._dev(y, torch.float32)
        wts_t = self._wts(wts, ids_t)
        B = ids_t.shape[0]
        mts, marr = None, None
        drawn = masks if isinstance(masks, Drawn) else None
        if masks is not None and drawn is None:
            mts = [self._dev(m, torch.uint8) for m in masks]
            assert len(mts) == len(self.hidden) + 1 and all(m.shape == (B, self.d[t]) for t, m in enumerate(mts))
            marr = (C.c_void_p * len(mts))(*[m.data_ptr() for m in mts])
        logits = torch.empty(B, dtype=torch.float32, device=self.device) if want_logits else None
        loss = C.c_float()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        if drawn is not None:
            self._ck(self.lib.ipnn_train_step_drawn(self.h, ids_t.data_ptr(), wts_t.data_ptr() if wts_t is not None else None, y_t.data_ptr(), B,
                                                    drawn.seed, drawn.step, logits.data_ptr() if want_logits else None,
                                                    C.byref(loss) if want_loss else None))
        elif wts_t is None:
            self._ck(self.lib.ipnn_train_step(self.h, ids_t.data_ptr(), y_t.data_ptr(), B, marr,
                                              logits.data_ptr() if want_logits else None, C.byref(loss) if want_loss else None))
        else:
            self._ck(self.lib.ipnn_train_step_w(self.h, ids_t.data_ptr(), wts_t.data_ptr(), y_t.data_ptr(), B, marr,
                                                logits.data_ptr() if want_logits else None, C.byref(loss) if want_loss else None))
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self._keep = (ids_t, y_t, mts, wts_t)
        scale = 1.0 if self.reduce == 'sum' else 1.0 / B     # the library returns the sum of the per-example losses
        return {'loss': float(loss.value) * scale if want_loss else None, 'logits': logits}

    def draw_masks(self, seed, step, B):
        """The keep-masks ipnn_train_step_drawn(seed, step) draws for a batch of B: a list of len(hidden)+1 device tensors uint8
        [B, d_t], what `masks=` takes (ipnn_draw_masks)."""
        torch = self._torch
        dr = Drawn(seed, step)
        out = [torch.empty((B, self.d[t]), dtype=torch.uint8, device=self.device) for t in range(len(self.hidden) + 1)]
        marr = (C.c_void_p * len(out))(*[m.data_ptr() for m in out])
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ck(self.lib.ipnn_draw_masks(self.h, dr.seed, dr.step, B, marr))
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return out

    def predict(self, ids, wts=None):
        torch = self._torch
        ids_t = self._dev(ids, torch.int32)
        wts_t = self._wts(wts, ids_t)
        out = torch.empty(ids_t.shape[0], dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, ids_t.shape[0], self.max_batch):          # ipnn_predict takes at most max_batch examples a call
            hi = min(ids_t.shape[0], lo + self.max_batch)
            if wts_t is None:
                self._ck(self.lib.ipnn_predict(self.h, ids_t[lo:hi].data_ptr(), hi - lo, out[lo:hi].data_ptr()))
            else:
                self._ck(self.lib.ipnn_predict_w(self.h, ids_t[lo:hi].data_ptr(), wts_t[lo:hi].data_ptr(), hi - lo, out[lo:hi].data_ptr()))
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return out

    def evaluate(self, ids, y, wts=None):
        """python/baseline.py:382-437: predictions + AUC / RMSE / logloss on the device (ipnn_eval / ipnn_eval_w).
        y: 0 / non-zero.  FNNError(FNN_ERR_RANGE) for one class only and for any prediction NaN or outside [0, 1]."""
        torch = self._torch
        ids_t, y_t = self._dev(ids, torch.int32), self._dev(y, torch.int32)
        wts_t = self._wts(wts, ids_t)
        auc, rmse, ll = C.c_double(), C.c_double(), C.c_double()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        if wts_t is None:
            self._ck(self.lib.ipnn_eval(self.h, ids_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0], C.byref(auc), C.byref(rmse), C.byref(ll)))
        else:
            self._ck(self.lib.ipnn_eval_w(self.h, ids_t.data_ptr(), wts_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0],
                                          C.byref(auc), C.byref(rmse), C.byref(ll)))
        return {'auc': auc.value, 'rmse': rmse.value, 'logloss': ll.value}

    def sync(self):
        self._ck(self.lib.ipnn_sync(self.h))


def _many_feed(engines, ids, wts, y=None, y_dtype=None, more=None):
    """The one feed of a group call on engines[0]'s device, and every engine's stream behind the caller's.  Everything the call
    reads is converted BEFORE the hand-shake -- a conversion of a device tensor is a kernel on the caller's stream -- so `more`,
    a function of the converted ids that makes whatever else the call feeds (keep-masks), runs in front of it too; its value is
    returned as the fourth entry."""
    e0 = engines[0]
    torch = e0._torch
    ids_t = e0._dev(ids, torch.int32)
    wts_t = e0._wts(wts, ids_t)
    y_t = e0._dev(y, y_dtype if y_dtype is not None else torch.int32) if y is not None else None
    extra = more(ids_t) if more is not None else None
    cur = torch.cuda.current_stream(e0.device)
    for e in engines:
        e.stream.wait_stream(cur)
    return ids_t, wts_t, y_t, extra


def predict_many(engines, ids, wts=None):
    """predict of every engine of a list on ONE feed, in one call (ipnn_predict_multi): a list of device tensors [N] float32,
    entry m bit for bit engines[m].predict(ids, wts).  N is not bounded by any engine's max_batch.  Nothing synchronises: an id
    outside an engine's table shows at that engine's sync(), as after predict.  Every refusal raises FNNError."""
    e0 = engines[0]
    torch = e0._torch
    M = len(engines)
    ids_t, wts_t, _, _ = _many_feed(engines, ids, wts)
    n = ids_t.shape[0]
    ps = [torch.empty(n, dtype=torch.float32, device=e0.device) for _ in engines]
    hs = (C.c_void_p * M)(*[e.h.value for e in engines])
    rc = e0.lib.ipnn_predict_multi(hs, M, ids_t.data_ptr(), wts_t.data_ptr() if wts_t is not None else None, n,
                                   (C.c_void_p * M)(*[t.data_ptr() for t in ps]))
    if rc != 0:
        raise FNNError(rc, (e0.lib.ipnn_last_error(e0.h) or b'').decode())
    cur = torch.cuda.current_stream(e0.device)
    for e in engines:
        cur.wait_stream(e.stream)
    e0._keep_many = (ids_t, wts_t)
    return ps


def evaluate_many(engines, ids, y, wts=None, want_p=False):
    """evaluate of every engine of a list on ONE feed, in one call (ipnn_eval_multi).  Returns a list: entry m is
    {'auc', 'rmse', 'logloss'[, 'p']}, the three metrics bit for bit what engines[m].evaluate(ids, y, wts) returns.  Where that
    call would raise FNNError(FNN_ERR_RANGE) for that model alone the entry says so instead, so that one diverged model does not
    cost the others their results: it then carries the further keys 'status' (FNN_ERR_RANGE) and 'error' (the call's message) --
      a model with a prediction NaN or outside [0, 1]: 'auc', 'rmse' and 'logloss' are NaN ('p' is still the predictions);
      only one class in y: every entry, 'auc' NaN, 'rmse' and 'logloss' as computed.
    An id outside [0, n_rows) of some engine's table is a fault of the feed and raises FNNError(FNN_ERR_RANGE) naming the
    models, as every other refusal of the call does."""
    e0 = engines[0]
    torch = e0._torch
    M = len(engines)
    ids_t, wts_t, y_t, _ = _many_feed(engines, ids, wts, y)
    n = ids_t.shape[0]
    ps = [torch.empty(n, dtype=torch.float32, device=e0.device) for _ in engines] if want_p else None
    auc, rmse, ll, status = (C.c_double * M)(), (C.c_double * M)(), (C.c_double * M)(), (C.c_int * M)()
    hs = (C.c_void_p * M)(*[e.h.value for e in engines])
    rc = e0.lib.ipnn_eval_multi(hs, M, ids_t.data_ptr(), wts_t.data_ptr() if wts_t is not None else None, y_t.data_ptr(), n,
                                auc, rmse, ll, status, (C.c_void_p * M)(*[t.data_ptr() for t in ps]) if want_p else None)
    msg = '' if rc == 0 else (e0.lib.ipnn_last_error(e0.h) or b'').decode()
    if rc != 0 and (rc != _capi.FNN_ERR_RANGE or 'feature id outside' in msg):
        raise FNNError(rc, msg)
    cur = torch.cuda.current_stream(e0.device)
    for e in engines:
        cur.wait_stream(e.stream)
    one_class = 'only one class' in msg
    outs = []
    for m in range(M):
        o = {'auc': auc[m], 'rmse': rmse[m], 'logloss': ll[m]}
        if want_p:
            o['p'] = ps[m]
        if status[m] != 0 or one_class:
            o['status'] = _capi.FNN_ERR_RANGE
            o['error'] = msg
        outs.append(o)
    return outs


def _step_masks(engines, masks):
    """The `masks` argument of train_step_many, checked before the library is called: None, or ('drawn' | 'arrays' | None, the
    list).  Entries are None (no dropout for that engine), lists of arrays as train_step takes, or Drawn; arrays and Drawn may
    not be mixed in one call (the library takes the caller's masks or its own draw, not both).  Nor may Drawn and None: the
    library draws for every model of a call or for none (ipnn_train_step_multi's seeds are one array for the list), so an engine
    that is to keep everything in a drawn call has keep_prob = 1 and its own Drawn."""
    if masks is None:
        return None, None
    masks = list(masks)
    if len(masks) != len(engines):
        raise ValueError("masks has %d entries for %d engines" % (len(masks), len(engines)))
    n_drawn = sum(isinstance(m, Drawn) for m in masks)
    n_arrays = sum(m is not None and not isinstance(m, Drawn) for m in masks)
    if n_drawn and n_arrays:
        raise ValueError("masks mixes Drawn entries and arrays: one call takes the caller's masks or the library's draw, not both")
    if n_drawn and n_drawn != len(masks):
        raise ValueError("masks mixes Drawn entries and None: a drawn call draws for every engine (keep_prob = 1 keeps everything)")
    return ('drawn' if n_drawn else 'arrays' if n_arrays else None), masks


def train_step_many(engines, ids, y, masks=None, wts=None, want_logits=False, want_loss=True):
    """train_step of every engine of a list on ONE feed, in one call (ipnn_train_step_multi).  masks: None, or a list with one
    entry per engine -- None, a list of arrays as train_step takes, or a Drawn; arrays and Drawn may not be mixed, and a drawn
    call has a Drawn for EVERY engine (the library draws for all models of a call or for none): ValueError otherwise.
    Returns a list: entry m is {'loss', 'logits'} scaled by engines[m].reduce, and afterwards every engine holds bit for bit
    what its own train_step(ids, y, masks[m], wts=wts) would have left.  Every refusal of the library raises FNNError."""
    kind, masks = _step_masks(engines, masks)
    e0 = engines[0]
    torch = e0._torch
    M = len(engines)

    def device_masks(ids_t):                  # every engine's masks on the device, in front of the stream hand-shake
        if kind != 'arrays':
            return None
        out = []
        for e, mk in zip(engines, masks):
            mts = [e0._dev(m, torch.uint8) for m in mk] if mk is not None else None
            if mts is not None and (len(mts) != len(e.hidden) + 1 or any(tuple(m.shape) != (ids_t.shape[0], e.d[t]) for t, m in enumerate(mts))):
                raise ValueError("masks: an engine takes len(hidden) + 1 arrays [B, d_t]")
            out.append(mts)
        return out
    ids_t, wts_t, y_t, keep = _many_feed(engines, ids, wts, y, torch.float32, device_masks)
    B = ids_t.shape[0]
    marr, seeds, steps = None, None, None
    if kind == 'arrays':
        rows = [(C.c_void_p * len(mts))(*[m.data_ptr() for m in mts]) if mts is not None else None for mts in keep]
        marr = (C.c_void_p * M)(*[C.cast(r, C.c_void_p).value if r is not None else None for r in rows])
        keep = (keep, rows)
    elif kind == 'drawn':
        seeds = (C.c_uint64 * M)(*[m.seed for m in masks])
        steps = (C.c_uint64 * M)(*[m.step for m in masks])
    logits = [torch.empty(B, dtype=torch.float32, device=e0.device) for _ in engines] if want_logits else None
    larr = (C.c_void_p * M)(*[t.data_ptr() for t in logits]) if want_logits else None
    loss = (C.c_float * M)()
    hs = (C.c_void_p * M)(*[e.h.value for e in engines])
    rc = e0.lib.ipnn_train_step_multi(hs, M, ids_t.data_ptr(), wts_t.data_ptr() if wts_t is not None else None, y_t.data_ptr(), B,
                                      marr, seeds, steps, larr, loss if want_loss else None)
    if rc != 0:
        raise FNNError(rc, (e0.lib.ipnn_last_error(e0.h) or b'').decode())
    cur = torch.cuda.current_stream(e0.device)
    for e in engines:
        cur.wait_stream(e.stream)
    e0._keep_many = (ids_t, wts_t, y_t, keep)
    outs = []
    for m, e in enumerate(engines):
        scale = 1.0 if e.reduce == 'sum' else 1.0 / B     # the library returns the sum of the per-example losses
        outs.append({'loss': float(loss[m]) * scale if want_loss else None, 'logits': logits[m] if want_logits else None})
    return outs


def train_epoch_many(engines, ids, y, batch_size, seeds=None, first_step=0, wts=None):
    """One pass of every engine over resident arrays in batches of batch_size (the last one ragged), every step one
    train_step_many.  With seeds, step s of engine m draws Drawn(seeds[m], first_step + s); without, no dropout.  Returns the
    list of per-step loss lists; bit for bit the loop of train_step on each engine."""
    e0 = engines[0]
    torch = e0._torch
    ids_t, y_t = e0._dev(ids, torch.int32), e0._dev(y, torch.float32)
    wts_t = e0._wts(wts, ids_t)
    if seeds is not None and len(seeds) != len(engines):
        raise ValueError("seeds has %d entries for %d engines" % (len(seeds), len(engines)))
    losses = []
    for s, lo in enumerate(range(0, ids_t.shape[0], batch_size)):
        hi = min(ids_t.shape[0], lo + batch_size)
        mk = [Drawn(sd, first_step + s) for sd in seeds] if seeds is not None else None
        out = train_step_many(engines, ids_t[lo:hi], y_t[lo:hi], masks=mk, wts=wts_t[lo:hi] if wts_t is not None else None)
        losses.append([o['loss'] for o in out])
    return losses


class _IPFamily(object):
    """Constructor signature of python/FNN_IP_L7.py:5: (cat_sizes, offsets, batch_size, _rch_argv,
    _init_argv, _ptmzr_argv, _reg_argv, mode, eval_size).  _rch_argv = [X_dim, X_feas, rank,
    h1.., act_func]; _init_argv = ['uniform', lo, hi, seeds, path] (python/tf_util.py:41-82: a
    pickle path seeds any subset of the variables); _ptmzr_argv = ['sgd', lr, ...].  X_feas is whatever ipnn_create takes
    (2..64 fields of rank <= 15, 2..32 above): an FM.dump of [D, 39, 10] seeds FNN_IP_L3 with X_feas = 39."""
    N_HIDDEN = 0
    PAIRS = True

    def __init__(self, cat_sizes, offsets, batch_size, _rch_argv, _init_argv, _ptmzr_argv, _reg_argv, mode='train',
                 eval_size=0, precision='bf16'):
        X_dim, X_feas, rank = _rch_argv[:3]
        hidden, act = list(_rch_argv[3:-1]), _rch_argv[-1]
        assert len(hidden) == self.N_HIDDEN
        if _ptmzr_argv[0] not in ('sgd', 'adam', 'ftrl'):            # python/tf_util.py:15-29 (anything else: plain gradient descent there)
            raise NotImplementedError("optimizer %r: sgd, adam and ftrl are built" % (_ptmzr_argv[0],))
        self.keep = _reg_argv[0] if mode == 'train' else 1.0
        self.eng = IPNNEngine(X_feas, rank + 1, hidden, act, max_batch=max(batch_size, eval_size, 1), precision=precision,
                              lr=_ptmzr_argv[1], keep_prob=self.keep, pairs=self.PAIRS, optimizer=_ptmzr_argv[0],
                              adam_eps=_ptmzr_argv[2] if _ptmzr_argv[0] == 'adam' else 1e-8,
                              reduce='sum' if _ptmzr_argv[-1] == 'sum' else 'mean')     # python/FNN_IP_L7.py:83-86
        lo, hi, seeds, path = _init_argv[1], _init_argv[2], _init_argv[3], _init_argv[-1]
        var_map = pickle.load(open(path, 'rb')) if path else {}
        d = self.eng.d
        rs = [np.random.RandomState(s) for s in seeds]
        j = 0

        def rnd(shape):
            nonlocal j
            v = rs[j % len(rs)].uniform(lo, hi, size=shape); j += 1
            return v
        W = var_map['W'] if 'W' in var_map else rnd((X_dim, 1))
        V = var_map['V'] if 'V' in var_map else rnd((X_dim, rank))
        b = float(np.asarray(var_map.get('b', 0.0)).ravel()[0])
        Ws, bs = [], []
        for i in range(1, len(d)):
            Ws.append(var_map['h%d_w' % i] if 'h%d_w' % i in var_map else rnd((d[i - 1], d[i])))
            bs.append(var_map['h%d_b' % i] if 'h%d_b' % i in var_map else np.zeros(d[i]))
        self.eng.set_params(np.concatenate([W, V], axis=1), b, Ws, bs)
        self.rank, self.X_dim = rank, X_dim

    def train_step(self, ids, y, masks=None, wts=None):
        return self.eng.train_step(ids, y, masks, wts=wts)

    def forward(self, ids, v_wts=None, wts=None):
        """Predictions for ids [N, X_feas] (global row ids) and, optionally, value weights wts [N, X_feas].  The reference's
        `forward(N, M, v_wts, c_ids, c_wts, ...)` (python/FNN_IP_L7.py:102-106) takes its 13 numeric and 26 categorical fields
        apart; here they are one (ids, wts) pair -- `criteo_feed(v_wts, c_ids, c_wts, offsets)` builds it -- so the reference's
        own `v_wts` keyword alone is refused."""
        if v_wts is not None:
            raise NotImplementedError("v_wts alone does not say which rows it weighs: pass wts= [N, X_feas] beside ids "
                                      "(ipnn.criteo_feed(v_wts, c_ids, c_wts, offsets) returns both)")
        return self.eng.predict(ids, wts=wts)

    def dump(self, model_path):
        """python/FNN_IP_L7.py:135-143: var_map pickle (touched rows only are current on the host:
        the full table is read back row by row)."""
        b, Ws, bs = self.eng.get_params()
        rows = self.eng.get_rows(np.arange(self.X_dim))
        var_map = {'W': rows[:, :1], 'V': rows[:, 1:], 'b': np.array([b], np.float32)}
        for i, (W, bb) in enumerate(zip(Ws, bs), start=1):
            var_map['h%d_w' % i] = W
            var_map['h%d_b' % i] = bb
        pickle.dump(var_map, open(model_path, 'wb'))


class FNN_IP_L3(_IPFamily):
    N_HIDDEN = 3


class FNN_IP_L5(_IPFamily):
    N_HIDDEN = 5


class FNN_IP_L7(_IPFamily):
    N_HIDDEN = 7


class FNN(_IPFamily):
    """The reference's plain TensorFlow `FNN` class (python/FNN.py:5-101): z1 = [e_0 .. e_{F-1} | b], two
    hidden layers, activation and inverted dropout before every matmul; var_map keys W, V, b, h1_w .. h3_b.
    (Its Criteo numeric fields -- a value times a row, :78 -- go through `wts`, as in the inner-product classes.)"""
    N_HIDDEN = 2
    PAIRS = False
