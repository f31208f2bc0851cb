"""Factorisation-machine pre-training on MI355X: the arithmetic of the reference's TensorFlow class
`FM` (python/FM.py) behind include/fm_hip.h, with the class's constructor signature, `dump` keys
(`W`, `V`, `b`) and the roles of its graph outputs (`train_step` = ptmzr + loss + train_preds,
`forward` = test_preds).  `write_fm_model` closes the loop the reference leaves open: it writes the
`fm.model.txt` text format that python/FNN_wnzh.py:62-84 parses, so that FM -> FNN runs end to end.
Optimisers: plain SGD, Adam and FTRL as python/tf_util.py:15-29 builds them (`parse_ptmzr`).
Value weights (the class's `sp_wt_hldr`, python/FM.py:24-29): `wts=` of train_step / forward / evaluate, one f32 value per
(example, field) beside its id; `model.train_step(_cols, _labels, wts=_vals)` is python/baseline.py:345's feed, and the
`(ids, wts)` pair that `ipnn.criteo_feed` makes for the inner-product family feeds FM / LR unchanged.  Without `wts` every
value is 1 (iPinYou).
The reference's own schedule -- batch_size = 1, a step per line (python/ipinyou.py:129-140, :167-173) -- is `train_online`: a
buffer of lines per call, one persistent workgroup walking them in order (fm_train_online); `ipinyou.run(..., online=True)`.
`train_online_many(models, ids, y)` runs that schedule for several models in one pass, a workgroup per model
(fm_train_online_multi), each ending bit for bit as its own `train_online` would; `ipinyou.run_many` is its driver.
`predict_many(models, ids)` / `evaluate_many(models, ids, y)` are the other half of such a search: every model's predictions and
metrics on one test feed in one call (fm_predict_multi / fm_eval_multi), each bit for bit its own `forward` / `evaluate`.
`train_step_many(models, ids, y)` is the mini-batch step of such a search: one `train_step` of every model on one batch in one
call (fm_train_step_multi), the batch's grouping shared; `ipinyou.run_many_batches` is its driver.
Rows shared between columns (`shared_rows=True`, fm_set_shared_rows): the columns of `ids` are then positions, not fields, as
python/ipinyou.py:42-65 feeds the reference -- `ipinyou.to_column_ids` makes such ids and `ipinyou.run` is the driver.
Random init uses NumPy RandomState(seed) streams (TensorFlow's cannot be reproduced here)."""
import ctypes as C
import pickle

import numpy as np

from . import _capi
from .engine import FNNError

OPTIMIZERS = {'sgd': 0, 'adam': 1, 'ftrl': 2}                      # FM_OPT_* of include/fm_hip.h


def parse_ptmzr(_ptmzr_argv):
    """python/tf_util.py:15-29's layouts: ['sgd', lr(, 'sum')], ['adam', lr, eps(, 'sum')], ['ftrl', lr(, 'sum')].
    Returns (FM_OPT_* code, lr, Adam's eps, reduce_mean); the loss is reduce_sum only when 'sum' is the LAST element
    (python/FM.py:38-41)."""
    name = _ptmzr_argv[0]
    if name not in OPTIMIZERS:
        raise NotImplementedError("optimizer %r: sgd, adam and ftrl are built (python/tf_util.py:15-29)" % (name,))
    if name == 'adam' and len(_ptmzr_argv) < 3:
        raise ValueError("adam needs ['adam', learning_rate, epsilon(, 'sum')] (python/tf_util.py:17)")
    eps = float(_ptmzr_argv[2]) if name == 'adam' else 1e-8
    return OPTIMIZERS[name], float(_ptmzr_argv[1]), eps, 0 if _ptmzr_argv[-1] == 'sum' else 1


class FM(object):
    def __init__(self, batch_size, _rch_argv, _init_argv, _ptmzr_argv, _reg_argv, mode='train', eval_size=0, device=0,
                 shared_rows=False):
        """_rch_argv = [X_dim, X_feas, rank]: X_feas fields (1..64, one id per field), rank 0..127 (python/FM.py:7).
        shared_rows: a row may sit under several columns of a batch (set_shared_rows)."""
        import torch
        X_dim, X_feas, rank = _rch_argv                              # python/FM.py:7
        self.optimizer, self.lr, self.eps, self.reduce_mean = parse_ptmzr(_ptmzr_argv)
        if not torch.cuda.is_available():
            raise FNNError(_capi.FNN_ERR_HIP, "no HIP device visible to PyTorch-ROCm; no CPU fallback")
        self._torch, self.lib = torch, _capi.load()
        self.device = torch.device('cuda', device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.X_dim, self.X_feas, self.rank = X_dim, X_feas, rank
        self.lam = float(_reg_argv[0]) if mode == 'train' else 0.0
        self.log = 'input dim: %d, features: %d, rank: %d, ' % (X_dim, X_feas, rank)
        h = C.c_void_p()
        self.max_batch = min(4096, max(batch_size, eval_size, 1))
        rc = self.lib.fm_create(X_feas, rank + 1, self.max_batch, device,
                                C.c_void_p(self.stream.cuda_stream), C.byref(h))
        if rc != 0:
            raise FNNError(rc, (self.lib.fm_last_error(None) or b'').decode())
        self.h = h
        self.shared_rows = False
        if self.optimizer:                                          # tf.train.AdamOptimizer's beta1 / beta2 defaults
            self._ck(self.lib.fm_set_optimizer(h, self.optimizer, 0.9, 0.999, self.eps))
        if shared_rows:
            self.set_shared_rows(True)
        lo, hi, seeds, path = _init_argv[1], _init_argv[2], _init_argv[3], _init_argv[-1]
        var_map = pickle.load(open(path, 'rb')) if path else {}     # python/tf_util.py:41-82
        W = var_map['W'] if 'W' in var_map else np.random.RandomState(seeds[0]).uniform(lo, hi, (X_dim, 1))
        V = var_map['V'] if 'V' in var_map else np.random.RandomState(seeds[1 % len(seeds)]).uniform(lo, hi, (X_dim, rank))
        b = float(np.asarray(var_map.get('b', 0.0)).ravel()[0])
        self.set_params(np.concatenate([np.asarray(W).reshape(X_dim, 1), np.asarray(V)], axis=1), b)

    def _ck(self, rc):
        if rc != 0:
            raise FNNError(rc, (self.lib.fm_last_error(self.h) or b'').decode())

    def close(self):
        if getattr(self, 'h', None):
            self.lib.fm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_shared_rows(self, on):
        """fm_set_shared_rows: on, a training step is right for any ids in [-1, X_dim) -- a row under several columns of a batch
        receives every column's contribution (float atomics; rows under one column keep their single rounded store)."""
        self._ck(self.lib.fm_set_shared_rows(self.h, 1 if on else 0))
        self.shared_rows = bool(on)

    def count_shared_rows(self):
        """Rows the last train_step found under more than one column (fm_count_shared_rows); FNNError(FNN_ERR_STATE) while the
        mode is off or before a step."""
        n = C.c_int64()
        self._ck(self.lib.fm_count_shared_rows(self.h, C.byref(n)))
        return int(n.value)

    def set_params(self, rows, b):
        t = np.ascontiguousarray(rows, dtype=np.float32)
        self._ck(self.lib.fm_set_table(self.h, t.ctypes.data, t.shape[0]))
        self.X_dim = t.shape[0]                  # get_params / get_opt_state size their buffers by it: fm_get_table writes n_rows rows
        self._ck(self.lib.fm_set_b(self.h, float(b)))

    def get_params(self):
        rows = np.empty((self.X_dim, self.rank + 1), np.float32)
        self._ck(self.lib.fm_get_table(self.h, rows.ctypes.data))
        b = C.c_float()
        self._ck(self.lib.fm_get_b(self.h, C.byref(b)))
        return rows, float(b.value)

    def _dev(self, a, dtype):
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _wts(self, wts, ids_t):
        """wts [B, X_feas] f32 on the device, or None (every value 1); ValueError unless its shape is ids'."""
        if wts is None:
            return None
        shape = tuple(wts.shape) if hasattr(wts, 'shape') else np.shape(wts)
        if shape != tuple(ids_t.shape):
            raise ValueError("wts has shape %s, ids %s: one weight per (example, field)" % (shape, tuple(ids_t.shape)))
        return self._dev(wts, self._torch.float32)

    def train_step(self, ids, y, want_p=False, want_loss=True, wts=None):
        """ids [B, X_feas] int32 (-1 = absent), y [B], wts [B, X_feas] f32 or None (every value 1): e_f = wts[t, f] * row(ids[t, f])
        (python/FM.py:55-64).  `model.train_step(_cols, _labels, wts=_vals)` is python/baseline.py:345's feed; the (ids, wts) pair
        of ipnn.criteo_feed feeds this unchanged.  Returns {'loss', 'p'} (python/ipinyou.py:171)."""
        torch = self._torch
        ids_t, y_t = self._dev(ids, torch.int32), self._dev(y, torch.float32)
        w_t = self._wts(wts, ids_t)
        B = ids_t.shape[0]
        p = torch.empty(B, dtype=torch.float32, device=self.device) if want_p else None
        loss = C.c_float()
        if B > 4096:                # one call = ONE optimiser step (python/ipinyou.py:171); splitting it would change the update
            raise FNNError(_capi.FNN_ERR_ARG, "FM.train_step: batch %d > 4096 (fm_create's largest step)" % B)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ck(self.lib.fm_train_step_w(self.h, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), B,
                                          self.lr, self.lam, self.reduce_mean, p.data_ptr() if want_p else None,
                                          C.byref(loss) if want_loss else None))
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self._keep = (ids_t, y_t, w_t)
        return {'loss': float(loss.value) if want_loss else None, 'p': p}

    def train_online(self, ids, y, wts=None, want_p=False, want_loss=True):
        """fm_train_online: the N lines of ids [N, X_feas] as N batch-1 SGD steps in line order (python/ipinyou.py:129-140 builds FM
        and LR with batch_size = 1, :167-173 runs a step per line), example n on the parameters examples 0..n-1 left; N is not
        bounded by max_batch.  Plain SGD only: FNNError(FNN_ERR_STATE) under Adam / FTRL.  Returns {'loss': the sum of the N
        data losses, 'loss_last': the last line's (the `l` python/ipinyou.py:177 prints), 'p': sigmoid(yhat_n) before line n's
        update, or None}; both losses are None without want_loss (no synchronisation then)."""
        torch = self._torch
        ids_t, y_t = self._dev(ids, torch.int32), self._dev(y, torch.float32)
        if ids_t.dim() != 2 or ids_t.shape[1] != self.X_feas or y_t.shape != (ids_t.shape[0],):
            raise ValueError("ids %s, y %s: need [N, %d] and [N]" % (tuple(ids_t.shape), tuple(y_t.shape), self.X_feas))
        w_t = self._wts(wts, ids_t)
        N = ids_t.shape[0]
        p = torch.empty(N, dtype=torch.float32, device=self.device) if want_p else None
        loss, last = C.c_double(), C.c_float()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ck(self.lib.fm_train_online(self.h, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), N,
                                          self.lr, self.lam, p.data_ptr() if want_p and N else None,
                                          C.byref(loss) if want_loss else None, C.byref(last) if want_loss else None))
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self._keep = (ids_t, y_t, w_t)
        return {'loss': float(loss.value) if want_loss else None, 'loss_last': float(last.value) if want_loss else None, 'p': p}

    def online_form(self):
        """fm_online_form: the form of the online kernel this handle runs."""
        return self.lib.fm_online_form(self.h).decode()

    def forward(self, ids, wts=None):
        """sigmoid(yhat) [N] (`test_preds`), max_batch examples a call; wts as in train_step."""
        torch = self._torch
        ids_t = self._dev(ids, torch.int32)
        w_t = self._wts(wts, ids_t)
        out = torch.empty(ids_t.shape[0], dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, ids_t.shape[0], self.max_batch):
            hi = min(ids_t.shape[0], lo + self.max_batch)
            self._ck(self.lib.fm_predict_w(self.h, ids_t[lo:hi].data_ptr(), None if w_t is None else w_t[lo:hi].data_ptr(), hi - lo,
                                           out[lo:hi].data_ptr()))
        self._ck(self.lib.fm_sync(self.h))
        return out

    def evaluate(self, ids, y, wts=None):
        """Predictions and (auc, rmse, logloss) on the device (fm_eval_w): exact AUC, ties at 1/2; wts as in train_step.
        y: 0 / non-zero.  FNNError(FNN_ERR_RANGE) for one class only and for any prediction NaN or outside [0, 1]."""
        torch = self._torch
        ids_t, y_t = self._dev(ids, torch.int32), self._dev(y, torch.int32)
        w_t = self._wts(wts, ids_t)
        auc, rmse, ll = C.c_double(), C.c_double(), C.c_double()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ck(self.lib.fm_eval_w(self.h, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), ids_t.shape[0],
                                    C.byref(auc), C.byref(rmse), C.byref(ll)))
        return auc.value, rmse.value, ll.value

    def get_opt_state(self):
        """Adam (m, v) or FTRL (accum, linear) of the rows [X_dim, rank + 1] and of the bias [2], and the step count."""
        K = self.rank + 1
        s0, s1 = np.empty((self.X_dim, K), np.float32), np.empty((self.X_dim, K), np.float32)
        sb, t = np.empty(2, np.float32), C.c_int64()
        self._ck(self.lib.fm_get_opt_state(self.h, s0.ctypes.data, s1.ctypes.data, sb.ctypes.data, C.byref(t)))
        return s0, s1, sb, t.value

    def dump(self, model_path):                                      # python/FM.py:66-69
        rows, b = self.get_params()
        pickle.dump({'W': rows[:, :1], 'V': rows[:, 1:], 'b': np.array([b], np.float32)}, open(model_path, 'wb'))
        print('model dumped at %s' % model_path)

    def write_fm_model(self, path, field_of_row, field_names, feat_ids=None):
        """`fm.model.txt` as python/FNN_wnzh.py:68-84 reads it: `w_0 feat_num rank`, then per feature
        `feat w v_1..v_rank <fieldname>:<feat>`.  repr() of the float32 values keeps them exact."""
        rows, b = self.get_params()
        feat_ids = np.arange(len(rows)) if feat_ids is None else np.asarray(feat_ids)
        with open(path, 'w') as f:
            f.write('%r %d %d\n' % (float(b), len(rows), self.rank))
            for i in range(len(rows)):
                f.write('%d %s %s:%d\n' % (feat_ids[i], ' '.join(repr(float(v)) for v in rows[i]),
                                           field_names[int(field_of_row[i])], feat_ids[i]))


def train_online_many(models, ids, y, wts=None, want_p=False, want_loss=True):
    """fm_train_online_multi: the online schedule of `train_online` for every model of `models` (FM / LR objects, ranks, table
    sizes, lr and lam their own) in ONE pass over the lines, a workgroup per model.  Every model ends bit for bit as its own
    `train_online(ids, y, wts, ...)` would have left it.  Returns the list of the dicts `train_online` returns, in the order
    of `models`.  ValueError for an empty list or models that differ in X_feas; FNNError for what the library refuses (a
    model twice, Adam / FTRL, different devices, ...: nothing is trained then)."""
    models = list(models)
    if not models:
        raise ValueError("train_online_many: no models")
    first = models[0]
    if any(m.X_feas != first.X_feas for m in models):
        raise ValueError("train_online_many: the models differ in X_feas %s: one feed, one width" % ([m.X_feas for m in models],))
    torch, lib, M = first._torch, first.lib, len(models)
    ids_t, y_t = first._dev(ids, torch.int32), first._dev(y, torch.float32)
    if ids_t.dim() != 2 or ids_t.shape[1] != first.X_feas or y_t.shape != (ids_t.shape[0],):
        raise ValueError("ids %s, y %s: need [N, %d] and [N]" % (tuple(ids_t.shape), tuple(y_t.shape), first.X_feas))
    w_t = first._wts(wts, ids_t)
    N = ids_t.shape[0]
    ps = [torch.empty(N, dtype=torch.float32, device=first.device) if want_p else None for _ in models]
    hs = (C.c_void_p * M)(*[m.h.value if m.h else None for m in models])
    lrs, lams = (C.c_float * M)(*[m.lr for m in models]), (C.c_float * M)(*[m.lam for m in models])
    p_arr = (C.c_void_p * M)(*[p.data_ptr() if want_p and N else None for p in ps])
    loss, last = (C.c_double * M)(), (C.c_float * M)()
    cur = torch.cuda.current_stream(first.device)
    for m in models:
        m.stream.wait_stream(cur)
    rc = lib.fm_train_online_multi(hs, M, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), N, lrs, lams,
                                   p_arr if want_p else None, loss if want_loss else None, last if want_loss else None)
    if rc != 0:
        # the message is with hs[0], or with the library when hs[0] is no handle (a closed model)
        raise FNNError(rc, (lib.fm_last_error(first.h if first.h else None) or b'').decode())
    for m in models:
        cur.wait_stream(m.stream)
        m._keep = (ids_t, y_t, w_t)
    return [{'loss': float(loss[i]) if want_loss else None, 'loss_last': float(last[i]) if want_loss else None, 'p': ps[i]}
            for i in range(M)]


def train_step_many(models, ids, y, wts=None, want_p=False, want_loss=True):
    """fm_train_step_multi: ONE optimiser step of `train_step` for every model of `models` (FM / LR objects; ranks, table sizes,
    optimisers, lr, lam and shared_rows their own) on the one mini-batch ids [B, X_feas], y [B], in one call: the models that agree
    in table size and shared_rows share the batch's grouping, and every other stage is one launch for all of them.  Every model
    ends bit for bit as its own `train_step(ids, y, wts=wts, ...)` would have left it (rows really shared between columns: to
    rounding, as there).  Returns the list of the {'loss', 'p'} dicts `train_step` returns, in the order of `models`.
    ValueError for an empty list, models that differ in X_feas or a bad wts shape; FNNError for what the library refuses (a model
    twice, B above a model's max_batch, ...: nothing is trained then) and for an id outside [-1, X_dim) of some model."""
    models = list(models)
    if not models:
        raise ValueError("train_step_many: no models")
    first = models[0]
    if any(m.X_feas != first.X_feas for m in models):
        raise ValueError("train_step_many: the models differ in X_feas %s: one feed, one width" % ([m.X_feas for m in models],))
    torch, lib, M = first._torch, first.lib, len(models)
    ids_t, y_t = first._dev(ids, torch.int32), first._dev(y, torch.float32)
    if ids_t.dim() != 2 or ids_t.shape[1] != first.X_feas or y_t.shape != (ids_t.shape[0],):
        raise ValueError("ids %s, y %s: need [B, %d] and [B]" % (tuple(ids_t.shape), tuple(y_t.shape), first.X_feas))
    w_t = first._wts(wts, ids_t)
    B = ids_t.shape[0]
    if B > 4096:                    # one call = ONE optimiser step per model, as in train_step
        raise FNNError(_capi.FNN_ERR_ARG, "train_step_many: batch %d > 4096 (fm_create's largest step)" % B)
    ps = [torch.empty(B, dtype=torch.float32, device=first.device) if want_p else None for _ in models]
    hs = (C.c_void_p * M)(*[m.h.value if m.h else None for m in models])
    lrs, lams = (C.c_float * M)(*[m.lr for m in models]), (C.c_float * M)(*[m.lam for m in models])
    means = (C.c_int * M)(*[m.reduce_mean for m in models])
    p_arr = (C.c_void_p * M)(*[p.data_ptr() if want_p else None for p in ps])
    loss = (C.c_float * M)()
    cur = torch.cuda.current_stream(first.device)
    for m in models:
        m.stream.wait_stream(cur)
    rc = lib.fm_train_step_multi(hs, M, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), B, lrs, lams,
                                 means, p_arr if want_p else None, loss if want_loss else None)
    if rc != 0:
        raise _many_error(first, rc)
    for m in models:
        cur.wait_stream(m.stream)
        m._keep = (ids_t, y_t, w_t)
    return [{'loss': float(loss[i]) if want_loss else None, 'p': ps[i]} for i in range(M)]


def _many_feed(what, models, ids, wts):
    """The checks and the one device feed of predict_many / evaluate_many: (models, ids_t, w_t, handle array)."""
    models = list(models)
    if not models:
        raise ValueError("%s: no models" % what)
    first = models[0]
    if any(m.X_feas != first.X_feas for m in models):
        raise ValueError("%s: the models differ in X_feas %s: one feed, one width" % (what, [m.X_feas for m in models]))
    ids_t = first._dev(ids, first._torch.int32)
    if ids_t.dim() != 2 or ids_t.shape[1] != first.X_feas:
        raise ValueError("ids %s: need [N, %d]" % (tuple(ids_t.shape), first.X_feas))
    hs = (C.c_void_p * len(models))(*[m.h.value if m.h else None for m in models])
    return models, ids_t, first._wts(wts, ids_t), hs


def _many_error(first, rc):
    # the message is with hs[0], or with the library when hs[0] is no handle (a closed model)
    return FNNError(rc, (first.lib.fm_last_error(first.h if first.h else None) or b'').decode())


def predict_many(models, ids, wts=None):
    """fm_predict_multi: sigmoid(yhat) [N] of every model of `models` (FM / LR objects; ranks, table sizes and optimisers their own)
    on the one feed `ids` [N, X_feas] (a device tensor is used as it is), in one call instead of N / max_batch calls per model.
    Returns the list of device tensors, each bit for bit what the model's `forward(ids, wts)` returns.  ValueError for an empty
    list or models that differ in X_feas; FNNError for what the library refuses and, as `forward`, for an id outside
    [-1, X_dim) of some model (the models' indices in the message; such an id is absent for that model)."""
    models, ids_t, w_t, hs = _many_feed("predict_many", models, ids, wts)
    first, M, N = models[0], len(models), ids_t.shape[0]
    torch = first._torch
    ps = [torch.empty(N, dtype=torch.float32, device=first.device) for _ in models]
    p_arr = (C.c_void_p * M)(*[p.data_ptr() for p in ps])
    cur = torch.cuda.current_stream(first.device)
    for m in models:
        m.stream.wait_stream(cur)
    rc = first.lib.fm_predict_multi(hs, M, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), N, p_arr)
    if rc != 0:
        raise _many_error(first, rc)
    bad = []
    for i, m in enumerate(models):
        cur.wait_stream(m.stream)
        m._keep = (ids_t, None, w_t)
        rs = m.lib.fm_sync(m.h)
        if rs == _capi.FNN_ERR_RANGE:
            bad.append(i)
        elif rs != 0:
            m._ck(rs)
    if bad:
        raise FNNError(_capi.FNN_ERR_RANGE, "predict_many: feature id outside [-1, n_rows) in model(s) " + ', '.join(map(str, bad)))
    return ps


def evaluate_many(models, ids, y, wts=None):
    """fm_eval_multi: what `evaluate(ids, y, wts)` gives for every model of `models`, on ONE upload of the feed, with one scratch
    allocation, one launch per stage for all the models and one synchronisation (per group of models that fit the scratch cap).
    ids / y / wts may be device tensors already.  Returns a list of {'auc', 'rmse', 'logloss', 'status'}, the three numbers bit for
    bit `evaluate`'s.  Nothing is raised for what `evaluate` reports about the numbers themselves: 'status' is FNN_ERR_RANGE (-4)
    and the three are NaN for a model with a prediction NaN or outside [0, 1] -- a search wants the other models' results -- and
    with one class only in y every 'auc' is NaN.  Every other error raises: ValueError for an empty list or models that differ
    in X_feas, FNNError for what the library refuses and for an id outside [-1, X_dim) of some model."""
    models, ids_t, w_t, hs = _many_feed("evaluate_many", models, ids, wts)
    first, M, N = models[0], len(models), ids_t.shape[0]
    torch = first._torch
    y_t = first._dev(y, torch.int32)
    if y_t.shape != (N,):
        raise ValueError("ids %s, y %s: need [N, %d] and [N]" % (tuple(ids_t.shape), tuple(y_t.shape), first.X_feas))
    auc, rmse, ll, status = (C.c_double * M)(), (C.c_double * M)(), (C.c_double * M)(), (C.c_int * M)()
    cur = torch.cuda.current_stream(first.device)
    for m in models:
        m.stream.wait_stream(cur)
    rc = first.lib.fm_eval_multi(hs, M, ids_t.data_ptr(), None if w_t is None else w_t.data_ptr(), y_t.data_ptr(), N,
                                 auc, rmse, ll, status)
    if rc != 0:
        err = _many_error(first, rc)
        if rc != _capi.FNN_ERR_RANGE or 'feature id' in str(err):
            raise err
    for m in models:
        cur.wait_stream(m.stream)
    return [{'auc': auc[i], 'rmse': rmse[i], 'logloss': ll[i], 'status': status[i]} for i in range(M)]
