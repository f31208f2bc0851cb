"""Loader interface #2: the iPinYou "yzx" readers of the reference's python/ipinyou.py
(`collect`, `stat`, `load_ipinyou_data`, `feed_zero`), same names, arguments and return values.
Line format: `y z idx:val idx:val ...` (token 1, `z`, is skipped).  The loaders are host logic; `run` is the
reference's FM / LR driver (python/ipinyou.py:113-199) on the device: `to_column_ids` turns the loaders' positional
arrays into the ids of FM / LR with `shared_rows=True`, where a column is a position of the line and not a field.
"""
import os
import sys
import time

import numpy as np


def collect(fin, size=100000):
    """python/ipinyou.py:11-20: up to `size` lines from the open file, shuffled in place with the
    global NumPy RNG."""
    buf = []
    for _ in range(size):
        line = next(fin, '')
        if line == '':
            break
        buf.append(line)
    np.random.shuffle(buf)
    return buf


def _indices(line):
    fields = line.strip().split()
    return int(fields[0]), [int(tok.split(':')[0]) for tok in fields[2:]]


def stat(path):
    """python/ipinyou.py:23-39: (max_dim, max_fea) over the whole file."""
    max_fea = 0
    max_dim = 0
    with open(path) as fin:
        while True:
            buf = collect(fin)
            if len(buf) < 1:
                break
            for line in buf:
                _, x_ind = _indices(line)
                max_fea = max(max_fea, len(x_ind))
                max_dim = max(max_dim, max(x_ind))
    return max_dim, max_fea


def load_ipinyou_data(fin, size, max_dim, max_fea):
    """python/ipinyou.py:42-65: next `size` lines -> X_ind [n,max_fea] int (pad id = max_dim),
    X_val [n,max_fea] (1 present, 0 pad), y [n]; (None, None, None) at EOF."""
    buf = collect(fin, size)
    if len(buf) < 1:
        return None, None, None
    X_ind, X_val, y = [], [], []
    for line in buf:
        yy, x_ind = _indices(line)
        pad = max_fea - len(x_ind)
        y.append(yy)
        X_ind.append(x_ind + [max_dim] * pad)
        X_val.append([1] * len(x_ind) + [0] * pad)
    return np.array(X_ind), np.array(X_val), np.array(y)


def feed_zero(X_ind, X_val, y, max_dim, max_fea):
    """python/ipinyou.py:68-89: pad ragged in-memory lists, then shuffle examples."""
    for i in range(len(y)):
        pad = max_fea - len(X_ind[i])
        X_ind[i].extend([max_dim] * pad)
        X_val[i].extend([0] * pad)
    X_ind = np.array(X_ind)
    X_val = np.array(X_val)
    y = np.array(y)
    inds = np.arange(len(y))
    np.random.shuffle(inds)
    return X_ind[inds], X_val[inds], y[inds]


def stat_file(path):
    """`stat` as one native pass (ctr_yzx_stat): (max_dim, max_fea).  Unlike `stat` it does not
    shuffle buffers, so it leaves the global NumPy RNG untouched."""
    from . import ingest
    md, mf, _ = ingest.yzx_stat(path)
    return md, mf


def load_ipinyou_file(path, max_dim, max_fea):
    """`load_ipinyou_data` for a whole file in one native pass (ctr_parse_yzx), FILE order: the
    reference shuffles each 10,000-line buffer with the global RNG (python/ipinyou.py:19) -- apply
    a permutation afterwards where that order matters."""
    from . import ingest
    return ingest.parse_yzx(path, max_dim, max_fea)


def to_field_ids(X_ind, X_val, field_of_row):
    """Bridge to the HIP path: padded index lists -> ids int32 [n, n_fields] with slot = field and -1 for
    empty fields (pads have X_val == 0)."""
    n = X_ind.shape[0]
    n_fields = int(field_of_row.max()) + 1
    ids = np.full((n, n_fields), -1, dtype=np.int32)
    for j in range(X_ind.shape[1]):
        present = X_val[:, j] != 0
        rows = X_ind[present, j]
        ids[np.nonzero(present)[0], field_of_row[rows]] = rows
    return ids


def to_column_ids(X_ind, X_val):
    """Bridge to FM / LR with shared_rows=True: the output of load_ipinyou_data / feed_zero / load_ipinyou_file unchanged ->
    (ids int32 [n, max_fea], wts).  Column j is position j of the line (python/ipinyou.py:42-65), X_val == 0 (the pads) becomes
    id -1; wts is None when every present value is 1, else X_val as float32.  Nothing is dropped: a row may sit under any
    number of columns of a batch, which is what shared_rows is for."""
    X_ind, X_val = np.asarray(X_ind), np.asarray(X_val)
    present = X_val != 0
    ids = np.where(present, X_ind, -1).astype(np.int32)
    wts = None if (X_val[present] == 1).all() else np.ascontiguousarray(X_val, dtype=np.float32)
    return np.ascontiguousarray(ids), wts


def exact_auc(labels, preds):
    """roc_auc_score (ties at 1/2) of a buffer's training predictions for the log line; -1 with one class only, as
    python/ipinyou.py:100-103 logs it."""
    labels, preds = np.asarray(labels) != 0, np.asarray(preds, dtype=np.float64)
    n1 = int(labels.sum())
    n0 = len(labels) - n1
    if n0 == 0 or n1 == 0:
        return -1
    _, inv, cnt = np.unique(preds, return_inverse=True, return_counts=True)
    rank = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv]           # mean rank of a tie group, 1-based
    return (rank[labels].sum() - n1 * (n1 + 1) / 2.0) / (n0 * float(n1))


def _dims(train_path, test_path):
    """(X_dim, X_feas) as python/ipinyou.py:117-121 takes them: `stat` of both files, X_dim = max + 2, X_feas = the longest line."""
    X_dim_train, X_feas_train = stat(train_path)
    X_dim_test, X_feas_test = stat(test_path)
    X_feas = max(X_feas_train, X_feas_test)
    if X_feas > 64:
        raise ValueError("the longest line has %d features: FM / LR take at most 64 columns (fm_create)" % X_feas)
    return max(X_dim_train, X_dim_test) + 2, X_feas


def _load_eval(test_path, eval_size, X_dim, X_feas):
    """The test lines one evaluation of `run` sees: chunks of eval_size lines, at most 10 * eval_size of them
    (python/ipinyou.py:196), each shuffled as load_ipinyou_data shuffles.  (ids, wts, y), or None for an empty file."""
    e_ids, e_wts, e_y = [], [], []
    with open(test_path) as test_data_set:
        while sum(len(v) for v in e_y) < 10 * eval_size:
            t_ind, t_val, t_y = load_ipinyou_data(test_data_set, eval_size, X_dim - 1, X_feas)
            if t_ind is None:
                break
            e_ids.append(t_ind), e_wts.append(t_val), e_y.append(t_y)
    if not e_y:
        return None
    return to_column_ids(np.concatenate(e_ids), np.concatenate(e_wts)) + (np.concatenate(e_y),)


def _eval_auc(model, test):
    """The model's AUC on _load_eval's lines; -1 without lines or with one class only, as watch_train logs it."""
    if test is None:
        return -1
    try:
        return model.evaluate(test[0], test[2], wts=test[1])[0]
    except RuntimeError as e:
        if getattr(e, 'code', None) != -4 or 'one class' not in str(e):
            raise
    return -1


def _eval_aucs(models, test):
    """_eval_auc for every model of run_many in one FM.evaluate_many call: the test lines are converted and uploaded once, not
    once per model.  A model whose predictions left [0, 1] raises, as its own `evaluate` would."""
    from .FM import evaluate_many
    from .engine import FNNError
    if test is None:
        return [-1] * len(models)
    out = evaluate_many(models, test[0], test[2], wts=test[1])
    for i, r in enumerate(out):
        if r['status'] != 0:
            raise FNNError(r['status'], "run_many: model %d has predictions NaN or outside [0, 1]" % i)
    return [-1 if r['auc'] != r['auc'] else r['auc'] for r in out]         # NaN: one class only


def _appender(log_file, echo):
    def write_log(line):
        if log_file:
            with open(log_file, 'a') as f:
                f.write(line + '\n')
        if echo:
            print(line)
    return write_log


def run(train_path, test_path, algo='FM', batch_size=4096, buffer=10000, eval_size=100000, epochs=1, log_file=None, device=0,
        echo=True, online=False):
    """python/ipinyou.py:113-199, the FM / LR driver, on the device.  `stat` both files, X_dim = max + 2, X_feas = the longest
    line; LR (:133) or FM rank 10 (:139-140) with the reference's init, optimiser and L2 weight and shared_rows=True; per pass
    over the training file, buffers of `buffer` shuffled lines (load_ipinyou_data) in mini-batches of `batch_size`, each one
    train_step; after every buffer the test file is evaluated on the device (fm_eval) in chunks of eval_size lines, at most
    10 * eval_size of them (:196), and watch_train's line `step\tbatch_auc\teval_auc\tloss\t` is written to log_file.
    online=True is the reference's schedule end to end: batch_size is ignored, every buffer is ONE train_online call -- a batch-1
    SGD step per line, in the buffer's shuffled order (python/ipinyou.py:129-140, :167-173) -- and the logged loss is the last
    line's, as :177 has it; give buffer=100000 for LR (:131), the 10000 default is FM's (:137).
    Differences from the reference: without `online`, batch_size is a parameter (its 1 is allowed but costs a whole step's launches
    per line; a buffer's tail shorter than batch_size is one shorter step); `epochs` passes instead of an endless loop, every
    buffer is evaluated (the reference skips a short last one) and a last test chunk shorter than eval_size counts.  Lines longer than fm_create's 64 columns raise ValueError.
    Returns {'model', 'log': [(step, batch_auc, eval_auc, loss)], 'X_dim', 'X_feas'}."""
    from .FM import FM
    from .LR import LR
    X_dim, X_feas = _dims(train_path, test_path)
    if online:
        batch_size = 1                                             # the models are built as the reference builds them
    if batch_size < 1 or batch_size > 4096:
        raise ValueError("batch_size %d: one step takes 1..4096 examples" % batch_size)
    max_eval = min(eval_size, 4096)
    if 'LR' in algo:
        model = LR(batch_size, [X_dim, X_feas], ['uniform', -0.001, 0.001, [0x89AB], None], ['sgd', 1e-3], [1e-3],
                   'train', max_eval, device, shared_rows=True)
    elif 'FM' in algo:
        model = FM(batch_size, [X_dim, X_feas, 10], ['uniform', -0.001, 0.001, [0x3210, 0x7654], None], ['sgd', 1e-3],
                   [1e-2], 'train', max_eval, device, shared_rows=True)
    else:
        raise ValueError("algo %r: 'LR' or 'FM'" % (algo,))

    write_log = _appender(log_file, echo)
    write_log(model.log)
    history = []
    for it in range(epochs):
        step = 0
        start_time = time.time()
        with open(train_path) as train_data_set:
            while True:
                X_ind, X_val, labels = load_ipinyou_data(train_data_set, buffer, X_dim - 1, X_feas)
                if X_ind is None:
                    break
                ids, wts = to_column_ids(X_ind, X_val)
                preds, loss = [], float('nan')
                if online:
                    out = model.train_online(ids, labels, wts=wts, want_p=True)
                    preds.append(out['p'].cpu().numpy())
                    loss = out['loss_last']
                for lo in range(0, 0 if online else len(labels), batch_size):
                    out = model.train_step(ids[lo:lo + batch_size], labels[lo:lo + batch_size], want_p=True,
                                           wts=None if wts is None else wts[lo:lo + batch_size])
                    preds.append(out['p'].cpu().numpy())
                    loss = out['loss']
                step += len(labels)
                if echo:
                    print('step: %d\ttime: %d\tloss: %g' % (step, time.time() - start_time, loss))
                eval_auc = _eval_auc(model, _load_eval(test_path, eval_size, X_dim, X_feas))
                batch_auc = exact_auc(labels, np.concatenate(preds))
                history.append((step, batch_auc, eval_auc, loss))
                write_log('%d\t%g\t%g\t%g\t' % (step, batch_auc, eval_auc, loss))
                start_time = time.time()
    return {'model': model, 'log': history, 'X_dim': X_dim, 'X_feas': X_feas}


def run_many(train_path, test_path, specs, buffer=10000, eval_size=100000, epochs=1, log_file=None, device=0, echo=True):
    """`run(..., online=True)` for several models in ONE pass over the training file: the reference's driver trains LR and FM on
    the same file (python/ipinyou.py:133, :139), its notebook FM10 / FM50 / FM100, each with a learning-rate and L2 search.
    specs: a list of (algo, rank, lr, lam), algo 'LR' | 'FM' (rank is ignored for LR); the models are built as `run` builds
    them (its init and seeds, plain SGD, shared_rows=True, batch_size 1).  Every buffer is one FM.train_online_many call -- a
    workgroup per model walks the buffer's lines, so every model sees the schedule `run(..., online=True)` gives it, bit for
    bit -- followed by ONE FM.evaluate_many call for all of them on the same test lines (fm_eval_multi: each model's numbers are
    its own `evaluate`'s, bit for bit).  One log line per model per buffer, `run`'s line behind
    the spec's index and a tab.  Returns a list of what `run` returns, one per spec."""
    from .FM import FM, train_online_many
    from .LR import LR
    specs = [tuple(s) for s in specs]
    if not specs:
        raise ValueError("run_many: no specs")
    for algo, rank, lr, lam in specs:
        if algo not in ('LR', 'FM'):
            raise ValueError("algo %r: 'LR' or 'FM'" % (algo,))
    X_dim, X_feas = _dims(train_path, test_path)
    max_eval = min(eval_size, 4096)
    models = []
    for algo, rank, lr, lam in specs:
        if algo == 'LR':
            models.append(LR(1, [X_dim, X_feas], ['uniform', -0.001, 0.001, [0x89AB], None], ['sgd', lr], [lam],
                             'train', max_eval, device, shared_rows=True))
        else:
            models.append(FM(1, [X_dim, X_feas, int(rank)], ['uniform', -0.001, 0.001, [0x3210, 0x7654], None], ['sgd', lr],
                             [lam], 'train', max_eval, device, shared_rows=True))
    write_log = _appender(log_file, echo)
    for i, model in enumerate(models):
        write_log('%d\t%s' % (i, model.log))
    history = [[] for _ in models]
    for it in range(epochs):
        step = 0
        with open(train_path) as train_data_set:
            while True:
                X_ind, X_val, labels = load_ipinyou_data(train_data_set, buffer, X_dim - 1, X_feas)
                if X_ind is None:
                    break
                ids, wts = to_column_ids(X_ind, X_val)
                outs = train_online_many(models, ids, labels, wts=wts, want_p=True)
                step += len(labels)
                eval_aucs = _eval_aucs(models, _load_eval(test_path, eval_size, X_dim, X_feas))
                for i, out in enumerate(outs):
                    rec = (step, exact_auc(labels, out['p'].cpu().numpy()), eval_aucs[i], out['loss_last'])
                    history[i].append(rec)
                    write_log('%d\t' % i + '%d\t%g\t%g\t%g\t' % rec)
    return [{'model': m, 'log': h, 'X_dim': X_dim, 'X_feas': X_feas} for m, h in zip(models, history)]


def run_many_batches(train_path, test_path, specs, batch_size=4096, buffer=10000, eval_size=100000, epochs=1, log_file=None,
                     device=0, echo=True):
    """`run`'s mini-batch schedule for several models in ONE pass over the training file: specs as in run_many, the models built
    as `run` builds them (its init and seeds, plain SGD, shared_rows=True, batch_size as given).  Every mini-batch of a buffer is
    one FM.train_step_many call (fm_train_step_multi: the models share the batch's grouping, and each ends as its own
    `train_step` would have left it), a buffer's tail shorter than batch_size one shorter step as in `run`; every buffer is
    followed by ONE FM.evaluate_many call on the test lines.  run_many's log format and return value; the logged loss is the
    last mini-batch's, as in `run`."""
    from .FM import FM, train_step_many
    from .LR import LR
    specs = [tuple(s) for s in specs]
    if not specs:
        raise ValueError("run_many_batches: no specs")
    for algo, rank, lr, lam in specs:
        if algo not in ('LR', 'FM'):
            raise ValueError("algo %r: 'LR' or 'FM'" % (algo,))
    if batch_size < 1 or batch_size > 4096:
        raise ValueError("batch_size %d: one step takes 1..4096 examples" % batch_size)
    X_dim, X_feas = _dims(train_path, test_path)
    max_eval = min(eval_size, 4096)
    models = []
    for algo, rank, lr, lam in specs:
        if algo == 'LR':
            models.append(LR(batch_size, [X_dim, X_feas], ['uniform', -0.001, 0.001, [0x89AB], None], ['sgd', lr], [lam],
                             'train', max_eval, device, shared_rows=True))
        else:
            models.append(FM(batch_size, [X_dim, X_feas, int(rank)], ['uniform', -0.001, 0.001, [0x3210, 0x7654], None],
                             ['sgd', lr], [lam], 'train', max_eval, device, shared_rows=True))
    write_log = _appender(log_file, echo)
    for i, model in enumerate(models):
        write_log('%d\t%s' % (i, model.log))
    history = [[] for _ in models]
    for it in range(epochs):
        step = 0
        with open(train_path) as train_data_set:
            while True:
                X_ind, X_val, labels = load_ipinyou_data(train_data_set, buffer, X_dim - 1, X_feas)
                if X_ind is None:
                    break
                ids, wts = to_column_ids(X_ind, X_val)
                preds, loss = [[] for _ in models], [float('nan')] * len(models)
                for lo in range(0, len(labels), batch_size):
                    outs = train_step_many(models, ids[lo:lo + batch_size], labels[lo:lo + batch_size], want_p=True,
                                           wts=None if wts is None else wts[lo:lo + batch_size])
                    for i, out in enumerate(outs):
                        preds[i].append(out['p'].cpu().numpy())
                        loss[i] = out['loss']
                step += len(labels)
                eval_aucs = _eval_aucs(models, _load_eval(test_path, eval_size, X_dim, X_feas))
                for i in range(len(models)):
                    rec = (step, exact_auc(labels, np.concatenate(preds[i])), eval_aucs[i], loss[i])
                    history[i].append(rec)
                    write_log('%d\t' % i + '%d\t%g\t%g\t%g\t' % rec)
    return [{'model': m, 'log': h, 'X_dim': X_dim, 'X_feas': X_feas} for m, h in zip(models, history)]


def parse_spec(text):
    """'FM:10:1e-3:1e-2' -> ('FM', 10, 1e-3, 1e-2): algo:rank:lr:lambda of run_many."""
    algo, rank, lr, lam = text.split(':')
    return algo, int(rank), float(lr), float(lam)


if __name__ == '__main__':
    # python/ipinyou.py:113-127: the campaign's yzx files under DEEPCTR_DATA_DIR (default ../data, as FNN.py), the log under
    # DEEPCTR_LOG_DIR (default ../log/); `python ipinyou.py [FM|LR] [batch_size | online]`, or
    # `python ipinyou.py many FM:10:1e-3:1e-2 LR:0:1e-3:1e-3 ...` (algo:rank:lr:lambda, run_many), or
    # `python ipinyou.py many-batch 4096 FM:10:1e-3:1e-2 LR:0:1e-3:1e-3 ...` (run_many_batches: mini-batches of 4096)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deep_ctr_amd import ipinyou as _drv
    cam = 'all'
    data_dir = os.environ.get('DEEPCTR_DATA_DIR', '../data')
    algo = sys.argv[1] if len(sys.argv) > 1 else 'FM'
    tag = (str(cam) + ' ' + time.strftime('%c') + ' ' + algo).replace(' ', '_')
    log_dir = os.environ.get('DEEPCTR_LOG_DIR', '../log/')
    if not os.path.exists(log_dir):
        os.makedirs(log_dir)
    print(os.path.join(log_dir, tag))
    if algo == 'many':
        _drv.run_many(os.path.join(data_dir, 'ipinyou-data/%s/train.yzx.txt.shuf' % cam),
                      os.path.join(data_dir, 'ipinyou-data/%s/test.yzx.txt.shuf' % cam), [_drv.parse_spec(a) for a in sys.argv[2:]],
                      epochs=int(os.environ.get('DEEPCTR_EPOCHS', 1)), log_file=os.path.join(log_dir, tag))
        sys.exit(0)
    if algo == 'many-batch':
        _drv.run_many_batches(os.path.join(data_dir, 'ipinyou-data/%s/train.yzx.txt.shuf' % cam),
                              os.path.join(data_dir, 'ipinyou-data/%s/test.yzx.txt.shuf' % cam),
                              [_drv.parse_spec(a) for a in sys.argv[3:]], batch_size=int(sys.argv[2]),
                              epochs=int(os.environ.get('DEEPCTR_EPOCHS', 1)), log_file=os.path.join(log_dir, tag))
        sys.exit(0)
    _drv.run(os.path.join(data_dir, 'ipinyou-data/%s/train.yzx.txt.shuf' % cam),
             os.path.join(data_dir, 'ipinyou-data/%s/test.yzx.txt.shuf' % cam), algo,
             batch_size=int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] != 'online' else 4096,
             buffer=100000 if 'LR' in algo else 10000, epochs=int(os.environ.get('DEEPCTR_EPOCHS', 1)),
             log_file=os.path.join(log_dir, tag), online=len(sys.argv) > 2 and sys.argv[2] == 'online')
