"""`python FNN.py [advertiser] [flag]` -- the FNN training script on MI355X.

Script behaviour (CLI, hyper-parameters, log lines, epoch loop, early stop, prediction pickles)
follows the reference's Theano script python/FNN_wnzh.py (the upstream `FNN.py`).
The Theano graph and the two Python loops around it are replaced by FNNEngine (libfnn_hip.so):
gather, MLP forward/backward, dense SGD and the sparse-row SGD all run as HIP kernels.

Differences a user can see: the data directory can be overridden with DEEPCTR_DATA_DIR (default
`../data`, as python/FNN_wnzh.py:28-30), DEEPCTR_EPOCHS caps the epoch count, DEEPCTR_PRECISION
selects f32 (default; parity mode) or bf16, and logloss is logged beside AUC and RMSE.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deep_ctr_amd  # noqa: E402,F401
from deep_ctr_amd import dl_utils as ut  # noqa: E402
from deep_ctr_amd.data_fm import DataFM  # noqa: E402
from deep_ctr_amd.engine import FNNEngine  # noqa: E402
from deep_ctr_amd.ipnn import FNN  # noqa: E402,F401  (the TensorFlow-style class of the same name, python/FNN.py:4)


def run(argv, out=None):
    """The module-level code of python/FNN_wnzh.py:15-348 as a function; returns the history."""
    srng = ut.RandomStreams(seed=234)                          # :15
    ut.seed_global(1234)                                       # :16-17 (and dl_utils.py:9-10)
    batch_size = 100                                           # :18-24
    lr = 0.002
    lambda1 = 0.1
    hidden1 = 300
    hidden2 = 100
    acti_type = 'tanh'
    epoch = int(os.environ.get('DEEPCTR_EPOCHS', 100))
    advertiser = '2997'
    if len(argv) > 1:
        advertiser = argv[1]
    data_dir = os.environ.get('DEEPCTR_DATA_DIR', '../data')
    train_file = os.path.join(data_dir, 'train.fm.txt')        # :28-30
    test_file = os.path.join(data_dir, 'test.fm.txt')
    fm_model_file = os.path.join(data_dir, 'fm.model.txt')
    if len(argv) > 2 and advertiser == 'all':                  # :32-35
        train_file = train_file + '.5.txt'
    elif len(argv) > 2:
        train_file = train_file + '.10.txt'
    print(train_file)

    train_size = ut.file_len(train_file)                       # :38-40
    n_batch = train_size // batch_size
    x_drop = 1
    if advertiser == '2997':                                   # :43-49
        lr = 0.001
        x_drop = dropout = 0.5
        hidden1 = 300
        hidden2 = 100
        lambda1 = 0.0
        lambda_fm = 0.1
    # any other advertiser: `dropout` / `lambda_fm` are undefined in the reference and the next
    # statement raises NameError there; same here.

    def log_p(msg, m=""):
        ut.logfile(msg, "fm" + str(advertiser))

    log_p('ad:' + str(advertiser))
    log_p('batch_size:' + str(batch_size))

    data = DataFM(fm_model_file)                               # :62-84
    k, xdim = data.k, data.xdim
    log_p('drop_mlp3fm.py|ad:' + advertiser + '|drop:' + str(dropout) + '|b_size:' + str(batch_size) +
          ' | X:' + str(xdim) + ' | Hidden 1:' + str(hidden1) + ' | Hidden 2:' + str(hidden2) +
          ' | L_r:' + str(lr) + ' | activation1:' + str(acti_type) + ' | lambda:' + str(lambda1))

    weights = ut.init_fnn_weights(xdim, hidden1, hidden2, acti_type)   # :106-130,140

    # dropout rows, in the graph's creation order (:144,154,166); r0 is dead but takes a seed
    r0 = srng.binomial(size=(1, xdim), n=1, p=x_drop)          # noqa: F841
    r1 = srng.binomial(size=(1, hidden1), n=1, p=dropout)
    r2 = srng.binomial(size=(1, hidden2), n=1, p=dropout)

    precision = os.environ.get('DEEPCTR_PRECISION', 'f32')
    eng = FNNEngine(n_fields=len(data.name_field), k=k, hidden1=hidden1, hidden2=hidden2,
                    max_batch=max(batch_size, 4096), precision=precision, acti_type=acti_type,
                    lr=lr, lambda1=lambda1, lambda_fm=lambda_fm)
    rows, field_of_row, w_0 = data.table()
    eng.set_table(rows, field_of_row, w_0)
    eng.set_dense(weights)
    data.engine = eng

    train_ids, train_y, train_sh = data.load_ids(train_file, want_shadowed=True)   # parsed once, not per epoch
    test_ids, test_y = data.load_ids(test_file)

    train_ids_d, train_y_d = eng.to_device(train_ids, train_y)   # resident in HBM for every epoch's passes
    test_ids_d, test_y_d = eng.to_device(test_ids, test_y)
    train_yf_d = train_y_d.float()

    def get_err_bat(ids, y):                                   # :193-221, metrics on the device (fnn_eval)
        m = eng.evaluate(ids, y)
        return m['auc'], m['rmse'], m['logloss']

    def fmt_time(t):
        return str(int(t / 60)) + 'm ' + str(int(t % 60)) + 's'

    print("Training model:")
    best = eng.get_dense()                                     # :278-284
    min_err = 0
    min_err_epoch = 0
    times_reduce = 0
    hist = []
    for i in range(epoch):                                     # :290
        start_time = time.time()
        pre_step = best
        # :293-306.  The epoch's dropout rows are drawn ahead (the same stream: _BinomialOp.draw_rows) and the steps run
        # through FNNEngine.train_epoch -- resident ids, raw C calls, the next batch announced to every step; `train` returns
        # PRE-update tensors (:298), so the dense state is read before the last batch
        n_run = n_batch if (n_batch - 1) * batch_size + 1 <= train_size else (train_size + batch_size - 1) // batch_size
        m1, m2 = r1.draw_rows(n_run), r2.draw_rows(n_run)
        if n_run > 1:
            eng.train_epoch(train_ids_d, train_yf_d, batch_size, m1, m2, 0, n_run - 1, train_sh)
        if n_run > 0:
            if n_run == n_batch:
                pre_step = eng.get_dense()
            eng.train_epoch(train_ids_d, train_yf_d, batch_size, m1, m2, n_run - 1, 1, train_sh)
        eng.sync()
        print('training: ' + fmt_time(time.time() - start_time))

        start_time = time.time()
        auc, rmse, ll = get_err_bat(train_ids_d, train_y_d)
        log_p('\t\tTraining Err: \t' + str(i) + '\t' + str(auc) + '\t' + str(rmse))
        print('training error: ' + fmt_time(time.time() - start_time))

        start_time = time.time()
        auc, rmse, ll = get_err_bat(test_ids_d, test_y_d)
        log_p('Test Err:' + str(i) + '\t' + str(auc) + '\t' + str(rmse))
        log_p('Test logloss:' + str(i) + '\t' + str(ll))
        print('test error: ' + fmt_time(time.time() - start_time))
        hist.append({'epoch': i, 'test_auc': auc, 'test_rmse': rmse, 'test_logloss': ll})

        if auc > min_err:                                      # :329-343
            best = pre_step
            min_err = auc
            min_err_epoch = i
            if times_reduce < 3:
                times_reduce += 1
        else:
            times_reduce -= 1
        if times_reduce < 0:
            break
    log_p('Minimal test error is ' + str(min_err) + ' , at EPOCH ' + str(min_err_epoch))

    eng.set_dense(best)                                        # get_pred, :257-276,345-348
    ut.save_weights("mlp3fm_train_" + advertiser + ".p", eng.predict(train_ids).cpu().numpy())
    ut.save_weights("mlp3fm_test_" + advertiser + ".p", eng.predict(test_ids).cpu().numpy())
    return hist


def parse_spec(s):
    """'LR:DROPOUT:LAMBDA1:LAMBDA_FM' -> (lr, dropout, lambda1, lambda_fm); a tuple of the four passes through."""
    if isinstance(s, str):
        s = s.split(':')
    lr, dropout, lambda1, lambda_fm = (float(v) for v in s)
    return lr, dropout, lambda1, lambda_fm


def run_many(argv, specs, out=None):
    """run()'s schedule for every (lr, dropout, lambda1, lambda_fm) of `specs` in ONE pass over the data: the files are loaded
    once and the ids are resident once; every model has its own engine, its initial weights from the same seeded draws as run()'s,
    its own RandomStreams(234) dropout stream, early-stop bookkeeping and best-weights snapshot.  The models still training
    step together (engine.train_epoch_many: one fnn_train_step_multi per batch) and are evaluated together
    (engine.evaluate_many: one fnn_eval_multi per feed and epoch); a model that stops leaves the group.
    Returns the list of histories; the prediction pickles are mlp3fm_{train,test}_<advertiser>_m<i>.p.  `out` (a dict)
    receives the engines under 'engines', each loaded with its model's best weights."""
    from deep_ctr_amd.engine import FNNError, evaluate_many, predict_many, train_epoch_many

    def _raise_status(r):
        if 'status' in r:
            raise FNNError(r['status'], r['error'])
        return r
    specs = [parse_spec(s) for s in specs]
    assert len(specs) >= 1
    batch_size = 100
    hidden1, hidden2 = 300, 100
    acti_type = 'tanh'
    epoch = int(os.environ.get('DEEPCTR_EPOCHS', 100))
    advertiser = argv[1] if len(argv) > 1 else '2997'
    data_dir = os.environ.get('DEEPCTR_DATA_DIR', '../data')
    train_file = os.path.join(data_dir, 'train.fm.txt')
    test_file = os.path.join(data_dir, 'test.fm.txt')
    fm_model_file = os.path.join(data_dir, 'fm.model.txt')
    if len(argv) > 2 and advertiser == 'all':
        train_file = train_file + '.5.txt'
    elif len(argv) > 2:
        train_file = train_file + '.10.txt'
    print(train_file)
    train_size = ut.file_len(train_file)
    n_batch = train_size // batch_size

    def log_p(m, msg):
        ut.logfile(msg, "fm" + str(advertiser) + "_m" + str(m))

    data = DataFM(fm_model_file)
    k, xdim = data.k, data.xdim
    rows, field_of_row, w_0 = data.table()
    precision = os.environ.get('DEEPCTR_PRECISION', 'f32')

    class Model(object):
        pass

    models = []
    for m, (lr, dropout, lambda1, lambda_fm) in enumerate(specs):
        mo = Model()
        log_p(m, 'ad:' + str(advertiser))
        log_p(m, 'batch_size:' + str(batch_size))
        log_p(m, 'drop_mlp3fm.py|ad:' + advertiser + '|drop:' + str(dropout) + '|b_size:' + str(batch_size) +
              ' | X:' + str(xdim) + ' | Hidden 1:' + str(hidden1) + ' | Hidden 2:' + str(hidden2) +
              ' | L_r:' + str(lr) + ' | activation1:' + str(acti_type) + ' | lambda:' + str(lambda1))
        srng = ut.RandomStreams(seed=234)
        ut.seed_global(1234)
        weights = ut.init_fnn_weights(xdim, hidden1, hidden2, acti_type)
        srng.binomial(size=(1, xdim), n=1, p=dropout)              # r0: dead, but takes a seed
        mo.r1 = srng.binomial(size=(1, hidden1), n=1, p=dropout)
        mo.r2 = srng.binomial(size=(1, hidden2), n=1, p=dropout)
        mo.eng = FNNEngine(n_fields=len(data.name_field), k=k, hidden1=hidden1, hidden2=hidden2,
                           max_batch=max(batch_size, 4096), precision=precision, acti_type=acti_type,
                           lr=lr, lambda1=lambda1, lambda_fm=lambda_fm)
        mo.eng.set_table(rows, field_of_row, w_0)
        mo.eng.set_dense(weights)
        mo.best = mo.eng.get_dense()
        mo.min_err, mo.min_err_epoch, mo.times_reduce, mo.hist, mo.live = 0, 0, 0, [], True
        models.append(mo)
    eng0 = models[0].eng
    data.engine = eng0

    train_ids, train_y, train_sh = data.load_ids(train_file, want_shadowed=True)
    test_ids, test_y = data.load_ids(test_file)
    train_ids_d, train_y_d = eng0.to_device(train_ids, train_y)
    test_ids_d, test_y_d = eng0.to_device(test_ids, test_y)
    train_yf_d = train_y_d.float()

    print("Training models:")
    n_run = n_batch if (n_batch - 1) * batch_size + 1 <= train_size else (train_size + batch_size - 1) // batch_size
    for i in range(epoch):
        live = [m for m, mo in enumerate(models) if mo.live]
        if not live:
            break
        start_time = time.time()
        engs = [models[m].eng for m in live]
        m1 = [models[m].r1.draw_rows(n_run) for m in live]
        m2 = [models[m].r2.draw_rows(n_run) for m in live]
        pre = [models[m].best for m in live]
        if n_run > 1:
            train_epoch_many(engs, train_ids_d, train_yf_d, batch_size, m1, m2, 0, n_run - 1, train_sh)
        if n_run > 0:
            if n_run == n_batch:
                pre = [e.get_dense() for e in engs]
            train_epoch_many(engs, train_ids_d, train_yf_d, batch_size, m1, m2, n_run - 1, 1, train_sh)
        for e in engs:
            e.sync()
        print('training: %d models, %.1fs' % (len(live), time.time() - start_time))
        # both passes of every live model in one call each (fnn_eval_multi); a model whose own evaluate would have raised
        # raises here, where its turn comes
        trs = evaluate_many(engs, train_ids_d, train_y_d)
        tes = evaluate_many(engs, test_ids_d, test_y_d)
        for j, m in enumerate(live):
            mo = models[m]
            tr = _raise_status(trs[j])
            log_p(m, '\t\tTraining Err: \t' + str(i) + '\t' + str(tr['auc']) + '\t' + str(tr['rmse']))
            te = _raise_status(tes[j])
            auc, rmse, ll = te['auc'], te['rmse'], te['logloss']
            log_p(m, 'Test Err:' + str(i) + '\t' + str(auc) + '\t' + str(rmse))
            log_p(m, 'Test logloss:' + str(i) + '\t' + str(ll))
            mo.hist.append({'epoch': i, 'test_auc': auc, 'test_rmse': rmse, 'test_logloss': ll})
            if auc > mo.min_err:
                mo.best = pre[j]
                mo.min_err = auc
                mo.min_err_epoch = i
                if mo.times_reduce < 3:
                    mo.times_reduce += 1
            else:
                mo.times_reduce -= 1
            if mo.times_reduce < 0:
                mo.live = False
    for m, mo in enumerate(models):
        log_p(m, 'Minimal test error is ' + str(mo.min_err) + ' , at EPOCH ' + str(mo.min_err_epoch))
        mo.eng.set_dense(mo.best)
    engs = [mo.eng for mo in models]
    p_train, p_test = predict_many(engs, train_ids_d), predict_many(engs, test_ids_d)     # fnn_predict_multi
    for m in range(len(models)):
        ut.save_weights("mlp3fm_train_" + advertiser + "_m" + str(m) + ".p", p_train[m].cpu().numpy())
        ut.save_weights("mlp3fm_test_" + advertiser + "_m" + str(m) + ".p", p_test[m].cpu().numpy())
    if out is not None:
        out['engines'] = [mo.eng for mo in models]
    return [mo.hist for mo in models]


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'many':           # python FNN.py many <advertiser> LR:DROPOUT:LAMBDA1:LAMBDA_FM ...
        run_many([sys.argv[0]] + sys.argv[2:3], sys.argv[3:])
    else:
        run(sys.argv)
