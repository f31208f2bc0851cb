"""Logistic regression on MI355X: the reference's TensorFlow class `LR` (python/LR.py) with its constructor
signature, `dump` keys (`W`, `b`) and graph outputs (`train_step` = ptmzr + loss + train_preds, `forward` =
test_preds, `evaluate` = eval_preds + metrics).  It runs on the factorisation machine of include/fm_hip.h at
rank 0 (rows [w]): yhat = b + sum_i w_i and the loss xent + lambda * (l2_loss(W) + l2_loss(b)) are exactly
python/LR.py:38-44 and :57-59.  SGD, Adam and FTRL as python/tf_util.py:15-29 builds them.  Value weights (the class's
`sp_wt_hldr`, python/LR.py:23-27 and :53-55: yhat = b + sum_i x_i w_i) are FM's `wts=`: `model.train_step(_cols, _labels,
wts=_vals)` is python/baseline.py:345's feed, and the (ids, wts) pair of ipnn.criteo_feed feeds it unchanged."""
import pickle

import numpy as np

from .FM import FM


class LR(FM):
    def __init__(self, batch_size, _rch_argv, _init_argv, _ptmzr_argv, _reg_argv, mode='train', eval_size=0, device=0,
                 shared_rows=False):
        """_rch_argv = [X_dim, X_feas]: X_feas fields (1..64, one id per field); shared_rows: FM's (columns are positions)."""
        X_dim, X_feas = _rch_argv                                    # python/LR.py:7
        # init_var_map (python/LR.py:15-16): W 'random' from the pickle or _init_argv's distribution, b 'zero'
        FM.__init__(self, batch_size, [X_dim, X_feas, 0], _init_argv, _ptmzr_argv, _reg_argv, mode, eval_size, device, shared_rows)
        self.log = 'input dim: %d, features: %d, ' % (X_dim, X_feas)

    def dump(self, model_path):                                      # python/LR.py:61-64
        rows, b = self.get_params()
        pickle.dump({'W': rows, 'b': np.array([b], np.float32)}, open(model_path, 'wb'))
        print('model dumped at %s' % model_path)
