"""SNN_RBM.run_many on tests/golden/demo: run()'s schedule for three (lr, dropout, lambda1) in one pass over the data -- the
pre-training once, every epoch's steps through engine.train_epoch_many (fnn_bag_train_step_multi), the scores through
engine.evaluate_many.  The demo feed has rows under several columns of a batch, whose updates are float atomics in the solo
step and in the group call alike: the own-spec model is held to run() at the bounds test_gpu_rbm holds run() to the oracle."""
import importlib.util
import os
import pickle

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import dl_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'deep-ctr_amd', 'SNN_RBM.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_many_tracks_run_on_the_demo_set(built, golden_dir, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('DEEPCTR_DATA_DIR', os.path.join(golden_dir, 'demo'))
    monkeypatch.setenv('DEEPCTR_EPOCHS', '2')
    monkeypatch.setenv('DEEPCTR_XDIM', 'auto')
    monkeypatch.delenv('DEEPCTR_PRECISION', raising=False)
    monkeypatch.setattr(dl_utils, 'log_path', str(tmp_path / 'log'))
    mod = _script('snn_script_many')
    writes = []
    dump = pickle.dump
    monkeypatch.setattr(mod.pickle, 'dump', lambda obj, f, *a, **k: (writes.append(getattr(f, 'name', '?')), dump(obj, f, *a, **k))[1])
    specs = ['1e-3:0.98:0', '5e-3:0.98:0', '1e-3:0.9:1e-4']              # the first: the script's own for advertiser 2997
    out = {}
    hists = mod.run_many(['SNN_RBM.py', '2997'], specs, out=out)
    for e in out['engines']:
        e.close()
    assert [os.path.basename(w) for w in writes] == ['rbm_2997_.p'] and (tmp_path / 'rbm_2997_.p').exists()      # the cache, once
    assert len(hists) == 3 and all(len(h) == 2 for h in hists)
    for h in hists:
        assert [sorted(r) for r in h] == [['epoch', 'test_auc', 'test_logloss', 'test_rmse']] * 2 and [r['epoch'] for r in h] == [0, 1]
    assert hists[1] != hists[0] and hists[2] != hists[0]                 # another lr, another dropout: another history
    ref = mod.run(['SNN_RBM.py', '2997'])                                # reads the cache run_many wrote
    assert len(writes) == 1 and len(ref) == 2
    for got, want in zip(hists[0], ref):
        print("SNN demo, run_many against run: auc %.6f vs %.6f, logloss %.6f vs %.6f"
              % (got['test_auc'], want['test_auc'], got['test_logloss'], want['test_logloss']))
        assert abs(got['test_auc'] - want['test_auc']) <= 2e-3
        assert abs(got['test_logloss'] - want['test_logloss']) <= 2e-4
    logs = os.listdir(str(tmp_path / 'log'))
    for m in range(3):                                                   # every model its own log (dl_utils.log: log-<date><name>.txt)
        mine = [f for f in logs if f.endswith('drop_mlp4da2997_m%d.txt' % m)]
        assert len(mine) == 1 and 'Minimal test error' in open(str(tmp_path / 'log' / mine[0])).read()
