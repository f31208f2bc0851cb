"""The shared-row entry points of include/fm_hip.h on the host side: declared, bound in _capi, exported by the built library,
taken by FM / LR as `shared_rows=` / set_shared_rows / count_shared_rows, and (on a device) refused in the states the header
names."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

NEW = ("fm_set_shared_rows", "fm_count_shared_rows")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_row_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    assert re.search(r"\bint fm_set_shared_rows\(fm_handle\* h, int on\);", hdr)
    assert re.search(r"\bint fm_count_shared_rows\(fm_handle\* h, int64_t\* n_out\);", hdr)
    assert _capi.FM_SIGNATURES["fm_set_shared_rows"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = _capi.FM_SIGNATURES["fm_count_shared_rows"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int64)
    assert "can be lost (both" not in hdr and "FNN_SCAT1_FORM" in hdr       # the old restriction is a default now


def test_library_exports_them(built):
    lib = _capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _capi.FM_SIGNATURES[name][1], name
    assert lib.fm_set_shared_rows(None, 1) == _capi.FNN_ERR_ARG
    assert lib.fm_count_shared_rows(None, None) == _capi.FNN_ERR_ARG


def test_python_signatures():
    for cls in (FM, LR):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == 'shared_rows' and p['shared_rows'].default is False
        assert list(inspect.signature(cls.set_shared_rows).parameters) == ['self', 'on']
        assert list(inspect.signature(cls.count_shared_rows).parameters) == ['self']
    p = inspect.signature(ipinyou.run).parameters
    assert list(p)[:3] == ['train_path', 'test_path', 'algo'] and p['algo'].default == 'FM'
    assert p['buffer'].default == 10000 and p['eval_size'].default == 100000 and p['epochs'].default == 1
    assert p['batch_size'].default != 1
    assert list(inspect.signature(ipinyou.to_column_ids).parameters) == ['X_ind', 'X_val']


@pytest.mark.gpu
def test_count_is_refused_while_the_mode_is_off_or_no_step_has_run(built):
    from deep_ctr_amd.engine import FNNError
    rows = np.zeros((20, 4), np.float32)
    m = FM(8, [20, 3, 3], ['uniform', -0.001, 0.001, [1, 2], None], ['sgd', 0.05], [0.0], 'train', 0)
    m.set_params(rows, 0.0)
    ids, y = np.array([[0, 1, 0], [2, -1, 1]], np.int32), np.array([1.0, 0.0])
    for state in ('off', 'off after a step', 'on, no step yet'):
        with pytest.raises(FNNError) as e:
            m.count_shared_rows()
        assert e.value.code == _capi.FNN_ERR_STATE, state
        if state == 'off':
            m.train_step(np.array([[0, 5, 10], [2, -1, 11]], np.int32), y)        # no row under two columns
        elif state == 'off after a step':
            m.set_shared_rows(True)
    m.train_step(ids, y)
    assert m.count_shared_rows() == 2                                       # rows 0 and 1
    m.set_params(rows, 0.0)                                                 # a new table: no step yet
    with pytest.raises(FNNError) as e:
        m.count_shared_rows()
    assert e.value.code == _capi.FNN_ERR_STATE
    m.train_step(ids[:, ::-1].copy(), y)
    assert m.count_shared_rows() == 2
    m.set_shared_rows(False)
    with pytest.raises(FNNError):
        m.count_shared_rows()
    m.close()
