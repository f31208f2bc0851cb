"""The value-weight entry points of include/fm_hip.h on the host side: declared with `wts` behind `ids`, bound in _capi with one
pointer more than the call they extend, exported by the built library, and taken by FM / LR as `wts=`."""
import ctypes as C
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

NEW = ("fm_train_step_w", "fm_predict_w", "fm_eval_w")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(fm_handle\* h, const int32_t\* ids, const float\* wts," % name, hdr), name
        res, args = _capi.FM_SIGNATURES[name]
        assert res is C.c_int
        # one pointer (wts, behind ids) more than the entry point it extends
        base_args = _capi.FM_SIGNATURES[name[:-2]][1]
        assert len(args) == len(base_args) + 1 and args[:2] == base_args[:2] and args[2] is C.c_void_p and args[3:] == base_args[2:]
    assert "One feature per field with value 1" not in hdr


def test_library_exports_them(built):
    lib = _capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _capi.FM_SIGNATURES[name][1], name


def test_python_signatures():
    for cls in (FM, LR):
        assert list(inspect.signature(cls.train_step).parameters) == ['self', 'ids', 'y', 'want_p', 'want_loss', 'wts']
        assert list(inspect.signature(cls.forward).parameters) == ['self', 'ids', 'wts']
        assert list(inspect.signature(cls.evaluate).parameters) == ['self', 'ids', 'y', 'wts']
        for fn in (cls.train_step, cls.forward, cls.evaluate):
            assert inspect.signature(fn).parameters['wts'].default is None
    assert 'baseline.py:345' in FM.train_step.__doc__ and 'criteo_feed' in FM.train_step.__doc__
