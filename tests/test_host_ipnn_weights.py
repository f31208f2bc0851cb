"""The value-weight entry points of include/ipnn_hip.h on the host side: bound in _capi, exported by the built library, and
ipnn_cfg untouched by them."""
import ctypes as C
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi
from deep_ctr_amd.ipnn import IPNNEngine, _IPFamily

NEW = ("ipnn_train_step_w", "ipnn_predict_w", "ipnn_eval_w")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ipnn_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(ipnn_handle\* h, const int32_t\* ids, const float\* wts," % name, hdr), name
        res, args = _capi.IPNN_SIGNATURES[name]
        assert res is C.c_int
        # one pointer (wts, behind ids) more than the entry point it extends
        base_args = _capi.IPNN_SIGNATURES[name[:-2]][1]
        assert len(args) == len(base_args) + 1 and args[:2] == base_args[:2] and args[3:] == base_args[2:]


def test_library_exports_them_and_cfg_stays_96_bytes(built):
    lib = _capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ipnn_cfg_size() == 96 == C.sizeof(_capi.ipnn_cfg)


def test_python_signatures():
    assert inspect.signature(IPNNEngine.train_step).parameters['wts'].default is None
    assert list(inspect.signature(IPNNEngine.predict).parameters) == ['self', 'ids', 'wts']
    assert list(inspect.signature(IPNNEngine.evaluate).parameters) == ['self', 'ids', 'y', 'wts']
    assert list(inspect.signature(_IPFamily.train_step).parameters) == ['self', 'ids', 'y', 'masks', 'wts']
    assert list(inspect.signature(_IPFamily.forward).parameters) == ['self', 'ids', 'v_wts', 'wts']
