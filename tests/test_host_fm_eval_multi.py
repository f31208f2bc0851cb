"""fm_predict_multi / fm_eval_multi of include/fm_hip.h on the host side: declared with their limit, bound in _capi with the
right arity, covered by the linker's export list, exported by the built library, and refused without handles before any device
is touched; FM.predict_many / FM.evaluate_many exist with their signatures and ipinyou.run_many keeps its own."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import FM as fm_module
from deep_ctr_amd import _capi, ipinyou

NAMES = ("fm_predict_multi", "fm_eval_multi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fm_hip.h")).read())
    assert "#define FM_EVAL_MAX_MODELS 1024" in hdr
    assert ("int fm_predict_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, int64_t N, "
            "float* const* p_out);") in hdr
    assert ("int fm_eval_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const int32_t* y, "
            "int64_t N, double* auc, double* rmse, double* logloss, int* status);") in hdr
    res, args = _capi.FM_SIGNATURES["fm_predict_multi"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_int and args[4] is C.c_int64
    res, args = _capi.FM_SIGNATURES["fm_eval_multi"]
    assert res is C.c_int and len(args) == 10 and args[1] is C.c_int and args[5] is C.c_int64
    assert args[6] is C.POINTER(C.c_double) and args[7] is C.POINTER(C.c_double) and args[8] is C.POINTER(C.c_double)
    assert args[9] is C.POINTER(C.c_int)


@pytest.mark.parametrize("name", NAMES)
def test_export_list_covers_them(name):
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats


def test_library_exports_them_and_refuses_no_models(built):
    lib = _capi.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _capi.FM_SIGNATURES[name][1]
    two = (C.c_void_p * 2)(None, None)
    for hs, n in ((None, 1), (two, 0), (two, 1025), (two, 2)):            # null hs; no models; too many; null entries
        auc, rmse, ll = (C.c_double * 2)(1.0, 2.0), (C.c_double * 2)(3.0, 4.0), (C.c_double * 2)(5.0, 6.0)
        status = (C.c_int * 2)(7, 8)
        assert lib.fm_eval_multi(hs, n, None, None, None, 5, auc, rmse, ll, status) == _capi.FNN_ERR_ARG
        assert (list(auc), list(rmse), list(ll), list(status)) == ([1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7, 8])     # nothing written
        assert b'fm_eval_multi' in lib.fm_last_error(None)
        assert lib.fm_predict_multi(hs, n, None, None, 5, None) == _capi.FNN_ERR_ARG
        assert b'fm_predict_multi' in lib.fm_last_error(None)


def test_each_refusal_keeps_its_text_and_a_second_try_is_refused_alike(built):
    """Every refusal that needs no device, twice in a row: the same code and the same whole message, nothing half-made between."""
    lib = _capi.load()
    two = (C.c_void_p * 2)(None, None)
    cases = [(None, 1, b'null hs'), (two, 0, b'n_models must be in [1, 1024]'), (two, 1025, b'n_models must be in [1, 1024]'),
             (two, 2, b'model 0: null handle')]
    for hs, n, text in cases:
        for _ in range(2):
            assert lib.fm_create(0, 0, 0, 0, None, C.byref(C.c_void_p())) == _capi.FNN_ERR_ARG      # some other message first
            assert lib.fm_eval_multi(hs, n, None, None, None, 5, None, None, None, None) == _capi.FNN_ERR_ARG
            assert lib.fm_last_error(None) == b'fm_eval_multi: ' + text
            assert lib.fm_predict_multi(hs, n, None, None, 5, None) == _capi.FNN_ERR_ARG
            assert lib.fm_last_error(None) == b'fm_predict_multi: ' + text


def test_python_signatures():
    p = inspect.signature(fm_module.predict_many).parameters
    assert list(p) == ['models', 'ids', 'wts'] and p['wts'].default is None
    p = inspect.signature(fm_module.evaluate_many).parameters
    assert list(p) == ['models', 'ids', 'y', 'wts'] and p['wts'].default is None
    p = inspect.signature(ipinyou.run_many).parameters
    assert list(p) == ['train_path', 'test_path', 'specs', 'buffer', 'eval_size', 'epochs', 'log_file', 'device', 'echo']


def test_empty_and_mismatched_lists_are_value_errors():
    class Stub(object):
        def __init__(self, feas):
            self.X_feas = feas
    for fn, args in ((fm_module.predict_many, ([[0]],)), (fm_module.evaluate_many, ([[0]], [0]))):
        with pytest.raises(ValueError):
            fn([], *args)
        with pytest.raises(ValueError):
            fn([Stub(16), Stub(15)], *args)
