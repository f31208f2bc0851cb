"""ipnn_predict_multi / ipnn_eval_multi of include/ipnn_hip.h on the host side: declared with their limit, bound in _capi,
covered by the linker's export list, exported by the built library, refused without handles before any device call;
ipnn.predict_many and ipnn.evaluate_many take them."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn

NAMES = ("ipnn_predict_multi", "ipnn_eval_multi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)


def test_the_entry_points_are_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ipnn_hip.h")).read())
    assert "#define IPNN_EVAL_MAX_MODELS 1024" in hdr
    assert ("int ipnn_predict_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, "
            "int64_t N, float* const* p_out);") in hdr
    assert ("int ipnn_eval_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, "
            "const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss, "
            "int* status, float* const* p_out);") in hdr
    res, args = _capi.IPNN_SIGNATURES["ipnn_predict_multi"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    res, args = _capi.IPNN_SIGNATURES["ipnn_eval_multi"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_int), C.c_void_p]


def test_each_refusal_keeps_its_text_and_a_second_try_is_refused_alike(built):
    """The linker's export list covers both entry points and the built library exports them with the bound prototypes; every
    refusal that needs no device, twice in a row: the same code and the same whole message, and the outputs untouched."""
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    lib = _capi.load()
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats
        assert getattr(lib, name).argtypes == _capi.IPNN_SIGNATURES[name][1]
    auc, rmse, ll = (C.c_double * 2)(3.0, 4.0), (C.c_double * 2)(5.0, 6.0), (C.c_double * 2)(7.0, 8.0)
    status = (C.c_int * 2)(9, 10)
    hs = (C.c_void_p * 2)(None, None)
    ps = (C.c_void_p * 2)(None, None)

    def ev(hs_, n):
        return lib.ipnn_eval_multi(hs_, n, None, None, None, 64, auc, rmse, ll, status, ps)

    def pr(hs_, n):
        return lib.ipnn_predict_multi(hs_, n, None, None, 64, ps)

    cases = [(None, 2, b'null hs'), (hs, 0, b'n_models must be in [1, 1024]'), (hs, 1025, b'n_models must be in [1, 1024]'),
             (hs, 2, b'model 0: null handle')]
    for name, call in (("ipnn_eval_multi", ev), ("ipnn_predict_multi", pr)):
        for hs_, n, text in cases:
            for _ in range(2):
                assert lib.ipnn_create(None, None) == _capi.FNN_ERR_ARG     # some other message first
                assert lib.ipnn_last_error(None) == b'null argument'
                assert call(hs_, n) == _capi.FNN_ERR_ARG
                assert lib.ipnn_last_error(None) == name.encode() + b': ' + text
                assert (list(auc), list(rmse), list(ll), list(status)) == ([3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9, 10])
                assert list(ps) == [None, None]


def test_python_signatures():
    p = inspect.signature(ipnn.predict_many).parameters
    assert list(p) == ['engines', 'ids', 'wts'] and p['wts'].default is None
    p = inspect.signature(ipnn.evaluate_many).parameters
    assert list(p) == ['engines', 'ids', 'y', 'wts', 'want_p'] and p['wts'].default is None and p['want_p'].default is False
