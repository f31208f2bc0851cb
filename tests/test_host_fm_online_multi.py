"""fm_train_online_multi of include/fm_hip.h on the host side: declared with its limit, bound in _capi, covered by the linker's
export list, exported by the built library, refused without handles; FM.train_online_many and ipinyou.run_many take it, and
ipinyou.run keeps its signature."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import FM as fm_module
from deep_ctr_amd import _capi, ipinyou

NAME = "fm_train_online_multi"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fm_hip.h")).read())
    assert "#define FM_ONLINE_MAX_MODELS 1024" in hdr
    assert ("int fm_train_online_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, "
            "int64_t N, const float* lr, const float* lambda, float* const* p_out, double* loss_sum_out, "
            "float* loss_last_out);") in hdr
    res, args = _capi.FM_SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 11
    assert args[1] is C.c_int and args[5] is C.c_int64
    assert args[6] is C.POINTER(C.c_float) and args[7] is C.POINTER(C.c_float)
    assert args[9] is C.POINTER(C.c_double) and args[10] is C.POINTER(C.c_float)


def test_export_list_covers_it():
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(NAME, p) for p in pats), pats


def test_library_exports_it_and_refuses_no_models(built):
    lib = _capi.load()
    assert getattr(lib, NAME).argtypes == _capi.FM_SIGNATURES[NAME][1]
    loss, last = (C.c_double * 2)(1.0, 2.0), (C.c_float * 2)(3.0, 4.0)
    assert lib.fm_train_online_multi(None, 0, None, None, None, 0, None, None, None, loss, last) == _capi.FNN_ERR_ARG
    assert (list(loss), list(last)) == ([1.0, 2.0], [3.0, 4.0])             # nothing written
    assert b'fm_train_online_multi' in lib.fm_last_error(None)
    # handles given, but none of them usable: still refused without touching anything
    hs, lr, lam = (C.c_void_p * 2)(None, None), (C.c_float * 2)(0.05, 0.05), (C.c_float * 2)(0.0, 0.0)
    assert lib.fm_train_online_multi(hs, 2, None, None, None, 0, lr, lam, None, loss, last) == _capi.FNN_ERR_ARG
    assert lib.fm_train_online_multi(hs, 1025, None, None, None, 0, lr, lam, None, loss, last) == _capi.FNN_ERR_ARG
    assert (list(loss), list(last)) == ([1.0, 2.0], [3.0, 4.0])


def test_each_refusal_keeps_its_text_and_a_second_try_is_refused_alike(built):
    """Every refusal that needs no device, twice in a row: the same code and the same whole message, nothing half-made between."""
    lib = _capi.load()
    lr, lam = (C.c_float * 2)(0.05, 0.05), (C.c_float * 2)(0.0, 0.0)
    hs = (C.c_void_p * 2)(None, None)
    cases = [((None, 2, None, None, None, 5, lr, lam, None, None, None), b'fm_train_online_multi: null hs, lr or lambda'),
             ((hs, 2, None, None, None, 5, None, lam, None, None, None), b'fm_train_online_multi: null hs, lr or lambda'),
             ((hs, 2, None, None, None, 5, lr, None, None, None, None), b'fm_train_online_multi: null hs, lr or lambda'),
             ((hs, 0, None, None, None, 5, lr, lam, None, None, None), b'fm_train_online_multi: n_models must be in [1, 1024]'),
             ((hs, 1025, None, None, None, 5, lr, lam, None, None, None), b'fm_train_online_multi: n_models must be in [1, 1024]'),
             ((hs, 2, None, None, None, 5, lr, lam, None, None, None), b'fm_train_online_multi: model 0: null handle')]
    for args, text in cases:
        for _ in range(2):
            assert lib.fm_create(0, 0, 0, 0, None, C.byref(C.c_void_p())) == _capi.FNN_ERR_ARG      # some other message first
            assert lib.fm_train_online_multi(*args) == _capi.FNN_ERR_ARG
            assert lib.fm_last_error(None) == text


def test_python_signatures():
    p = inspect.signature(fm_module.train_online_many).parameters
    assert list(p) == ['models', 'ids', 'y', 'wts', 'want_p', 'want_loss']
    assert p['wts'].default is None and p['want_p'].default is False and p['want_loss'].default is True
    p = inspect.signature(ipinyou.run_many).parameters
    assert list(p) == ['train_path', 'test_path', 'specs', 'buffer', 'eval_size', 'epochs', 'log_file', 'device', 'echo']
    assert (p['buffer'].default, p['eval_size'].default, p['epochs'].default) == (10000, 100000, 1)
    assert p['log_file'].default is None and p['device'].default == 0 and p['echo'].default is True
    assert ipinyou.parse_spec('FM:10:1e-3:1e-2') == ('FM', 10, 1e-3, 1e-2)


def test_run_keeps_its_signature():
    p = inspect.signature(ipinyou.run).parameters
    assert list(p) == ['train_path', 'test_path', 'algo', 'batch_size', 'buffer', 'eval_size', 'epochs', 'log_file', 'device',
                       'echo', 'online']
    assert p['online'].default is False and p['batch_size'].default == 4096 and p['buffer'].default == 10000
