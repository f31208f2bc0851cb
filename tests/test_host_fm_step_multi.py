"""fm_train_step_multi of include/fm_hip.h on the host side: declared with its limit, bound in _capi, covered by the linker's
export list, exported by the built library, refused without handles before any device call; FM.train_step_many and
ipinyou.run_many_batches take it, and ipinyou.run / run_many keep their signatures."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import FM as fm_module
from deep_ctr_amd import _capi, ipinyou

NAME = "fm_train_step_multi"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fm_hip.h")).read())
    assert "#define FM_STEP_MAX_MODELS 1024" in hdr
    assert ("int fm_train_step_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, "
            "int B, const float* lr, const float* lambda, const int* reduce_mean, float* const* p_out, float* loss_out);") in hdr
    res, args = _capi.FM_SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 11
    assert args[1] is C.c_int and args[5] is C.c_int
    assert args[6] is C.POINTER(C.c_float) and args[7] is C.POINTER(C.c_float)
    assert args[8] is C.POINTER(C.c_int) and args[10] is C.POINTER(C.c_float)
    assert all(args[i] is C.c_void_p for i in (0, 2, 3, 4, 9))


def test_export_list_covers_it():
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(NAME, p) for p in pats), pats


def test_library_exports_it_and_refuses_no_models(built):
    lib = _capi.load()
    assert getattr(lib, NAME).argtypes == _capi.FM_SIGNATURES[NAME][1]
    loss = (C.c_float * 2)(3.0, 4.0)
    lr, lam = (C.c_float * 2)(0.05, 0.05), (C.c_float * 2)(0.0, 0.0)
    hs = (C.c_void_p * 2)(None, None)

    def refused(*a):
        assert lib.fm_create(0, 0, 0, 0, None, C.byref(C.c_void_p())) == _capi.FNN_ERR_ARG      # some other message first
        assert lib.fm_train_step_multi(*a) == _capi.FNN_ERR_ARG
        assert list(loss) == [3.0, 4.0]                                        # nothing written
        assert b'fm_train_step_multi' in lib.fm_last_error(None)
        return lib.fm_last_error(None)

    assert b'null hs' in refused(None, 2, None, None, None, 64, lr, lam, None, None, loss)
    assert b'n_models' in refused(hs, 0, None, None, None, 64, lr, lam, None, None, loss)
    assert b'n_models' in refused(hs, 1025, None, None, None, 64, lr, lam, None, None, loss)
    # handles given, but none of them usable: still refused without touching anything
    assert b'model 0: null handle' in refused(hs, 2, None, None, None, 64, lr, lam, None, None, loss)
    assert b'null hs, lr or lambda' in refused(hs, 2, None, None, None, 64, None, lam, None, None, loss)


def test_each_refusal_keeps_its_text_and_a_second_try_is_refused_alike(built):
    """Every refusal that needs no device, twice in a row: the same code and the same whole message, nothing half-made between."""
    lib = _capi.load()
    lr, lam = (C.c_float * 2)(0.05, 0.05), (C.c_float * 2)(0.0, 0.0)
    hs = (C.c_void_p * 2)(None, None)
    cases = [((None, 2, None, None, None, 64, lr, lam, None, None, None), b'fm_train_step_multi: null hs, lr or lambda'),
             ((hs, 2, None, None, None, 64, None, lam, None, None, None), b'fm_train_step_multi: null hs, lr or lambda'),
             ((hs, 2, None, None, None, 64, lr, None, None, None, None), b'fm_train_step_multi: null hs, lr or lambda'),
             ((hs, 0, None, None, None, 64, lr, lam, None, None, None), b'fm_train_step_multi: n_models must be in [1, 1024]'),
             ((hs, 1025, None, None, None, 64, lr, lam, None, None, None), b'fm_train_step_multi: n_models must be in [1, 1024]'),
             ((hs, 2, None, None, None, 64, lr, lam, None, None, None), b'fm_train_step_multi: model 0: null handle')]
    for args, text in cases:
        for _ in range(2):
            assert lib.fm_create(0, 0, 0, 0, None, C.byref(C.c_void_p())) == _capi.FNN_ERR_ARG      # some other message first
            assert lib.fm_train_step_multi(*args) == _capi.FNN_ERR_ARG
            assert lib.fm_last_error(None) == text


def test_python_signatures():
    p = inspect.signature(fm_module.train_step_many).parameters
    assert list(p) == ['models', 'ids', 'y', 'wts', 'want_p', 'want_loss']
    assert p['wts'].default is None and p['want_p'].default is False and p['want_loss'].default is True
    p = inspect.signature(ipinyou.run_many_batches).parameters
    assert list(p) == ['train_path', 'test_path', 'specs', 'batch_size', 'buffer', 'eval_size', 'epochs', 'log_file', 'device', 'echo']
    assert (p['batch_size'].default, p['buffer'].default, p['eval_size'].default, p['epochs'].default) == (4096, 10000, 100000, 1)
    assert p['log_file'].default is None and p['device'].default == 0 and p['echo'].default is True


def test_run_and_run_many_keep_their_signatures():
    p = inspect.signature(ipinyou.run).parameters
    assert list(p) == ['train_path', 'test_path', 'algo', 'batch_size', 'buffer', 'eval_size', 'epochs', 'log_file', 'device',
                       'echo', 'online']
    assert p['online'].default is False and p['batch_size'].default == 4096 and p['buffer'].default == 10000
    p = inspect.signature(ipinyou.run_many).parameters
    assert list(p) == ['train_path', 'test_path', 'specs', 'buffer', 'eval_size', 'epochs', 'log_file', 'device', 'echo']
    assert ipinyou.parse_spec('FM:10:1e-3:1e-2') == ('FM', 10, 1e-3, 1e-2)
