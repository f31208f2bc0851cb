"""fnn_bag_train_step_multi of include/fnn_hip.h on the host side: declared, bound in _capi, covered by the linker's export
list, exported by the built library, refused without handles before any device call; SNN_RBM.run_many / parse_spec and
SNN_DAE.run_many take it, and SNN_RBM.run / SNN_DAE.run keep their signatures."""
import ctypes as C
import fnmatch
import importlib.util
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

NAME = "fnn_bag_train_step_multi"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fnn_hip.h")).read())
    assert ("int fnn_bag_train_step_multi(fnn_handle* const* hs, int n_models, const int32_t* ids, const float* y, int B, "
            "const uint8_t* const* mask1, const uint8_t* const* mask2, int b_size, const int32_t* next_ids, int next_B, "
            "float* const* p_out, float* loss_sum_out);") in hdr
    res, args = _capi.SIGNATURES[NAME]
    assert (res, args) == _capi.SIGNATURES["fnn_train_step_multi"]
    assert res is C.c_int and len(args) == 12
    assert all(args[i] is C.c_int for i in (1, 4, 7, 9))
    assert all(args[i] is C.c_void_p for i in (0, 2, 3, 5, 6, 8, 10))
    assert args[11] is C.POINTER(C.c_float)


def test_each_refusal_keeps_its_text_and_a_second_try_is_refused_alike(built):
    """The linker's export list covers the entry point and the built library exports it with the bound prototype; every refusal
    that needs no device, twice in a row: the same code and the same whole message, and the losses untouched."""
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(NAME, p) for p in pats), pats
    lib = _capi.load()
    assert getattr(lib, NAME).argtypes == _capi.SIGNATURES[NAME][1]
    loss = (C.c_float * 2)(3.0, 4.0)
    hs = (C.c_void_p * 2)(None, None)
    cases = [((None, 2, None, None, 64, None, None, 0, None, 0, None, loss), b'fnn_bag_train_step_multi: null hs'),
             ((hs, 0, None, None, 64, None, None, 0, None, 0, None, loss), b'fnn_bag_train_step_multi: n_models must be in [1, 256]'),
             ((hs, 257, None, None, 64, None, None, 0, None, 0, None, loss), b'fnn_bag_train_step_multi: n_models must be in [1, 256]'),
             ((hs, 2, None, None, 64, None, None, 0, None, 0, None, loss), b'fnn_bag_train_step_multi: model 0: null handle')]
    for args, text in cases:
        for _ in range(2):
            assert lib.fnn_create(None, None) == _capi.FNN_ERR_ARG      # some other message first
            assert lib.fnn_last_error(None) == b'null argument'
            assert lib.fnn_bag_train_step_multi(*args) == _capi.FNN_ERR_ARG
            assert lib.fnn_last_error(None) == text
            assert list(loss) == [3.0, 4.0]                            # nothing written


def _script(name):
    spec = importlib.util.spec_from_file_location(name.lower() + '_script_sig', os.path.join(ROOT, 'deep-ctr_amd', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_many_and_run_signatures():
    mod = _script('SNN_RBM')
    p = inspect.signature(mod.run_many).parameters
    assert list(p) == ['argv', 'specs', 'kind', 'pretrain_kw', 'out']
    assert (p['kind'].default, p['pretrain_kw'].default, p['out'].default) == ('rbm', None, None)
    assert mod.parse_spec('1e-3:0.98:0') == (1e-3, 0.98, 0.0)
    assert mod.parse_spec((5e-4, 0.99, 1e-4)) == (5e-4, 0.99, 1e-4)
    p = inspect.signature(mod.run).parameters                           # unchanged
    assert list(p) == ['argv', 'kind', 'pretrain_kw'] and (p['kind'].default, p['pretrain_kw'].default) == ('rbm', None)
    dae = _script('SNN_DAE')
    assert list(inspect.signature(dae.run).parameters) == ['argv']      # unchanged
    p = inspect.signature(dae.run_many).parameters
    assert list(p) == ['argv', 'specs', 'out'] and p['out'].default is None
