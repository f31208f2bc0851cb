"""ipnn_train_step_multi of include/ipnn_hip.h on the host side: declared with its limit, bound in _capi with the declared
argument types, covered by the linker's export list, exported by the built library beside nothing undeclared, refused without
handles before any device call; ipnn.train_step_many checks its `masks` before it touches a device."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn
from deep_ctr_amd.ipnn import Drawn

NAME = "ipnn_train_step_multi"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ipnn_hip.h")).read())
    assert "#define IPNN_STEP_MAX_MODELS 256" in hdr
    assert ("int ipnn_train_step_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int B, "
            "const uint8_t* const* const* masks, const uint64_t* seeds, const uint64_t* steps, "
            "float* const* logits_out, float* loss_sum_out);") in hdr
    res, args = _capi.IPNN_SIGNATURES[NAME]
    u64p = C.POINTER(C.c_uint64)
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, u64p, u64p, C.c_void_p, C.POINTER(C.c_float)]


def test_library_exports_it_and_nothing_undeclared(built):
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(NAME, p) for p in pats), pats
    lib = _capi.load()
    assert getattr(lib, NAME).argtypes == _capi.IPNN_SIGNATURES[NAME][1]
    out = subprocess.run(['nm', '-D', '--defined-only', _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    ours = {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith('ipnn_')}
    assert NAME in ours
    assert ours == set(_capi.IPNN_SIGNATURES), ours ^ set(_capi.IPNN_SIGNATURES)


def test_refusals_that_need_no_device(built):
    lib = _capi.load()
    loss = (C.c_float * 2)(3.0, 4.0)
    hs = (C.c_void_p * 2)(None, None)
    cases = [(None, 2, b'null hs'), (hs, 0, b'n_models must be in [1, 256]'), (hs, 257, b'n_models must be in [1, 256]'),
             (hs, 2, b'model 0: null handle')]
    for hs_, n, text in cases:
        for _ in range(2):
            assert lib.ipnn_create(None, None) == _capi.FNN_ERR_ARG     # some other message first
            assert lib.ipnn_last_error(None) == b'null argument'
            assert lib.ipnn_train_step_multi(hs_, n, None, None, None, 10, None, None, None, None, loss) == _capi.FNN_ERR_ARG
            assert lib.ipnn_last_error(None) == NAME.encode() + b': ' + text
            assert list(loss) == [3.0, 4.0]


def test_python_signatures():
    p = inspect.signature(ipnn.train_step_many).parameters
    assert list(p) == ['engines', 'ids', 'y', 'masks', 'wts', 'want_logits', 'want_loss']
    assert p['masks'].default is None and p['wts'].default is None and p['want_logits'].default is False and p['want_loss'].default is True
    p = inspect.signature(ipnn.train_epoch_many).parameters
    assert list(p) == ['engines', 'ids', 'y', 'batch_size', 'seeds', 'first_step', 'wts']
    assert p['seeds'].default is None and p['first_step'].default == 0 and p['wts'].default is None


def test_masks_are_checked_before_any_device_is_touched():
    """engines that are no engines: the checks come before the first attribute of one is read"""
    import numpy as np
    engines = [object(), object()]
    arrays = [np.ones((4, 3), np.uint8)]
    with pytest.raises(ValueError, match="mixes Drawn entries and arrays"):
        ipnn.train_step_many(engines, None, None, masks=[arrays, Drawn(1, 2)])
    with pytest.raises(ValueError, match="3 entries for 2 engines"):
        ipnn.train_step_many(engines, None, None, masks=[None, None, None])
    with pytest.raises(ValueError, match="1 entries for 2 engines"):
        ipnn.train_step_many(engines, None, None, masks=[Drawn(1, 2)])
