"""fm_train_online / fm_online_form of include/fm_hip.h on the host side: declared, bound in _capi, covered by the linker's
export list, exported by the built library, refused without a handle; FM / LR and ipinyou.run take them."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipinyou
from deep_ctr_amd.FM import FM
from deep_ctr_amd.LR import LR

NEW = ("fm_train_online", "fm_online_form")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_online_entry_points_are_declared_and_bound():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fm_hip.h")).read())
    assert ("int fm_train_online(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int64_t N, float lr, "
            "float lambda, float* p_out, double* loss_sum_out, float* loss_last_out);") in hdr
    assert "const char* fm_online_form(const fm_handle* h);" in hdr
    assert "FNN_ERR_STATE under Adam or FTRL" in hdr and "FM_ONLINE_CHUNK" in hdr
    res, args = _capi.FM_SIGNATURES["fm_train_online"]
    assert res is C.c_int and len(args) == 10 and args[4] is C.c_int64 and args[5] is C.c_float and args[6] is C.c_float
    assert args[8] is C.POINTER(C.c_double) and args[9] is C.POINTER(C.c_float)
    assert _capi.FM_SIGNATURES["fm_online_form"] == (C.c_char_p, [C.c_void_p])


def test_export_list_covers_them():
    text = open(os.path.join(ROOT, "deep-ctr_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), (name, pats)


def test_library_exports_them(built):
    lib = _capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _capi.FM_SIGNATURES[name][1], name
    loss, last = C.c_double(1.0), C.c_float(1.0)
    assert lib.fm_train_online(None, None, None, None, 0, 0.05, 0.0, None, C.byref(loss), C.byref(last)) == _capi.FNN_ERR_ARG
    assert (loss.value, last.value) == (1.0, 1.0)                           # nothing written
    assert lib.fm_online_form(None) == b'plain'                             # the one form built: no knob to read


def test_python_signatures():
    for cls in (FM, LR):
        p = inspect.signature(cls.train_online).parameters
        assert list(p) == ['self', 'ids', 'y', 'wts', 'want_p', 'want_loss']
        assert p['wts'].default is None and p['want_p'].default is False and p['want_loss'].default is True
    p = inspect.signature(ipinyou.run).parameters
    assert list(p)[-1] == 'online' and p['online'].default is False
    assert p['batch_size'].default == 4096 and p['buffer'].default == 10000
