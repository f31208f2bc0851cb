"""ipnn_create's field-count limits, checked before any device is touched: narrow rows (k = rank + 1 in 1..16) take 2..64 fields
-- the reference's inner-product classes are 39-field models (X_feas = 13 + len(cat_sizes)) -- and wide rows (k = 17..128) stay
at 2..32.  They hold on a machine without a GPU as on one with."""
import ctypes as C
import itertools

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, F, k, pairs=1, precision=0, optimizer=0, max_batch=4096):
    h = C.c_void_p()
    hid = (C.c_int32 * 8)(400, 400, 200, 0, 0, 0, 0, 0)
    cfg = _capi.ipnn_cfg(F, k, 3, hid, _capi.IPNN_ACTS['relu'], pairs, max_batch, precision, 0.001, 0.5, optimizer, 0.9, 0.999, 1e-8, 0, None)
    rc = lib.ipnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.ipnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.ipnn_destroy(h)
    return rc, msg


@pytest.mark.parametrize("F,k", [(33, 1), (39, 11), (45, 16), (46, 16), (64, 16), (64, 1)])
def test_many_fields_pass_argument_checks(built, F, k):
    """33..64 fields of narrow rows get past every argument check, with and without the pairs, in both precisions and under all
    three optimisers: a handle (GPU) or the no-device error (no GPU), never FNN_ERR_ARG."""
    lib = _capi.load()
    for pairs, prec, opt in itertools.product((1, 0), (0, 1), (0, 1, 2)):
        rc, msg = _create(lib, F, k, pairs, prec, opt)
        assert rc in (0, _capi.FNN_ERR_HIP), (pairs, prec, opt, rc, msg)
        if rc != 0:
            assert 'no CPU fallback' in msg


@pytest.mark.parametrize("F,k,text", [(65, 11, '2..64'), (1, 11, '2..64'), (33, 17, '2..32'), (64, 128, '2..32')])
def test_field_limits_are_refused(built, F, k, text):
    """More than 64 fields, fewer than 2, and more than 32 fields of wide rows are refused, each with a message naming its limit."""
    for prec in (0, 1):
        rc, msg = _create(_capi.load(), F, k, precision=prec)
        assert rc == _capi.FNN_ERR_ARG and text in msg, (rc, msg)


def test_batch_limit_stays(built):
    rc, msg = _create(_capi.load(), 39, 11, max_batch=4097)
    assert rc == _capi.FNN_ERR_ARG and '2..64' in msg and '2..32' in msg and '4096' in msg, (rc, msg)


def test_cfg_struct_is_unchanged(built):
    lib = _capi.load()
    assert lib.ipnn_cfg_size() == C.sizeof(_capi.ipnn_cfg) == 96
