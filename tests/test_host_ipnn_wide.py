"""ipnn_create's limits for wide rows (k = rank + 1 in 17..128, 2..32 fields: layer-one field columns F * rup(k, 4) <= 4096),
checked before any device is touched: they hold on a machine without a GPU as on one with."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, F, k, pairs=1, precision=0, optimizer=0):
    h = C.c_void_p()
    hid = (C.c_int32 * 8)(400, 400, 200, 0, 0, 0, 0, 0)
    cfg = _capi.ipnn_cfg(F, k, 3, hid, _capi.IPNN_ACTS['relu'], pairs, 4096, precision, 0.001, 0.5, optimizer, 0.9, 0.999, 1e-8, 0, None)
    rc = lib.ipnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.ipnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.ipnn_destroy(h)
    return rc, msg


@pytest.mark.parametrize("F,k", [(16, 17), (16, 51), (16, 101), (16, 128), (32, 128), (2, 128), (23, 101)])
def test_wide_k_passes_argument_checks(built, F, k):
    """Accepted shapes get past every argument check, with and without the pairs, in both precisions and under all three
    optimisers: a handle (GPU) or the no-device error (no GPU), never FNN_ERR_ARG."""
    lib = _capi.load()
    for pairs, prec, opt in ((1, 0, 0), (0, 1, 1), (1, 1, 2), (0, 0, 2), (1, 1, 0)):
        rc, msg = _create(lib, F, k, pairs, prec, opt)
        assert rc in (0, _capi.FNN_ERR_HIP), (pairs, prec, opt, rc, msg)
        if rc != 0:
            assert 'no CPU fallback' in msg


@pytest.mark.parametrize("F,k,prec,text", [(16, 129, 0, '1..128'), (16, 0, 1, '1..128'), (33, 101, 1, '2..32')])
def test_wide_limits_are_refused(built, F, k, prec, text):
    """k above 128, k below 1 and more than 32 fields are refused, each with a message that names its limit."""
    rc, msg = _create(_capi.load(), F, k, precision=prec)
    assert rc == _capi.FNN_ERR_ARG and text in msg, (rc, msg)
