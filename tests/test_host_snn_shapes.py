"""fnn_create's limits for FNN_MODE_BAG (the SNN fine-tune step): h0 a multiple of 4 in [192, 316] and 2 to 64 columns,
checked before any device is touched: they hold on a machine without a GPU as on one with."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, F, h0, H1=300, H2=100):
    h = C.c_void_p()
    cfg = _capi.fnn_cfg(F, 0, H1, H2, 256, 0, 0, 1, 0.01, 0.001, 0.0, 0, None, _capi.FNN_MODE_BAG, h0)
    rc = lib.fnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.fnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.fnn_destroy(h)
    return rc, msg


@pytest.mark.parametrize("F,h0", [(2, 192), (64, 316), (16, 252), (39, 256), (17, 300), (3, 200)])
def test_bag_shapes_pass_argument_checks(built, F, h0):
    """Accepted shapes get past every argument check: a handle (GPU) or the no-device error (no GPU), never FNN_ERR_ARG."""
    rc, msg = _create(_capi.load(), F, h0)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg


@pytest.mark.parametrize("F,h0,text", [(16, 188, 'h0 must be a multiple of 4 in [192, 316]'),
                                       (16, 320, 'h0 must be a multiple of 4 in [192, 316]'),
                                       (16, 254, 'h0 must be a multiple of 4 in [192, 316]'),
                                       (1, 200, 'n_fields must be in [2, 64]'), (65, 200, 'n_fields must be in [2, 64]')])
def test_bag_limits_are_refused(built, F, h0, text):
    """h0 below 192, above 316 or not a multiple of 4, and a column count outside 2..64, are FNN_ERR_ARG with their message."""
    rc, msg = _create(_capi.load(), F, h0)
    assert rc == _capi.FNN_ERR_ARG and text in msg, (rc, msg)
