"""fnn_create's limits for wide FM rows (k = rank + 1 in 17..128, n_fields * rup(k, 4) <= 4096), checked before any device is
touched: they hold on a machine without a GPU as on one with."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, F, k):
    h = C.c_void_p()
    cfg = _capi.fnn_cfg(F, k, 300, 100, 256, 0, 0, 0, 0.001, 0.0, 0.1, 0, None)
    rc = lib.fnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.fnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.fnn_destroy(h)
    return rc, msg


@pytest.mark.parametrize("F,k", [(16, 17), (16, 20), (16, 51), (16, 101), (16, 128), (39, 101), (64, 64), (2, 128)])
def test_wide_k_passes_argument_checks(built, F, k):
    """Accepted shapes get past every argument check: a handle (GPU) or the no-device error (no GPU), never FNN_ERR_ARG."""
    rc, msg = _create(_capi.load(), F, k)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg


@pytest.mark.parametrize("F,k,text", [(16, 16, 'k = rank+1'), (16, 129, 'k = rank+1'), (16, 0, 'k = rank+1'),
                                      (40, 101, '4096'), (64, 65, '4096'), (33, 128, '4096')])
def test_wide_limits_are_refused(built, F, k, text):
    """k = 16 keeps its refusal (its message still names k = rank+1), k above 128 is refused, and so is a layer-one width
    n_fields * rup(k, 4) above 4096."""
    rc, msg = _create(_capi.load(), F, k)
    assert rc == _capi.FNN_ERR_ARG and text in msg, (rc, msg)
