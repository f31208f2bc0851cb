"""FNN_WGRAD_FORM=direct|lds selects the form of the bf16 weight-gradient products (wgrad_tile).  fnn_create reads it once and
checks it with its other arguments, before any device is touched: the check holds on a machine without a GPU as on one with."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, prec):
    h = C.c_void_p()
    cfg = _capi.fnn_cfg(16, 11, 300, 100, 256, prec, 0, 0, 0.01, 0.0, 0.1, 0, None, _capi.FNN_MODE_FM, 0)
    rc = lib.fnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.fnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.fnn_destroy(h)
    return rc, msg


@pytest.mark.parametrize("prec", [_capi.FNN_PREC_BF16, _capi.FNN_PREC_F32, _capi.FNN_PREC_BF16X3])
@pytest.mark.parametrize("form", [None, 'direct', 'lds'])
def test_known_forms_pass_argument_checks(built, monkeypatch, form, prec):
    """Unset, direct and lds get past every argument check in every precision: a handle (GPU) or the no-device error (no GPU)."""
    if form is None:
        monkeypatch.delenv('FNN_WGRAD_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_WGRAD_FORM', form)
    rc, msg = _create(_capi.load(), prec)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg


@pytest.mark.parametrize("form", ['', 'LDS', 'lds ', 'ring', '1'])
def test_unknown_forms_are_refused(built, monkeypatch, form):
    monkeypatch.setenv('FNN_WGRAD_FORM', form)
    rc, msg = _create(_capi.load(), _capi.FNN_PREC_BF16)
    assert rc == _capi.FNN_ERR_ARG and 'FNN_WGRAD_FORM must be direct or lds' in msg, (rc, msg)
