"""FNN_SCAT1_FORM=slot|quarter|half selects the body of level 1 of the sparse-row update on 16-float rows.  The handles read it
where they are created; fnn_scat1_form() reports what they would read, without a device.  An unset or unknown value leaves every
handle its own default -- and, unlike FNN_WGRAD_FORM, is not refused: fnn_create gets past its argument checks with any value."""
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


@pytest.mark.parametrize("form", ['slot', 'quarter', 'half'])
def test_the_three_values_select_their_form(built, monkeypatch, form):
    monkeypatch.setenv('FNN_SCAT1_FORM', form)
    assert _capi.load().fnn_scat1_form() == form.encode()


@pytest.mark.parametrize("form", [None, '', 'HALF', 'half ', 'halves', 'quarters', '2'])
def test_unset_and_unknown_values_select_the_default(built, monkeypatch, form):
    if form is None:
        monkeypatch.delenv('FNN_SCAT1_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
    assert _capi.load().fnn_scat1_form() == b'default'


@pytest.mark.parametrize("prec", [_capi.FNN_PREC_BF16, _capi.FNN_PREC_F32, _capi.FNN_PREC_BF16X3])
@pytest.mark.parametrize("form", [None, 'slot', 'quarter', 'half', 'ring'])
def test_every_value_passes_the_argument_checks(built, monkeypatch, form, prec):
    """A handle (GPU) or the no-device error (no GPU), in every precision."""
    if form is None:
        monkeypatch.delenv('FNN_SCAT1_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT1_FORM', form)
    rc, msg = _create(_capi.load(), prec)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg
