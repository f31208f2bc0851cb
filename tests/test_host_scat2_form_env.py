"""FNN_SCAT2_FORM=block|wave selects the body of level 2 of the sparse-row update on 16-float rows (scat2_body: a workgroup per
multi-chunk segment; scat2w_body: a wave per segment).  The handles read it where they are created; fnn_scat2_form() reports what
they would read, without a device.  An unset or unknown value leaves every handle its own default and is not refused."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


@pytest.mark.parametrize("form", ['block', 'wave'])
def test_the_two_values_select_their_form(built, monkeypatch, form):
    monkeypatch.setenv('FNN_SCAT2_FORM', form)
    assert _capi.load().fnn_scat2_form() == form.encode()


@pytest.mark.parametrize("form", [None, '', 'WAVE', 'wave ', 'waves', 'blocks', '1'])
def test_unset_and_unknown_values_select_the_default(built, monkeypatch, form):
    if form is None:
        monkeypatch.delenv('FNN_SCAT2_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT2_FORM', form)
    assert _capi.load().fnn_scat2_form() == b'default'


def test_the_level_1_switch_is_read_on_its_own(built, monkeypatch):
    monkeypatch.setenv('FNN_SCAT1_FORM', 'quarter')
    monkeypatch.setenv('FNN_SCAT2_FORM', 'wave')
    lib = _capi.load()
    assert lib.fnn_scat1_form() == b'quarter' and lib.fnn_scat2_form() == b'wave'


@pytest.mark.parametrize("form", [None, 'block', 'wave', 'ring'])
def test_every_value_passes_the_argument_checks(built, monkeypatch, form):
    """A handle (GPU) or the no-device error (no GPU)."""
    if form is None:
        monkeypatch.delenv('FNN_SCAT2_FORM', raising=False)
    else:
        monkeypatch.setenv('FNN_SCAT2_FORM', form)
    lib = _capi.load()
    h = C.c_void_p()
    cfg = _capi.fnn_cfg(16, 11, 300, 100, 256, _capi.FNN_PREC_BF16, 0, 0, 0.01, 0.0, 0.1, 0, None, _capi.FNN_MODE_FM, 0)
    rc = lib.fnn_create(C.byref(cfg), C.byref(h))
    msg = (lib.fnn_last_error(None) or b'').decode()
    if rc == 0:
        lib.fnn_destroy(h)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg
