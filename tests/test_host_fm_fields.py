"""fm_create's field range (1 <= n_fields <= 64, both row layouts), checked before any device is touched: it holds on a machine
without a GPU as on one with."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi


def _create(lib, F, k):
    h = C.c_void_p()
    rc = lib.fm_create(F, k, 256, 0, None, C.byref(h))
    msg = (lib.fm_last_error(None) or b'').decode()
    if rc == 0:
        lib.fm_destroy(h)
    return rc, msg, h.value


@pytest.mark.parametrize("F", [17, 26, 32, 39, 64])
@pytest.mark.parametrize("k", [1, 11, 16, 17, 51, 101, 128])
def test_fm_fields_pass_argument_checks(built, F, k):
    """17..64 fields on the narrow (k <= 16) and the wide (k >= 17) rows get past every argument check: a handle (GPU) or the
    no-device error (no GPU), never FNN_ERR_ARG."""
    rc, msg, _ = _create(_capi.load(), F, k)
    assert rc in (0, _capi.FNN_ERR_HIP), (rc, msg)
    if rc != 0:
        assert 'no CPU fallback' in msg


@pytest.mark.parametrize("F", [0, 65, 128])
def test_fm_fields_outside_the_range_are_refused(built, F):
    rc, msg, h = _create(_capi.load(), F, 11)
    assert rc == _capi.FNN_ERR_ARG and not h, (rc, msg)
    assert '1 <= n_fields <= 64' in msg


@pytest.mark.parametrize("k", [0, 129])
def test_fm_k_limits_hold_at_39_fields(built, k):
    rc, msg, h = _create(_capi.load(), 39, k)
    assert rc == _capi.FNN_ERR_ARG and not h, (rc, msg)
    assert '1 <= k <= 128' in msg
