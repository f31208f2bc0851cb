"""The limits include/rbm_hip.h and include/dae_hip.h state, refused with FNN_ERR_ARG and their message before any device is
touched: they hold on a machine without a GPU as on one with.  ONLY refused calls: the pointers are small host dummies, which an
accepted call would hand to a kernel."""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi

_buf = (C.c_double * 64)()
P = C.addressof(_buf)                       # non-null, never dereferenced by a refused call
SHAPE_RBM = 'need 1 <= H <= 256, 1 <= S <= 32, N >= 1'
SHAPE_DAE = 'need N >= 1, 1 <= H <= 256, 1 <= S <= 32'
DENSE_DAE = 'need N >= 1, 1 <= row <= 2048, 1 <= col <= 1024'
BAG_DAE = 'need 1 <= H <= 1024, n >= 1, F >= 1'


def _refused(lib, rc, err, text):
    msg = (err() or b'').decode()
    assert rc == _capi.FNN_ERR_ARG and text in msg, (rc, msg)


@pytest.mark.parametrize("N,H,S", [(10, 0, 8), (10, 257, 8), (10, 8, 0), (10, 8, 33), (0, 8, 8)])
def test_rbm_sparse_epoch_limits(built, N, H, S):
    lib = _capi.load()
    _refused(lib, lib.rbm_sparse_epoch(P, P, P, P, P, P, P, N, H, S, 2e-4, 1e-4, 1e-4, 1e-4, 0.9, None, None), lib.rbm_last_error, SHAPE_RBM)


@pytest.mark.parametrize("N,M,H,S", [(10, 4, 0, 8), (10, 4, 257, 8), (10, 4, 8, 0), (10, 4, 8, 33), (0, 4, 8, 8), (10, 0, 8, 8)])
def test_rbm_sparse_batch_limits(built, N, M, H, S):
    lib = _capi.load()
    _refused(lib, lib.rbm_sparse_batch(P, P, P, P, P, P, P, P, P, N, M, H, S, 2e-4, 1e-4, 1e-4, 1e-4, 0.9, None, None), lib.rbm_last_error,
             SHAPE_RBM + ', M >= 1')


@pytest.mark.parametrize("null", range(7))
def test_rbm_sparse_epoch_null_pointers(built, null):
    lib = _capi.load()
    a = [P] * 7
    a[null] = None
    _refused(lib, lib.rbm_sparse_epoch(*a, 10, 8, 8, 2e-4, 1e-4, 1e-4, 1e-4, 0.9, None, None), lib.rbm_last_error, 'null pointer')


@pytest.mark.parametrize("null", range(9))
def test_rbm_sparse_batch_null_pointers(built, null):
    lib = _capi.load()
    a = [P] * 9
    a[null] = None
    _refused(lib, lib.rbm_sparse_batch(*a, 10, 4, 8, 8, 2e-4, 1e-4, 1e-4, 1e-4, 0.9, None, None), lib.rbm_last_error, 'null pointer')


@pytest.mark.parametrize("nvis,nhid,max_n,prec,text", [(0, 8, 4, 0, 'bad shape'), (4096, 8, 4, 0, 'bad shape'), (8, 0, 4, 0, 'bad shape'),
                                                       (8, 4096, 4, 0, 'bad shape'), (8, 8, 0, 0, 'bad shape'),
                                                       (8, 8, 4, 2, 'bad precision'), (8, 8, 4, -1, 'bad precision')])
def test_rbm_dense_create_limits(built, nvis, nhid, max_n, prec, text):
    lib = _capi.load()
    h = C.c_void_p(P)
    _refused(lib, lib.rbm_dense_create(nvis, nhid, max_n, prec, 0, None, C.byref(h)), lib.rbm_last_error, text)
    assert h.value is None                                    # *out is cleared on every refusal


def test_rbm_dense_null_pointers(built):
    lib = _capi.load()
    _refused(lib, lib.rbm_dense_create(8, 8, 4, 0, 0, None, None), lib.rbm_last_error, 'null out')
    _refused(lib, lib.rbm_dense_set(None, P, P, P), lib.rbm_last_error, 'null pointer')
    _refused(lib, lib.rbm_dense_get(None, P, P, P), lib.rbm_last_error, 'null pointer')
    _refused(lib, lib.rbm_dense_cd1(None, P, 1, P, 2e-4, 1e-4, 1e-4, 1e-4, 0.9, None), lib.rbm_last_error, 'null pointer')
    assert lib.rbm_dense_destroy(None) == _capi.FNN_ERR_ARG


def test_rbm_helper_limits(built):
    lib = _capi.load()
    for a in ((None, P, 4, 9, P, 2, 3, P), (P, None, 4, 9, P, 2, 3, P), (P, P, 4, 9, None, 2, 3, P), (P, P, 4, 9, P, 2, 3, None)):
        _refused(lib, lib.rbm_bag_sum(*a, None), lib.rbm_last_error, 'null pointer')
    for H, n, F in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        _refused(lib, lib.rbm_bag_sum(P, P, H, 9, P, n, F, P, None), lib.rbm_last_error, 'need H >= 1, n >= 1, F >= 1')
    for a in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        _refused(lib, lib.rbm_affine(a[0], a[1], a[2], 2, 3, 4, a[3], None), lib.rbm_last_error, 'null pointer')
    for n, a, b in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        _refused(lib, lib.rbm_affine(P, P, P, n, a, b, P, None), lib.rbm_last_error, 'need n >= 1, a >= 1, b >= 1')
    _refused(lib, lib.rbm_sigmoid(None, 4, None), lib.rbm_last_error, 'null pointer')
    _refused(lib, lib.rbm_sigmoid(P, 0, None), lib.rbm_last_error, 'need count >= 1')


@pytest.mark.parametrize("fn", ['dae_sparse_epoch', 'dae_sparse_epoch_f64'])
@pytest.mark.parametrize("N,H,S", [(10, 0, 8), (10, 257, 8), (10, 8, 0), (10, 8, 33), (0, 8, 8)])
def test_dae_sparse_epoch_limits(built, fn, N, H, S):
    lib = _capi.load()
    _refused(lib, getattr(lib, fn)(P, 100, P, P, P, P, P, N, H, S, 0.1, None, None), lib.dae_last_error, SHAPE_DAE)
    _refused(lib, getattr(lib, fn)(P, 0, P, P, P, P, P, 10, 8, 8, 0.1, None, None), lib.dae_last_error, SHAPE_DAE)       # an empty table


@pytest.mark.parametrize("fn", ['dae_sparse_epoch', 'dae_sparse_epoch_f64'])
@pytest.mark.parametrize("null", range(6))
def test_dae_sparse_epoch_null_pointers(built, fn, null):
    lib = _capi.load()
    a = [P] * 6
    a[null] = None
    _refused(lib, getattr(lib, fn)(a[0], 100, a[1], a[2], a[3], a[4], a[5], 10, 8, 8, 0.1, None, None), lib.dae_last_error, 'null pointer')


@pytest.mark.parametrize("fn", ['dae_dense_epoch', 'dae_dense_epoch_f64'])
@pytest.mark.parametrize("N,row,col", [(5, 2049, 8), (5, 8, 1025), (5, 2049, 1025)])
def test_dae_dense_epoch_limits(built, fn, N, row, col):
    lib = _capi.load()
    _refused(lib, getattr(lib, fn)(P, P, P, P, N, row, col, 0.1, 0, None, None), lib.dae_last_error, DENSE_DAE)


@pytest.mark.parametrize("fn,text", [('dae_dense_epoch', 'need N, row, col >= 1'), ('dae_dense_epoch_f64', DENSE_DAE)])
def test_dae_dense_epoch_empty_shapes_and_null_pointers(built, fn, text):
    lib = _capi.load()
    for N, row, col in ((0, 8, 8), (5, 0, 8), (5, 8, 0)):
        _refused(lib, getattr(lib, fn)(P, P, P, P, N, row, col, 0.1, 0, None, None), lib.dae_last_error, text)
    for null in range(4):
        a = [P] * 4
        a[null] = None
        _refused(lib, getattr(lib, fn)(*a, 5, 8, 8, 0.1, 0, None, None), lib.dae_last_error, 'null pointer')


@pytest.mark.parametrize("fn", ['dae_bag_cumsum_sigmoid', 'dae_bag_cumsum_sigmoid_f64'])
def test_dae_bag_limits(built, fn):
    lib = _capi.load()
    for H, n, F in ((1025, 2, 3), (0, 2, 3), (8, 0, 3), (8, 2, 0)):
        _refused(lib, getattr(lib, fn)(P, P, H, 9, P, n, F, P, None), lib.dae_last_error, BAG_DAE)
    for a in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        _refused(lib, getattr(lib, fn)(a[0], a[1], 8, 9, a[2], 2, 3, a[3], None), lib.dae_last_error, 'null pointer')


def test_dae_affine_limits(built):
    lib = _capi.load()
    for n, a, b in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        _refused(lib, lib.dae_affine_sigmoid_f64(P, P, P, n, a, b, P, None), lib.dae_last_error, 'null pointer or empty shape')
    for a in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        _refused(lib, lib.dae_affine_sigmoid_f64(a[0], a[1], a[2], 2, 3, 4, a[3], None), lib.dae_last_error, 'null pointer or empty shape')
