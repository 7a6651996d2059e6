"""Argument errors and field refusals of multipoint evaluation and interpolation (ronk_poly_eval_many*, ronk_poly_interpolate*): all
of them are decided before any device work, so this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

P = 0xFFFFFFFF00000001
NAMES = ("ronk_poly_eval_many", "ronk_poly_eval_many_dev", "ronk_poly_interpolate", "ronk_poly_interpolate_dev")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_eval_many_arguments(L):
    c, x, out = np.ones(4, np.uint64), np.ones(3, np.uint64), np.zeros(3, np.uint64)
    f = L.lib.ronk_poly_eval_many
    assert f(P, None, 4, _p(x), 3, _p(out)) == L.ERR_INVALID
    assert f(P, _p(c), 4, None, 3, _p(out)) == L.ERR_INVALID
    assert f(P, _p(c), 4, _p(x), 3, None) == L.ERR_INVALID
    assert f(P, _p(c), 0, _p(x), 3, _p(out)) == L.ERR_INVALID
    assert f(P, _p(c), 4, _p(x), 0, _p(out)) == L.ERR_INVALID
    assert f(100, _p(c), 4, _p(x), 3, _p(out)) == L.ERR_NOT_PRIME
    assert f(91, _p(c), 4, _p(x), 3, _p(out)) == L.ERR_NOT_PRIME
    d = C.c_void_p(16)   # never dereferenced: refused first
    g = L.lib.ronk_poly_eval_many_dev
    assert g(P, None, 4, d, 3, d, None) == L.ERR_INVALID
    assert g(P, d, 4, None, 3, d, None) == L.ERR_INVALID
    assert g(P, d, 4, d, 3, None, None) == L.ERR_INVALID
    assert g(P, d, 0, d, 3, d, None) == L.ERR_INVALID
    assert g(P, d, 4, d, 0, d, None) == L.ERR_INVALID
    assert g(100, d, 4, d, 3, d, None) == L.ERR_NOT_PRIME


def test_interpolate_arguments(L):
    x, y, out = np.arange(3, dtype=np.uint64), np.ones(3, np.uint64), np.zeros(3, np.uint64)
    f = L.lib.ronk_poly_interpolate
    assert f(P, None, _p(y), 3, _p(out)) == L.ERR_INVALID
    assert f(P, _p(x), None, 3, _p(out)) == L.ERR_INVALID
    assert f(P, _p(x), _p(y), 3, None) == L.ERR_INVALID
    assert f(P, _p(x), _p(y), 0, _p(out)) == L.ERR_INVALID
    assert f(100, _p(x), _p(y), 3, _p(out)) == L.ERR_NOT_PRIME
    assert f(91, _p(x), _p(y), 3, _p(out)) == L.ERR_NOT_PRIME
    d = C.c_void_p(16)
    g = L.lib.ronk_poly_interpolate_dev
    assert g(P, None, d, 3, d, d, None) == L.ERR_INVALID
    assert g(P, d, None, 3, d, d, None) == L.ERR_INVALID
    assert g(P, d, d, 3, None, d, None) == L.ERR_INVALID
    assert g(P, d, d, 3, d, None, None) == L.ERR_INVALID     # d_status is required
    assert g(P, d, d, 0, d, d, None) == L.ERR_INVALID


def test_fields_without_the_two_adicity(L):
    """F_101 (p - 1 = 4 * 25) has no tree form: interpolation stops at the O(m^2) kernels' 2^14 nodes, evaluation at m d = 2^34"""
    d = C.c_void_p(16)
    assert L.lib.ronk_poly_interpolate_dev(101, d, d, 2**15, d, d, None) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_poly_interpolate_dev(101, d, d, 2**14 + 1, d, d, None) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_poly_eval_many_dev(101, d, 2**18, d, 2**16 + 1, d, None) == L.ERR_UNSUPPORTED
    # beyond 2^24 points no form serves any field
    assert L.lib.ronk_poly_interpolate_dev(P, d, d, 2**24 + 1, d, d, None) == L.ERR_UNSUPPORTED


def test_no_device(L):
    if L.device_count() > 0:
        return   # a device is present: the calls would run (tests/test_gpu_multipoint.py)
    c, x, out = np.ones(4, np.uint64), np.arange(4, dtype=np.uint64), np.zeros(4, np.uint64)
    assert L.lib.ronk_poly_eval_many(P, _p(c), 4, _p(x), 4, _p(out)) == L.ERR_NO_DEVICE
    assert L.lib.ronk_poly_interpolate(P, _p(x), _p(c), 4, _p(out)) == L.ERR_NO_DEVICE
    assert L.lib.ronk_poly_eval_many(101, _p(c), 4, _p(x), 4, _p(out)) == L.ERR_NO_DEVICE
    d = C.c_void_p(16)
    assert L.lib.ronk_poly_eval_many_dev(P, d, 4, d, 4, d, None) == L.ERR_NO_DEVICE
    assert L.lib.ronk_poly_interpolate_dev(P, d, d, 4, d, d, None) == L.ERR_NO_DEVICE
