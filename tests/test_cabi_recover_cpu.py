"""Argument errors of the erasure-recovery and product-tree entry points (ronk_rs_recover*, ronk_poly_from_roots*): all of them are
refused before any device work, so this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_error_code_and_text(L):
    assert L.ERR_NOT_CODEWORD == -14
    assert L.lib.ronk_strerror(-14) == b"the surviving values lie on no polynomial of degree < k"
    for name in ("ronk_poly_from_roots", "ronk_poly_from_roots_dev", "ronk_rs_recover", "ronk_rs_recover_batch_dev"):
        assert name in L.EXPORTS


def test_recover_null_pointers(L):
    ys, msg, er = np.zeros(16, np.uint64), np.zeros(8, np.uint64), np.zeros(2, np.uint64)
    f = L.lib.ronk_rs_recover
    assert f(P, 7, 16, 8, _p(er), 2, None, _p(msg), None) == L.ERR_INVALID           # ys
    assert f(P, 7, 16, 8, _p(er), 2, _p(ys), None, None) == L.ERR_INVALID            # msg
    assert f(P, 7, 16, 8, None, 2, _p(ys), _p(msg), None) == L.ERR_INVALID           # erased with n_erased > 0
    d = C.c_void_p(16)   # never dereferenced: refused first
    g = L.lib.ronk_rs_recover_batch_dev
    assert g(None, 8, d, 2, d, d, None, d, None) == L.ERR_INVALID                     # plan
    assert g(d, 8, d, 2, None, d, None, d, None) == L.ERR_INVALID                     # d_ys
    assert g(d, 8, d, 2, d, None, None, d, None) == L.ERR_INVALID                     # d_msgs
    assert g(d, 8, d, 2, d, d, None, None, None) == L.ERR_INVALID                     # d_status is required
    assert g(d, 8, None, 2, d, d, None, d, None) == L.ERR_INVALID                     # d_erased with n_erased > 0


def test_recover_sizes(L):
    ys, msg, er = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.arange(16, dtype=np.uint64)
    f = L.lib.ronk_rs_recover
    assert f(P, 7, 16, 0, _p(er), 0, _p(ys), _p(msg), None) == L.ERR_INVALID        # k == 0
    assert f(P, 7, 16, 17, _p(er), 0, _p(ys), _p(msg), None) == L.ERR_INDEX         # k > N
    assert f(P, 7, 16, 8, _p(er), 9, _p(ys), _p(msg), None) == L.ERR_INDEX          # n_erased > N - k
    assert f(P, 7, 16, 1, _p(er), 16, _p(ys), _p(msg), None) == L.ERR_INDEX
    assert f(P, 7, 12, 4, _p(er), 2, _p(ys), _p(msg), None) == L.ERR_NOT_POW2
    assert f(101, 2, 16, 4, _p(er), 2, _p(ys), _p(msg), None) == L.ERR_NO_ROOT      # 16 does not divide 100


def test_poly_from_roots_arguments(L):
    r, out = np.zeros(4, np.uint64), np.zeros(5, np.uint64)
    f = L.lib.ronk_poly_from_roots
    assert f(P, None, 4, _p(out)) == L.ERR_INVALID
    assert f(P, _p(r), 4, None) == L.ERR_INVALID
    assert f(100, _p(r), 4, _p(out)) == L.ERR_NOT_PRIME
    assert f(91, _p(r), 4, _p(out)) == L.ERR_NOT_PRIME
    # F_101 beyond one leaf: its p - 1 has no 2^7 | p - 1 for the tree's products
    r = np.zeros(L.ROOTS_LEAF + 1, np.uint64)
    out = np.zeros(L.ROOTS_LEAF + 2, np.uint64)
    assert f(101, _p(r), r.size, _p(out)) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_poly_from_roots_dev(P, None, 3, C.c_void_p(16), None) == L.ERR_INVALID
