"""The order in which the host-pointer entry points of the base-field half of the library report what is wrong with a call: NULL
arguments, size or index checks, prime / root / field checks, then the missing device, and the shortcuts that need no device.
Every case trips the check it names AND every later one, and asserts the earlier check's code.  All of it is decided before any
device work, so this runs without a GPU (with one, the RONK_ERR_NO_DEVICE assertions are skipped)."""
import ctypes as C

import numpy as np
import pytest

P = 0xFFFFFFFF00000001
NAMES = ("ronk_vec_add", "ronk_vec_sub", "ronk_vec_mul", "ronk_poly_add", "ronk_poly_sub", "ronk_vec_neg", "ronk_vec_pow", "ronk_vec_inv",
         "ronk_vec_euler", "ronk_vec_sqrt", "ronk_poly_eval", "ronk_lagrange_eval", "ronk_poly_divrem", "ronk_rs_decode", "ronk_curve_msm",
         "ronk_lagrange_nodes", "ronk_dft", "ronk_poly_mul", "ronk_poly_from_roots", "ronk_rs_recover", "ronk_poly_eval_many",
         "ronk_poly_interpolate", "ronk_poseidon_hash", "ronk_merkle_commit", "ronk_merkle_verify", "ronk_msm_bn254",
         "ronk_kzg_open_bn254", "ronk_ntt_forward_bn254", "ronk_ntt_inverse_bn254", "ronk_poly_mul_bn254", "ronk_trim_workspace")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _no_device(L, rc):
    """the call got past every argument check: without a device that is RONK_ERR_NO_DEVICE (with one it would run)"""
    return L.device_count() > 0 or rc() == L.ERR_NO_DEVICE


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_vector_ops(L):
    a, out = np.ones(4, np.uint64), np.zeros(4, np.uint64)
    # NULL first, with a modulus no field accepts (p = 0) behind it
    for name in ("ronk_vec_add", "ronk_vec_sub", "ronk_vec_mul"):
        f = getattr(L.lib, name)
        assert f(0, None, _p(a), _p(out), 4) == L.ERR_INVALID
        assert f(0, _p(a), None, _p(out), 4) == L.ERR_INVALID
        assert f(0, _p(a), _p(a), None, 4) == L.ERR_INVALID
        assert _no_device(L, lambda: f(101, _p(a), _p(a), _p(out), 4))
    for name in ("ronk_poly_add", "ronk_poly_sub"):
        f = getattr(L.lib, name)
        assert f(0, None, 4, _p(a), 2, _p(out)) == L.ERR_INVALID
        assert f(0, _p(a), 4, None, 2, _p(out)) == L.ERR_INVALID
        assert f(0, _p(a), 4, _p(a), 2, None) == L.ERR_INVALID
        assert _no_device(L, lambda: f(101, _p(a), 4, _p(a), 2, _p(out)))
    for name in ("ronk_vec_neg", "ronk_vec_euler"):
        f = getattr(L.lib, name)
        assert f(0, None, _p(out), 4) == L.ERR_INVALID
        assert f(0, _p(a), None, 4) == L.ERR_INVALID
        assert _no_device(L, lambda: f(101, _p(a), _p(out), 4))
    f = L.lib.ronk_vec_pow
    assert f(0, None, 3, _p(out), 4) == L.ERR_INVALID
    assert f(0, _p(a), 3, None, 4) == L.ERR_INVALID
    assert _no_device(L, lambda: f(101, _p(a), 3, _p(out), 4))
    f = L.lib.ronk_vec_sqrt
    assert f(0, None, _p(out), _p(out), 4) == L.ERR_INVALID
    assert f(0, _p(a), None, _p(out), 4) == L.ERR_INVALID
    assert f(0, _p(a), _p(out), None, 4) == L.ERR_INVALID
    assert _no_device(L, lambda: f(101, _p(a), _p(out), _p(out), 4))


def test_vec_inv_refuses_p_below_two_before_the_device(L):
    a, out = np.ones(4, np.uint64), np.zeros(4, np.uint64)
    f = L.lib.ronk_vec_inv
    assert f(0, _p(a), _p(out), 4) == L.ERR_INVALID
    assert f(1, _p(a), _p(out), 4) == L.ERR_INVALID
    assert f(101, None, _p(out), 4) == L.ERR_INVALID
    assert f(101, _p(a), None, 4) == L.ERR_INVALID
    assert _no_device(L, lambda: f(101, _p(a), _p(out), 4))
    # (an even p > 2 is a field error, looked at once a device is there)
    assert L.device_count() > 0 or f(100, _p(a), _p(out), 4) == L.ERR_NO_DEVICE


def test_poly_eval_asks_for_the_device_before_the_empty_polynomial(L):
    c = np.ones(4, np.uint64)
    out = C.c_uint64(77)
    f = L.lib.ronk_poly_eval
    assert f(0, None, 0, 5, C.byref(out)) == L.ERR_INVALID
    assert f(0, _p(c), 0, 5, None) == L.ERR_INVALID
    if L.device_count() == 0:
        assert f(P, _p(c), 0, 5, C.byref(out)) == L.ERR_NO_DEVICE and out.value == 77   # d == 0 is no shortcut
        assert f(0, _p(c), 4, 5, C.byref(out)) == L.ERR_NO_DEVICE                       # nor is the field looked at first


def test_lagrange_eval_and_divrem(L):
    c, out = np.ones(4, np.uint64), np.zeros(4, np.uint64)
    o = C.c_uint64(0)
    f = L.lib.ronk_lagrange_eval
    assert f(0, None, _p(c), 4, 5, C.byref(o)) == L.ERR_INVALID
    assert f(0, _p(c), None, 4, 5, C.byref(o)) == L.ERR_INVALID
    assert f(0, _p(c), _p(c), 4, 5, None) == L.ERR_INVALID
    assert f(0, _p(c), _p(c), 0, 5, C.byref(o)) == L.ERR_INVALID
    assert _no_device(L, lambda: f(P, _p(c), _p(c), 4, 5, C.byref(o)))
    g = L.lib.ronk_poly_divrem
    assert g(0, None, 4, _p(c), 2, _p(out), _p(out)) == L.ERR_INVALID
    assert g(0, _p(c), 4, None, 2, _p(out), _p(out)) == L.ERR_INVALID
    assert g(0, _p(c), 4, _p(c), 2, None, _p(out)) == L.ERR_INVALID
    assert g(0, _p(c), 4, _p(c), 2, _p(out), None) == L.ERR_INVALID
    assert g(0, _p(c), 0, _p(c), 2, _p(out), _p(out)) == L.ERR_INVALID
    assert g(0, _p(c), 4, _p(c), 0, _p(out), _p(out)) == L.ERR_INVALID
    if L.device_count() == 0:
        assert g(0, _p(c), 4, _p(c), 2, _p(out), _p(out)) == L.ERR_NO_DEVICE     # the field comes after the device
        assert g(P, _p(c), 4, _p(c), 2, _p(out), _p(out)) == L.ERR_NO_DEVICE


def test_rs_decode(L):
    x, out = np.arange(4, dtype=np.uint64), np.zeros(4, np.uint64)
    f = L.lib.ronk_rs_decode
    assert f(0, None, None, 0, None) == L.OK                                  # k == 0: before anything else
    assert f(0, None, _p(x), 2**21 + 1, _p(out)) == L.ERR_INVALID             # NULL before the size
    assert f(0, _p(x), None, 2**21 + 1, _p(out)) == L.ERR_INVALID
    assert f(0, _p(x), _p(x), 2**21 + 1, None) == L.ERR_INVALID
    assert f(P, _p(x), _p(x), 2**21 + 1, _p(out)) == L.ERR_UNSUPPORTED        # k > 2^21: before the device, nothing is read
    assert _no_device(L, lambda: f(P, _p(x), _p(x), 4, _p(out)))


def test_curve_msm(L):
    from ronkathon_amd.callers import Curve
    pts, sc, out = np.zeros(10, np.uint64), np.ones(2, np.uint64), np.full(5, 9, np.uint64)
    f = L.lib.ronk_curve_msm
    big, composite, pluto = Curve(2**32 + 2, 99, 0, 3), Curve(91, 99, 0, 3), Curve(101, 99, 0, 3)
    assert f(None, _p(pts), 1, _p(sc), 2, _p(out)) == L.ERR_INVALID
    assert f(C.byref(big), _p(pts), 1, _p(sc), 2, None) == L.ERR_INVALID
    assert f(C.byref(big), None, 1, _p(sc), 2, _p(out)) == L.ERR_INVALID
    assert f(C.byref(big), _p(pts), 1, None, 2, _p(out)) == L.ERR_INVALID
    assert f(C.byref(big), _p(pts), 1, _p(sc), 2, _p(out)) == L.ERR_UNSUPPORTED      # p >= 2^32 (and even), n_points < n
    assert f(C.byref(Curve(2, 1, 0, 1)), _p(pts), 1, _p(sc), 2, _p(out)) == L.ERR_UNSUPPORTED
    assert f(C.byref(composite), _p(pts), 1, _p(sc), 2, _p(out)) == L.ERR_NOT_PRIME  # 7 * 13, n_points < n
    assert f(C.byref(pluto), _p(pts), 1, _p(sc), 2, _p(out)) == L.ERR_INDEX
    assert f(C.byref(composite), _p(pts), 0, _p(sc), 0, _p(out)) == L.ERR_NOT_PRIME  # the empty sum does not excuse the field
    assert out.tolist() == [9] * 5
    assert f(C.byref(pluto), None, 0, None, 0, _p(out)) == L.OK                      # the empty sum: Infinity, without a device
    assert out.tolist() == [0, 0, 0, 0, 1]
    assert _no_device(L, lambda: f(C.byref(pluto), _p(pts), 2, _p(sc), 2, _p(out)))


def test_lagrange_nodes_dft_and_poly_mul(L):
    a, out = np.ones(8, np.uint64), np.zeros(16, np.uint64)
    f = L.lib.ronk_lagrange_nodes
    assert f(101, 2, None, 3) == L.ERR_INVALID            # NULL before 3 does not divide 100
    assert f(101, 2, _p(out), 0) == L.ERR_INVALID
    assert f(1, 2, _p(out), 3) == L.ERR_INVALID           # p < 2
    assert f(101, 2, _p(out), 3) == L.ERR_NO_ROOT
    assert _no_device(L, lambda: f(101, 2, _p(out), 4))
    g = L.lib.ronk_dft
    assert g(101, 2, None, _p(out), 3) == L.ERR_INVALID
    assert g(101, 2, _p(a), None, 3) == L.ERR_INVALID
    assert g(101, 2, _p(a), _p(out), 0) == L.ERR_INVALID
    assert g(101, 2, _p(a), _p(out), 3) == L.ERR_NO_ROOT          # n does not divide p - 1
    assert g(P, 7, _p(a), _p(out), 2**17 + 1) == L.ERR_NO_ROOT    # ... before the direct kernel's size limit
    assert _no_device(L, lambda: g(101, 2, _p(a), _p(out), 4))
    # 2^17 * 3 divides P - 1 but is beyond the direct kernel and no power of two: the size is refused only once a device is there
    assert L.device_count() > 0 or g(P, 7, _p(a), _p(out), 3 * 2**17) == L.ERR_NO_DEVICE
    h = L.lib.ronk_poly_mul
    assert h(0, 7, None, 8, _p(a), 8, _p(out)) == L.ERR_INVALID
    assert h(0, 7, _p(a), 8, None, 8, _p(out)) == L.ERR_INVALID
    assert h(0, 7, _p(a), 8, _p(a), 8, None) == L.ERR_INVALID
    assert h(0, 7, _p(a), 0, _p(a), 8, _p(out)) == L.ERR_INVALID
    assert h(0, 7, _p(a), 8, _p(a), 0, _p(out)) == L.ERR_INVALID
    assert L.device_count() > 0 or h(0, 7, _p(a), 8, _p(a), 8, _p(out)) == L.ERR_NO_DEVICE


def test_poly_from_roots_refuses_the_field_before_the_device(L):
    r, out = np.ones(4, np.uint64), np.zeros(5, np.uint64)
    f = L.lib.ronk_poly_from_roots
    assert f(100, _p(r), 4, None) == L.ERR_INVALID
    assert f(100, None, 4, _p(out)) == L.ERR_INVALID
    assert f(2, _p(r), 4, _p(out)) == L.ERR_UNSUPPORTED
    assert f(100, _p(r), 4, _p(out)) == L.ERR_NOT_PRIME
    assert f(91, _p(r), 4, _p(out)) == L.ERR_NOT_PRIME
    assert f(91, None, 0, _p(out)) == L.ERR_NOT_PRIME                 # the empty product does not excuse the field
    assert f(101, _p(r), 1 << 12, _p(out)) == L.ERR_UNSUPPORTED       # beyond one leaf F_101 lacks the 2-adicity (nothing is read)
    assert _no_device(L, lambda: f(101, _p(r), 4, _p(out)))
    assert _no_device(L, lambda: f(P, None, 0, _p(out)))


def test_rs_recover_sequence(L):
    """INVALID -> INDEX -> NOT_POW2 -> prime -> NO_ROOT -> device"""
    e, y, out = np.zeros(4, np.uint64), np.ones(16, np.uint64), np.zeros(16, np.uint64)
    f = L.lib.ronk_rs_recover
    # n = 12: no power of two; p = 91: composite, and 12 does not divide 90; k > n behind the NULLs
    assert f(91, 2, 12, 13, _p(e), 1, None, _p(out), None) == L.ERR_INVALID
    assert f(91, 2, 12, 13, _p(e), 1, _p(y), None, None) == L.ERR_INVALID
    assert f(91, 2, 12, 13, None, 1, _p(y), _p(out), None) == L.ERR_INVALID
    assert f(91, 2, 12, 0, _p(e), 1, _p(y), _p(out), None) == L.ERR_INVALID
    assert f(91, 2, 0, 4, _p(e), 1, _p(y), _p(out), None) == L.ERR_INVALID
    assert f(91, 2, 12, 13, _p(e), 1, _p(y), _p(out), None) == L.ERR_INDEX          # k > n
    assert f(91, 2, 12, 10, _p(e), 3, _p(y), _p(out), None) == L.ERR_INDEX          # more erasures than n - k
    assert f(91, 2, 12, 4, _p(e), 1, _p(y), _p(out), None) == L.ERR_NOT_POW2
    assert f(91, 2, 16, 4, _p(e), 1, _p(y), _p(out), None) == L.ERR_NOT_PRIME       # 16 does not divide 90 either
    assert f(101, 2, 16, 4, _p(e), 1, _p(y), _p(out), None) == L.ERR_NO_ROOT
    assert _no_device(L, lambda: f(97, 5, 16, 4, _p(e), 1, _p(y), _p(out), None))


def test_multipoint(L):
    c, x, out = np.ones(4, np.uint64), np.arange(4, dtype=np.uint64), np.zeros(4, np.uint64)
    f = L.lib.ronk_poly_eval_many
    assert f(100, None, 4, _p(x), 4, _p(out)) == L.ERR_INVALID
    assert f(100, _p(c), 0, _p(x), 4, _p(out)) == L.ERR_INVALID
    assert f(100, _p(c), 4, _p(x), 4, _p(out)) == L.ERR_NOT_PRIME
    assert f(2, _p(c), 4, _p(x), 4, _p(out)) == L.ERR_UNSUPPORTED
    assert _no_device(L, lambda: f(P, _p(c), 4, _p(x), 4, _p(out)))
    g = L.lib.ronk_poly_interpolate
    assert g(100, None, _p(c), 4, _p(out)) == L.ERR_INVALID
    assert g(100, _p(x), _p(c), 0, _p(out)) == L.ERR_INVALID
    assert g(100, _p(x), _p(c), 4, _p(out)) == L.ERR_NOT_PRIME
    assert g(101, _p(x), _p(c), 2**14 + 1, _p(out)) == L.ERR_UNSUPPORTED    # no form serves F_101 there (nothing is read)
    assert _no_device(L, lambda: g(P, _p(x), _p(c), 4, _p(out)))


def test_hash_forms_refuse_a_null_handle_first(L):
    d = C.c_void_p(16)   # never dereferenced
    assert L.lib.ronk_poseidon_hash(None, None, 99, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_commit(None, None, 0, 3, 0, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_verify(None, None, 1, 3, None, None, 0, 0, None, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_verify(None, d, 0, 3, d, d, 4, 1, d, d) == L.ERR_INVALID     # n_idx == 0 is no shortcut past the handle


def test_bn254_forms(L):
    a, out = np.ones(64, np.uint64), np.zeros(64, np.uint64)
    f = L.lib.ronk_msm_bn254
    assert f(_p(a), _p(a), 2, None) == L.ERR_INVALID
    assert f(None, _p(a), 2, _p(out)) == L.ERR_INVALID
    assert f(_p(a), None, 2, _p(out)) == L.ERR_INVALID
    assert _no_device(L, lambda: f(None, None, 0, _p(out)))            # the empty sum asks for the device as well
    assert _no_device(L, lambda: f(_p(a), _p(a), 2, _p(out)))
    g = L.lib.ronk_kzg_open_bn254
    z = np.ones(4, np.uint64)
    assert g(None, 3, _p(z), _p(a), 2, _p(out), None) == L.ERR_INVALID  # NULL before n_srs < n
    assert g(_p(a), 3, None, _p(a), 2, _p(out), None) == L.ERR_INVALID
    assert g(_p(a), 3, _p(z), None, 2, _p(out), None) == L.ERR_INVALID
    assert g(_p(a), 3, _p(z), _p(a), 2, None, None) == L.ERR_INVALID
    assert g(_p(a), 0, _p(z), _p(a), 0, _p(out), None) == L.ERR_INVALID
    assert g(_p(a), 3, _p(z), _p(a), 2, _p(out), None) == L.ERR_INDEX
    assert _no_device(L, lambda: g(_p(a), 3, _p(z), _p(a), 3, _p(out), None))
    for name in ("ronk_ntt_forward_bn254", "ronk_ntt_inverse_bn254"):
        t = getattr(L.lib, name)
        assert t(29, None, _p(out)) == L.ERR_INVALID                    # NULL before the 2-adicity (28)
        assert t(29, _p(a), None) == L.ERR_INVALID
        assert t(29, _p(a), _p(out)) == L.ERR_NO_ROOT
        assert _no_device(L, lambda: t(2, _p(a), _p(out)))
    m = L.lib.ronk_poly_mul_bn254
    assert m(None, 2**28, _p(a), 2, _p(out)) == L.ERR_INVALID
    assert m(_p(a), 2**28, None, 2, _p(out)) == L.ERR_INVALID
    assert m(_p(a), 2**28, _p(a), 2, None) == L.ERR_INVALID
    assert m(_p(a), 0, _p(a), 2, _p(out)) == L.ERR_INVALID
    assert m(_p(a), 2, _p(a), 0, _p(out)) == L.ERR_INVALID
    assert m(_p(a), 2**28, _p(a), 2, _p(out)) == L.ERR_UNSUPPORTED      # 2^28 + 1 coefficients: no transform of that size (nothing is read)
    assert _no_device(L, lambda: m(_p(a), 2, _p(a), 2, _p(out)))


def test_trim_workspace_needs_no_device(L):
    assert L.lib.ronk_trim_workspace() == L.OK
