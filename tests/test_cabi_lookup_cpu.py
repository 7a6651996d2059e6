"""Argument errors of the lookup multiplicities and the logUp quotient (ronk_lookup_check, ronk_lookup_mult*,
ronk_logup_quotient*) and the workspace size: all settled by host-side integer logic before any device work, so this runs without
a GPU."""
import ctypes as C

import pytest

import prime_classes as PC

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
NAMES = ("ronk_lookup_workspace_words", "ronk_lookup_check", "ronk_lookup_mult_dev", "ronk_lookup_mult", "ronk_logup_quotient_dev",
         "ronk_logup_quotient")
MAX = 1 << 28


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_workspace_words(L):
    f = L.lib.ronk_lookup_workspace_words
    # two words per slot of a power-of-two capacity of at least 2 T slots (and at least 2)
    assert f(0) == 0 and f(1) == 4 and f(2) == 8 and f(3) == 16 and f(MAX) == 2 * (2 * MAX) and f(MAX + 1) == 0
    assert f(256) == 1024 and f(257) == 2048 and f(1024) == 4096 and f(1025) == 8192        # both sides of a capacity step
    for T in (1, 2, 5, 255, 1000, 2**20 + 1):
        cap = f(T) // 2
        assert cap & (cap - 1) == 0 and 2 * T <= cap < max(4 * T, 3)


def test_check_codes_in_their_order(L):
    f = L.lib.ronk_lookup_check
    assert f(GL, 1, 1, 1) == L.OK and f(MONT, MAX, 16, MAX) == L.OK and f(17, 40, 2, 1000) == L.OK and f(PC.P_32, 5, 3, 7) == L.OK
    # 1. RONK_ERR_INVALID: an empty table, no rows or no columns, whatever else is wrong
    assert f(GL, 0, 1, 1) == L.ERR_INVALID and f(GL, 1, 0, 1) == L.ERR_INVALID and f(GL, 1, 1, 0) == L.ERR_INVALID
    assert f(91, 0, 17, MAX + 1) == L.ERR_INVALID and f(2, MAX + 1, 0, 1) == L.ERR_INVALID
    # 2. RONK_ERR_UNSUPPORTED: more than 2^28 entries or rows, more than 16 columns, before the field's codes
    assert f(GL, MAX + 1, 1, 1) == L.ERR_UNSUPPORTED and f(GL, 1, 1, MAX + 1) == L.ERR_UNSUPPORTED and f(GL, 1, 17, 1) == L.ERR_UNSUPPORTED
    assert f(91, MAX + 1, 1, 1) == L.ERR_UNSUPPORTED and f(0, 1, 17, 1) == L.ERR_UNSUPPORTED
    # 3. the field, as for the base-field scans
    assert f(0, 1, 1, 1) == L.ERR_INVALID and f(1, 1, 1, 1) == L.ERR_INVALID and f(2, 1, 1, 1) == L.ERR_UNSUPPORTED
    assert f(91, 1, 1, 1) == L.ERR_NOT_PRIME and f(2**64 - 1, 4, 2, 8) == L.ERR_NOT_PRIME


def test_mult_codes_in_their_order(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    dev, hst = L.lib.ronk_lookup_mult_dev, L.lib.ronk_lookup_mult
    # dev: p, table, T, vals, C, n, negate, mult, missing, work, stream;  host: .., negate, mult, missing
    ok_dev, ok_hst = [GL, d, 4, d, 2, 8, 0, d, d, d, None], [GL, d, 4, d, 2, 8, 0, d, d]
    for fn, ok, pointers in ((dev, ok_dev, (1, 3, 7, 8, 9)), (hst, ok_hst, (1, 3, 7, 8))):
        # 1. RONK_ERR_INVALID: a NULL pointer (d_missing is required) or an empty shape, before everything else
        for k in pointers:
            args = list(ok); args[k] = None; args[0] = 91; args[2] = MAX + 1; args[6] = 5
            assert fn(*args) == L.ERR_INVALID, k
        for k in (2, 4, 5):
            args = list(ok); args[k] = 0; args[0] = 91
            assert fn(*args) == L.ERR_INVALID, k
        # 2. RONK_ERR_UNSUPPORTED: the limits, before the field and negate
        for k, v in ((2, MAX + 1), (5, MAX + 1), (4, 17)):
            args = list(ok); args[k] = v; args[0] = 91; args[6] = 5
            assert fn(*args) == L.ERR_UNSUPPORTED, k
        # 3. the field, before negate
        for p, code in ((0, L.ERR_INVALID), (2, L.ERR_UNSUPPORTED), (91, L.ERR_NOT_PRIME), (2**64 - 1, L.ERR_NOT_PRIME)):
            args = list(ok); args[0] = p; args[6] = 5
            assert fn(*args) == code, p
        # 4. negate is 0 or 1
        for bad in (2, -1, 256):
            args = list(ok); args[6] = bad
            assert fn(*args) == L.ERR_INVALID, bad


def test_quotient_codes(L):
    d, h = C.c_void_p(16), C.c_void_p(32)   # never dereferenced: refused first
    dev, hst = L.lib.ronk_logup_quotient_dev, L.lib.ronk_logup_quotient
    # h, vals, mult, C, S, alpha, lambda, T_in, T_out[, stream]
    for fn, ok in ((dev, [h, d, d, 2, d, d, d, d, d, None]), (hst, [h, d, d, 2, d, d, d, d, d])):
        for k in (0, 1, 4, 5, 6, 8):                       # d_mult (2) and d_T_in (7) may be NULL; nothing else
            args = list(ok); args[k] = None; args[3] = 17
            assert fn(*args) == L.ERR_INVALID, k
        args = list(ok); args[3] = 0
        assert fn(*args) == L.ERR_INVALID
        for n_columns in (17, 2**32 - 1):
            args = list(ok); args[3] = n_columns; args[2] = None; args[7] = None
            assert fn(*args) == L.ERR_UNSUPPORTED


def test_no_device(L):
    """the multiplicities need a device: RONK_ERR_NO_DEVICE without one, after the argument checks"""
    if L.device_count() != 0:     # the GPU suite covers the rest
        return
    import numpy as np
    t, v = np.arange(4, dtype=np.uint64), np.arange(8, dtype=np.uint64)
    m, miss = np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert L.lib.ronk_lookup_mult(GL, L.ptr(t), 4, L.ptr(v), 1, 8, 0, L.ptr(m), L.ptr(miss)) == L.ERR_NO_DEVICE
    d = C.c_void_p(16)
    assert L.lib.ronk_lookup_mult_dev(GL, d, 4, d, 1, 8, 1, d, d, d, None) == L.ERR_NO_DEVICE
