"""Argument errors of the PLONK quotient (ronk_plonk_check, ronk_plonk_create, ronk_plonk_quotient*, ronk_plonk_destroy): all of
them are settled by host-side integer logic before any device work, so this runs without a GPU."""
import ctypes as C

import pytest

import prime_classes as PC

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
NAMES = ("ronk_plonk_check", "ronk_plonk_create", "ronk_plonk_destroy", "ronk_plonk_quotient_dev", "ronk_plonk_quotient")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def labels(*k):
    return (C.c_uint64 * 3)(*k)


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_check_codes_in_their_order(L):
    f = L.lib.ronk_plonk_check
    K = labels(1, 2, 3)
    assert f(GL, 7, 7, 10, 2, 7, K) == L.OK and f(GL, 7, 11, 1, 0, 7, K) == L.OK and f(MONT, 10, 10, 26, 2, 10, K) == L.OK
    assert f(GL, 7, 7, 20, 8, 7, labels(GL - 1, 5, 2**64 - 1)) == L.OK
    # 1. the codes of ronk_ext2_check, whatever else is wrong
    assert f(2, 1, 1, 0, 0, 0, None) == L.ERR_UNSUPPORTED
    assert f(91, 3, 3, 0, 40, 0, None) == L.ERR_NOT_PRIME
    assert f(GL, 7, 49, 0, 40, 0, None) == L.ERR_INVALID and f(GL, 7, 0, 4, 2, 7, K) == L.ERR_INVALID and f(0, 7, 7, 4, 2, 7, K) == L.ERR_INVALID
    # 2. RONK_ERR_INVALID: the shift or a label multiplier is zero (mod p), before NO_ROOT and UNSUPPORTED
    assert f(GL, 7, 7, 4, 2, 0, K) == L.ERR_INVALID and f(GL, 7, 7, 4, 2, GL, K) == L.ERR_INVALID
    for bad in (labels(0, 2, 3), labels(1, GL, 3), labels(1, 2, 0)):
        assert f(GL, 7, 7, 4, 2, 7, bad) == L.ERR_INVALID
        assert f(GL, 7, 7, 30, 10, 7, bad) == L.ERR_INVALID and f(GL, 7, 7, 0, 2, 7, bad) == L.ERR_INVALID
    assert f(GL, 7, 7, 4, 2, 7, None) == L.ERR_INVALID
    # 3. RONK_ERR_NO_ROOT: M does not divide p - 1 (Goldilocks: 2^32, MONT_P: 2^34), before UNSUPPORTED
    assert f(GL, 7, 7, 30, 3, 7, K) == L.ERR_NO_ROOT and f(GL, 7, 7, 0, 33, 7, K) == L.ERR_NO_ROOT
    assert f(MONT, 10, 10, 20, 15, 10, K) == L.ERR_NO_ROOT and f(GL, 7, 7, 40, 40, 7, K) == L.ERR_NO_ROOT
    assert f(GL, 7, 7, 2**32 - 1, 2**32 - 1, 7, K) == L.ERR_NO_ROOT
    assert f(17, 3, 3, 4, 1, 3, K) == L.ERR_NO_ROOT
    # 4. RONK_ERR_UNSUPPORTED: no trace rows to speak of, more than 2^28 rows, or s^M = 1
    assert f(GL, 7, 7, 0, 4, 7, K) == L.ERR_UNSUPPORTED
    assert f(GL, 7, 7, 27, 2, 7, K) == L.ERR_UNSUPPORTED and f(GL, 7, 7, 28, 0, 7, K) == L.OK and f(GL, 7, 7, 29, 0, 7, K) == L.ERR_UNSUPPORTED
    assert f(GL, 7, 7, 4, 2, 1, K) == L.ERR_UNSUPPORTED and f(GL, 7, 7, 4, 2, GL - 1, K) == L.ERR_UNSUPPORTED
    w64 = pow(7, (GL - 1) // 64, GL)
    assert f(GL, 7, 7, 4, 2, w64, K) == L.ERR_UNSUPPORTED and f(GL, 7, 7, 4, 1, w64, K) == L.OK      # s^64 = 1, s^32 = -1


def test_f17_has_no_coset_of_sixteen_rows(L):
    """every non-zero s of F_17 has s^16 = 1: some x_i - 1 or x_i^N - 1 always vanishes"""
    f = L.lib.ronk_plonk_check
    K = labels(1, 2, 3)
    for s in range(1, 17):
        for log2_n, log2_b in ((4, 0), (3, 1), (2, 2), (1, 3)):
            assert f(17, 3, 3, log2_n, log2_b, s, K) == L.ERR_UNSUPPORTED
    assert f(17, 3, 3, 2, 1, 3, K) == L.OK and f(17, 3, 3, 2, 1, 2, K) == L.ERR_UNSUPPORTED          # 2^8 = 1, 3^8 = -1
    assert f(17, 3, 3, 2, 1, 0, K) == L.ERR_INVALID and f(17, 3, 3, 2, 1, 17, K) == L.ERR_INVALID


def test_null_pointers(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    h = C.c_void_p(32)
    dev, hst = L.lib.ronk_plonk_quotient_dev, L.lib.ronk_plonk_quotient
    ok = [h, d, d, d, d, d, d, d, d, d, None]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):                 # d_pi (4) may be NULL; nothing else
        args = list(ok); args[k] = None
        assert dev(*args) == L.ERR_INVALID, k
    ok = [h, d, d, d, d, d, d, d, d, d]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        args = list(ok); args[k] = None
        assert hst(*args) == L.ERR_INVALID, k
    assert L.lib.ronk_plonk_destroy(None) == L.ERR_INVALID
    K = labels(1, 2, 3)
    assert L.lib.ronk_plonk_create(None, GL, 7, 7, 4, 2, 7, K) == L.ERR_INVALID
    out = C.c_void_p(99)
    assert L.lib.ronk_plonk_create(C.byref(out), GL, 7, 7, 4, 2, 7, None) == L.ERR_INVALID and not out.value
    # the codes of the check come back from create, with no handle
    for args, code in (((GL, 7, 49, 4, 2, 7, K), L.ERR_INVALID), ((GL, 7, 7, 30, 3, 7, K), L.ERR_NO_ROOT),
                       ((GL, 7, 7, 0, 3, 7, K), L.ERR_UNSUPPORTED), ((17, 3, 3, 3, 1, 3, K), L.ERR_UNSUPPORTED)):
        out = C.c_void_p(99)
        assert L.lib.ronk_plonk_create(C.byref(out), *args) == code and not out.value


def test_no_device(L):
    """a handle needs a device: RONK_ERR_NO_DEVICE without one, after the argument checks"""
    out = C.c_void_p(99)
    K = labels(1, 2, 3)
    if L.device_count() != 0:     # the GPU suite covers the rest
        assert L.lib.ronk_plonk_create(C.byref(out), GL, 7, 7, 4, 2, 7, K) == L.OK and out.value
        assert L.lib.ronk_plonk_destroy(out) == L.OK
        return
    assert L.lib.ronk_plonk_create(C.byref(out), GL, 7, 7, 4, 2, 7, K) == L.ERR_NO_DEVICE and not out.value
