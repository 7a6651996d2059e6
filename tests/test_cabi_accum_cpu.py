"""Argument errors and the size function of the scans and accumulators (ronk_vec_prefix_*, ronk_ext2_vec_prefix_*,
ronk_perm_product*, ronk_logup_sum*, ronk_accum_check): all of them are settled before any device work, so this runs without a
GPU."""
import ctypes as C

import pytest

GL, MONT = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001
BIG = (1 << 28) + 1
BASE = ("ronk_vec_prefix_prod", "ronk_vec_prefix_sum")
EXT = ("ronk_ext2_vec_prefix_prod", "ronk_ext2_vec_prefix_sum")
NAMES = BASE + EXT + ("ronk_perm_product", "ronk_logup_sum")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name) and name + "_dev" in L.EXPORTS and hasattr(L.lib, name + "_dev")
    for name in ("ronk_scan_workspace_words", "ronk_accum_check"):
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_workspace_words(L):
    f = L.lib.ronk_scan_workspace_words
    assert f(0) == 0 and f(BIG) == 0 and f(1 << 40) == 0
    # three words per block of 2048 elements: two planes of totals, one of flags
    for n in (1, 2047, 2048, 2049, 1 << 19, (1 << 19) + 1, 1 << 28):
        assert f(n) == 3 * ((n + 2047) // 2048), n
    assert f(1 << 28) * 8 <= 4 << 20, "a few MiB at the largest size"


def test_accum_check_codes(L):
    f = L.lib.ronk_accum_check
    assert f(GL, 7, 3, 1 << 20) == L.OK and f(MONT, 10, 16, 1 << 28) == L.OK and f(17, 3, 1, 1) == L.OK
    # the codes of ronk_ext2_check come first
    assert f(2, 1, 3, 4) == L.ERR_UNSUPPORTED
    assert f(91, 3, 3, 4) == L.ERR_NOT_PRIME and f(GL - 2, 7, 0, 0) == L.ERR_NOT_PRIME
    assert f(GL, 49, 3, 4) == L.ERR_INVALID and f(GL, 0, 17, 4) == L.ERR_INVALID and f(0, 1, 3, 4) == L.ERR_INVALID
    # then its own
    assert f(GL, 7, 0, 4) == L.ERR_INVALID and f(GL, 7, 3, 0) == L.ERR_INVALID
    assert f(GL, 7, 0, BIG) == L.ERR_INVALID                                   # INVALID before UNSUPPORTED
    assert f(GL, 7, 17, 4) == L.ERR_UNSUPPORTED and f(GL, 7, 16, BIG) == L.ERR_UNSUPPORTED


def test_scan_argument_errors(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    for name in BASE:
        dev, hst = getattr(L.lib, name + "_dev"), getattr(L.lib, name)
        assert dev(GL, None, d, 4, 0, None, d, None) == L.ERR_INVALID
        assert dev(GL, d, None, 4, 0, None, d, None) == L.ERR_INVALID
        assert dev(GL, d, d, 4, 0, None, None, None) == L.ERR_INVALID           # the workspace is required
        assert dev(GL, d, d, 0, 0, None, d, None) == L.ERR_INVALID
        assert dev(GL, d, d, 4, 2, None, d, None) == L.ERR_INVALID and dev(GL, d, d, 4, -1, None, d, None) == L.ERR_INVALID
        assert dev(GL, d, d, BIG, 0, None, d, None) == L.ERR_UNSUPPORTED
        assert dev(2, d, d, 4, 0, None, d, None) == L.ERR_UNSUPPORTED
        assert dev(91, d, d, 4, 1, d, d, None) == L.ERR_NOT_PRIME and dev(1, d, d, 4, 1, d, d, None) == L.ERR_INVALID
        assert hst(GL, None, d, 4, 0, None) == L.ERR_INVALID and hst(GL, d, None, 4, 0, None) == L.ERR_INVALID
        assert hst(GL, d, d, 0, 0, None) == L.ERR_INVALID and hst(GL, d, d, 4, 3, None) == L.ERR_INVALID
        assert hst(GL, d, d, BIG, 0, None) == L.ERR_UNSUPPORTED and hst(91, d, d, 4, 0, None) == L.ERR_NOT_PRIME
    for name in EXT:
        dev, hst = getattr(L.lib, name + "_dev"), getattr(L.lib, name)
        assert dev(GL, 7, None, d, 4, 0, None, d, None) == L.ERR_INVALID
        assert dev(GL, 7, d, d, 4, 0, None, None, None) == L.ERR_INVALID
        assert dev(GL, 7, d, d, 0, 1, None, d, None) == L.ERR_INVALID
        assert dev(GL, 7, d, d, 4, 2, None, d, None) == L.ERR_INVALID
        assert dev(GL, 7, d, d, BIG, 0, None, d, None) == L.ERR_UNSUPPORTED
        assert dev(GL, 49, d, d, 4, 0, None, d, None) == L.ERR_INVALID          # w a residue
        assert dev(2, 1, d, d, 4, 0, None, d, None) == L.ERR_UNSUPPORTED and dev(91, 3, d, d, 4, 0, None, d, None) == L.ERR_NOT_PRIME
        assert hst(GL, 7, None, d, 4, 0, None) == L.ERR_INVALID and hst(GL, 7, d, d, 4, 2, None) == L.ERR_INVALID
        assert hst(GL, 7, d, d, BIG, 0, None) == L.ERR_UNSUPPORTED and hst(GL, 49, d, d, 4, 0, None) == L.ERR_INVALID
    # the host forms report the arguments' codes before the field's, the _dev forms likewise
    for name in BASE:
        hst = getattr(L.lib, name)
        assert hst(91, None, d, 4, 0, None) == L.ERR_INVALID and hst(91, d, d, 4, 2, None) == L.ERR_INVALID
        assert hst(91, d, d, BIG, 0, None) == L.ERR_UNSUPPORTED and hst(2, d, d, 4, 0, None) == L.ERR_UNSUPPORTED
    for name in EXT:
        hst = getattr(L.lib, name)
        assert hst(91, 3, d, None, 4, 0, None) == L.ERR_INVALID and hst(91, 3, d, d, 0, 0, None) == L.ERR_INVALID
        assert hst(91, 3, d, d, BIG, 0, None) == L.ERR_UNSUPPORTED and hst(91, 3, d, d, 4, 0, None) == L.ERR_NOT_PRIME


def test_accumulator_argument_errors(L):
    d = C.c_void_p(16)
    st = C.c_int(7)
    perm, logup = L.lib.ronk_perm_product_dev, L.lib.ronk_logup_sum_dev
    ok = [GL, 7, d, d, d, 3, 8, d, d, d, d, d, d, None]
    for k in (2, 3, 4, 7, 8, 9, 10, 11, 12):                                  # every pointer is required
        args = list(ok); args[k] = None
        assert perm(*args) == L.ERR_INVALID, k
    for k, v, code in ((5, 0, L.ERR_INVALID), (6, 0, L.ERR_INVALID), (5, 17, L.ERR_UNSUPPORTED), (6, BIG, L.ERR_UNSUPPORTED),
                       (1, 49, L.ERR_INVALID), (0, 91, L.ERR_NOT_PRIME), (0, 2, L.ERR_UNSUPPORTED)):
        args = list(ok); args[k] = v
        assert perm(*args) == code, (k, v)
    ok = [GL, 7, d, d, 2, 8, d, d, d, d, d, None]
    for k in (2, 6, 7, 8, 9, 10):                                              # d_mult (3) may be NULL
        args = list(ok); args[k] = None
        assert logup(*args) == L.ERR_INVALID, k
    for k, v, code in ((4, 0, L.ERR_INVALID), (5, 0, L.ERR_INVALID), (4, 17, L.ERR_UNSUPPORTED), (5, BIG, L.ERR_UNSUPPORTED),
                       (1, 49, L.ERR_INVALID), (0, 91, L.ERR_NOT_PRIME)):
        args = list(ok); args[k] = v
        assert logup(*args) == code, (k, v)
    # the host forms
    assert L.lib.ronk_perm_product(GL, 7, d, d, d, 3, 8, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_perm_product(GL, 7, d, d, d, 0, 8, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_perm_product(GL, 7, d, d, d, 17, 8, d, d, d, d, C.byref(st)) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_logup_sum(GL, 7, None, None, 2, 8, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_logup_sum(GL, 7, d, None, 2, BIG, d, d, d, C.byref(st)) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_logup_sum(GL, 49, d, None, 2, 8, d, d, d, C.byref(st)) == L.ERR_INVALID
    # a missing pointer before the field, the field before the shape (the order of ronk_accum_check)
    assert L.lib.ronk_perm_product(91, 3, d, d, d, 3, 8, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_perm_product(91, 3, d, d, d, 17, 8, d, d, d, d, C.byref(st)) == L.ERR_NOT_PRIME
    assert L.lib.ronk_logup_sum(91, 3, d, None, 2, 8, None, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_logup_sum(91, 3, d, None, 2, BIG, d, d, d, C.byref(st)) == L.ERR_NOT_PRIME
    assert st.value == 7


def test_no_device(L):
    """the compute entry points check their arguments, then need a device: RONK_ERR_NO_DEVICE without one"""
    a, out, work = L.arr([1, 2, 3, 4]), L.arr([0, 0, 0, 0]), L.arr([0] * 3)
    st = C.c_int(7)
    if L.device_count() != 0:     # the GPU suite covers the compute entry points; the argument check still comes first
        assert L.lib.ronk_vec_prefix_sum(GL, L.ptr(a), L.ptr(out), 4, 2, None) == L.ERR_INVALID
        assert L.lib.ronk_logup_sum(17, 4, L.ptr(a), None, 2, 2, L.ptr(a), L.ptr(out), L.ptr(out), C.byref(st)) == L.ERR_INVALID
        return
    for name in BASE:
        assert getattr(L.lib, name)(GL, L.ptr(a), L.ptr(out), 4, 0, None) == L.ERR_NO_DEVICE
        assert getattr(L.lib, name + "_dev")(GL, L.ptr(a), L.ptr(out), 4, 0, None, L.ptr(work), None) == L.ERR_NO_DEVICE
    for name in EXT:
        assert getattr(L.lib, name)(17, 3, L.ptr(a), L.ptr(out), 2, 1, None) == L.ERR_NO_DEVICE
        assert getattr(L.lib, name + "_dev")(17, 3, L.ptr(a), L.ptr(out), 2, 1, None, L.ptr(work), None) == L.ERR_NO_DEVICE
    assert L.lib.ronk_perm_product(17, 3, L.ptr(a), L.ptr(a), L.ptr(a), 2, 2, L.ptr(a), L.ptr(a), L.ptr(out), L.ptr(out),
                                   C.byref(st)) == L.ERR_NO_DEVICE
    assert L.lib.ronk_logup_sum(17, 3, L.ptr(a), None, 2, 2, L.ptr(a), L.ptr(out), L.ptr(out), C.byref(st)) == L.ERR_NO_DEVICE
    assert out.tolist() == [0, 0, 0, 0] and st.value == 7
