"""Argument errors and sizes of the quadratic-extension entry points (ronk_ext2_*) and of FRI with extension challenges
(ronk_fri_*_ext): all of them are settled before any device work, so this runs without a GPU."""
import ctypes as C

import pytest

import fri_ext_ref as FX
import poseidon_ref as PR

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
VEC3 = ("ronk_ext2_vec_add", "ronk_ext2_vec_sub", "ronk_ext2_vec_mul", "ronk_ext2_vec_mul_base")
NAMES = ("ronk_ext2_check", "ronk_ext2_vec_neg", "ronk_ext2_vec_pow", "ronk_ext2_vec_inv", "ronk_fri_check_ext",
         "ronk_fri_proof_words_ext", "ronk_fri_workspace_words_ext", "ronk_fri_create_ext") + VEC3


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)
    for name in VEC3 + ("ronk_ext2_vec_neg", "ronk_ext2_vec_pow", "ronk_ext2_vec_inv"):
        assert name + "_dev" in L.EXPORTS and hasattr(L.lib, name + "_dev")


def test_ext2_check_codes(L):
    f = L.lib.ronk_ext2_check
    assert f(101, 99) == L.OK and f(GL, 7) == L.OK and f(MONT, 10) == L.OK and f(101, 99 + 101) == L.OK
    assert f(2, 1) == L.ERR_UNSUPPORTED
    assert f(91, 3) == L.ERR_NOT_PRIME and f(GL - 2, 7) == L.ERR_NOT_PRIME and f(100, 3) == L.ERR_NOT_PRIME
    assert f(101, 0) == L.ERR_INVALID and f(101, 101) == L.ERR_INVALID       # w = 0 (mod p)
    assert f(101, 4) == L.ERR_INVALID and f(GL, 49) == L.ERR_INVALID         # a quadratic residue
    assert f(101, 1) == L.ERR_INVALID and f(0, 1) == L.ERR_INVALID


def test_fri_check_ext_codes(L):
    """(p, rate, g, w, log2_n, shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, input_ext)"""
    f = L.lib.ronk_fri_check_ext
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 0) == L.OK
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 2, 1) == L.OK
    assert f(MONT, 4, 10, 10, 34, 10, 2, 8, 0, 1 << 16, 2, 1) == L.OK
    # the codes of ronk_fri_check
    assert f(GL, 8, 7, 7, 33, 7, 3, 3, 1, 64, 4, 0) == L.ERR_NO_ROOT
    assert f(GL, 8, 7, 7, 20, 0, 3, 5, 2, 64, 4, 0) == L.ERR_INVALID            # s = 0
    assert f(GL, 8, 7, 7, 20, 7, 3, 9, 2, 64, 4, 0) == L.ERR_UNSUPPORTED        # log2_final > 8
    assert f(GL, 8, 7, 7, 20, 7, 4, 4, 2, 64, 4, 0) == L.ERR_INVALID            # arity 16
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 9, 0) == L.ERR_INVALID            # digest_len > rate
    assert f(GL, 8, 49, 7, 20, 7, 3, 5, 2, 64, 4, 0) == L.ERR_INVALID           # g without the full power-of-two order
    # the codes of ronk_ext2_check
    assert f(GL, 8, 7, 49, 20, 7, 3, 5, 2, 64, 4, 0) == L.ERR_INVALID           # w a residue
    assert f(GL, 8, 7, 0, 20, 7, 3, 5, 2, 64, 4, 0) == L.ERR_INVALID            # w = 0
    assert f(GL, 8, 7, GL, 20, 7, 3, 5, 2, 64, 4, 0) == L.ERR_INVALID           # w = 0 (mod p)
    assert f(0xC0000001 * 3 - 2, 8, 7, 7, 4, 7, 1, 2, 1, 4, 2, 0) == L.ERR_NOT_PRIME   # 9663676417 = 73 * 132379129; 2^4 | p - 1
    # its own
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 1, 0) == L.ERR_INVALID            # a challenge takes two sponge words
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 2) == L.ERR_INVALID            # input_ext is 0 or 1


def test_null_arguments(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    h = C.c_void_p()
    assert L.lib.ronk_fri_create_ext(None, d, 7, 7, 12, 7, 3, 3, 1, 8, 2, 0) == L.ERR_INVALID
    assert L.lib.ronk_fri_create_ext(C.byref(h), None, 7, 7, 12, 7, 3, 3, 1, 8, 2, 0) == L.ERR_INVALID and not h.value
    for name in VEC3:
        assert getattr(L.lib, name)(GL, 7, None, d, d, 4) == L.ERR_INVALID
        assert getattr(L.lib, name + "_dev")(GL, 7, d, d, None, 4, None) == L.ERR_INVALID
    assert L.lib.ronk_ext2_vec_neg(GL, 7, None, d, 4) == L.ERR_INVALID
    assert L.lib.ronk_ext2_vec_pow_dev(GL, 7, d, 3, None, 4, None) == L.ERR_INVALID
    assert L.lib.ronk_ext2_vec_inv_dev(GL, 7, None, d, 4, None, None) == L.ERR_INVALID


def test_host_form_precedence(L):
    """a missing pointer is reported before the field, the field before the device; every host form goes through one helper"""
    d = C.c_void_p(16)   # never dereferenced: refused first
    for name in VEC3:
        f = getattr(L.lib, name)
        assert f(91, 3, d, None, d, 4) == L.ERR_INVALID and f(91, 3, d, d, None, 4) == L.ERR_INVALID     # the second operand, out
        assert f(91, 3, d, d, d, 4) == L.ERR_NOT_PRIME and f(2, 1, d, d, d, 4) == L.ERR_UNSUPPORTED
    for f, extra in ((L.lib.ronk_ext2_vec_neg, ()), (L.lib.ronk_ext2_vec_pow, (5,)), (L.lib.ronk_ext2_vec_inv, ())):
        assert f(91, 3, None, *extra, d, 4) == L.ERR_INVALID and f(91, 3, d, *extra, None, 4) == L.ERR_INVALID
        assert f(91, 3, d, *extra, d, 4) == L.ERR_NOT_PRIME and f(2, 1, d, *extra, d, 4) == L.ERR_UNSUPPORTED
        assert f(GL, 49, d, *extra, d, 4) == L.ERR_INVALID                                                # w a residue


@pytest.mark.parametrize("input_ext", [0, 1])
@pytest.mark.parametrize("shape", [(6, 1, 2, 8, 2), (9, 3, 3, 8, 2), (12, 2, 4, 5, 3), (12, 3, 3, 64, 4), (24, 3, 3, 64, 4), (3, 3, 0, 1, 2),
                                   (20, 2, 8, 100, 8)])
def test_sizes_against_the_restatement(L, shape, input_ext):
    n, eta, log2_final, q, d = shape
    F = FX.FriExt(PR.derive_params(GL, 12, 7, 2, 2, 8), 7, 7, n, 7, eta, log2_final, 0, q, d, input_ext)
    assert L.lib.ronk_fri_proof_words_ext(n, eta, log2_final, q, d, input_ext) == F.proof_words()
    assert L.lib.ronk_fri_workspace_words_ext(n, eta, log2_final, q, d, input_ext) == F.workspace_words()
    # the header's formulas
    A, layers = 1 << eta, (n - log2_final) // eta
    size = [1 << (n - eta * l) for l in range(layers + 1)]
    depth = [n - eta * (l + 1) for l in range(layers)]
    leaf = [(2 if l or input_ext else 1) * A for l in range(layers)]
    assert F.proof_words() == layers * d + 2 * size[layers] + sum(q * (leaf[l] + depth[l] * d) for l in range(layers))
    assert F.workspace_words() == (sum(2 * size[l + 1] + L.merkle_tree_words(size[l] // A, d) for l in range(layers))
                                   + 2 * layers + (layers + 2) * d + layers * q + q)


def test_sizes_of_refused_shapes(L):
    for shape in ((12, 0, 3, 8, 2, 0), (12, 4, 4, 8, 2, 0), (12, 3, 9, 8, 2, 0), (12, 2, 3, 8, 2, 0), (2, 3, 0, 8, 2, 0), (12, 3, 3, 0, 2, 0),
                  (12, 3, 3, 8, 0, 0), (12, 3, 3, 8, 1, 0), (12, 3, 3, 8, 2, 2)):
        assert L.lib.ronk_fri_proof_words_ext(*shape) == 0 and L.lib.ronk_fri_workspace_words_ext(*shape) == 0


def test_no_device(L):
    """the compute entry points check their arguments, then need a device: RONK_ERR_NO_DEVICE without one"""
    a = L.arr([1, 2, 3, 4])
    out = L.arr([0, 0, 0, 0])
    if L.device_count() != 0:     # the GPU suite covers the compute entry points; the argument check still comes first
        for name in VEC3:
            assert getattr(L.lib, name)(GL, 49, L.ptr(a), L.ptr(a), L.ptr(out), 2) == L.ERR_INVALID
        return
    for name in VEC3:
        assert getattr(L.lib, name)(GL, 7, L.ptr(a), L.ptr(a), L.ptr(out), 2) == L.ERR_NO_DEVICE
        assert getattr(L.lib, name + "_dev")(GL, 7, L.ptr(a), L.ptr(a), L.ptr(out), 2, None) == L.ERR_NO_DEVICE
        assert getattr(L.lib, name)(GL, 49, L.ptr(a), L.ptr(a), L.ptr(out), 2) == L.ERR_INVALID      # the argument check comes first
    assert L.lib.ronk_ext2_vec_neg(101, 99, L.ptr(a), L.ptr(out), 2) == L.ERR_NO_DEVICE
    assert L.lib.ronk_ext2_vec_pow(101, 99, L.ptr(a), 5, L.ptr(out), 2) == L.ERR_NO_DEVICE
    assert L.lib.ronk_ext2_vec_inv(101, 99, L.ptr(a), L.ptr(out), 2) == L.ERR_NO_DEVICE
    assert L.lib.ronk_ext2_vec_inv_dev(101, 99, L.ptr(a), L.ptr(out), 2, None, None) == L.ERR_NO_DEVICE
    assert out.tolist() == [0, 0, 0, 0]
    h = C.c_void_p()
    rc, mds = L.arr([1] * 20), L.arr([1] * 4)
    assert L.lib.ronk_poseidon_create(C.byref(h), GL, 2, 5, 2, 2, 1, L.ptr(rc), L.ptr(mds)) == L.ERR_NO_DEVICE and not h.value
