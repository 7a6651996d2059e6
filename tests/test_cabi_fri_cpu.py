"""Argument errors and sizes of the FRI entry points (ronk_fri_*): all of them are settled before any device work, so this runs
without a GPU."""
import ctypes as C

import pytest

import fri_ref as FR
import poseidon_ref as PR

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
NAMES = ("ronk_fri_check", "ronk_fri_proof_words", "ronk_fri_workspace_words", "ronk_fri_create", "ronk_fri_destroy", "ronk_fri_fold_dev",
         "ronk_fri_prove_dev", "ronk_fri_verify_dev", "ronk_fri_prove", "ronk_fri_verify")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_argument_codes(L):
    """(p, rate, g, log2_n, shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len)"""
    f = L.lib.ronk_fri_check
    assert f(GL, 8, 7, 20, 7, 3, 5, 2, 64, 4) == L.OK
    assert f(GL, 8, 7, 32, 1, 3, 8, 8, 1, 8) == L.OK
    assert f(MONT, 4, 10, 34, 10, 2, 8, 0, 1 << 16, 1) == L.OK
    assert f(GL, 8, 7, 33, 7, 3, 3, 1, 64, 4) == L.ERR_NO_ROOT          # 2^33 does not divide p - 1
    assert f(MONT, 8, 10, 35, 7, 3, 5, 1, 64, 4) == L.ERR_NO_ROOT
    assert f(101, 8, 2, 3, 2, 1, 0, 0, 4, 1) == L.ERR_NO_ROOT           # 100 = 4 * 25
    assert f(GL, 8, 7, 64, 7, 3, 1, 1, 64, 4) == L.ERR_NO_ROOT
    assert f(GL, 8, 7, 20, 0, 3, 5, 2, 64, 4) == L.ERR_INVALID          # s = 0
    assert f(GL, 8, 7, 20, GL, 3, 5, 2, 64, 4) == L.ERR_INVALID         # s = 0 (mod p)
    assert f(GL, 8, 7, 20, 7, 3, 9, 2, 64, 4) == L.ERR_UNSUPPORTED      # log2_final > 8
    assert f(GL, 8, 7, 20, 7, 3, 5, 2, (1 << 16) + 1, 4) == L.ERR_UNSUPPORTED
    assert f(GL, 8, 7, 20, 7, 0, 5, 2, 64, 4) == L.ERR_INVALID          # arity 1
    assert f(GL, 8, 7, 20, 7, 4, 4, 2, 64, 4) == L.ERR_INVALID          # arity 16
    assert f(GL, 8, 7, 20, 7, 3, 4, 2, 64, 4) == L.ERR_INVALID          # 16 layers' bits do not split in threes
    assert f(GL, 8, 7, 5, 7, 3, 5, 2, 64, 4) == L.ERR_INVALID           # no committed layer
    assert f(GL, 8, 7, 20, 7, 3, 5, 6, 64, 4) == L.ERR_INVALID          # blowup beyond the final layer
    assert f(GL, 8, 7, 20, 7, 3, 5, 2, 0, 4) == L.ERR_INVALID           # no query
    assert f(GL, 8, 7, 20, 7, 3, 5, 2, 64, 0) == L.ERR_INVALID
    assert f(GL, 8, 7, 20, 7, 3, 5, 2, 64, 9) == L.ERR_INVALID          # digest_len > rate
    assert f(GL, 8, 49, 20, 7, 3, 5, 2, 64, 4) == L.ERR_INVALID         # a square has not the full power-of-two order
    assert f(100, 8, 7, 2, 7, 1, 0, 0, 4, 1) == L.ERR_INVALID           # an even modulus


def test_null_arguments(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    h = C.c_void_p()
    assert L.lib.ronk_fri_create(None, d, 7, 12, 7, 3, 3, 1, 8, 2) == L.ERR_INVALID
    assert L.lib.ronk_fri_create(C.byref(h), None, 7, 12, 7, 3, 3, 1, 8, 2) == L.ERR_INVALID and not h.value
    assert L.lib.ronk_fri_destroy(None) == L.ERR_INVALID
    assert L.lib.ronk_fri_fold_dev(None, 0, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_fri_prove_dev(None, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_fri_verify_dev(None, d, d, d, None) == L.ERR_INVALID
    st = C.c_int(5)
    assert L.lib.ronk_fri_prove(None, d, d, d) == L.ERR_INVALID
    assert L.lib.ronk_fri_verify(None, d, d, C.byref(st)) == L.ERR_INVALID
    # every other pointer of the host forms is required too, and is tested before the handle is read
    assert L.lib.ronk_fri_prove(d, None, d, d) == L.ERR_INVALID and L.lib.ronk_fri_prove(d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_fri_verify(d, d, None, C.byref(st)) == L.ERR_INVALID and L.lib.ronk_fri_verify(d, d, d, None) == L.ERR_INVALID
    assert st.value == 5


@pytest.mark.parametrize("shape", [(6, 1, 2, 8, 2), (9, 3, 3, 8, 2), (12, 2, 4, 5, 3), (12, 3, 3, 64, 4), (24, 3, 3, 64, 4), (3, 3, 0, 1, 1),
                                   (20, 2, 8, 100, 8)])
def test_sizes_against_the_layout_formula(L, shape):
    n, eta, log2_final, q, d = shape
    A, layers = 1 << eta, (n - log2_final) // eta
    size = [1 << (n - eta * l) for l in range(layers + 1)]
    depth = [n - eta * (l + 1) for l in range(layers)]
    proof = layers * d + size[layers] + sum(q * A + q * depth[l] * d for l in range(layers))
    work = sum(size[l + 1] + L.merkle_tree_words(size[l] // A, d) for l in range(layers)) + layers + (layers + 2) * d + layers * q + q
    assert L.lib.ronk_fri_proof_words(n, eta, log2_final, q, d) == proof
    assert L.lib.ronk_fri_workspace_words(n, eta, log2_final, q, d) == work
    F = FR.Fri(PR.derive_params(GL, 12, 7, 2, 2, 8), 7, n, 7, eta, log2_final, 0, q, d)
    assert F.proof_words() == proof and F.workspace_words() == work


def test_sizes_of_refused_shapes(L):
    for shape in ((12, 0, 3, 8, 2), (12, 4, 4, 8, 2), (12, 3, 9, 8, 2), (12, 2, 3, 8, 2), (2, 3, 0, 8, 2), (12, 3, 3, 0, 2), (12, 3, 3, 8, 0)):
        assert L.lib.ronk_fri_proof_words(*shape) == 0 and L.lib.ronk_fri_workspace_words(*shape) == 0


def test_no_device(L):
    """every compute call needs a ronk_fri handle, and that a ronk_poseidon handle: without a GPU the chain ends at the first link
    with RONK_ERR_NO_DEVICE, after the argument checks above"""
    h = C.c_void_p()
    rc, mds = L.arr([1] * 20), L.arr([1] * 4)
    got = L.lib.ronk_poseidon_create(C.byref(h), GL, 2, 5, 2, 2, 1, L.ptr(rc), L.ptr(mds))
    if L.device_count() == 0:
        assert got == L.ERR_NO_DEVICE and not h.value
    else:
        assert got == L.OK
        f = C.c_void_p()
        assert L.lib.ronk_fri_create(C.byref(f), h, 7, 12, 7, 3, 3, 1, 8, 2) == L.ERR_INVALID and not f.value   # digest_len > rate
        assert L.lib.ronk_poseidon_destroy(h) == L.OK
