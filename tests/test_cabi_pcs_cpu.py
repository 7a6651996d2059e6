"""Argument errors and sizes of the batched FRI polynomial commitment (ronk_pcs_*, ronk_deep_combine_dev,
ronk_ext2_poly_eval_batch*, ronk_fri_query_indices_dev): all of them are settled before any device work, so this runs without a
GPU."""
import ctypes as C

import pytest

import deep_ref as DR
import poseidon_ref as PR

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
NAMES = ("ronk_pcs_check", "ronk_pcs_proof_words", "ronk_pcs_workspace_words", "ronk_pcs_create", "ronk_pcs_destroy",
         "ronk_ext2_poly_eval_batch_dev", "ronk_ext2_poly_eval_batch", "ronk_deep_combine_dev", "ronk_fri_query_indices_dev",
         "ronk_pcs_commit_dev", "ronk_pcs_open_dev", "ronk_pcs_verify_dev", "ronk_pcs_commit", "ronk_pcs_open", "ronk_pcs_verify")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert hasattr(L, "PcsHandle") and hasattr(L, "ext2_poly_eval_batch")
    from ronkathon_amd import callers
    assert hasattr(callers, "FriPcs")


def test_argument_codes(L):
    """(p, rate, g, w, log2_n, shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_columns, n_points): the codes of
    ronk_fri_check_ext with input_ext = 1 first, then those of the batch"""
    f = L.lib.ronk_pcs_check
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 16, 2) == L.OK
    assert f(GL, 8, 7, 11, 22, 1, 3, 4, 1, 64, 4, 1024, 8) == L.OK
    assert f(MONT, 4, 10, 10, 12, 10, 2, 4, 0, 8, 2, 1, 1) == L.OK
    assert f(GL, 8, 7, 7, 2, 7, 1, 1, 1, 8, 2, 1, 1) == L.OK                # the smallest domain a lane's four points fit
    # the FRI codes come first, whatever the batch says
    assert f(GL, 8, 7, 7, 33, 7, 3, 3, 1, 64, 4, 0, 0) == L.ERR_NO_ROOT
    assert f(GL, 8, 7, 7, 20, 0, 3, 5, 2, 64, 4, 16, 2) == L.ERR_INVALID     # s = 0
    assert f(GL, 8, 7, 7, 20, 7, 3, 9, 2, 64, 4, 16, 2) == L.ERR_UNSUPPORTED   # log2_final > 8
    assert f(GL, 8, 7, 7, 20, 7, 3, 4, 2, 64, 4, 16, 2) == L.ERR_INVALID     # a remainder in the layer count
    # ... then those of the extension
    assert f(GL, 8, 7, 49, 20, 7, 3, 5, 2, 64, 4, 16, 2) == L.ERR_INVALID    # w a square
    assert f(GL, 8, 7, 0, 20, 7, 3, 5, 2, 64, 4, 16, 2) == L.ERR_INVALID
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 1, 16, 2) == L.ERR_INVALID     # a challenge takes two sponge words
    assert f(GL, 8, 7, 49, 20, 7, 3, 5, 2, 64, 4, 2000, 2) == L.ERR_INVALID  # ... before the batch is looked at
    # the batch
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 0, 2) == L.ERR_INVALID      # no column
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 16, 0) == L.ERR_INVALID     # no point
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 0, 9) == L.ERR_INVALID      # invalid before unsupported
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 1025, 2) == L.ERR_UNSUPPORTED
    assert f(GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4, 16, 9) == L.ERR_UNSUPPORTED
    assert f(GL, 8, 7, 7, 1, 7, 1, 0, 0, 8, 2, 1, 1) == L.ERR_UNSUPPORTED    # N = 2: FRI takes it, a lane's four points do not fit


def test_eval_batch_argument_codes(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    f = L.lib.ronk_ext2_poly_eval_batch_dev
    assert f(GL, 7, None, 1, 1, d, 1, d, None) == L.ERR_INVALID
    assert f(GL, 7, d, 0, 1, d, 1, d, None) == L.ERR_INVALID
    assert f(GL, 7, d, 1, 0, d, 1, d, None) == L.ERR_INVALID
    assert f(GL, 7, d, 1, 1, d, 0, d, None) == L.ERR_INVALID
    assert f(GL, 49, d, 1, 1, d, 1, d, None) == L.ERR_INVALID            # w a square
    assert f(2, 1, d, 1, 1, d, 1, d, None) == L.ERR_UNSUPPORTED          # p = 2
    assert f(GL - 2, 7, d, 1, 1, d, 1, d, None) == L.ERR_NOT_PRIME
    assert f(GL, 7, d, 1, 1, d, 9, d, None) == L.ERR_UNSUPPORTED         # more than 8 points
    assert L.lib.ronk_ext2_poly_eval_batch(GL, 7, d, 1, 1, d, 9, d) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_ext2_poly_eval_batch(GL, 7, d, 1, 1, None, 1, d) == L.ERR_INVALID
    # the host form in the order of the _dev form: pointers and counts, the field, the limits
    assert L.lib.ronk_ext2_poly_eval_batch(GL - 2, 7, d, 0, 1, d, 1, d) == L.ERR_INVALID
    assert L.lib.ronk_ext2_poly_eval_batch(GL - 2, 7, d, 1, 1, d, 9, d) == L.ERR_NOT_PRIME
    assert L.lib.ronk_ext2_poly_eval_batch(GL, 49, d, 1, 1, d, 1, d) == L.ERR_INVALID
    assert f(GL - 2, 7, d, 0, 1, d, 1, d, None) == L.ERR_INVALID and f(GL - 2, 7, d, 1, 1, d, 9, d, None) == L.ERR_NOT_PRIME


def test_null_arguments(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    h = C.c_void_p()
    st = C.c_int(5)
    assert L.lib.ronk_pcs_create(None, d, 7, 7, 12, 7, 3, 3, 1, 8, 2, 4, 2) == L.ERR_INVALID
    assert L.lib.ronk_pcs_create(C.byref(h), None, 7, 7, 12, 7, 3, 3, 1, 8, 2, 4, 2) == L.ERR_INVALID and not h.value
    assert L.lib.ronk_pcs_destroy(None) == L.ERR_INVALID
    assert L.lib.ronk_deep_combine_dev(None, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_commit_dev(None, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_open_dev(None, d, d, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_verify_dev(None, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_fri_query_indices_dev(None, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_commit(None, d, d) == L.ERR_INVALID
    assert L.lib.ronk_pcs_open(None, d, d, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_pcs_verify(None, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    # every other pointer of the host forms is required too, and is tested before the handle is read
    assert L.lib.ronk_pcs_commit(d, None, d) == L.ERR_INVALID and L.lib.ronk_pcs_commit(d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_open(d, d, d, None, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_pcs_open(d, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pcs_verify(d, d, None, d, d, C.byref(st)) == L.ERR_INVALID and L.lib.ronk_pcs_verify(d, d, d, d, d, None) == L.ERR_INVALID
    assert st.value == 5


SHAPES = [(6, 1, 2, 8, 2, 1, 1), (9, 3, 3, 8, 2, 5, 2), (12, 2, 4, 5, 3, 33, 3), (12, 3, 3, 64, 4, 16, 2), (20, 3, 5, 64, 4, 16, 2),
          (22, 3, 4, 64, 4, 1024, 8), (2, 1, 1, 1, 2, 1, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_sizes_against_the_restatement(L, shape):
    n, eta, log2_final, q, d, c, k = shape
    S = DR.Pcs(PR.derive_params(GL, 12, 7, 2, 2, 8), 7, 7, n, 7, eta, log2_final, 0, q, d, c, k)
    fri_proof = L.lib.ronk_fri_proof_words_ext(n, eta, log2_final, q, d, 1)
    fri_work = L.lib.ronk_fri_workspace_words_ext(n, eta, log2_final, q, d, 1)
    assert fri_proof == S.F.proof_words() and fri_work == S.F.workspace_words()
    A = 1 << eta
    # claims, the FRI proof, [Q][C A] leaves, [Q][log2 m][D] paths;  a, open status, G, the FRI workspace
    assert L.lib.ronk_pcs_proof_words(*shape) == S.proof_words() == 2 * k * c + fri_proof + q * c * A + q * (n - eta) * d
    assert L.lib.ronk_pcs_workspace_words(*shape) == S.workspace_words() == d + q + (2 << n) + fri_work


def test_sizes_of_refused_shapes(L):
    for shape in ((12, 0, 3, 8, 2, 4, 2), (12, 4, 4, 8, 2, 4, 2), (12, 3, 9, 8, 2, 4, 2), (12, 2, 3, 8, 2, 4, 2), (12, 3, 3, 0, 2, 4, 2),
                  (12, 3, 3, 8, 1, 4, 2), (12, 3, 3, 8, 2, 0, 2), (12, 3, 3, 8, 2, 4, 0), (12, 3, 3, 8, 2, 1025, 2), (12, 3, 3, 8, 2, 4, 9),
                  (1, 1, 0, 8, 2, 1, 1)):
        assert L.lib.ronk_pcs_proof_words(*shape) == 0 and L.lib.ronk_pcs_workspace_words(*shape) == 0, shape


def test_no_device(L):
    """a ronk_pcs handle needs a ronk_poseidon handle: without a GPU the chain ends at the first link with RONK_ERR_NO_DEVICE,
    after the argument checks above"""
    h = C.c_void_p()
    rc, mds = L.arr([1] * 12), L.arr([1] * 9)
    got = L.lib.ronk_poseidon_create(C.byref(h), GL, 3, 5, 2, 2, 2, L.ptr(rc), L.ptr(mds))
    if L.device_count() == 0:
        assert got == L.ERR_NO_DEVICE and not h.value
        d = C.c_void_p(16)
        assert L.lib.ronk_ext2_poly_eval_batch_dev(GL, 7, d, 1, 1, d, 1, d, None) == L.ERR_NO_DEVICE
    else:
        assert got == L.OK
        f = C.c_void_p()
        assert L.lib.ronk_pcs_create(C.byref(f), h, 7, 7, 12, 7, 3, 3, 1, 8, 3, 4, 2) == L.ERR_INVALID and not f.value   # digest_len > rate
        assert L.lib.ronk_pcs_create(C.byref(f), h, 7, 7, 12, 7, 3, 3, 1, 8, 2, 4, 9) == L.ERR_UNSUPPORTED and not f.value
        assert L.lib.ronk_poseidon_destroy(h) == L.OK
