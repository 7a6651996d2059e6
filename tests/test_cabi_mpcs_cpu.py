"""Argument errors and sizes of the multi-matrix polynomial commitment (ronk_mpcs_*): all of them are settled before any device
work, so this runs without a GPU."""
import ctypes as C

import pytest

import mpcs_ref as MR
import poseidon_ref as PR

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
NAMES = ("ronk_mpcs_check", "ronk_mpcs_proof_words", "ronk_mpcs_workspace_words", "ronk_mpcs_create", "ronk_mpcs_destroy",
         "ronk_mpcs_set_pow", "ronk_mpcs_handle_proof_words", "ronk_mpcs_handle_workspace_words", "ronk_mpcs_commit_dev",
         "ronk_mpcs_combine_dev", "ronk_mpcs_open_dev", "ronk_mpcs_verify_dev", "ronk_mpcs_commit", "ronk_mpcs_open", "ronk_mpcs_verify")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def u32s(values):
    return (C.c_uint32 * max(len(values), 1))(*values)


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert hasattr(L, "MpcsHandle")
    from ronkathon_amd import callers
    assert hasattr(callers, "FriMultiPcs")


def check(L, fri, K, Cs, masks, R=None):
    """fri: (p, rate, g, w, log2_n, shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len)"""
    return L.lib.ronk_mpcs_check(*fri, K, len(Cs) if R is None else R, None if Cs is None else u32s(Cs), None if masks is None else u32s(masks))


GOOD = (GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 4)


def test_argument_codes(L):
    """the codes of ronk_fri_check_ext with input_ext = 1 first, then RONK_ERR_INVALID, then RONK_ERR_UNSUPPORTED"""
    assert check(L, GOOD, 2, (8, 3, 2, 8), (1, 1, 3, 1)) == L.OK
    assert check(L, GOOD, 1, (5,), (1,)) == L.OK
    assert check(L, (MONT, 4, 10, 10, 12, 10, 2, 4, 0, 8, 2), 8, (1, 2), (0xFF, 0x80)) == L.OK
    assert check(L, (GL, 8, 7, 7, 2, 7, 1, 1, 1, 8, 2), 1, (1,), (1,)) == L.OK       # the smallest domain a lane's four points fit
    # the FRI codes come first, whatever the rounds say
    assert check(L, (GL, 8, 7, 7, 33, 7, 3, 3, 1, 64, 4), 0, (0,), (0,)) == L.ERR_NO_ROOT
    assert check(L, (GL, 8, 7, 7, 20, 0, 3, 5, 2, 64, 4), 2, (1,), (3,)) == L.ERR_INVALID        # s = 0
    assert check(L, (GL, 8, 7, 7, 20, 7, 3, 9, 2, 64, 4), 2, (1,), (3,)) == L.ERR_UNSUPPORTED    # log2_final > 8
    assert check(L, (GL, 8, 7, 49, 20, 7, 3, 5, 2, 64, 4), 2, (1,), (3,)) == L.ERR_INVALID       # w a square
    assert check(L, (GL, 8, 7, 7, 20, 7, 3, 5, 2, 64, 1), 2, (1,), (3,)) == L.ERR_INVALID        # a challenge takes two sponge words
    assert check(L, (GL, 8, 7, 7, 20, 7, 3, 9, 2, 64, 4), 2, None, None, R=1) == L.ERR_UNSUPPORTED   # ... before the arrays are looked at
    # RONK_ERR_INVALID
    assert check(L, GOOD, 2, None, (3,), R=1) == L.ERR_INVALID
    assert check(L, GOOD, 2, (1,), None) == L.ERR_INVALID
    assert check(L, GOOD, 0, (1,), (1,)) == L.ERR_INVALID                  # no point
    assert check(L, GOOD, 1, (1,), (1,), R=0) == L.ERR_INVALID             # no round
    assert check(L, GOOD, 2, (4, 0), (3, 3)) == L.ERR_INVALID              # a round without columns
    assert check(L, GOOD, 2, (4, 4), (3, 0)) == L.ERR_INVALID              # a round without points
    assert check(L, GOOD, 2, (4, 4), (3, 4)) == L.ERR_INVALID              # a mask >= 2^K
    assert check(L, GOOD, 2, (4, 4), (1, 1)) == L.ERR_INVALID              # a point that no mask selects
    # invalid before unsupported
    assert check(L, GOOD, 9, (4, 0), (511, 1)) == L.ERR_INVALID
    assert check(L, GOOD, 9, (4, 4), (255, 255)) == L.ERR_INVALID          # point 8 is not selected
    assert check(L, GOOD, 1, (1,) * 8 + (0,), (1,) * 9) == L.ERR_INVALID
    assert check(L, GOOD, 2, (1025, 1), (1, 1)) == L.ERR_INVALID
    assert check(L, (GL, 8, 7, 7, 1, 7, 1, 0, 0, 8, 2), 1, (1,), (2,)) == L.ERR_INVALID
    # RONK_ERR_UNSUPPORTED
    assert check(L, GOOD, 9, (4,), (511,)) == L.ERR_UNSUPPORTED
    assert check(L, GOOD, 1, (1,) * 9, (1,) * 9) == L.ERR_UNSUPPORTED
    assert check(L, GOOD, 2, (1000, 25), (3, 1)) == L.ERR_UNSUPPORTED
    assert check(L, (GL, 8, 7, 7, 1, 7, 1, 0, 0, 8, 2), 1, (1,), (1,)) == L.ERR_UNSUPPORTED   # N = 2: a lane's four points do not fit


def test_limits(L):
    """C_tot = 1024 accepted and 1025 refused; R = 8 accepted and 9 refused; K = 8 accepted and 9 refused"""
    assert check(L, GOOD, 2, (1000, 24), (3, 1)) == L.OK and check(L, GOOD, 2, (1000, 25), (3, 1)) == L.ERR_UNSUPPORTED
    assert check(L, GOOD, 1, (1024,), (1,)) == L.OK and check(L, GOOD, 1, (1025,), (1,)) == L.ERR_UNSUPPORTED
    assert check(L, GOOD, 1, (2,) * 8, (1,) * 8) == L.OK and check(L, GOOD, 1, (2,) * 9, (1,) * 9) == L.ERR_UNSUPPORTED
    assert check(L, GOOD, 8, (2,), (255,)) == L.OK and check(L, GOOD, 9, (2,), (511,)) == L.ERR_UNSUPPORTED
    shape = (20, 3, 5, 64, 4)
    for K, Cs, masks, ok in ((2, (1000, 24), (3, 1), True), (2, (1000, 25), (3, 1), False), (1, (2,) * 8, (1,) * 8, True),
                             (1, (2,) * 9, (1,) * 9, False), (9, (2,), (511,), False)):
        words = L.lib.ronk_mpcs_proof_words(*shape, K, len(Cs), u32s(Cs), u32s(masks))
        assert (words != 0) == ok and (L.lib.ronk_mpcs_workspace_words(*shape, K, len(Cs), u32s(Cs), u32s(masks)) != 0) == ok


def test_the_restatement_agrees_on_the_round_codes(L):
    codes = {0: L.OK, "invalid": L.ERR_INVALID, "unsupported": L.ERR_UNSUPPORTED}
    for K, Cs, masks in ((2, (1, 1), (1, 2)), (0, (1,), (1,)), (2, (), ()), (2, (1, 0), (1, 2)), (2, (1, 1), (1, 4)), (2, (1, 1), (1, 0)),
                         (2, (1, 1), (1, 1)), (9, (1,), (511,)), (1, (1,) * 9, (1,) * 9), (1, (1024, 1), (1, 1)), (1, (1023, 1), (1, 1)),
                         (9, (1, 0), (511, 1)), (3, (1, 2, 3), (1, 2, 4))):
        assert check(L, GOOD, K, Cs, masks) == codes[MR.check_shape(K, Cs, masks, 20)], (K, Cs, masks)


def test_null_arguments(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    h = C.c_void_p()
    st = C.c_int(5)
    cs, ms = u32s((4, 2)), u32s((3, 1))
    assert L.lib.ronk_mpcs_create(None, d, 7, 7, 12, 7, 3, 3, 1, 8, 2, 2, 2, cs, ms) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_create(C.byref(h), None, 7, 7, 12, 7, 3, 3, 1, 8, 2, 2, 2, cs, ms) == L.ERR_INVALID and not h.value
    assert L.lib.ronk_mpcs_destroy(None) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_set_pow(None, 4, 10) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_handle_proof_words(None) == 0 and L.lib.ronk_mpcs_handle_workspace_words(None) == 0
    assert L.lib.ronk_mpcs_commit_dev(None, 0, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_combine_dev(None, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_open_dev(None, d, d, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_verify_dev(None, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_commit(None, 0, d, d) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_open(None, d, d, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert L.lib.ronk_mpcs_verify(None, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert st.value == 5


SHAPES = [((6, 1, 2, 8, 2), 1, (1,), (1,)), ((9, 3, 3, 8, 2), 2, (5,), (3,)), ((9, 3, 3, 8, 2), 2, (3, 5), (1, 2)),
          ((12, 2, 4, 5, 3), 2, (33, 1, 2), (3, 1, 3)), ((20, 3, 5, 64, 4), 2, (8, 3, 2, 8), (1, 1, 3, 1)),
          ((22, 3, 4, 64, 4), 8, (1000, 24), (0xFF, 0x80)), ((2, 1, 1, 1, 2), 1, (1, 1, 1, 1, 1, 1, 1, 1), (1,) * 8)]


@pytest.mark.parametrize("shape", SHAPES)
def test_sizes_against_the_restatement(L, shape):
    (n, eta, log2_final, q, d), K, Cs, masks = shape
    S = MR.Mpcs(PR.derive_params(GL, 12, 7, 2, 2, 8), 7, 7, n, 7, eta, log2_final, 0, q, d, K, Cs, masks)
    fri_proof = L.lib.ronk_fri_proof_words_ext(n, eta, log2_final, q, d, 1)
    fri_work = L.lib.ronk_fri_workspace_words_ext(n, eta, log2_final, q, d, 1)
    A = 1 << eta
    Y = sum(bin(m).count("1") * c for c, m in zip(Cs, masks))
    args = (n, eta, log2_final, q, d, K, len(Cs), u32s(Cs), u32s(masks))
    # claims, the FRI proof, per round [Q][C_r A] leaves and [Q][log2 m][D] paths;  a, open status, G, the FRI workspace
    assert L.lib.ronk_mpcs_proof_words(*args) == S.proof_words() == 2 * Y + fri_proof + sum(q * c * A + q * (n - eta) * d for c in Cs)
    assert L.lib.ronk_mpcs_workspace_words(*args) == S.workspace_words() == d + q + (2 << n) + fri_work
    # the workspace is that of the batched commitment whatever the rounds; one round with the full mask has its proof size too
    assert L.lib.ronk_mpcs_workspace_words(*args) == L.lib.ronk_pcs_workspace_words(n, eta, log2_final, q, d, Cs[0], K)
    if len(Cs) == 1:
        assert masks[0] == (1 << K) - 1
        assert L.lib.ronk_mpcs_proof_words(*args) == L.lib.ronk_pcs_proof_words(n, eta, log2_final, q, d, Cs[0], K)
    # one proof against one batched proof per round (every column of a round at every one of ITS points): R - 1 FRI proofs saved
    per_round = sum(L.lib.ronk_pcs_proof_words(n, eta, log2_final, q, d, c, bin(m).count("1")) for c, m in zip(Cs, masks))
    assert per_round - L.lib.ronk_mpcs_proof_words(*args) == (len(Cs) - 1) * fri_proof


def test_sizes_of_refused_shapes(L):
    for shape, K, Cs, masks in (((12, 0, 3, 8, 2), 2, (4,), (3,)), ((12, 4, 4, 8, 2), 2, (4,), (3,)), ((12, 3, 9, 8, 2), 2, (4,), (3,)),
                                ((12, 3, 3, 0, 2), 2, (4,), (3,)), ((12, 3, 3, 8, 1), 2, (4,), (3,)), ((12, 3, 3, 8, 2), 2, (0,), (3,)),
                                ((12, 3, 3, 8, 2), 0, (4,), (1,)), ((12, 3, 3, 8, 2), 2, (4,), (1,)), ((12, 3, 3, 8, 2), 2, (4,), (4,)),
                                ((12, 3, 3, 8, 2), 2, (1025,), (3,)), ((12, 3, 3, 8, 2), 9, (4,), (511,)), ((1, 1, 0, 8, 2), 1, (1,), (1,))):
        args = shape + (K, len(Cs), u32s(Cs), u32s(masks))
        assert L.lib.ronk_mpcs_proof_words(*args) == 0 and L.lib.ronk_mpcs_workspace_words(*args) == 0, (shape, K, Cs, masks)
    assert L.lib.ronk_mpcs_proof_words(12, 3, 3, 8, 2, 2, 1, None, None) == 0
    assert L.lib.ronk_mpcs_proof_words(12, 3, 3, 8, 2, 2, 0, u32s((1,)), u32s((3,))) == 0


def test_no_device(L):
    """a ronk_mpcs handle needs a ronk_poseidon handle: without a GPU the chain ends at the first link with RONK_ERR_NO_DEVICE,
    after the argument checks above"""
    h = C.c_void_p()
    rc, mds = L.arr([1] * 12), L.arr([1] * 9)
    got = L.lib.ronk_poseidon_create(C.byref(h), GL, 3, 5, 2, 2, 2, L.ptr(rc), L.ptr(mds))
    if L.device_count() == 0:
        assert got == L.ERR_NO_DEVICE and not h.value
    else:
        assert got == L.OK
        f = C.c_void_p()
        cs, ms = u32s((4, 2)), u32s((3, 1))
        assert L.lib.ronk_mpcs_create(C.byref(f), h, 7, 7, 12, 7, 3, 3, 1, 8, 3, 2, 2, cs, ms) == L.ERR_INVALID and not f.value   # digest_len > rate
        ms9 = u32s((511, 1))
        assert L.lib.ronk_mpcs_create(C.byref(f), h, 7, 7, 12, 7, 3, 3, 1, 8, 2, 9, 2, cs, ms9) == L.ERR_UNSUPPORTED and not f.value
        assert L.lib.ronk_poseidon_destroy(h) == L.OK
