"""Argument errors and sizes of the proof-of-work entry points (ronk_pow_*, ronk_fri_set_pow, ronk_pcs_set_pow and the handle size
functions): ronk_pow_check is host integer logic and the NULL checks come first, so this runs without a GPU.  The codes of the
setters need a handle, and a handle needs a device: without one, ronk_poseidon_create returns RONK_ERR_NO_DEVICE and so nothing
further along can be reached (test_no_device); with one, the setters and the size functions are checked against the restated
formulas of tests/pow_ref.py."""
import ctypes as C

import pytest

import deep_ref as DR
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR
import pow_ref as PW

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
NAMES = ("ronk_pow_check", "ronk_pow_workspace_words", "ronk_pow_grind_dev", "ronk_pow_verify_dev", "ronk_pow_grind", "ronk_pow_verify",
         "ronk_fri_set_pow", "ronk_fri_handle_proof_words", "ronk_fri_handle_workspace_words", "ronk_pcs_set_pow",
         "ronk_pcs_handle_proof_words", "ronk_pcs_handle_workspace_words")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.lib.ronk_pow_workspace_words() == PW.WORK_WORDS


def test_check_codes_in_their_order(L):
    """(p, rate, seed_len, bits, log2_limit): the field's codes, then INVALID, then UNSUPPORTED"""
    f = L.lib.ronk_pow_check
    assert f(GL, 4, 2, 20, 26) == L.OK and f(MONT, 8, 4096, 40, 40) == L.OK and f(GL, 1, 0, 0, 0) == L.OK
    # the field first, whatever the rest
    assert f(0, 4, 2, 50, 50) == L.ERR_INVALID and f(1, 4, 2, 6, 6) == L.ERR_INVALID
    assert f(2, 4, 5000, 50, 50) == L.ERR_UNSUPPORTED
    assert f(100, 4, 5000, 50, 50) == L.ERR_NOT_PRIME
    assert f(9, 4, 5000, 50, 50) == L.ERR_NOT_PRIME and f(2**32 + 1, 4, 2, 6, 12) == L.ERR_NOT_PRIME   # odd composites
    assert f(GL, 0, 2, 6, 6) == L.ERR_INVALID
    # a nonce must be a canonical, distinct field element: F_101 takes 6 bits, not 7
    assert f(101, 2, 1, 6, 6) == L.OK
    assert f(101, 2, 1, 7, 6) == L.ERR_INVALID and f(101, 2, 1, 6, 7) == L.ERR_INVALID
    assert f(GL, 4, 2, 64, 26) == L.ERR_INVALID and f(GL, 4, 2, 20, 64) == L.ERR_INVALID and f(GL, 4, 2, 200, 26) == L.ERR_INVALID
    assert f(GL, 4, 2, 63, 63) == L.ERR_UNSUPPORTED and f(3 * 2**30 + 1, 4, 2, 31, 31) == L.OK and f(3 * 2**30 + 1, 4, 2, 32, 31) == L.ERR_INVALID
    # INVALID before UNSUPPORTED
    assert f(101, 2, 5000, 7, 6) == L.ERR_INVALID
    assert f(GL, 4, 2, 41, 26) == L.ERR_UNSUPPORTED and f(GL, 4, 2, 20, 41) == L.ERR_UNSUPPORTED
    assert f(GL, 4, 4097, 20, 26) == L.ERR_UNSUPPORTED and f(GL, 4, 4096, 20, 26) == L.OK
    for args in ((GL, 4, 2, 20, 26), (101, 2, 1, 7, 6), (GL, 4, 4097, 20, 26), (MONT, 4, 1, 40, 41)):
        want = PW.check(*args)
        assert f(*args) == {0: L.OK, "invalid": L.ERR_INVALID, "unsupported": L.ERR_UNSUPPORTED}[want]


def test_null_arguments(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    n, ok = C.c_uint64(5), C.c_int(5)
    assert L.lib.ronk_pow_grind_dev(None, d, 2, 6, 12, 0, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pow_verify_dev(None, d, 2, 6, 12, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_pow_grind(None, d, 2, 6, 12, 0, C.byref(n)) == L.ERR_INVALID
    assert L.lib.ronk_pow_verify(None, d, 2, 6, 12, 0, C.byref(ok)) == L.ERR_INVALID
    assert n.value == 5 and ok.value == 5
    assert L.lib.ronk_fri_set_pow(None, 6, 12) == L.ERR_INVALID and L.lib.ronk_pcs_set_pow(None, 6, 12) == L.ERR_INVALID
    for f in (L.lib.ronk_fri_handle_proof_words, L.lib.ronk_fri_handle_workspace_words, L.lib.ronk_pcs_handle_proof_words,
              L.lib.ronk_pcs_handle_workspace_words):
        assert f(None) == 0


def test_default_limit(L):
    for p, bits in ((GL, 20), (GL, 38), (101, 4), (101, 0), (MONT, 34), (3 * 2**30 + 1, 28)):
        lam = L.pow_default_limit(p, bits)
        assert lam == PW.default_limit(p, bits) and L.lib.ronk_pow_check(p, 2, 1, 0, lam) == L.OK


def test_no_device(L):
    """Every compute call and both setters need a handle whose chain starts at ronk_poseidon_create: without a GPU that call
    returns RONK_ERR_NO_DEVICE (after its own argument checks), so the setters' codes -- those of ronk_pow_check with
    seed_len = D -- and the handle size functions are reachable on a device only, where the rest of this test checks them."""
    P = PR.derive_params(GL, 8, 7, 2, 4, 4)
    if L.device_count() == 0:
        h = C.c_void_p()
        rc, mds = L.arr(P.rc), L.arr([v for row in P.mds for v in row])
        assert L.lib.ronk_poseidon_create(C.byref(h), GL, 8, 7, 2, 4, 4, L.ptr(rc), L.ptr(mds)) == L.ERR_NO_DEVICE and not h.value
        return
    pos = L.PoseidonHandle(*P.create_args())
    W = PW.Pow(6, 12)
    for ext in (False, True):
        F = FX.FriExt(P, 7, 7, 9, 7, 3, 3, 1, 5, 2, 0) if ext else FR.Fri(P, 7, 9, 7, 3, 3, 1, 5, 2)
        h = L.FriHandle(pos, 7, 9, 7, 3, 3, 1, 5, 2, w=7 if ext else None)
        plain = (h.proof_words, h.workspace_words)
        assert plain == (F.proof_words(), F.workspace_words())
        assert (L.lib.ronk_fri_handle_proof_words(h.h), L.lib.ronk_fri_handle_workspace_words(h.h)) == plain
        assert L.lib.ronk_fri_set_pow(h.h, 64, 12) == L.ERR_INVALID and L.lib.ronk_fri_set_pow(h.h, 41, 12) == L.ERR_UNSUPPORTED
        assert (L.lib.ronk_fri_handle_proof_words(h.h), L.lib.ronk_fri_handle_workspace_words(h.h)) == plain   # a refused call changes nothing
        h.set_pow(6, 12)
        assert (h.proof_words, h.workspace_words) == (PW.proof_words(F, W), PW.workspace_words(F, W))
        h.set_pow(0, 0)
        assert (h.proof_words, h.workspace_words) == plain
        h.close()
    S = DR.Pcs(P, 7, 7, 6, 7, 1, 2, 1, 5, 2, 3, 2)
    h = L.PcsHandle(pos, 7, 7, 6, 7, 1, 2, 1, 5, 2, 3, 2)
    plain = (h.proof_words, h.workspace_words)
    assert plain == (S.proof_words(), S.workspace_words())
    assert L.lib.ronk_pcs_set_pow(h.h, 20, 64) == L.ERR_INVALID
    h.set_pow(6)
    assert h.pow_log2_limit == 12 and (h.proof_words, h.workspace_words) == (PW.pcs_proof_words(S, W), PW.pcs_workspace_words(S, W))
    h.set_pow(0)
    assert (h.proof_words, h.workspace_words) == plain
    h.close()
    pos.close()
