"""FRI with extension challenges on the device (a handle of ronk_fri_create_ext through ronk_fri_fold_dev / prove_dev /
verify_dev), word for word against the Python restatement (tests/fri_ext_ref.py).  W is the field's generator.  The 64-bit primes
run with TEST Poseidon parameters derived in poseidon_ref.py (not a standard instance)."""
import ctypes as C
import random

import numpy as np
import pytest

import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from test_gpu_fri import CASES, CLASS_FIELDS, D, FIELDS, GEN, Q, _Field, dev, fold_final, host, params, words
from test_gpu_fri import reference as base_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class Instance:
    """a library handle and the restatement's object for the same parameters"""

    def __init__(self, p, n, eta, log2_final, log2_blowup, input_ext, shift=None, pos=None, w=None):
        self.P = params(p)
        shift = GEN[p] if shift is None else shift
        w = GEN[p] if w is None else w
        self.F = FX.FriExt(self.P, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, input_ext)
        self.own_pos = pos is None
        self.pos = L.PoseidonHandle(*self.P.create_args()) if pos is None else pos
        self.h = L.FriHandle(self.pos, GEN[p], n, shift, eta, log2_final, log2_blowup, Q, D, w=w, input_ext=input_ext)
        assert self.h.proof_words == self.F.proof_words() and self.h.workspace_words == self.F.workspace_words()

    def fold_dev(self, torch, layer, values, beta):
        d_in, d_beta = dev(torch, values), dev(torch, np.array(beta, dtype=np.uint64))
        d_out = torch.full((2 * (self.F.size(layer) >> self.F.eta),), -1, dtype=torch.int64, device="cuda")
        self.h.fold_dev(layer, d_in.data_ptr(), d_beta.data_ptr(), d_out.data_ptr())
        return host(torch, d_out).tolist()

    def prove_dev(self, torch, evals, seed, fill=-1):
        d_ev, d_seed = dev(torch, evals), dev(torch, seed)
        d_work = torch.full((self.h.workspace_words,), fill, dtype=torch.int64, device="cuda")
        d_proof = torch.full((self.h.proof_words,), fill, dtype=torch.int64, device="cuda")
        self.h.prove_dev(d_ev.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr())
        return host(torch, d_proof)

    def verify_dev(self, torch, proof, seed):
        d_proof, d_seed = dev(torch, proof), dev(torch, seed)
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.verify_dev(d_proof.data_ptr(), d_seed.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        return int(d_st.item())

    def close(self):
        self.h.close()
        if self.own_pos:
            self.pos.close()


def want_fold(F, v, beta, layer):
    f = FX.layer0(F, v) if layer == 0 else ER.pairs([int(x) for x in v])
    return ER.planar(FX.fold(F, f, beta, layer))


# ------------------------------------------------------------------------------------------------ (a) the fold, whole vectors
def check_folds(torch, p, eta, input_ext, sizes):
    rng = random.Random(eta + 10 * input_ext)
    for n in sizes:
        for shift in (1, GEN[p]):
            I = Instance(p, n, eta, fold_final(n, eta), 0, input_ext, shift=shift)
            v = words(100 * n + eta, (1 + input_ext) << n, p)
            rnd = (rng.randrange(p), rng.randrange(p))
            betas = ((0, 0), (1, 0), (0, 1), (p - 1, p - 1), rnd, (p + 1, rng.randrange(p))) if n < 16 else (rnd,)
            for beta in betas:
                assert I.fold_dev(torch, 0, v, beta) == want_fold(I.F, v, beta, 0), (p, eta, n, shift, beta)
            I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
@pytest.mark.parametrize("input_ext", [0, 1])
def test_fold_against_restatement(torch, p, eta, input_ext):
    """one lane, one workgroup, several workgroups, both levels of the inverse-point table; s = 1 and s = g; edge words; beta with
    zero, one, p - 1 and a word >= p among its components"""
    check_folds(torch, p, eta, input_ext, (eta + 1, 9, 12, 16))


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
@pytest.mark.parametrize("input_ext", [0, 1])
def test_fold_prime_classes(torch, p, eta, input_ext):
    """the primes of tests/prime_classes.py (every outcome of mont64::add), several workgroups"""
    check_folds(torch, p, eta, input_ext, (9,))


@pytest.mark.parametrize("p", FIELDS)
def test_fold_inner_layers_and_host_form(torch, p):
    """layers past the first are planar and have their own domain (s^(A^l), w_(N_l)); callers.Fri.fold is the same call on host
    arrays"""
    I = Instance(p, 11, 2, 3, 0, 0)
    fri = callers.Fri((_Field(p),) + I.P.create_args()[1:], 11, GEN[p], 2, 3, 0, Q, D, w=GEN[p])
    for layer in range(I.F.L):
        v = words(7 + layer, I.F.vw(layer) * I.F.size(layer), p)
        beta = [int(x) for x in words(70 + layer, 2, p)]
        want = want_fold(I.F, v, beta, layer)
        assert I.fold_dev(torch, layer, v, beta) == want, (p, layer)
        assert fri.fold(v, beta, layer).tolist() == want, (p, layer)
    with pytest.raises(L.RonkPanic) as e:
        I.h.fold_dev(I.F.L, 16, 16, 16)
    assert e.value.code == L.ERR_INVALID
    I.close()


@pytest.mark.parametrize("eta", [1, 2, 3])
@pytest.mark.parametrize("input_ext", [0, 1])
def test_goldilocks_with_another_w(torch, eta, input_ext):
    """W = 7 over Goldilocks has a product with W of its own (a shift); any other non-residue, here 11 and p - 7, takes the
    ordinary product on the same shift roots: folds, and a proof through prover and verifier"""
    p = PR.GOLDILOCKS
    rng = random.Random(40 + eta)
    for w in (11, p - 7):
        I = Instance(p, 9, eta, fold_final(9, eta), 0, input_ext, w=w)
        v = words(900 + eta, (1 + input_ext) << 9, p)
        for beta in ((rng.randrange(p), rng.randrange(p)), (p - 1, p + 2)):
            assert I.fold_dev(torch, 0, v, beta) == want_fold(I.F, v, beta, 0), (eta, input_ext, w, beta)
        I.close()
    n, log2_final = 6 + eta, 6 + eta - 2 * eta
    I = Instance(p, n, eta, log2_final, 1, input_ext, w=11)
    f = FR.evaluate(I.F, [rng.randrange(p) for _ in range(1 << (n - 1))])
    if input_ext:
        f = f + FR.evaluate(I.F, [rng.randrange(p) for _ in range(1 << (n - 1))])
    got = I.prove_dev(torch, f, [3, 4])
    assert got.tolist() == FX.prove(I.F, f, [3, 4])
    assert I.verify_dev(torch, got, [3, 4]) == 0
    bad = got.copy()
    bad[I.F.L * D + (1 << log2_final) + 1] ^= np.uint64(1 << 7)          # a c1 word of the final layer
    want = FX.verify(I.F, bad.tolist(), [3, 4])
    assert want & 4 and I.verify_dev(torch, bad, [3, 4]) == want
    I.close()


# ------------------------------------------------------------------------------------------------ (b) the proof, word for word
_REF = {}


def reference(p, case, input_ext):
    """(codeword, seed, the restatement's proof), computed once per case"""
    key = (p, case, input_ext)
    if key not in _REF:
        n, eta, log2_final = case
        F = FX.FriExt(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, input_ext)
        rng = random.Random(n * 100 + eta + 7 * input_ext)
        f = FR.evaluate(F, [rng.randrange(p) for _ in range(1 << (n - 1))])
        if input_ext:
            f = f + FR.evaluate(F, [rng.randrange(p) for _ in range(1 << (n - 1))])
        seed = [3, 4]
        _REF[key] = (f, seed, FX.prove(F, f, seed))
    return _REF[key]


def check_proof(torch, p, case, input_ext):
    n, eta, log2_final = case
    f, seed, want = reference(p, case, input_ext)
    I = Instance(p, n, eta, log2_final, 1, input_ext)
    got = I.prove_dev(torch, f, seed)
    assert got.tolist() == want, (p, case, input_ext)
    assert I.verify_dev(torch, got, seed) == 0
    # a second identical call over a differently poisoned workspace: bit-identical
    assert np.array_equal(I.prove_dev(torch, f, seed, fill=0x55), got)
    I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("input_ext", [0, 1])
def test_proof_word_for_word(torch, p, case, input_ext):
    check_proof(torch, p, case, input_ext)


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("input_ext", [0, 1])
def test_proof_word_for_word_prime_classes(torch, p, input_ext):
    check_proof(torch, p, CASES[1], input_ext)


# ------------------------------------------------------------------------------------------------ (c) the verifier
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("input_ext", [0, 1])
def test_verifier_statuses(torch, p, input_ext):
    case = CASES[1]
    n, eta, log2_final = case
    f, seed, proof = reference(p, case, input_ext)
    I = Instance(p, n, eta, log2_final, 1, input_ext)
    F = I.F
    A, nl = F.A, F.size(F.L)
    assert I.verify_dev(torch, proof, seed) == 0 == FX.verify(F, proof, seed)
    off_final = F.L * D
    off_leaf0 = off_final + 2 * nl
    off_path0 = off_leaf0 + Q * F.leaf_len(0)
    off_leaf1 = off_path0 + Q * F.depth(0) * D
    flips = {"root": 1, "final c0": off_final + 3, "final c1": off_final + nl + 3, "leaf value": off_leaf0 + 2 * F.leaf_len(0) + 5,
             "inner leaf c0": off_leaf1 + 4 * 2 * A + 1, "inner leaf c1": off_leaf1 + 4 * 2 * A + A + 1,
             "path": off_path0 + 3 * F.depth(0) * D + 2}
    if input_ext:
        flips["leaf value c1"] = off_leaf0 + 2 * F.leaf_len(0) + A + 5
    seen = {}
    for what, at in flips.items():
        bad = list(proof)
        bad[at] ^= 1 << 7
        want = FX.verify(F, bad, seed)
        seen[what] = want
        assert want != 0 and I.verify_dev(torch, bad, seed) == want, (p, what)
    assert seen["path"] == 1 and seen["inner leaf c0"] & 2 and seen["inner leaf c1"] & 2 and seen["final c1"] & 4
    # values on no low-degree polynomial, proved honestly: only the final layer tells; a bad c1 plane alone is enough
    rnd = [int(v) % p for v in words(5, (1 + input_ext) << n, p)]
    pr = I.prove_dev(torch, rnd, seed)
    assert FX.verify(F, pr.tolist(), seed) == 4 and I.verify_dev(torch, pr, seed) == 4
    if input_ext:
        pr = I.prove_dev(torch, f[:1 << n] + rnd[1 << n:], seed)
        assert FX.verify(F, pr.tolist(), seed) == 4 and I.verify_dev(torch, pr, seed) == 4
    # a c1 word >= p in the place of its residue is no fold value
    j = FX.transcript(F, seed, *FX.split(F, proof)[:2])[1][0][F.L - 1]
    if proof[off_final + nl + j] + p < 2**64:
        bad = list(proof)
        bad[off_final + nl + j] += p
        want = FX.verify(F, bad, seed)
        assert want != 0 and I.verify_dev(torch, bad, seed) == want
    # everything at once: a path word, a leaf word and the final layer
    bad = list(proof)
    for at in (flips["path"], flips["inner leaf c1"], flips["final c1"]):
        bad[at] ^= 1 << 7
    want = FX.verify(F, bad, seed)
    assert want == 7 and I.verify_dev(torch, bad, seed) == 7
    # another seed
    other = [seed[0] + 1, seed[1]]
    want = FX.verify(F, proof, other)
    assert want != 0 and I.verify_dev(torch, proof, other) == want
    I.close()


# ------------------------------------------------------------------------------------------------ (d) host forms, the base handle
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("input_ext", [0, 1])
def test_host_forms(torch, p, input_ext):
    case = CASES[0]
    n, eta, log2_final = case
    f, seed, want = reference(p, case, input_ext)
    fri = callers.Fri((_Field(p),) + params(p).create_args()[1:], n, GEN[p], eta, log2_final, 1, Q, D, w=GEN[p], input_ext=input_ext)
    proof = fri.prove(f, seed)
    assert proof.tolist() == want
    assert fri.verify(proof, seed) == 0
    bad = proof.copy()
    bad[-1] ^= np.uint64(1)
    F = FX.FriExt(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, input_ext)
    assert fri.verify(bad, seed) == FX.verify(F, bad.tolist(), seed) == 1
    with pytest.raises(L.RonkPanic):
        fri.prove(f[:-1], seed)


@pytest.mark.parametrize("p", FIELDS)
def test_base_handle_beside_an_extension_handle(torch, p):
    """a handle of ronk_fri_create on the same Poseidon handle still produces its old proof, before and after the extension
    handle has worked"""
    case = CASES[1]
    n, eta, log2_final = case
    f, seed, want = base_reference(p, case)
    fx, seedx, wantx = reference(p, case, 0)
    I = Instance(p, n, eta, log2_final, 1, 0)
    base = L.FriHandle(I.pos, GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)
    assert base.proof_words == len(want) and not base.ext

    def base_proof():
        d_ev, d_seed = dev(torch, f), dev(torch, seed)
        d_work = torch.full((base.workspace_words,), -1, dtype=torch.int64, device="cuda")
        d_proof = torch.full((base.proof_words,), -1, dtype=torch.int64, device="cuda")
        base.prove_dev(d_ev.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr())
        return host(torch, d_proof).tolist()

    assert base_proof() == want
    assert I.prove_dev(torch, fx, seedx).tolist() == wantx
    assert base_proof() == want
    base.close()
    I.close()


def test_create_errors_on_the_device():
    """the codes of ronk_fri_check_ext through ronk_fri_create_ext, with a live Poseidon handle"""
    P = params(PR.GOLDILOCKS)
    pos = L.PoseidonHandle(*P.create_args())
    for args, kw, code in (((7, 33, 7, 3, 3, 1, 8, 2), dict(w=7), L.ERR_NO_ROOT), ((7, 12, 0, 3, 3, 1, 8, 2), dict(w=7), L.ERR_INVALID),
                           ((7, 12, 7, 3, 9, 1, 8, 2), dict(w=7), L.ERR_UNSUPPORTED), ((7, 12, 7, 3, 3, 1, 8, 2), dict(w=49), L.ERR_INVALID),
                           ((7, 12, 7, 3, 3, 1, 8, 2), dict(w=0), L.ERR_INVALID), ((7, 12, 7, 3, 3, 1, 8, 1), dict(w=7), L.ERR_INVALID),
                           ((7, 12, 7, 3, 3, 1, 8, 5), dict(w=7), L.ERR_INVALID)):
        with pytest.raises(L.RonkPanic) as e:
            L.FriHandle(pos, *args, **kw)
        assert e.value.code == code, (args, kw)
    h = C.c_void_p()
    assert L.lib.ronk_fri_create_ext(C.byref(h), pos.h, 7, 7, 12, 7, 3, 3, 1, 8, 2, 2) == L.ERR_INVALID and not h.value
    pos.close()
