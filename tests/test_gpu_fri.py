"""The FRI prover and verifier on the device (ronk_fri_*), word for word against the Python restatement (tests/fri_ref.py) and, for
the roots of a 2^16 codeword, against the C restatement of tests/emu/emu_poseidon.cpp.  The 64-bit primes run with TEST Poseidon
parameters derived in poseidon_ref.py (not a standard instance)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import fri_ref as FR
import poseidon_ref as PR
import prime_classes as PC
from ronkathon_amd import _lib as L
from ronkathon_amd import callers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [PR.GOLDILOCKS, PR.MONT_P]
GEN = {PR.GOLDILOCKS: 7, PR.MONT_P: 10}
# MONT_P's sums all but never land in [p, 2^64): the primes of tests/prime_classes.py take every outcome of mont64::add
CLASS_FIELDS = PC.CLASS_FIELDS
GEN.update({p: PC.GEN[p] for p in CLASS_FIELDS})
Q, D = 8, 2
CASES = [(6, 1, 2), (9, 3, 3), (12, 2, 4), (12, 3, 3)]


class _Field:
    def __init__(self, p):
        self.ORDER, self._G = p, GEN[p]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def params(p):
    return PR.derive_params(p, 8, 7, 2, 4, 4)


def words(seed, size, p):
    """field words with the edges mixed in: 0, p - 1 and values >= p (reduced by the library)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    k = rng.integers(0, 8, size=size)
    v[k == 0] = np.uint64(p - 1)
    v[k == 1] = 0
    v[k == 2] = np.uint64(p) + rng.integers(0, min(5, 2**64 - p), size=int((k == 2).sum()), dtype=np.uint64)
    return v


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


class Instance:
    """a library handle and the restatement's object for the same parameters"""

    def __init__(self, p, n, eta, log2_final, log2_blowup, shift=None, queries=Q):
        self.P = params(p)
        shift = GEN[p] if shift is None else shift
        self.F = FR.Fri(self.P, GEN[p], n, shift, eta, log2_final, log2_blowup, queries, D)
        self.pos = L.PoseidonHandle(*self.P.create_args())
        self.h = L.FriHandle(self.pos, GEN[p], n, shift, eta, log2_final, log2_blowup, queries, D)
        assert self.h.proof_words == self.F.proof_words() and self.h.workspace_words == self.F.workspace_words()

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
        self.pos.close()


def fold_final(n, eta):
    """a final size for a handle that is used for its layer-0 fold only"""
    k = max(1, -(-(n - 8) // eta))
    return n - eta * k


# ------------------------------------------------------------------------------------------------ (a) the fold, whole vectors
def check_folds(torch, p, eta, sizes):
    rng = random.Random(eta)
    for n in sizes:
        for shift in (1, GEN[p]):
            I = Instance(p, n, eta, fold_final(n, eta), 0, shift=shift)
            v = words(100 * n + eta, 1 << n, p)
            d_in = dev(torch, v)
            for beta in (0, 1, p - 1, rng.randrange(p)) if n < 16 else (rng.randrange(p),):
                d_beta = dev(torch, np.array([beta], dtype=np.uint64))
                d_out = torch.full(((1 << n) >> eta,), -1, dtype=torch.int64, device="cuda")
                I.h.fold_dev(0, d_in.data_ptr(), d_beta.data_ptr(), d_out.data_ptr())
                assert host(torch, d_out).tolist() == FR.fold(I.F, v, beta, 0), (p, eta, n, shift, beta)
            I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_fold_against_restatement(torch, p, eta):
    """one lane, one workgroup, several workgroups, both levels of the inverse-point table; s = 1 and s = g; edge words"""
    check_folds(torch, p, eta, (eta + 1, 9, 12, 16))


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_fold_prime_classes(torch, p, eta):
    check_folds(torch, p, eta, (eta + 1, 9, 12))


@pytest.mark.parametrize("p", FIELDS)
def test_fold_inner_layers_and_host_form(torch, p):
    """layers past the first have their own domain (s^(A^l), w_(N_l)); callers.Fri.fold is the same call on host arrays"""
    I = Instance(p, 11, 2, 3, 0)
    fri = callers.Fri((_Field(p),) + I.P.create_args()[1:], 11, GEN[p], 2, 3, 0, Q, D)
    for layer in range(I.F.L):
        v = words(7 + layer, I.F.size(layer), p)
        beta = int(words(70 + layer, 1, p)[0])
        want = FR.fold(I.F, v, beta, layer)
        d_in, d_beta = dev(torch, v), dev(torch, np.array([beta], dtype=np.uint64))
        d_out = torch.full((len(want),), -1, dtype=torch.int64, device="cuda")
        I.h.fold_dev(layer, d_in.data_ptr(), d_beta.data_ptr(), d_out.data_ptr())
        assert host(torch, d_out).tolist() == want, (p, layer)
        assert fri.fold(v, beta, layer).tolist() == want, (p, layer)
    with pytest.raises(L.RonkPanic) as e:
        I.h.fold_dev(I.F.L, 16, 16, 16)
    assert e.value.code == L.ERR_INVALID
    I.close()


# ------------------------------------------------------------------------------------------------ (b) a known polynomial
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_fold_of_known_polynomial(torch, p, eta):
    """the fold of the values of sum c_k x^k is the values of sum_k (sum_(j < A) beta^j c_(A k + j)) x^k on the next domain"""
    n = 12
    I = Instance(p, n, eta, fold_final(n, eta), 0)
    rng = random.Random(p % 1000 + eta)
    c = [rng.randrange(p) for _ in range(1 << n)]
    beta = rng.randrange(p)
    A = 1 << eta
    g = [sum(pow(beta, j, p) * c[A * k + j] for j in range(A)) % p for k in range((1 << n) // A)]
    d_in = dev(torch, np.array(FR.evaluate(I.F, c), dtype=np.uint64))
    d_beta = dev(torch, np.array([beta], dtype=np.uint64))
    d_out = torch.full((len(g),), -1, dtype=torch.int64, device="cuda")
    I.h.fold_dev(0, d_in.data_ptr(), d_beta.data_ptr(), d_out.data_ptr())
    assert host(torch, d_out).tolist() == FR.evaluate(I.F, g, 1)
    I.close()


# ------------------------------------------------------------------------------------------------ (c) the proof, word for word
_REF = {}


def reference(p, case):
    """(instance parameters, codeword, seed, the restatement's proof), computed once per case"""
    key = (p, case)
    if key not in _REF:
        n, eta, log2_final = case
        F = FR.Fri(params(p), GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)
        rng = random.Random(n * 100 + eta)
        f = FR.evaluate(F, [rng.randrange(p) for _ in range(1 << (n - 1))])
        seed = [3, 4]
        if case == CASES[0]:
            # 8 queries into 32 leaves: pick a seed under which two queries meet
            for s in range(200):
                seed = [s, 4]
                layers, trees, roots, betas = FR.commit_phase(F, f, seed)
                j0 = [i[0] for i in FR.transcript(F, seed, roots, layers[F.L])[1]]
                if len(set(j0)) < len(j0):
                    break
            assert len(set(j0)) < len(j0)
        _REF[key] = (f, seed, FR.prove(F, f, seed))
    return _REF[key]


def check_proof(torch, p, case):
    n, eta, log2_final = case
    f, seed, want = reference(p, case)
    I = Instance(p, n, eta, log2_final, 1)
    got = I.prove_dev(torch, f, seed)
    assert got.tolist() == want, (p, case)
    assert I.verify_dev(torch, got, seed) == 0
    # (f) a second identical call over a differently poisoned workspace: bit-identical
    assert np.array_equal(I.prove_dev(torch, f, seed, fill=0x55), got)
    I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("case", CASES)
def test_proof_word_for_word(torch, p, case):
    check_proof(torch, p, case)


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("case", CASES[:2])
def test_proof_word_for_word_prime_classes(torch, p, case):
    check_proof(torch, p, case)


@pytest.fixture(scope="module")
def cref():
    """the C restatement of the tree as a shared object (OpenMP over the nodes of a level)"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libposref.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        tmp = "%s.tmp.%d" % (so, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-DEMU_POSEIDON_LIB", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    lib.posref_merkle.argtypes = [u64, u32, u64, u32, u32, u32, vp, vp, vp, sz, sz, sz, sz, sz, vp]
    lib.posref_merkle.restype = None
    lib.posref_tree_words.argtypes = [sz, sz]
    lib.posref_tree_words.restype = sz
    return lib


@pytest.mark.parametrize("p", FIELDS)
def test_roots_of_a_large_codeword(torch, cref, p):
    """n = 16, eta = 3: the trees through the C restatement (pinned by the Python one in test_gpu_poseidon.py), the challenges and
    the folds through the Python one; the roots and the final layer of the device proof"""
    n, eta, log2_final = 16, 3, 4
    I = Instance(p, n, eta, log2_final, 1)
    F, P = I.F, I.P
    rng = random.Random(16)
    f = FR.evaluate(F, [rng.randrange(p) for _ in range(1 << (n - 1))])
    seed = [5, 6]
    rc = L.arr(P.rc); mds = L.arr([v for row in P.mds for v in row])
    c, cur, want = list(seed), f, []
    for l in range(F.L):
        m = F.leaves(l)
        tree = np.empty(cref.posref_tree_words(m, D), dtype=np.uint64)
        a = np.array(cur, dtype=np.uint64)
        cref.posref_merkle(P.p, P.width, P.alpha, P.num_p, P.num_f, P.rate, L.ptr(rc), L.ptr(mds), L.ptr(a), m, F.A, 1, m, D, L.ptr(tree))
        root = [int(w) for w in tree[-D:]]
        want += root
        c = PR.sponge(P, c + root, D)
        cur = FR.fold(F, cur, c[0], l)
    want += cur
    got = I.prove_dev(torch, f, seed)
    assert got[:len(want)].tolist() == want
    assert I.verify_dev(torch, got, seed) == 0
    I.close()


# ------------------------------------------------------------------------------------------------ (d) the verifier
def check_verifier_statuses(torch, p, case):
    n, eta, log2_final = case
    f, seed, proof = reference(p, case)
    I = Instance(p, n, eta, log2_final, 1)
    F = I.F
    assert I.verify_dev(torch, proof, seed) == 0
    off_final = F.L * D
    off_leaf0 = off_final + F.size(F.L)
    off_path0 = off_leaf0 + Q * F.A
    off_leaf1 = off_path0 + Q * F.depth(0) * D
    flips = {"root": 1, "last root": (F.L - 1) * D, "final": off_final + 3, "leaf value": off_leaf0 + 2 * F.A + 5,
             "inner leaf value": off_leaf1 + 4 * F.A, "path": off_path0 + 3 * F.depth(0) * D + 2}
    for what, at in flips.items():
        bad = list(proof)
        bad[at] ^= 1 << 7
        want = FR.verify(F, bad, seed)
        assert want != 0 and I.verify_dev(torch, bad, seed) == want, (p, what)
    assert FR.verify(F, [proof[i] ^ (1 if i == flips["path"] else 0) for i in range(len(proof))], seed) == 1
    # a word >= p in the place of its residue is no fold value: at the final-layer position of the first query (the verifier
    # compares words there; a position no query reaches only enters the degree check, which reduces it)
    j = FR.transcript(F, seed, *FR.split(F, proof)[:2])[1][0][F.L - 1]
    if proof[off_final + j] + p < 2**64:
        bad = list(proof)
        bad[off_final + j] += p
        want = FR.verify(F, bad, seed)
        assert want & 2 and I.verify_dev(torch, bad, seed) == want
    # another seed
    other = [seed[0] + 1, seed[1]]
    want = FR.verify(F, proof, other)
    assert want != 0 and I.verify_dev(torch, proof, other) == want
    # values on no low-degree polynomial, proved honestly: only the final layer tells
    rnd = [int(v) % p for v in words(5, 1 << n, p)]
    pr = I.prove_dev(torch, rnd, seed)
    assert FR.verify(F, pr.tolist(), seed) == 4 and I.verify_dev(torch, pr, seed) == 4
    # a codeword corrupted on half of its cosets: whatever the restatement says of the device's proof
    m = F.leaves(0)
    g = [(v + 1) % p if (k % m) % 2 else v for k, v in enumerate(f)]
    pr = I.prove_dev(torch, g, seed)
    want = FR.verify(F, pr.tolist(), seed)
    assert want != 0 and I.verify_dev(torch, pr, seed) == want
    I.close()


@pytest.mark.parametrize("p", FIELDS)
def test_verifier_statuses(torch, p):
    check_verifier_statuses(torch, p, CASES[1])


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("case", CASES[:2])
def test_verifier_statuses_prime_classes(torch, p, case):
    check_verifier_statuses(torch, p, case)


# ------------------------------------------------------------------------------------------------ (e) host forms
@pytest.mark.parametrize("p", FIELDS)
def test_host_forms(torch, p):
    case = CASES[0]
    n, eta, log2_final = case
    f, seed, want = reference(p, case)
    fri = callers.Fri((_Field(p),) + params(p).create_args()[1:], n, GEN[p], eta, log2_final, 1, Q, D)
    proof = fri.prove(f, seed)
    assert proof.tolist() == want
    assert fri.verify(proof, seed) == 0
    bad = proof.copy()
    bad[-1] ^= np.uint64(1)
    assert fri.verify(bad, seed) == FR.verify(fri_ref_instance(p, case), bad.tolist(), seed) == 1
    with pytest.raises(L.RonkPanic):
        fri.prove(f[:-1], seed)


def fri_ref_instance(p, case):
    n, eta, log2_final = case
    return FR.Fri(params(p), GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)


def test_create_errors_on_the_device():
    """the codes of ronk_fri_check through ronk_fri_create, with a live Poseidon handle"""
    P = params(PR.GOLDILOCKS)
    pos = L.PoseidonHandle(*P.create_args())
    for args, code in (((7, 33, 7, 3, 3, 1, 8, 2), L.ERR_NO_ROOT), ((7, 12, 0, 3, 3, 1, 8, 2), L.ERR_INVALID),
                       ((7, 12, 7, 3, 9, 1, 8, 2), L.ERR_UNSUPPORTED), ((7, 12, 7, 2, 3, 1, 8, 2), L.ERR_INVALID),
                       ((7, 12, 7, 3, 3, 1, 8, 5), L.ERR_INVALID)):
        with pytest.raises(L.RonkPanic) as e:
            L.FriHandle(pos, *args)
        assert e.value.code == code, args
    pos.close()
