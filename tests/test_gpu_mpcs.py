"""The multi-matrix polynomial commitment on the device (ronk_mpcs_*), word for word against the Python restatement
(tests/mpcs_ref.py): the combination of R matrices at per-matrix points, one round with a full mask against ronk_pcs_* of the same
build, proofs, verifier statuses, the host-pointer forms, and a PLONK proof assembled from the library's own parts.  Fields,
TEST Poseidon parameters, Q and D are those of tests/test_gpu_pcs.py."""
import ctypes as C
import random

import numpy as np
import pytest

import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import mpcs_ref as MR
import plonk_ref as PL
import pow_ref as PW
import test_gpu_pcs as TP
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from test_gpu_pcs import CLASS_FIELDS, D, FIELDS, GEN, Q, SEED, _Field, dev, host, params, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class PowFri:
    """mpcs_ref's embedded FRI with grinding, as tests/pow_ref.py states it"""

    def __init__(self, W):
        self.W = W

    def proof_words(self, F):
        return PW.proof_words(F, self.W)

    def workspace_words(self, F):
        return PW.workspace_words(F, self.W)

    def prove(self, F, evals, seed):
        return PW.fri_prove_pow(F, self.W, evals, seed)

    def verify(self, F, proof, seed):
        return PW.fri_verify_pow(F, self.W, proof, seed)

    def opened(self, F, proof, seed):
        body, _ = PW.fri_split_pow(F, self.W, proof)
        return PW.fri_indices_pow(F, self.W, proof, seed), FX.split(F, body)[2][0]


class Instance:
    """a library handle and the restatement's object for the same parameters"""

    def __init__(self, p, n, eta, log2_final, log2_blowup, K, Cs, masks, shift=None, w=None, pow_bits=0):
        self.P = params(p)
        self.p = p
        shift = GEN[p] if shift is None else shift
        w = GEN[p] if w is None else w
        fri = PowFri(PW.Pow(pow_bits, PW.default_limit(p, pow_bits))) if pow_bits else None
        self.S = MR.Mpcs(self.P, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, K, Cs, masks, fri=fri)
        self.pos = L.PoseidonHandle(*self.P.create_args())
        self.h = L.MpcsHandle(self.pos, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, K, Cs, masks)
        plain = MR.Mpcs(self.P, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, K, Cs, masks)
        assert self.h.proof_words == plain.proof_words() and self.h.workspace_words == plain.workspace_words()
        if pow_bits:
            self.h.set_pow(pow_bits)
        assert self.h.proof_words == self.S.proof_words() and self.h.workspace_words == self.S.workspace_words()
        assert self.h.claims == self.S.Y

    def combine_dev(self, torch, d_Ms, ys, zs, alpha):
        S = self.S
        d_y = dev(torch, np.array(MR.claim_words(S, ys), dtype=np.uint64))
        d_z, d_a = dev(torch, np.array(ER.planar(zs), dtype=np.uint64)), dev(torch, np.array(alpha, dtype=np.uint64))
        d_G = torch.full((2 * S.N,), -1, dtype=torch.int64, device="cuda")
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.combine_dev([m.data_ptr() for m in d_Ms], d_y.data_ptr(), d_z.data_ptr(), d_a.data_ptr(), d_G.data_ptr(), d_st.data_ptr())
        return host(torch, d_G).tolist(), int(d_st.item())

    def commit_dev(self, torch, r, d_M):
        d_tree = torch.full((self.h.tree_words,), -1, dtype=torch.int64, device="cuda")
        self.h.commit_dev(r, d_M.data_ptr(), d_tree.data_ptr())
        return d_tree

    def open_raw(self, torch, d_Ms, d_trees, d_coefs, zs, seed, fill=-1):
        d_seed = dev(torch, seed)
        d_z = dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
        d_work = torch.full((self.h.workspace_words,), fill, dtype=torch.int64, device="cuda")
        d_proof = torch.full((self.h.proof_words,), fill, dtype=torch.int64, device="cuda")
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.open_dev([m.data_ptr() for m in d_Ms], [t.data_ptr() for t in d_trees], [c.data_ptr() for c in d_coefs], d_z.data_ptr(),
                        d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr(), d_st.data_ptr())
        return host(torch, d_proof), int(d_st.item())

    def open_dev(self, torch, d_Ms, d_trees, coefs, zs, seed, fill=-1):
        return self.open_raw(torch, d_Ms, d_trees, [dev(torch, np.array(c, dtype=np.uint64).ravel()) for c in coefs], zs, seed, fill)

    def verify_dev(self, torch, roots, zs, seed, proof):
        d_roots = dev(torch, np.array(roots, dtype=np.uint64).ravel())
        d_seed, d_proof = dev(torch, seed), dev(torch, proof)
        d_z = dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.verify_dev(d_roots.data_ptr(), d_z.data_ptr(), d_seed.data_ptr(), d_proof.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        return int(d_st.item())

    def close(self):
        self.h.close()
        self.pos.close()


# ------------------------------------------------------------------------------------------------ (a) the codeword
# ((log2_n, log2_arity, log2_final), K, columns, masks): sixteen lanes (less than a wavefront) and four workgroups; one, two and
# three rounds; masks full, disjoint, nested, and eight points with the second round at the last only
COMBINE_CASES = [((6, 1, 2), 1, (1,), (1,)), ((6, 1, 2), 2, (3, 5), (0b01, 0b10)), ((6, 1, 2), 2, (33, 1, 2), (0b11, 0b01, 0b11)),
                 ((6, 1, 2), 8, (3, 5), (0xFF, 0x80)), ((12, 2, 4), 2, (3, 5), (0b11, 0b11)), ((12, 2, 4), 2, (33, 1, 2), (0b11, 0b01, 0b11)),
                 ((12, 2, 4), 8, (3, 5), (0xFF, 0x80)), ((12, 2, 4), 2, (1,), (0b11,))]


def random_claims(S, rng):
    p = S.p
    return [[[(int(a), int(b)) for a, b in zip(words(rng.randrange(1 << 30), S.Cs[r], p), words(rng.randrange(1 << 30), S.Cs[r], p))]
             if k in S.points_of(r) else None for k in range(S.K)] for r in range(S.R)]


def check_combine(torch, p, case, shift=None):
    (n, eta, log2_final), K, Cs, masks = case
    I = Instance(p, n, eta, log2_final, 0, K, Cs, masks, shift=shift)
    S = I.S
    rng = random.Random(n * 100 + K + len(Cs))
    Mw = [words(100 * n + 7 * r + C, C << n, p) for r, C in enumerate(Cs)]      # 0, p - 1 and words >= p among them
    Ms, d_Ms = [m.reshape(C, 1 << n).tolist() for m, C in zip(Mw, Cs)], [dev(torch, m) for m in Mw]
    rnd = (rng.randrange(p), rng.randrange(p))
    big = p + 1 if p + 1 < 2**64 else p
    alphas = (rnd, (big, rng.randrange(p)), (0, 1)) if n <= 6 else (rnd,)
    for variant in ("plain", "words >= p", "base point", "last domain point", "first domain point"):
        zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(K)]
        want_st = 0
        if variant == "words >= p" and 2 * p < 2**64:
            zs[0] = (zs[0][0] + p, zs[0][1] + p)
        if variant == "base point":
            zs[0] = (rng.randrange(p), 0)                 # z1 = 0, off the domain
            assert not MR.on_domain(S, zs[0])
        if variant == "last domain point":
            zs[K - 1], want_st = (S.point(S.N - 1), 0), 32
        if variant == "first domain point":
            zs[0], want_st = (S.point(0), 0), 32
        ys = random_claims(S, rng)
        for alpha in (alphas if variant == "plain" else alphas[:1]):
            want, st = MR.combine_sy(S, Ms, ys, zs, alpha)
            got, got_st = I.combine_dev(torch, d_Ms, ys, zs, alpha)
            assert st == want_st == got_st and got == ER.planar(want), (p, case, variant, alpha)
            if want_st:     # the zero term: at the domain point itself only the other points contribute
                i = S.N - 1 if variant == "last domain point" else 0
                assert want[i] == MR.combine_point(S, [[Ms[r][c][i] for c in range(S.Cs[r])] for r in range(S.R)], S.point(i), ys, zs, alpha)
    I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("case", COMBINE_CASES)
def test_combine_against_restatement(torch, p, case):
    check_combine(torch, p, case, shift=1 if case[1] == 1 else None)


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_combine_prime_classes(torch, p):
    """the primes of tests/prime_classes.py (every outcome of mont64::add): three rounds with nested masks, below a wavefront"""
    check_combine(torch, p, COMBINE_CASES[2])


def test_goldilocks_with_another_w(torch):
    """W = 7 over Goldilocks has a product with W of its own; another non-residue takes the ordinary product"""
    p = FIELDS[0]
    (n, eta, log2_final), K, Cs, masks = COMBINE_CASES[1]
    I = Instance(p, n, eta, log2_final, 0, K, Cs, masks, w=11)
    rng = random.Random(11)
    Mw = [words(11 + r, C << n, p) for r, C in enumerate(Cs)]
    Ms, d_Ms = [m.reshape(C, 1 << n).tolist() for m, C in zip(Mw, Cs)], [dev(torch, m) for m in Mw]
    zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(K)]
    ys, alpha = random_claims(I.S, rng), (rng.randrange(p), rng.randrange(p))
    want, _ = MR.combine_sy(I.S, Ms, ys, zs, alpha)
    assert I.combine_dev(torch, d_Ms, ys, zs, alpha) == (ER.planar(want), 0)
    I.close()


# ------------------------------------------------------------------------------------------------ (b) one round, full mask
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("oc", [TP.OPEN_CASES[1], TP.OPEN_CASES[3]])
def test_one_round_full_mask_is_the_batched_commitment(torch, p, oc):
    """the proof of ronk_mpcs_open_dev equals that of ronk_pcs_open_dev of the same build word for word (and the restatement's);
    both verifiers accept both proofs"""
    (n, eta, log2_final), log2_blowup, Cc, K = oc
    coef, M, zs, tree, want = TP.reference(p, oc)
    one = TP.instance_of(p, oc)
    I = Instance(p, n, eta, log2_final, log2_blowup, K, (Cc,), ((1 << K) - 1,))
    assert (I.h.proof_words, I.h.workspace_words) == (one.h.proof_words, one.h.workspace_words)
    d_M = dev(torch, np.array(M, dtype=np.uint64).ravel())
    d_tree = I.commit_dev(torch, 0, d_M)
    assert np.array_equal(host(torch, d_tree), host(torch, one.commit_dev(torch, d_M)))
    pcs_proof, pcs_st = one.open_dev(torch, d_M, d_tree, coef, zs, SEED)
    got, st = I.open_dev(torch, [d_M], [d_tree], [coef], zs, SEED)
    assert st == pcs_st == 0 and np.array_equal(got, pcs_proof) and got.tolist() == want
    root = tree.root_hash()
    for proof in (got, pcs_proof):
        assert I.verify_dev(torch, [root], zs, SEED, proof) == 0 == one.verify_dev(torch, root, zs, SEED, proof)
    bad = got.copy()
    bad[-1] ^= np.uint64(1)
    assert I.verify_dev(torch, [root], zs, SEED, bad) == 8 == one.verify_dev(torch, root, zs, SEED, bad)
    I.close()
    one.close()


# ------------------------------------------------------------------------------------------------ (c) open and verify
# ((log2_n, log2_arity, log2_final), log2_blowup, K, columns, masks, grinding bits)
OPEN_CASES = [((6, 1, 2), 1, 2, (2, 3), (0b01, 0b10), 0), ((9, 3, 3), 2, 2, (1, 3, 2), (0b11, 0b01, 0b11), 0),
              ((6, 1, 2), 2, 3, (2, 1, 2), (0b101, 0b010, 0b111), 6), ((9, 3, 3), 1, 1, (5, 1), (1, 1), 0)]
_REF = {}


def instance_of(p, oc):
    (n, eta, log2_final), log2_blowup, K, Cs, masks, bits = oc
    return Instance(p, n, eta, log2_final, log2_blowup, K, Cs, masks, pow_bits=bits)


def reference(p, oc):
    """(coefs, Ms, zs, trees, the restatement's proof), computed once per case"""
    key = (p, oc)
    if key not in _REF:
        (n, eta, log2_final), log2_blowup, K, Cs, masks, bits = oc
        fri = PowFri(PW.Pow(bits, PW.default_limit(p, bits))) if bits else None
        S = MR.Mpcs(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, K, Cs, masks, fri=fri)
        rng = random.Random(n * 100 + eta + 7 * len(Cs) + K)
        coefs = [[[rng.randrange(p) for _ in range(S.d)] for _ in range(C)] for C in Cs]
        coefs[0][0][0], coefs[-1][-1][S.d - 1] = 0, p - 1
        Ms = MR.columns(S, coefs)
        zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(K)]
        trees = [MR.commit(S, r, Ms[r]) for r in range(S.R)]
        proof, st = MR.open_(S, Ms, trees, coefs, zs, SEED)
        assert st == 0
        _REF[key] = (coefs, Ms, zs, trees, proof)
    return _REF[key]


def on_device(torch, I, Ms):
    d_Ms = [dev(torch, np.array(M, dtype=np.uint64).ravel()) for M in Ms]
    return d_Ms, [I.commit_dev(torch, r, d_Ms[r]) for r in range(len(Ms))]


def check_proof(torch, p, oc):
    coefs, Ms, zs, trees, want = reference(p, oc)
    I = instance_of(p, oc)
    d_Ms, d_trees = on_device(torch, I, Ms)
    for r, t in enumerate(trees):
        assert host(torch, d_trees[r]).tolist() == t.flat()
    got, st = I.open_dev(torch, d_Ms, d_trees, coefs, zs, SEED)
    assert st == 0 and got.tolist() == want, (p, oc)
    roots = [t.root_hash() for t in trees]
    assert I.verify_dev(torch, roots, zs, SEED, got) == 0
    # buffers poisoned with another pattern: no word is left unwritten; and a third call in a row on the same handle
    again, _ = I.open_dev(torch, d_Ms, d_trees, coefs, zs, SEED, fill=0x55)
    assert np.array_equal(again, got)
    assert np.array_equal(I.open_dev(torch, d_Ms, d_trees, coefs, zs, SEED)[0], got)
    assert I.verify_dev(torch, roots, zs, SEED, got) == 0
    I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("oc", OPEN_CASES)
def test_proof_word_for_word(torch, p, oc):
    check_proof(torch, p, oc)


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_proof_word_for_word_prime_classes(torch, p):
    check_proof(torch, p, OPEN_CASES[0])


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("oc", OPEN_CASES[:3])
def test_verifier_statuses(torch, p, oc):
    coefs, Ms, zs, trees, proof = reference(p, oc)
    I = instance_of(p, oc)
    S, F = I.S, I.S.F
    R = S.R
    roots = [t.root_hash() for t in trees]
    assert MR.verify(S, roots, zs, SEED, proof) == 0 == I.verify_dev(torch, roots, zs, SEED, proof)
    # a false claim in the last round, proved honestly by the restatement's prover
    ys = MR.claims(S, coefs, zs)
    k = S.points_of(R - 1)[-1]
    ys[R - 1][k][S.Cs[R - 1] - 1] = S.E.add(ys[R - 1][k][S.Cs[R - 1] - 1], (1, 0))
    bad, _ = MR.open_(S, Ms, trees, coefs, zs, SEED, ys=ys)
    want = MR.verify(S, roots, zs, SEED, bad)
    assert want != 0 and I.verify_dev(torch, roots, zs, SEED, bad) == want
    # FRI run on another low-degree codeword than the combination: the DEEP check alone
    shifted, _ = MR.open_(S, Ms, trees, coefs, zs, SEED, tweak=lambda G: [S.E.add(g, (1, 0)) for g in G])
    assert MR.verify(S, roots, zs, SEED, shifted) == 16 == I.verify_dev(torch, roots, zs, SEED, shifted)
    # one word of each section; a path and a leaf of every round, the last included
    off = MR.section_offsets(S)
    fri_leaves = off["fri"] + F.L * D + 2 * F.size(F.L)
    flips = {"claim": off["claims"] + S.Y, "fri root": off["fri"] + 1, "final": fri_leaves - 1, "fri leaf": fri_leaves + 3 * F.leaf_len(0) + 1,
             "fri path": fri_leaves + Q * F.leaf_len(0) + 1}
    for r in range(R):
        flips["matrix leaf %d" % r] = off["leaves"][r] + 5 * S.leaf_len(r) + 1
        flips["matrix path %d" % r] = off["paths"][r] + 6 * F.depth(0) * D + 1
    seen = {}
    for what, at in flips.items():
        t = list(proof)
        t[at] ^= 1 << 9
        seen[what] = MR.verify(S, roots, zs, SEED, t)
        assert seen[what] != 0 and I.verify_dev(torch, roots, zs, SEED, t) == seen[what], (p, oc, what)
    assert all(seen["matrix path %d" % r] == 8 and seen["matrix leaf %d" % r] == 8 | 16 for r in range(R))
    assert seen["fri path"] == 1 and seen["fri leaf"] & 16 and seen["fri leaf"] & 2 and seen["final"] & 4
    # a matrix leaf word >= p in the place of its residue: the same value for the DEEP check, another leaf for the tree
    at = off["leaves"][R - 1] + 1
    if proof[at] + p < 2**64:
        t = list(proof)
        t[at] += p
        want = MR.verify(S, roots, zs, SEED, t)
        assert want == 8 and I.verify_dev(torch, roots, zs, SEED, t) == want
    # everything at once; another seed, another root of the last round, another point; a point on the domain
    t = list(proof)
    for at in flips.values():
        t[at] ^= 1 << 9
    assert I.verify_dev(torch, roots, zs, SEED, t) == MR.verify(S, roots, zs, SEED, t)
    other_root = roots[:-1] + [[roots[-1][0] ^ 1, roots[-1][1]]]
    for rt, z, s in ((roots, zs, [SEED[0] + 1, SEED[1]]), (other_root, zs, SEED), (roots, [(zs[0][0] ^ 1, zs[0][1])] + zs[1:], SEED)):
        want = MR.verify(S, rt, z, s, proof)
        assert want != 0 and I.verify_dev(torch, rt, z, s, proof) == want
    zd = [(S.point(5), 0)] + zs[1:]
    d_Ms, d_trees = on_device(torch, I, Ms)
    pd, st = I.open_dev(torch, d_Ms, d_trees, coefs, zd, SEED)
    wd, wst = MR.open_(S, Ms, trees, coefs, zd, SEED)
    assert st == wst == 32 and pd.tolist() == wd
    want = MR.verify(S, roots, zd, SEED, wd)
    assert want & 32 and I.verify_dev(torch, roots, zd, SEED, wd) == want
    if oc[5]:     # the nonce: out of range, bit 64 alone
        t = list(proof)
        t[off["leaves"][0] - 1] += p
        assert MR.verify(S, roots, zs, SEED, t) == 64 == I.verify_dev(torch, roots, zs, SEED, t)
    I.close()


@pytest.mark.parametrize("p", FIELDS)
def test_host_forms(torch, p):
    oc = OPEN_CASES[1]
    (n, eta, log2_final), log2_blowup, K, Cs, masks, _ = oc
    coefs, Ms, zs, trees, want = reference(p, oc)
    pcs = callers.FriMultiPcs((_Field(p),) + params(p).create_args()[1:], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, K, Cs, masks)
    Mw, z = [np.array(M, dtype=np.uint64) for M in Ms], np.array(ER.planar(zs), dtype=np.uint64)
    ts = [pcs.commit(r, Mw[r]) for r in range(len(Cs))]
    assert [t.tolist() for t in ts] == [t.flat() for t in trees]
    S = MR.Mpcs(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, K, Cs, masks)
    ys = MR.claims(S, coefs, zs)
    for r in range(S.R):
        assert pcs.evaluate(r, coefs[r], z).tolist() == ER.planar([ys[r][k][c] for k in S.points_of(r) for c in range(Cs[r])])
    proof, st = pcs.open(Mw, ts, [np.array(c, dtype=np.uint64) for c in coefs], z, SEED)
    assert st == 0 and proof.tolist() == want
    roots = np.concatenate([pcs.root(t) for t in ts])
    assert pcs.verify(roots, z, SEED, proof) == 0
    bad = proof.copy()
    bad[-1] ^= np.uint64(1)
    assert pcs.verify(roots, z, SEED, bad) == MR.verify(S, [t.root_hash() for t in trees], zs, SEED, bad.tolist()) == 8
    with pytest.raises(L.RonkPanic):
        pcs.open([Mw[0].ravel()[:-1]] + Mw[1:], ts, [np.array(c, dtype=np.uint64) for c in coefs], z, SEED)
    with pytest.raises(L.RonkPanic):
        pcs.open(Mw[:-1], ts, [np.array(c, dtype=np.uint64) for c in coefs], z, SEED)


def test_create_errors_on_the_device():
    """the codes of ronk_mpcs_check through ronk_mpcs_create, with a live Poseidon handle"""
    pos = L.PoseidonHandle(*params(FIELDS[0]).create_args())
    for args, code in (((7, 7, 33, 7, 3, 3, 1, 8, 2, 2, (4, 2), (3, 1)), L.ERR_NO_ROOT), ((7, 49, 12, 7, 3, 3, 1, 8, 2, 2, (4, 2), (3, 1)), L.ERR_INVALID),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 2, (4, 0), (3, 1)), L.ERR_INVALID), ((7, 7, 12, 7, 3, 3, 1, 8, 2, 2, (4, 2), (1, 1)), L.ERR_INVALID),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 2, (4, 2), (3, 4)), L.ERR_INVALID), ((7, 7, 12, 7, 3, 3, 1, 8, 2, 9, (4,), (511,)), L.ERR_UNSUPPORTED),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 1, (1,) * 9, (1,) * 9), L.ERR_UNSUPPORTED),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 2, (1000, 25), (3, 1)), L.ERR_UNSUPPORTED)):
        with pytest.raises(L.RonkPanic) as e:
            L.MpcsHandle(pos, *args)
        assert e.value.code == code, args
    pos.close()


# ------------------------------------------------------------------------------------------------ (d) a PLONK proof from the parts
PLONK_LOG2_N, PLONK_LOG2_B = 4, 2
PLONK_COLUMNS, PLONK_MASKS = (8, 3, 2, 8), (0b01, 0b01, 0b11, 0b01)      # preprocessed (5 selectors, 3 sigma), wires, Z planes, T chunks


def plonk_identity(E, dom, ys, zeta, pi_zeta, alpha, beta, gamma):
    """G + alpha P1 + alpha^2 P2 == T(zeta) (zeta^N - 1) from the claims of the four rounds alone (and the public input's value):
    Z at zeta and at zeta w_N, everything else at zeta, T(zeta) = sum_j zeta^(j N) T_j(zeta)"""
    t = (0, 1)
    N = dom.N
    ql, qr, qm, qo, qc = ys[0][0][:5]
    sigma = ys[0][0][5:8]
    a, b, o = ys[1][0]
    Z, Zw = (E.add(y[0], E.mul(t, y[1])) for y in (ys[2][0], ys[2][1]))
    Tj = [E.add(ys[3][0][j], E.mul(t, ys[3][0][4 + j])) for j in range(4)]
    G = E.add(E.add(E.add(E.mul(a, ql), E.mul(b, qr)), E.add(E.mul(E.mul(a, b), qm), E.mul(o, qo))), E.add(qc, pi_zeta))
    num, den = Z, Zw
    for c, wv in enumerate((a, b, o)):
        num = E.mul(num, E.add(E.add(wv, E.mul(beta, E.mul_base(zeta, PL.LABELS[c] % E.p))), gamma))
        den = E.mul(den, E.add(E.add(wv, E.mul(beta, sigma[c])), gamma))
    vanish = E.sub(E.pow(zeta, N), E.one)
    L1 = E.mul(vanish, E.inv(E.mul_base(E.sub(zeta, E.one), N % E.p)))
    P2 = E.mul(E.sub(Z, E.one), L1)
    lhs = E.add(E.add(G, E.mul(alpha, E.sub(num, den))), E.mul(E.mul(alpha, alpha), P2))
    T, zN = E.zero, E.pow(zeta, N)
    for tj in reversed(Tj):
        T = E.add(E.mul(T, zN), tj)
    return lhs == E.mul(T, vanish)


def plonk_cpu_claims(E, dom, c, wires, sigma, alpha, beta, gamma, zs):
    """the claims of the four rounds from the restatement alone (tests/plonk_ref.py): ys[r][k][c] at the rounds' points"""
    p, N = dom.p, dom.N
    t, _ = PL.trace_columns(E, dom, c, wires, sigma, beta, gamma)
    T = PL.quotient(E, dom, PL.on_coset(dom, t), alpha, beta, gamma)
    planes = [PL.coset_coefficients(dom, [v[plane] for v in T]) for plane in (0, 1)]
    chunks = [plane[j * N:(j + 1) * N] for plane in planes for j in range(4)]
    rounds = [[PL.interpolate(p, dom.wN, col) for col in cols] for cols in (list(t.sel) + list(t.sigma), t.wires, t.Z)] + [chunks]
    return [[[PL.evaluate_ext(E, f, zs[k]) for f in rounds[r]] if (PLONK_MASKS[r] >> k) & 1 else None for k in range(2)] for r in range(4)]


@pytest.mark.parametrize("p", FIELDS)
def test_plonk_proof_from_the_library_parts(torch, p):
    """trace N = 2^4, B = 4, FRI domain 2^6, arity 2: ronk_lde_batch_dev, ronk_perm_product_dev, ronk_plonk_quotient_dev, the inverse
    coset transform and the chunking of both planes of T; four rounds opened at zeta and zeta w_N under ONE FRI.  The verifier
    accepts, and the PLONK identity recomputed from the proof's claims holds at zeta; with one witness word changed the openings
    still verify and the identity fails (the restatement shows both on the CPU before the device runs)."""
    log2_n, log2_b = PLONK_LOG2_N, PLONK_LOG2_B
    g = shift = w = GEN[p]
    N, M = 1 << log2_n, 1 << (log2_n + log2_b)
    rng = np.random.default_rng(64)
    dom = PL.Domain(p, g, log2_n, log2_b, shift)
    E = PL.Ext2(p, w)
    c = PL.circuit(rng, p, log2_n)
    ids = PL.labels(dom)
    sigma = PL.sigma_of(c, ids)
    alpha, beta, gamma, zeta = ([int(v) % p for v in rng.integers(0, 2**62, size=2)] for _ in range(4))
    alpha, beta, gamma, zeta = E.el(alpha), E.el(beta), E.el(gamma), E.el(zeta)
    zs = [zeta, E.mul_base(zeta, dom.wN)]
    pi_zeta = PL.evaluate_ext(E, PL.interpolate(p, dom.wN, c.pi), zeta)       # public: the verifier evaluates it itself
    good = PL.witness(c)
    bad = [list(col) for col in good]
    gate_rows = [i for i in range(N) if c.sel[3][i]]
    bad[2][gate_rows[-1]] = (bad[2][gate_rows[-1]] + 1) % p
    # the restatement, before the device runs: the identity holds for the witness and fails with one word changed
    cpu = {name: plonk_cpu_claims(E, dom, c, wires, sigma, alpha, beta, gamma, zs) for name, wires in (("good", good), ("bad", bad))}
    assert plonk_identity(E, dom, cpu["good"], zeta, pi_zeta, alpha, beta, gamma)
    assert not plonk_identity(E, dom, cpu["bad"], zeta, pi_zeta, alpha, beta, gamma)

    I = Instance(p, log2_n + log2_b, 1, 2, log2_b, 2, PLONK_COLUMNS, PLONK_MASKS)
    S = I.S
    d_ch = [dev(torch, np.array(v, dtype=np.uint64)) for v in (alpha, beta, gamma)]
    handle = C.c_void_p()
    L.check(L.lib.ronk_plonk_create(C.byref(handle), p, g, w, log2_n, log2_b, shift, (C.c_uint64 * 3)(*PL.LABELS)))
    pk, pn, inv = L.Plan(p, g, log2_n, 16), L.Plan(p, g, log2_n + log2_b, 16), L.Plan(p, g, log2_n + log2_b, 1)
    sinv = pow(shift, -1, p)
    unshift = [pow(sinv, j, p) for j in range(M)]
    xs = dom.points()

    def garbage(n):
        return torch.full((n,), -1, dtype=torch.int64, device="cuda")

    def prove(wires):
        d_w, d_i, d_s = (dev(torch, np.array(a, dtype=np.uint64).ravel()) for a in (wires, ids, sigma))
        d_Z, d_last, d_work = garbage(2 * N), garbage(2), garbage(L.lib.ronk_scan_workspace_words(N))
        d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        L.check(L.lib.ronk_perm_product_dev(p, w, d_w.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), 3, N, d_ch[1].data_ptr(),
                                            d_ch[2].data_ptr(), d_Z.data_ptr(), d_last.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), 0))
        assert int(d_st.item()) == 0
        # one batch of 16 columns in round order: selectors 5, sigma 3 | wires 3 | the planes of Z | pi and two spare
        d_in = torch.cat([dev(torch, np.array(list(c.sel) + sigma + wires, dtype=np.uint64).ravel()), d_Z,
                          dev(torch, np.array(c.pi, dtype=np.uint64)), torch.zeros(2 * N, dtype=torch.int64, device="cuda")])
        d_co, d_cols = garbage(16 * N), garbage(16 * M)
        L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_in.data_ptr(), d_co.data_ptr(), d_cols.data_ptr(), shift, 0))
        base = d_cols.data_ptr()
        d_T = garbage(2 * M)
        L.check(L.lib.ronk_plonk_quotient_dev(handle, base + 8 * 8 * M, base, base + 8 * 5 * M, base + 8 * 13 * M, base + 8 * 11 * M,
                                              d_ch[0].data_ptr(), d_ch[1].data_ptr(), d_ch[2].data_ptr(), d_T.data_ptr(), 0))
        d_c = garbage(2 * M)
        for plane in (0, 1):
            L.check(L.lib.ronk_ntt_inverse_dev(inv.h, d_T.data_ptr() + 8 * plane * M, d_c.data_ptr() + 8 * plane * M, 0))
        planes = [[v * u % p for v, u in zip(plane, unshift)] for plane in host(torch, d_c).reshape(2, M).tolist()]
        chunks = [plane[j * N:(j + 1) * N] for plane in planes for j in range(4)]
        d_tc = dev(torch, np.array(chunks, dtype=np.uint64).ravel())
        d_tm = dev(torch, np.array([[PL.evaluate(p, f, x) for x in xs] for f in chunks], dtype=np.uint64).ravel())
        d_Ms = [d_cols[0:8 * M], d_cols[8 * M:11 * M], d_cols[11 * M:13 * M], d_tm]
        # the coefficients of the thirteen committed columns (d_co is scratch of the extension: scaled by s^j), from the trace
        # values as the device holds them
        co = [PL.interpolate(p, dom.wN, col) for col in host(torch, d_in).reshape(16, N)[:13].tolist()]
        d_coefs = [dev(torch, np.array(co[a:b], dtype=np.uint64).ravel()) for a, b in ((0, 8), (8, 11), (11, 13))] + [d_tc]
        d_trees = [I.commit_dev(torch, r, d_Ms[r]) for r in range(4)]
        proof, st = I.open_raw(torch, d_Ms, d_trees, d_coefs, zs, SEED)
        assert st == 0
        roots = [host(torch, t)[-D:].tolist() for t in d_trees]
        return proof, roots

    for name, wires in (("good", good), ("bad", bad)):
        proof, roots = prove(wires)
        assert I.verify_dev(torch, roots, zs, SEED, proof) == 0, name
        ys = MR.claims_from_words(S, proof[:2 * S.Y].tolist())
        assert ys == cpu[name], name
        assert plonk_identity(E, dom, ys, zeta, pi_zeta, alpha, beta, gamma) == (name == "good")
    L.check(L.lib.ronk_plonk_destroy(handle))
    I.close()
