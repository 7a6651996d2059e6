"""The batched FRI polynomial commitment on the device (ronk_pcs_*, ronk_deep_combine_dev, ronk_ext2_poly_eval_batch*,
ronk_fri_query_indices_dev), word for word against the Python restatement (tests/deep_ref.py).  W is the field's generator.  The
64-bit primes run with TEST Poseidon parameters derived in poseidon_ref.py (not a standard instance)."""
import random

import numpy as np
import pytest

import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from test_gpu_fri import CASES, CLASS_FIELDS, D, FIELDS, GEN, Q, _Field, dev, fold_final, host, params, words
from test_gpu_fri import reference as base_reference
from test_gpu_fri_ext import reference as ext_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class Instance:
    """a library handle and the restatement's object for the same parameters"""

    def __init__(self, p, n, eta, log2_final, log2_blowup, C, K, shift=None, w=None):
        self.P = params(p)
        self.p = p
        shift = GEN[p] if shift is None else shift
        w = GEN[p] if w is None else w
        self.S = DR.Pcs(self.P, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, C, K)
        self.pos = L.PoseidonHandle(*self.P.create_args())
        self.h = L.PcsHandle(self.pos, GEN[p], w, n, shift, eta, log2_final, log2_blowup, Q, D, C, K)
        assert self.h.proof_words == self.S.proof_words() and self.h.workspace_words == self.S.workspace_words()

    def combine_dev(self, torch, d_M, ys, zs, alpha):
        S = self.S
        d_y = dev(torch, np.array(ER.planar([y for row in ys for y in row]), dtype=np.uint64))
        d_z, d_a = dev(torch, np.array(ER.planar(zs), dtype=np.uint64)), dev(torch, np.array(alpha, dtype=np.uint64))
        d_G = torch.full((2 * S.N,), -1, dtype=torch.int64, device="cuda")
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.combine_dev(d_M.data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_a.data_ptr(), d_G.data_ptr(), d_st.data_ptr())
        return host(torch, d_G).tolist(), int(d_st.item())

    def commit_dev(self, torch, d_M):
        d_tree = torch.full((self.h.tree_words,), -1, dtype=torch.int64, device="cuda")
        self.h.commit_dev(d_M.data_ptr(), d_tree.data_ptr())
        return d_tree

    def open_dev(self, torch, d_M, d_tree, coef, zs, seed, fill=-1):
        d_coef, d_seed = dev(torch, np.array(coef, dtype=np.uint64).ravel()), dev(torch, seed)
        d_z = dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
        d_work = torch.full((self.h.workspace_words,), fill, dtype=torch.int64, device="cuda")
        d_proof = torch.full((self.h.proof_words,), fill, dtype=torch.int64, device="cuda")
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.open_dev(d_M.data_ptr(), d_tree.data_ptr(), d_coef.data_ptr(), d_z.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(),
                        d_proof.data_ptr(), d_st.data_ptr())
        return host(torch, d_proof), int(d_st.item())

    def verify_dev(self, torch, root, zs, seed, proof):
        d_root, d_seed, d_proof = dev(torch, root), dev(torch, seed), dev(torch, proof)
        d_z = dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        self.h.verify_dev(d_root.data_ptr(), d_z.data_ptr(), d_seed.data_ptr(), d_proof.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        return int(d_st.item())

    def close(self):
        self.h.close()
        self.pos.close()


# ------------------------------------------------------------------------------------------------ (a) evaluation at extension points
EVAL_CASES = [(1, 1, 1), (1, 33, 3), (2, 3, 3), (255, 16, 1), (256, 33, 3), (257, 3, 3), (257, 1, 1), (4096, 16, 3), (4096, 3, 1)]


def check_eval_batch(torch, p, cases):
    E = ER.Ext2(p, GEN[p])
    rng = random.Random(3)
    special = [(0, 0), (1, 0), (0, 1), (rng.randrange(p), rng.randrange(p)), (p + 1, p + 2) if p + 2 < 2**64 else (p, 2**64 - 1)]
    for d, C, K in cases:
        it = EVAL_CASES.index((d, C, K))
        coef = words(50 + it, C * d, p).reshape(C, d)
        zs = [special[(it + k) % 5] for k in range(K)] if d < 4096 else [special[3], special[4], special[2]][:K]
        want = ER.planar([DR.evaluate_ext(E, coef[c].tolist(), z) for z in zs for c in range(C)])
        d_coef, d_z = dev(torch, coef.ravel()), dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
        d_y = torch.full((2 * K * C,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.ronk_ext2_poly_eval_batch_dev(p, GEN[p], d_coef.data_ptr(), C, d, d_z.data_ptr(), K, d_y.data_ptr(), None))
        assert host(torch, d_y).tolist() == want, (p, d, C, K)
        if d <= 257:
            assert L.ext2_poly_eval_batch(p, GEN[p], coef, np.array(ER.planar(zs), dtype=np.uint64)).tolist() == want, (p, d, C, K)


@pytest.mark.parametrize("p", FIELDS)
def test_eval_batch_against_restatement(torch, p):
    """one and several rounds per lane with a partial last round (d around the 256 lanes of a workgroup), one and several columns,
    edge words in the coefficients; points zero, one, t, random and with components >= p"""
    check_eval_batch(torch, p, EVAL_CASES)


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_eval_batch_prime_classes(torch, p):
    """the primes of tests/prime_classes.py (every outcome of mont64::add): a partial last round, and a full one with 33 columns"""
    check_eval_batch(torch, p, [(257, 3, 3), (256, 33, 3)])


# ------------------------------------------------------------------------------------------------ (b) the DEEP codeword
def combine_case(torch, I, M, d_M, rng, alpha, on_domain=None, base_point=False):
    S, p = I.S, I.p
    zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(S.K)]
    if base_point:
        zs[0] = (rng.randrange(p), 0)                 # z1 = 0, off the domain
        assert not DR.on_domain(S, zs[0])
    if on_domain is not None:
        zs[S.K - 1] = (S.point(on_domain), 0)
    ys = [[(int(a), int(b)) for a, b in zip(words(rng.randrange(1 << 30), S.C, p), words(rng.randrange(1 << 30), S.C, p))] for _ in range(S.K)]
    want, st = DR.combine_sy(S, M, ys, zs, alpha)
    got, got_st = I.combine_dev(torch, d_M, ys, zs, alpha)
    assert st == (32 if on_domain is not None else 0)
    assert got_st == st and got == ER.planar(want), (p, S.F.n, S.F.eta, S.C, S.K, alpha, on_domain, base_point)


def check_combine(torch, p, eta, shapes):
    rng = random.Random(eta)
    rnd = (rng.randrange(p), rng.randrange(p))
    alphas = ((0, 0), (1, 0), (0, 1), (p - 1, p - 1), rnd, (p + 1 if p + 1 < 2**64 else p, rng.randrange(p)))
    for n, cases in shapes.items():
        for C, K, shift in cases:
            I = Instance(p, n, eta, fold_final(n, eta), 0, C, K, shift=shift)
            Mw = words(100 * n + eta + C, C << n, p)
            M, d_M = Mw.reshape(C, 1 << n).tolist(), dev(torch, Mw)
            for alpha in (alphas if n <= 9 else alphas[4:] if n == 12 else alphas[4:5]):
                combine_case(torch, I, M, d_M, rng, alpha)
            if n <= 12:
                combine_case(torch, I, M, d_M, rng, rnd, base_point=True)
                combine_case(torch, I, M, d_M, rng, rnd, on_domain=(1 << n) - 1)
                combine_case(torch, I, M, d_M, rng, rnd, on_domain=0)
            I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_combine_against_restatement(torch, p, eta):
    """one lane, one workgroup, several workgroups, both levels of the point table; one and several columns and points; s = 1 and
    s = g; alpha with zero, one, p - 1 and a word >= p among its components; a base-field point off the domain (status 0) and a
    domain point (status 32, the term is zero)"""
    check_combine(torch, p, eta, {eta + 1: [(C, K, s) for C in (1, 2, 16, 33) for K in (1, 2, 3) for s in ((1,) if (C + K) % 2 else (GEN[p],))],
                                  9: [(1, 1, 1), (2, 2, GEN[p]), (16, 3, 1), (33, 1, GEN[p])],
                                  12: [(16, 2, GEN[p]), (33, 3, 1)],
                                  16: [(2, 1, GEN[p])]})


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_combine_prime_classes(torch, p, eta):
    """the primes of tests/prime_classes.py (every outcome of mont64::add): one lane and several workgroups, one and 33 columns,
    one and three points, s = 1 and s = g; the base-field point and the domain points (status 32) with each"""
    corners = [(1, 1, 1), (1, 3, GEN[p]), (33, 1, GEN[p]), (33, 3, 1)]
    check_combine(torch, p, eta, {eta + 1: corners, 9: corners})


@pytest.mark.parametrize("p", [PR.GOLDILOCKS, CLASS_FIELDS[0]])
def test_combine_four_and_eight_points(torch, p):
    """the larger instantiations of the point count, which the cases above (K <= 3) do not reach: one lane with one column at
    eight points and five columns at four, and four workgroups over both levels of the point table at eight points with s = g"""
    check_combine(torch, p, 1, {2: [(1, 8, 1), (5, 4, GEN[p])], 12: [(3, 8, GEN[p])]})


def test_goldilocks_with_another_w(torch):
    """W = 7 over Goldilocks has a product with W of its own; another non-residue takes the ordinary product"""
    p = PR.GOLDILOCKS
    rng = random.Random(11)
    for w in (11, p - 7):
        I = Instance(p, 9, 2, 3, 0, 3, 2, w=w)
        Mw = words(w % 1000, 3 << 9, p)
        combine_case(torch, I, Mw.reshape(3, 1 << 9).tolist(), dev(torch, Mw), rng, (rng.randrange(p), rng.randrange(p)))
        I.close()


# ------------------------------------------------------------------------------------------------ (c) the query indices of a FRI proof
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("case", CASES)
def test_query_indices(torch, p, case):
    """the indices a proof's transcript implies, for a base handle and for extension handles; an existing proof is produced as the
    same words before and after the call"""
    n, eta, log2_final = case
    pos = L.PoseidonHandle(*params(p).create_args())
    for kind in ("base", 0, 1):
        if kind == "base":
            f, seed, want = base_reference(p, case)
            F = FR.Fri(params(p), GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)
            h = L.FriHandle(pos, GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)
            idx = FR.transcript(F, seed, *FR.split(F, want)[:2])[1]
        else:
            f, seed, want = ext_reference(p, case, kind)
            F = FX.FriExt(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, kind)
            h = L.FriHandle(pos, GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, w=GEN[p], input_ext=kind)
            idx = FX.transcript(F, seed, *FX.split(F, want)[:2])[1]

        def prove():
            d_ev, d_seed = dev(torch, f), dev(torch, seed)
            d_work = torch.full((h.workspace_words,), -1, dtype=torch.int64, device="cuda")
            d_proof = torch.full((h.proof_words,), -1, dtype=torch.int64, device="cuda")
            h.prove_dev(d_ev.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr())
            return d_proof

        d_proof = prove()
        assert host(torch, d_proof).tolist() == want
        d_idx = torch.full((Q,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.ronk_fri_query_indices_dev(h.h, d_proof.data_ptr(), dev(torch, seed).data_ptr(), d_idx.data_ptr(), None))
        assert host(torch, d_idx).tolist() == [idx[q][0] for q in range(Q)], (p, case, kind)
        assert host(torch, prove()).tolist() == want
        d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        h.verify_dev(d_proof.data_ptr(), dev(torch, seed).data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        assert int(d_st.item()) == 0
        h.close()
    pos.close()


# ------------------------------------------------------------------------------------------------ (d) open and verify
OPEN_CASES = [((6, 1, 2), 1, 1, 1), ((6, 1, 2), 2, 5, 2), ((9, 3, 3), 2, 5, 1), ((9, 3, 3), 1, 1, 2), ((12, 2, 4), 1, 5, 2)]
SEED = [3, 4]
_REF = {}


def reference(p, oc):
    """(coef, M, zs, tree, the restatement's proof), computed once per case"""
    key = (p, oc)
    if key not in _REF:
        (n, eta, log2_final), log2_blowup, C, K = oc
        S = DR.Pcs(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, C, K)
        rng = random.Random(n * 100 + eta + 7 * C + K)
        coef = [[rng.randrange(p) for _ in range(S.d)] for _ in range(C)]
        coef[0][0], coef[C - 1][S.d - 1] = 0, p - 1
        M = DR.columns(S, coef)
        zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(K)]
        tree = DR.commit(S, M)
        proof, st = DR.open_(S, M, tree, coef, zs, SEED)
        assert st == 0
        _REF[key] = (coef, M, zs, tree, proof)
    return _REF[key]


def instance_of(p, oc):
    (n, eta, log2_final), log2_blowup, C, K = oc
    return Instance(p, n, eta, log2_final, log2_blowup, C, K)


def check_proof(torch, p, oc):
    coef, M, zs, tree, want = reference(p, oc)
    I = instance_of(p, oc)
    d_M = dev(torch, np.array(M, dtype=np.uint64).ravel())
    d_tree = I.commit_dev(torch, d_M)
    assert host(torch, d_tree).tolist() == tree.flat()
    got, st = I.open_dev(torch, d_M, d_tree, coef, zs, SEED)
    assert st == 0 and got.tolist() == want, (p, oc)
    root = tree.root_hash()
    assert I.verify_dev(torch, root, zs, SEED, got) == 0
    # buffers poisoned with another pattern: no word is left unwritten; and a third call in a row on the same handle
    again, _ = I.open_dev(torch, d_M, d_tree, coef, zs, SEED, fill=0x55)
    assert np.array_equal(again, got)
    assert np.array_equal(I.open_dev(torch, d_M, d_tree, coef, zs, SEED)[0], got)
    assert I.verify_dev(torch, root, zs, SEED, got) == 0
    I.close()


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("oc", OPEN_CASES)
def test_proof_word_for_word(torch, p, oc):
    check_proof(torch, p, oc)


@pytest.mark.parametrize("p", CLASS_FIELDS)
@pytest.mark.parametrize("oc", [OPEN_CASES[1], OPEN_CASES[2]])
def test_proof_word_for_word_prime_classes(torch, p, oc):
    check_proof(torch, p, oc)


@pytest.mark.parametrize("p", FIELDS + CLASS_FIELDS)
@pytest.mark.parametrize("oc", [OPEN_CASES[1], OPEN_CASES[2]])
def test_verifier_statuses(torch, p, oc):
    coef, M, zs, tree, proof = reference(p, oc)
    I = instance_of(p, oc)
    S, F = I.S, I.S.F
    root = tree.root_hash()
    assert DR.verify(S, root, zs, SEED, proof) == 0 == I.verify_dev(torch, root, zs, SEED, proof)
    # a false claim, proved honestly by the restatement's prover
    ys = DR.claims(S, coef, zs)
    ys[S.K - 1][S.C - 1] = S.E.add(ys[S.K - 1][S.C - 1], (1, 0))
    bad, _ = DR.open_(S, M, tree, coef, zs, SEED, ys=ys)
    want = DR.verify(S, root, zs, SEED, bad)
    assert want != 0 and I.verify_dev(torch, root, zs, SEED, bad) == want
    # FRI run on another low-degree codeword than the combination: the DEEP check alone
    shifted, _ = DR.open_(S, M, tree, coef, zs, SEED, tweak=lambda G: [S.E.add(g, (1, 0)) for g in G])
    assert DR.verify(S, root, zs, SEED, shifted) == 16 == I.verify_dev(torch, root, zs, SEED, shifted)
    # one word of each section
    off = DR.section_offsets(S)
    flips = {"claim": off["claims"] + S.K * S.C, "fri root": off["fri"] + 1, "final": off["fri"] + F.L * D + 2 * F.size(F.L) - 1,
             "fri leaf": off["fri"] + F.L * D + 2 * F.size(F.L) + 3 * F.leaf_len(0) + 1, "matrix leaf": off["leaves"] + 5 * S.leaf_len() + 2,
             "matrix path": off["paths"] + 6 * F.depth(0) * D + 1}
    seen = {}
    for what, at in flips.items():
        t = list(proof)
        t[at] ^= 1 << 9
        seen[what] = DR.verify(S, root, zs, SEED, t)
        assert seen[what] != 0 and I.verify_dev(torch, root, zs, SEED, t) == seen[what], (p, oc, what)
    assert seen["matrix path"] == 8 and seen["matrix leaf"] == 8 | 16 and seen["fri leaf"] & 16 and seen["final"] & 4
    # a matrix leaf word >= p in the place of its residue: the same value for the DEEP check, another leaf for the tree
    at = off["leaves"] + 1
    if proof[at] + p < 2**64:
        t = list(proof)
        t[at] += p
        want = DR.verify(S, root, zs, SEED, t)
        assert I.verify_dev(torch, root, zs, SEED, t) == want
    # everything at once; another seed, another root, another point; a point on the domain
    t = list(proof)
    for at in flips.values():
        t[at] ^= 1 << 9
    assert I.verify_dev(torch, root, zs, SEED, t) == DR.verify(S, root, zs, SEED, t)
    for r, z, s in ((root, zs, [SEED[0] + 1, SEED[1]]), ([root[0] ^ 1, root[1]], zs, SEED), (root, [(zs[0][0] ^ 1, zs[0][1])] + zs[1:], SEED)):
        want = DR.verify(S, r, z, s, proof)
        assert want != 0 and I.verify_dev(torch, r, z, s, proof) == want
    zd = [(S.point(5), 0)] + zs[1:]
    d_M = dev(torch, np.array(M, dtype=np.uint64).ravel())
    pd, st = I.open_dev(torch, d_M, I.commit_dev(torch, d_M), coef, zd, SEED)
    wd, wst = DR.open_(S, M, tree, coef, zd, SEED)
    assert st == wst == 32 and pd.tolist() == wd
    want = DR.verify(S, root, zd, SEED, wd)
    assert want & 32 and I.verify_dev(torch, root, zd, SEED, wd) == want
    I.close()


@pytest.mark.parametrize("p", FIELDS)
def test_host_forms(torch, p):
    oc = OPEN_CASES[1]
    (n, eta, log2_final), log2_blowup, C, K = oc
    coef, M, zs, tree, want = reference(p, oc)
    pcs = callers.FriPcs((_Field(p),) + params(p).create_args()[1:], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, C, K)
    Mw, z = np.array(M, dtype=np.uint64), np.array(ER.planar(zs), dtype=np.uint64)
    t = pcs.commit(Mw)
    assert t.tolist() == tree.flat() and pcs.root(t).tolist() == tree.root_hash()
    S = DR.Pcs(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, D, C, K)
    assert pcs.evaluate(coef, z).tolist() == DR.claim_words(S, DR.claims(S, coef, zs))
    proof, st = pcs.open(Mw, t, np.array(coef, dtype=np.uint64), z, SEED)
    assert st == 0 and proof.tolist() == want
    assert pcs.verify(pcs.root(t), z, SEED, proof) == 0
    bad = proof.copy()
    bad[-1] ^= np.uint64(1)
    assert pcs.verify(pcs.root(t), z, SEED, bad) == DR.verify(S, tree.root_hash(), zs, SEED, bad.tolist()) == 8
    with pytest.raises(L.RonkPanic):
        pcs.open(Mw.ravel()[:-1], t, np.array(coef, dtype=np.uint64), z, SEED)


def test_create_errors_on_the_device():
    """the codes of ronk_pcs_check through ronk_pcs_create, with a live Poseidon handle"""
    pos = L.PoseidonHandle(*params(PR.GOLDILOCKS).create_args())
    for args, code in (((7, 7, 33, 7, 3, 3, 1, 8, 2, 4, 2), L.ERR_NO_ROOT), ((7, 49, 12, 7, 3, 3, 1, 8, 2, 4, 2), L.ERR_INVALID),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 0, 2), L.ERR_INVALID), ((7, 7, 12, 7, 3, 3, 1, 8, 2, 4, 9), L.ERR_UNSUPPORTED),
                       ((7, 7, 12, 7, 3, 3, 1, 8, 2, 1025, 1), L.ERR_UNSUPPORTED), ((7, 7, 12, 7, 3, 3, 1, 8, 5, 4, 2), L.ERR_INVALID)):
        with pytest.raises(L.RonkPanic) as e:
            L.PcsHandle(pos, *args)
        assert e.value.code == code, args
    pos.close()
