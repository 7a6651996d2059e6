"""Pins tests/fri_ext_ref.py, the restatement of FRI with extension challenges: the coefficient identity of the fold with beta in
the extension for every arity, the tie to the pinned base restatement (tests/fri_ref.py) under beta = (b, 0), leaf locality in the
planar addressing, and the verifier's status bits on an honest and on tampered proofs."""
import random

import pytest

import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR

FIELDS = [(PR.GOLDILOCKS, 7), (PR.MONT_P, 10)]   # (p, g); W = g, a generator is a non-residue
Q, D = 8, 2


def params(p):
    return PR.derive_params(p, 8, 7, 2, 4, 4)


def instance(p, g, n, eta, log2_final, log2_blowup, input_ext, shift=None):
    return FX.FriExt(params(p), g, g, n, g if shift is None else shift, eta, log2_final, log2_blowup, Q, D, input_ext)


def ext_codeword(F, rng, degree):
    """the planar values on layer 0 of a polynomial with extension coefficients, and those coefficients as pairs"""
    c = [(rng.randrange(F.p), rng.randrange(F.p)) for _ in range(degree)]
    return FR.evaluate(F, [v[0] for v in c]) + FR.evaluate(F, [v[1] for v in c]), c


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_fold_is_the_coefficient_identity(p, g, eta):
    """the fold of the values of sum c_k x^k is the values of sum_k (sum_(j < A) beta^j c_(A k + j)) x^k on the next domain"""
    n = 6
    F = instance(p, g, n, eta, n - eta, 0, 1)
    E, A = F.E, F.A
    rng = random.Random(eta)
    words, c = ext_codeword(F, rng, 1 << n)
    for beta in ((rng.randrange(p), rng.randrange(p)), (0, 1), (p - 1, p - 1)):
        gk = []
        for k in range((1 << n) // A):
            acc = E.zero
            for j in range(A):
                acc = E.add(acc, E.mul(E.pow(beta, j), c[A * k + j]))
            gk.append(acc)
        want = ER.pairs(FR.evaluate(F, [v[0] for v in gk], 1) + FR.evaluate(F, [v[1] for v in gk], 1))
        assert FX.fold(F, FX.layer0(F, words), beta, 0) == want


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_base_challenge_gives_the_base_fold(p, g, eta):
    """input_ext = 0 and beta = (b, 0): the c0 plane is fri_ref.fold, the c1 plane is zero"""
    n = 7
    F = instance(p, g, n, eta, n - eta, 0, 0)
    B = FR.Fri(params(p), g, n, g, eta, n - eta, 0, Q, D)
    rng = random.Random(eta + 10)
    v = [rng.randrange(2 ** 64) for _ in range(1 << n)]
    b = rng.randrange(p)
    got = FX.fold(F, FX.layer0(F, v), (b, 0), 0)
    assert [x[0] for x in got] == FR.fold(B, v, b, 0) and all(x[1] == 0 for x in got)


def test_leaf_locality_in_the_planar_addressing():
    """output i of a layer reads only Merkle leaf i, whose word j = c A + t sits at offset i + j m of the planar layer"""
    p, g = FIELDS[0]
    F = instance(p, g, 8, 2, 2, 0, 1)
    rng = random.Random(3)
    f = [(rng.randrange(p), rng.randrange(p)) for _ in range(F.size(1))]
    words, m, A = ER.planar(f), F.leaves(1), F.A
    beta = (rng.randrange(p), rng.randrange(p))
    out = FX.fold(F, f, beta, 1)
    for i in (0, 1, m - 1):
        leaf = FX.leaf_words(F, f, 1, i)
        assert len(leaf) == 2 * A == F.leaf_len(1)
        assert leaf == [words[FX.planar_address(F, 1, i, j)] for j in range(2 * A)]
        # the fold of the leaf alone, as a one-leaf layer on the point x_i
        x, w, b = F.layer_shift(1) * pow(F.root(F.size(1)), i, p) % p, F.root(A), beta
        one = [(leaf[t], leaf[A + t]) for t in range(A)]
        while len(one) > 1:
            one = FX.fold2(F.E, one, b, x, w)
            x, w, b = x * x % p, w * w % p, F.E.mul(b, b)
        assert one[0] == out[i]
        # and no other leaf's words matter
        g2 = list(f)
        for k in range(len(f)):
            if k % m != i:
                g2[k] = (0, 0)
        assert FX.fold(F, g2, beta, 1)[i] == out[i]
    assert FX.leaf_words(instance(p, g, 8, 2, 2, 0, 0), [(v, 0) for v in range(256)], 0, 5) == [5, 69, 133, 197]


def test_sizes():
    p, g = FIELDS[0]
    for input_ext in (0, 1):
        F = instance(p, g, 9, 3, 3, 1, input_ext)
        A, L = 8, 2
        assert F.proof_words() == L * D + 2 * 8 + Q * ((1 + input_ext) * A + 6 * D) + Q * (2 * A + 3 * D)
        assert F.workspace_words() == 2 * 64 + (2 * 64 - 1) * D + 2 * 8 + (2 * 8 - 1) * D + 2 * L + (L + 2) * D + L * Q + Q


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("input_ext", [0, 1])
def test_verifier_statuses(p, g, input_ext):
    n, eta, log2_final = 6, 1, 2
    F = instance(p, g, n, eta, log2_final, 1, input_ext)
    rng = random.Random(p % 1000 + input_ext)
    if input_ext:
        f, _ = ext_codeword(F, rng, 1 << (n - 1))
    else:
        f = FR.evaluate(F, [rng.randrange(p) for _ in range(1 << (n - 1))])
    seed = [3, 4]
    proof = FX.prove(F, f, seed)
    assert FX.verify(F, proof, seed) == 0
    A, L, nl = F.A, F.L, F.size(F.L)
    off_final = L * D
    off_leaf0 = off_final + 2 * nl
    off_path0 = off_leaf0 + Q * F.leaf_len(0)
    off_leaf1 = off_path0 + Q * F.depth(0) * D

    def status(at, bit=7):
        bad = list(proof)
        bad[at] ^= 1 << bit
        return FX.verify(F, bad, seed)

    assert status(off_path0 + 3 * F.depth(0) * D + 1, 0) == 1                 # a path word
    # a leaf word of an inner (planar) layer, c0 half and c1 half: the leaf's digest changes too
    assert status(off_leaf1 + 2 * 2 * A + 1) == 3
    assert status(off_leaf1 + 2 * 2 * A + A + 1) == 3
    # a final word of the c1 plane: the plane's degree (and, as u changes, other queries are asked: the other bits may follow)
    assert status(off_final + nl + 1) & 4 and status(off_final + 1) & 4
    # a c1 word >= p in the place of its residue is no fold value, and the transcript absorbs the word as it stands
    j = FX.transcript(F, seed, *FX.split(F, proof)[:2])[1][0][L - 1]     # where query 0 lands in the final layer
    if proof[off_final + nl + j] + p < 2 ** 64:
        bad = list(proof)
        bad[off_final + nl + j] += p
        assert FX.verify(F, bad, seed) != 0
    # values on no low-degree polynomial, proved honestly: only the final layer tells
    rnd = [rng.randrange(p) for _ in range((1 + input_ext) << n)]
    assert FX.verify(F, FX.prove(F, rnd, seed), seed) == 4
    # a c1 plane on no low-degree polynomial under a low-degree c0 plane
    if input_ext:
        mixed = f[:1 << n] + rnd[1 << n:]
        assert FX.verify(F, FX.prove(F, mixed, seed), seed) == 4
