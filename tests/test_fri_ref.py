"""The Python restatement of the library's FRI (tests/fri_ref.py) against the definitions it restates: the coefficient identity of a
layer, the locality of an output in its coset, an honest proof, and the status bit of every tampering class.  No GPU."""
import random

import pytest

import fri_ref as FR
import poseidon_ref as PR

GL, MONT, SMALL = PR.GOLDILOCKS, PR.MONT_P, 0xC0000001
GEN = {GL: 7, MONT: 10, SMALL: 5}


def instance(p, n, eta, log2_final, log2_blowup=1, queries=5, d=2, shift=None):
    P = PR.derive_params(p, 5, 5, 2, 4, 3)
    return FR.Fri(P, GEN[p], n, GEN[p] if shift is None else shift, eta, log2_final, log2_blowup, queries, d)


def codeword(F, seed):
    rng = random.Random(seed)
    coeffs = [rng.randrange(F.p) for _ in range(F.size(0) >> F.log2_blowup)]
    return coeffs, FR.evaluate(F, coeffs)


@pytest.mark.parametrize("p", [GL, MONT, SMALL])
@pytest.mark.parametrize("eta", [1, 2, 3])
def test_coefficient_identity(p, eta):
    """a layer maps the coefficients c to g_k = sum_(j < A) beta^j c_(A k + j), on the domain s^A <w_(N/A)>"""
    for shift in (1, GEN[p]):
        F = instance(p, 6, eta, 6 - eta, shift=shift)
        rng = random.Random(eta)
        c = [rng.randrange(p) for _ in range(64)]
        f = FR.evaluate(F, c)
        assert f[5] == sum(ck * pow(F.shift * pow(F.root(64), 5, p), k, p) for k, ck in enumerate(c)) % p
        for beta in (0, 1, p - 1, rng.randrange(p)):
            g = [sum(pow(beta, j, p) * c[F.A * k + j] for j in range(F.A)) % p for k in range(64 // F.A)]
            assert FR.fold(F, f, beta, 0) == FR.evaluate(F, g, 1), (p, eta, beta)


@pytest.mark.parametrize("eta", [1, 2, 3])
def test_leaf_locality(eta):
    """output i reads only f[i + t N/A]: every other word may change"""
    F = instance(GL, 7, eta, 7 - eta)
    rng = random.Random(3)
    f = [rng.randrange(F.p) for _ in range(128)]
    beta = rng.randrange(F.p)
    out = FR.fold(F, f, beta, 0)
    m = F.leaves(0)
    for i in (0, 1, m - 1):
        g = [v if k % m == i else rng.randrange(F.p) for k, v in enumerate(f)]
        assert FR.fold(F, g, beta, 0)[i] == out[i]
        g = list(f)
        g[i + (F.A - 1) * m] ^= 1
        assert FR.fold(F, g, beta, 0)[i] != out[i]


CASES = [(GL, 6, 1, 2), (MONT, 6, 2, 2), (SMALL, 7, 3, 1), (GL, 6, 3, 0)]


@pytest.mark.parametrize("p,n,eta,log2_final", CASES)
def test_honest_proof_and_tampering(p, n, eta, log2_final):
    F = instance(p, n, eta, log2_final, log2_blowup=min(1, log2_final))
    _, f = codeword(F, n * 10 + eta)
    seed = [11, 22]
    proof = FR.prove(F, f, seed)
    assert len(proof) == F.proof_words() and all(0 <= w < p for w in proof)
    assert FR.verify(F, proof, seed) == 0
    assert FR.verify(F, proof, [11, 23]) != 0                      # another seed: other challenges and indices
    roots, final, vals, paths = FR.split(F, proof)
    D, Q, A = F.D, F.Q, F.A
    off_final = F.L * D
    off_leaf0 = off_final + F.size(F.L)
    # a path word: only the Merkle check sees it
    if F.depth(0):
        bad = list(proof)
        bad[off_leaf0 + Q * A + 1] ^= 1
        assert FR.verify(F, bad, seed) == 1
    # a leaf value: its path fails and its fold no longer matches
    bad = list(proof)
    bad[off_leaf0 + 2 * A + 1] ^= 1
    assert FR.verify(F, bad, seed) == 3
    # a root: the transcript moves, and the root itself is wrong
    bad = list(proof)
    bad[0] ^= 1
    assert FR.verify(F, bad, seed) & 1
    # a final word: the queries move, and (with a blowup) the degree check fails
    bad = list(proof)
    bad[off_final] ^= 1
    st = FR.verify(F, bad, seed)
    assert st != 0 and (st & 4 or F.log2_blowup == 0)


def test_not_low_degree_is_bit_4():
    """an honest prover on random values: every opening and fold is consistent, the final layer is not of low degree"""
    F = instance(GL, 6, 2, 2)
    rng = random.Random(9)
    f = [rng.randrange(F.p) for _ in range(64)]
    assert FR.verify(F, FR.prove(F, f, [1, 2]), [1, 2]) == 4


def test_layout_formula():
    F = instance(GL, 12, 3, 3, queries=7, d=3)
    assert F.L == 3 and [F.size(l) for l in range(4)] == [4096, 512, 64, 8] and [F.depth(l) for l in range(3)] == [9, 6, 3]
    assert F.proof_words() == 3 * 3 + 8 + sum(7 * 8 + 7 * dp * 3 for dp in (9, 6, 3))
