"""tests/deep_ref.py, the restatement of the batched FRI polynomial commitment, against the definitions it restates: the codeword
G of correct claims is of low degree and that of a wrong claim is not, the S_i / Y_k form equals the double sum, the leaf
addressing, an honest proof verifies and each tampered section gives its status bit.  No device."""
import random

import pytest

import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR

FIELDS = [PR.GOLDILOCKS, PR.MONT_P]
GEN = {PR.GOLDILOCKS: 7, PR.MONT_P: 10}


def params(p):
    return PR.derive_params(p, 8, 7, 2, 4, 4)


def instance(p, n, C, K, eta=1, log2_final=2, log2_blowup=1, shift=None, Q=4):
    return DR.Pcs(params(p), GEN[p], GEN[p], n, GEN[p] if shift is None else shift, eta, log2_final, log2_blowup, Q, 2, C, K)


def random_case(S, seed):
    rng = random.Random(seed)
    coef = [[rng.randrange(S.p) for _ in range(S.d)] for _ in range(S.C)]
    zs = [(rng.randrange(S.p), rng.randrange(1, S.p)) for _ in range(S.K)]
    return coef, DR.columns(S, coef), zs, (rng.randrange(S.p), rng.randrange(S.p))


def plane_coefficients(S, plane):
    """the interpolant of N values on the domain s <w_N>"""
    p, N = S.p, S.N
    c = FR.fft(p, plane, pow(S.F.root(N), -1, p))
    ninv, sinv = pow(N, -1, p), pow(S.F.shift, -1, p)
    return [v * ninv * pow(sinv, k, p) % p for k, v in enumerate(c)]


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("n", [6, 8])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("K", [1, 2])
def test_codeword_degree(p, n, C, K):
    """each quotient (f_c - f_c(z)) / (x - z) has degree d - 2, so both planes of G have zero coefficients from d - 1 on; with one
    wrong claim a pole remains and they do not"""
    S = instance(p, n, C, K)
    coef, M, zs, alpha = random_case(S, 1000 * n + 10 * C + K)
    ys = DR.claims(S, coef, zs)
    assert M[0][5] == sum(c * pow(S.point(5), j, p) for j, c in enumerate(coef[0])) % p
    G, status = DR.combine(S, M, ys, zs, alpha)
    assert status == 0
    for plane in (0, 1):
        assert not any(plane_coefficients(S, [g[plane] for g in G])[S.d - 1:])
    bad = [list(row) for row in ys]
    bad[K - 1][C - 1] = S.E.add(bad[K - 1][C - 1], (1, 0))
    Gb, _ = DR.combine(S, M, bad, zs, alpha)
    assert any(any(plane_coefficients(S, [g[plane] for g in Gb])[S.d - 1:]) for plane in (0, 1))


@pytest.mark.parametrize("p", FIELDS)
def test_sy_form_equals_the_double_sum(p):
    S = instance(p, 6, 3, 2)
    coef, M, zs, alpha = random_case(S, 5)
    ys = DR.claims(S, coef, zs)
    for a in (alpha, (0, 0), (1, 0), (0, 1), (p - 1, p - 1)):
        assert DR.combine_sy(S, M, ys, zs, a) == DR.combine(S, M, ys, zs, a)
    # raw words >= p in the matrix and the points, a point with z1 = 0 off the domain, a point ON the domain (zero inverse, bit 32)
    if p + 5 < 2**64:
        M[1][3] += p
        zs[0] = (zs[0][0] + p, zs[0][1])
    zs[1] = (12345, 0)
    assert not DR.on_domain(S, zs[1])
    assert DR.combine_sy(S, M, ys, zs, alpha) == DR.combine(S, M, ys, zs, alpha)
    zs[1] = (S.point(9), 0)
    G, status = DR.combine_sy(S, M, ys, zs, alpha)
    assert status == 32 and (G, status) == DR.combine(S, M, ys, zs, alpha)
    E = S.E
    want9 = E.zero      # at i = 9 only the terms of z_0 remain
    q = E.inv(E.sub(E.embed(S.point(9)), E.el(zs[0])))
    for c in range(S.C):
        want9 = E.add(want9, E.mul(E.pow(E.el(alpha), c), E.mul(E.sub(E.embed(M[c][9]), ys[0][c]), q)))
    assert G[9] == want9


def test_evaluation_and_layout():
    p = PR.GOLDILOCKS
    S = instance(p, 6, 3, 2, eta=2, log2_final=2)
    coef, M, zs, _ = random_case(S, 9)
    E = S.E
    z = zs[0]
    direct, zp = E.zero, E.one
    for c in coef[1]:
        direct = E.add(direct, E.mul_base(zp, c))
        zp = E.mul(zp, z)
    ys = DR.claims(S, coef, zs)
    assert ys[0][1] == direct
    assert DR.evaluate_ext(E, coef[2], (S.point(7), 0)) == (M[2][7], 0)
    words = DR.claim_words(S, ys)
    assert len(words) == 2 * S.K * S.C and (words[1 * S.C + 2], words[S.K * S.C + 1 * S.C + 2]) == ys[1][2]
    flat = [v for row in M for v in row]
    for j in (0, 5, S.m - 1):
        leaf = DR.leaf_words(S, M, j)
        assert len(leaf) == S.C * S.A
        assert leaf == [flat[DR.leaf_address(S, j, q)] for q in range(S.C * S.A)]
        # every column's values on the coset of FRI's layer-0 leaf j
        assert [leaf[c * S.A + t] for c in range(S.C) for t in range(S.A)] == [M[c][j + t * S.m] for c in range(S.C) for t in range(S.A)]
    assert S.proof_words() == 2 * 6 + S.F.proof_words() + S.Q * 12 + S.Q * 4 * S.D
    assert S.workspace_words() == S.D + S.Q + 2 * 64 + S.F.workspace_words()


@pytest.mark.parametrize("p", FIELDS)
def test_prover_and_verifier(p):
    S = instance(p, 6, 2, 2, eta=1, log2_final=2, Q=4)
    coef, M, zs, _ = random_case(S, 21)
    seed = [3, 4]
    tree = DR.commit(S, M)
    root = tree.root_hash()
    proof, status = DR.open_(S, M, tree, coef, zs, seed)
    assert status == 0 and DR.verify(S, root, zs, seed, proof) == 0
    ys, fri, leaves, paths = DR.split(S, proof)
    assert ys == DR.claims(S, coef, zs)
    a = DR.challenge(S, seed, root, zs, ys)
    assert FX.verify(S.F, fri, a) == 0
    roots, final, vals, _ = FX.split(S.F, fri)
    idx = FX.transcript(S.F, a, roots, final)[1]
    assert leaves == [DR.leaf_words(S, M, idx[q][0]) for q in range(S.Q)]
    G = DR.combine(S, M, ys, zs, (a[0], a[1]))[0]
    for q in range(S.Q):
        assert vals[0][q] == FX.leaf_words(S.F, G, 0, idx[q][0])
    # a false claim, proved honestly: the codeword is not of low degree
    bad_ys = [list(r) for r in ys]
    bad_ys[1][0] = S.E.add(bad_ys[1][0], (0, 1))
    bad, _ = DR.open_(S, M, tree, coef, zs, seed, ys=bad_ys)
    assert DR.verify(S, root, zs, seed, bad) == 4
    # one word of each section
    off = DR.section_offsets(S)
    F = S.F
    flips = {"claim": off["claims"] + 1, "fri root": off["fri"], "final": off["fri"] + F.L * S.D + 1,
             "fri leaf": off["fri"] + F.L * S.D + 2 * F.size(F.L) + 1, "matrix leaf": off["leaves"] + 2 * S.leaf_len() + 1,
             "matrix path": off["paths"] + 1}
    seen = {}
    for what, at in flips.items():
        t = list(proof)
        t[at] ^= 1 << 5
        seen[what] = DR.verify(S, root, zs, seed, t)
        assert seen[what] != 0, what
    assert seen["matrix path"] == 8 and seen["matrix leaf"] == 8 | 16 and seen["fri leaf"] & 16 and seen["final"] & 4
    # the DEEP check alone: FRI run on another low-degree codeword than the combination of the committed matrix
    shifted, _ = DR.open_(S, M, tree, coef, zs, seed, tweak=lambda G: [S.E.add(g, (1, 0)) for g in G])
    assert DR.verify(S, root, zs, seed, shifted) == 16
    # an untouched proof against another point or another root
    other = [(zs[0][0] + 1, zs[0][1]), zs[1]]
    assert DR.verify(S, root, other, seed, proof) & 16
    assert DR.verify(S, [root[0] ^ 1, root[1]], zs, seed, proof) & 8
    # a point on the domain is reported by prover and verifier
    zd = [(S.point(3), 0), zs[1]]
    pd, st = DR.open_(S, M, tree, coef, zd, seed)
    assert st == 32 and DR.verify(S, root, zd, seed, pd) & 32
