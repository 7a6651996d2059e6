"""tests/mpcs_ref.py, the restatement of the multi-matrix polynomial commitment, against the definitions it restates: the codeword
G of correct claims is of low degree and that of one wrong claim in any single round is not, the per-round S_r / Y_r,k form equals
the triple sum (zero-inverse convention included), one round with a full mask is tests/deep_ref.py word for word, an honest proof
verifies and each tampered section gives its status bit.  No device."""
import random

import pytest

import deep_ref as DR
import mpcs_ref as MR
import poseidon_ref as PR
from test_deep_ref import FIELDS, GEN, params, plane_coefficients

SHAPES = [(1, (2,), (1,)), (2, (2, 1), (0b01, 0b10)), (2, (1, 3, 2), (0b11, 0b01, 0b11)), (2, (3, 2), (0b11, 0b11))]


def instance(p, n, K, Cs, masks, eta=1, log2_final=2, log2_blowup=1, Q=4):
    return MR.Mpcs(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, log2_blowup, Q, 2, K, Cs, masks)


def random_case(S, seed):
    rng = random.Random(seed)
    coefs = [[[rng.randrange(S.p) for _ in range(S.d)] for _ in range(C)] for C in S.Cs]
    zs = [(rng.randrange(S.p), rng.randrange(1, S.p)) for _ in range(S.K)]
    return coefs, MR.columns(S, coefs), zs, (rng.randrange(S.p), rng.randrange(S.p))


def bumped(S, ys, r):
    """one wrong claim in round r: its last point, its last column"""
    out = [[None if row is None else list(row) for row in rnd] for rnd in ys]
    k = S.points_of(r)[-1]
    out[r][k][S.Cs[r] - 1] = S.E.add(out[r][k][S.Cs[r] - 1], (1, 0))
    return out


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_codeword_degree(p, shape):
    """both planes of G have zero coefficients from d - 1 on for correct claims, and not for one wrong claim in any single round"""
    K, Cs, masks = shape
    S = instance(p, 6, K, Cs, masks)
    coefs, Ms, zs, alpha = random_case(S, 17 * len(Cs) + K)
    ys = MR.claims(S, coefs, zs)
    assert all((ys[r][k] is None) == (k not in S.points_of(r)) for r in range(S.R) for k in range(K))
    G, status = MR.combine(S, Ms, ys, zs, alpha)
    assert status == 0
    for plane in (0, 1):
        assert not any(plane_coefficients(S.rounds[0], [g[plane] for g in G])[S.d - 1:])
    for r in range(S.R):
        Gb, _ = MR.combine(S, Ms, bumped(S, ys, r), zs, alpha)
        assert any(any(plane_coefficients(S.rounds[0], [g[plane] for g in Gb])[S.d - 1:]) for plane in (0, 1)), r


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_sy_form_equals_the_triple_sum(p, shape):
    K, Cs, masks = shape
    S = instance(p, 6, K, Cs, masks)
    coefs, Ms, zs, alpha = random_case(S, 5)
    ys = MR.claims(S, coefs, zs)
    for a in (alpha, (0, 0), (1, 0), (0, 1), (p - 1, p - 1)):
        assert MR.combine_sy(S, Ms, ys, zs, a) == MR.combine(S, Ms, ys, zs, a)
    # raw words >= p in a matrix and a point, a point with z1 = 0 off the domain, a point ON the domain (zero inverse, bit 32)
    if p + 5 < 2**64:
        Ms[S.R - 1][0][3] += p
        zs[0] = (zs[0][0] + p, zs[0][1])
    zs[K - 1] = (12345, 0)
    assert not MR.on_domain(S, zs[K - 1])
    assert MR.combine_sy(S, Ms, ys, zs, alpha) == MR.combine(S, Ms, ys, zs, alpha)
    zs[K - 1] = (S.point(9), 0)
    G, status = MR.combine_sy(S, Ms, ys, zs, alpha)
    assert status == 32 and (G, status) == MR.combine(S, Ms, ys, zs, alpha)
    # at i = 9 only the terms of the other points remain, each with the power of alpha of its (r, k, c)
    E = S.E
    want9 = E.zero
    for r in range(S.R):
        for k in S.points_of(r):
            if k == K - 1:
                continue
            q = E.inv(E.sub(E.embed(S.point(9)), E.el(zs[k])))
            for c in range(S.Cs[r]):
                term = E.mul(E.sub(E.embed(Ms[r][c][9]), ys[r][k][c]), q)
                want9 = E.add(want9, E.mul(E.pow(E.el(alpha), k * S.Ctot + S.off[r] + c), term))
    assert G[9] == want9


def test_claim_order_and_sizes():
    p = PR.GOLDILOCKS
    S = instance(p, 6, 2, (1, 3, 2), (0b10, 0b01, 0b11), eta=2)
    coefs, Ms, zs, _ = random_case(S, 9)
    ys = MR.claims(S, coefs, zs)
    words = MR.claim_words(S, ys)
    assert S.Y == 1 + 3 + 4 and len(words) == 2 * S.Y
    order = [(0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 0, 2), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)]
    assert [(words[i], words[S.Y + i]) for i in range(S.Y)] == [ys[r][k][c] for r, k, c in order]
    assert MR.claims_from_words(S, words) == ys
    assert S.off == [0, 1, 4] and S.Ctot == 6
    assert S.proof_words() == 2 * 8 + S.F.proof_words() + sum(S.Q * C * 4 + S.Q * S.F.depth(0) * S.D for C in S.Cs)
    assert S.workspace_words() == S.D + S.Q + 2 * 64 + S.F.workspace_words()
    for args, want in ((((2, (1, 1), (1, 2))), 0), ((0, (1,), (1,)), "invalid"), ((2, (), ()), "invalid"), ((2, (1, 0), (1, 2)), "invalid"),
                       ((2, (1, 1), (1, 4)), "invalid"), ((2, (1, 1), (1, 0)), "invalid"), ((2, (1, 1), (1, 1)), "invalid"),
                       ((9, (1,), (511,)), "unsupported"), ((1, (1,) * 9, (1,) * 9), "unsupported"), ((1, (1024, 1), (1, 1)), "unsupported"),
                       ((1, (1023, 1), (1, 1)), 0)):
        assert MR.check_shape(*args) == want, args


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("C,K", [(1, 1), (3, 2)])
def test_one_round_full_mask_is_the_batched_commitment(p, C, K):
    """codeword, challenge, proof and verdicts of deep_ref, word for word"""
    S = instance(p, 6, K, (C,), ((1 << K) - 1,))
    D1 = S.rounds[0]
    coefs, Ms, zs, alpha = random_case(S, 31 + C)
    seed = [3, 4]
    ys = MR.claims(S, coefs, zs)
    ys1 = DR.claims(D1, coefs[0], zs)
    assert ys[0] == ys1 and MR.claim_words(S, ys) == DR.claim_words(D1, ys1)
    assert MR.combine(S, Ms, ys, zs, alpha) == DR.combine(D1, Ms[0], ys1, zs, alpha)
    assert MR.combine_sy(S, Ms, ys, zs, alpha) == DR.combine_sy(D1, Ms[0], ys1, zs, alpha)
    tree = MR.commit(S, 0, Ms[0])
    assert tree.flat() == DR.commit(D1, Ms[0]).flat()
    root = tree.root_hash()
    assert MR.challenge(S, seed, [root], zs, MR.claim_words(S, ys)) == DR.challenge(D1, seed, root, zs, ys1)
    proof, st = MR.open_(S, Ms, [tree], coefs, zs, seed)
    assert (proof, st) == DR.open_(D1, Ms[0], tree, coefs[0], zs, seed)
    assert S.proof_words() == D1.proof_words() and S.workspace_words() == D1.workspace_words()
    assert MR.verify(S, [root], zs, seed, proof) == 0 == DR.verify(D1, root, zs, seed, proof)
    for at in (0, 2 * S.Y + 1, len(proof) - 1, MR.section_offsets(S)["leaves"][0] + 1):
        t = list(proof)
        t[at] ^= 1 << 5
        v = MR.verify(S, [root], zs, seed, t)
        assert v != 0 and v == DR.verify(D1, root, zs, seed, t), at


@pytest.mark.parametrize("p", FIELDS)
def test_prover_and_verifier(p):
    S = instance(p, 6, 2, (1, 2, 2), (0b01, 0b11, 0b10))
    coefs, Ms, zs, _ = random_case(S, 21)
    seed = [3, 4]
    trees = [MR.commit(S, r, Ms[r]) for r in range(S.R)]
    roots = [t.root_hash() for t in trees]
    proof, status = MR.open_(S, Ms, trees, coefs, zs, seed)
    assert status == 0 and MR.verify(S, roots, zs, seed, proof) == 0
    yw, fri, leaves, paths = MR.split(S, proof)
    assert MR.claims_from_words(S, yw) == MR.claims(S, coefs, zs)
    a = MR.challenge(S, seed, roots, zs, yw)
    idx, vals = S.fri.opened(S.F, fri, a)
    for r in range(S.R):
        assert leaves[r] == [DR.leaf_words(S.rounds[r], Ms[r], idx[q]) for q in range(S.Q)]
    # a false claim in each round in turn, proved honestly: the codeword is not of low degree
    for r in range(S.R):
        bad, _ = MR.open_(S, Ms, trees, coefs, zs, seed, ys=bumped(S, MR.claims(S, coefs, zs), r))
        assert MR.verify(S, roots, zs, seed, bad) == 4, r
    # one word of each section: one status bit per section, bit 8 by a path of each round in turn
    off = MR.section_offsets(S)
    F = S.F
    flips = {"fri path": (off["fri"] + F.L * S.D + 2 * F.size(F.L) + S.Q * F.leaf_len(0) + 1, 1),
             "final": (off["fri"] + F.L * S.D + 1, None), "claim": (off["claims"] + 1, None)}
    for r in range(S.R):
        flips["path %d" % r] = (off["paths"][r] + 1, 8)
        flips["leaf %d" % r] = (off["leaves"][r] + 2 * S.leaf_len(r) + 1, 8 | 16)
    seen = {}
    for what, (at, want) in flips.items():
        t = list(proof)
        t[at] ^= 1 << 5
        seen[what] = MR.verify(S, roots, zs, seed, t)
        assert seen[what] != 0 and (want is None or seen[what] == want), (what, seen[what])
    assert seen["final"] & 4 and seen["claim"] & 16
    # bit 2: FRI's own layer-1 leaf no longer folds from layer 0 (its path then fails too); bit 16 alone: FRI run on another
    # low-degree codeword than the combination of the committed matrices
    if F.L > 1:
        t = list(proof)
        t[off["fri"] + F.L * S.D + 2 * F.size(F.L) + S.Q * F.leaf_len(0) + S.Q * F.depth(0) * S.D] ^= 1 << 5
        assert MR.verify(S, roots, zs, seed, t) & 2
    shifted, _ = MR.open_(S, Ms, trees, coefs, zs, seed, tweak=lambda G: [S.E.add(g, (1, 0)) for g in G])
    assert MR.verify(S, roots, zs, seed, shifted) == 16
    # an untouched proof against another point, or another root of the last round
    assert MR.verify(S, roots, [(zs[0][0] + 1, zs[0][1]), zs[1]], seed, proof) & 16
    assert MR.verify(S, roots[:-1] + [[roots[-1][0] ^ 1, roots[-1][1]]], zs, seed, proof) & 8
    # a point on the domain is reported by prover and verifier
    zd = [(S.point(3), 0), zs[1]]
    pd, st = MR.open_(S, Ms, trees, coefs, zd, seed)
    assert st == 32 and MR.verify(S, roots, zd, seed, pd) & 32
