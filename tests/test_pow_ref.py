"""The restatement of the proof of work (tests/pow_ref.py) against itself and against the helpers it is built on: an honest proof
verifies, a changed nonce word is reported by bit 64 (and only by it where the indices stay), no grinding is fri_ref / fri_ext_ref /
deep_ref word for word, and grinding changes u and the indices.  CPU only; pins the semantics the device tests compare with."""
import random

import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR
import pow_ref as PW

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
GEN = {GL: 7, MONT: 10}
Q, BITS, LIMIT = 5, 6, 12
W6, W0 = PW.Pow(BITS, LIMIT), PW.Pow(0, 0)


def params(p):
    return PR.derive_params(p, 8, 7, 2, 4, 4)


def codeword(F, rng):
    return FR.evaluate(F, [rng.randrange(F.p) for _ in range(F.size(0) >> 1)])


def base(p, D=2):
    return FR.Fri(params(p), GEN[p], 6, GEN[p], 1, 2, 1, Q, D)


def test_grind_is_the_smallest_solution():
    P = params(GL)
    rng = random.Random(1)
    for seed_len in (0, 1, 4, 5):
        seed = [rng.randrange(GL) for _ in range(seed_len)]
        n = PW.grind(P, seed, BITS, LIMIT)
        assert n != PW.NONE and PW.verify(P, seed, BITS, LIMIT, n)
        assert not any(PW.meets(P, seed, k, BITS) for k in range(n))
        assert PW.pow_word(P, seed, n) == PR.sponge(P, seed + [n], 3)[0]      # the word is the first of any squeeze
        assert PW.grind(P, seed, 0, 0) == 0
    assert not PW.verify(P, [1], BITS, 3, 8)                                    # out of range whatever the word
    assert PW.check(101, 2, 1, 7, 6) == "invalid" and PW.check(101, 2, 1, 6, 6) == 0
    assert PW.check(GL, 4, 4097, 6, 12) == "unsupported" and PW.check(GL, 4, 1, 41, 12) == "unsupported"
    assert PW.default_limit(GL, 20) == 26 and PW.default_limit(101, 4) == 6 and PW.default_limit(GL, 38) == 40


def honest(p, D=2, seed0=0):
    """an instance, a codeword and a seed under which nonce + 1 fails the condition too"""
    F = base(p, D)
    f = codeword(F, random.Random(p % 97 + D))
    for s in range(seed0, seed0 + 50):
        seed = [s] + [4] * (D - 1)
        proof = PW.fri_prove_pow(F, W6, f, seed)
        roots, final = FR.split(F, proof[:-1])[:2]
        u = PW.fri_transcript_pow(F, W6, seed, roots, final, proof[-1])[0]
        if not PW.meets(F.P, u, proof[-1] + 1, BITS):
            return F, f, seed, proof, u
    raise AssertionError("no seed found")


def test_honest_proof_and_tampered_nonce():
    for p, D in ((GL, 2), (MONT, 4)):
        F, f, seed, proof, u = honest(p, D)
        nonce = proof[-1]
        assert len(proof) == FR.Fri.proof_words(F) + 1 and nonce < (1 << LIMIT)
        assert nonce == PW.grind(F.P, u, BITS, LIMIT)
        assert PW.fri_verify_pow(F, W6, proof, seed) == 0
        # nonce + 1 fails the restated condition: bit 64 (the indices move, so the other checks may speak too)
        assert not PW.verify(F.P, u, BITS, LIMIT, nonce + 1)
        assert PW.fri_verify_pow(F, W6, proof[:-1] + [nonce + 1], seed) & 64
        # the same residue as a word >= 2^limit: out of range, but u' and the indices are the honest ones -- bit 64 alone
        assert PW.fri_verify_pow(F, W6, proof[:-1] + [nonce + p], seed) == 64
        assert PW.fri_verify_pow(F, W6, proof[:-1] + [PW.NONE], seed) & 64
        # the next solution is no minimum, which the verifier does not ask: bit 64 stays clear, the moved indices are caught
        nxt = next(n for n in range(nonce + 1, 1 << LIMIT) if PW.meets(F.P, u, n, BITS))
        st = PW.fri_verify_pow(F, W6, proof[:-1] + [nxt], seed)
        assert st != 0 and not st & 64
        # a tampered leaf beside a clean nonce
        bad = list(proof)
        bad[F.L * F.D + F.size(F.L) + 1] ^= 4
        st = PW.fri_verify_pow(F, W6, bad, seed)
        assert st != 0 and not st & 64


def test_no_grinding_is_the_base_restatement():
    for p in (GL, MONT):
        F = base(p)
        f = codeword(F, random.Random(3))
        seed = [3, 4]
        proof = PW.fri_prove_pow(F, W0, f, seed)
        assert proof == FR.prove(F, f, seed)
        assert PW.fri_verify_pow(F, W0, proof, seed) == FR.verify(F, proof, seed) == 0
        bad = list(proof)
        bad[-1] ^= 1
        assert PW.fri_verify_pow(F, W0, bad, seed) == FR.verify(F, bad, seed) != 0
        assert PW.proof_words(F, W0) == F.proof_words() and PW.workspace_words(F, W0) == F.workspace_words()
        assert PW.proof_words(F, W6) == F.proof_words() + 1 and PW.workspace_words(F, W6) == F.workspace_words() + PW.WORK_WORDS


def test_grinding_moves_u_and_the_indices():
    F, f, seed, proof, u = honest(GL)
    roots, final = FR.split(F, proof[:-1])[:2]
    u0, nonce, u2, idx = PW.fri_transcript_pow(F, W6, seed, roots, final)
    assert u0 == u and nonce == proof[-1] and u2 != u
    assert u2 == PR.sponge(F.P, u + [nonce], F.D) and u2[0] & ((1 << BITS) - 1) == 0
    plain = FR.transcript(F, seed, roots, final)[1]
    assert idx != plain and PW.fri_transcript_pow(F, W0, seed, roots, final)[3] == plain
    assert PW.fri_indices_pow(F, W6, proof, seed) == [i[0] for i in idx]


def test_extension_and_commitment():
    p = GL
    P = params(p)
    F = FX.FriExt(P, 7, 7, 6, 7, 1, 2, 1, Q, 2, 0)
    f = codeword(F, random.Random(5))
    seed = [3, 4]
    assert PW.fri_prove_pow(F, W0, f, seed) == FX.prove(F, f, seed)
    proof = PW.fri_prove_pow(F, W6, f, seed)
    assert len(proof) == F.proof_words() + 1 and PW.fri_verify_pow(F, W6, proof, seed) == 0
    assert PW.fri_verify_pow(F, W6, proof[:-1] + [proof[-1] + p], seed) == 64
    # the batched commitment: C = 3 columns at K = 2 points
    S = DR.Pcs(P, 7, 7, 6, 7, 1, 2, 1, Q, 2, 3, 2)
    rng = random.Random(6)
    coef = [[rng.randrange(p) for _ in range(S.d)] for _ in range(S.C)]
    zs = [(rng.randrange(p), rng.randrange(p)) for _ in range(S.K)]
    M = DR.columns(S, coef)
    tree = DR.commit(S, M)
    assert PW.pcs_open_pow(S, W0, M, tree, coef, zs, seed) == DR.open_(S, M, tree, coef, zs, seed)
    proof, st = PW.pcs_open_pow(S, W6, M, tree, coef, zs, seed)
    assert st == 0 and len(proof) == S.proof_words() + 1
    assert PW.pcs_verify_pow(S, W6, tree.root_hash(), zs, seed, proof) == 0
    off = PW.pcs_section_offsets(S, W6)
    assert off["leaves"] == DR.section_offsets(S)["leaves"] + 1 and off["nonce"] == off["leaves"] - 1
    bad = list(proof)
    bad[off["nonce"]] += p
    assert PW.pcs_verify_pow(S, W6, tree.root_hash(), zs, seed, bad) == 64
    bad = list(proof)
    bad[off["leaves"]] ^= 2
    st = PW.pcs_verify_pow(S, W6, tree.root_hash(), zs, seed, bad)
    assert st & 8 and not st & 64
