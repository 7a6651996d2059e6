"""Pure-Python restatement of the library's proof of work (include/ronk_ntt.h "proof of work") on Python integers, on top of
tests/poseidon_ref.py, fri_ref.py, fri_ext_ref.py and deep_ref.py: the grinding condition and search, and FRI (base and extension)
and the batched commitment with the grinding step between the commit phase and the query phase.  The nonce is the proof's last
word.  A test helper, not product code; it shares nothing with the library and changes none of the helpers it imports."""
import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR

NONE = 2**64 - 1
WORK_WORDS = 16   # ronk_pow_workspace_words


# ---------------------------------------------------------------------------------------------------- stand-alone
def pow_word(P, seed, n):
    """the first word of the one-shot sponge(seed || [n])"""
    return PR.sponge(P, [int(v) for v in seed] + [int(n)], 1)[0]


def meets(P, seed, n, bits):
    return pow_word(P, seed, n) & ((1 << bits) - 1) == 0


def grind(P, seed, bits, log2_limit):
    """the smallest n < 2^log2_limit that meets the condition, or NONE"""
    for n in range(1 << log2_limit):
        if meets(P, seed, n, bits):
            return n
    return NONE


def verify(P, seed, bits, log2_limit, nonce):
    """in range and meets the condition; minimality is not checked"""
    return nonce < (1 << log2_limit) and meets(P, seed, nonce, bits)


def check(p, rate, seed_len, bits, log2_limit):
    """ronk_pow_check for a prime p: 0, 'invalid' or 'unsupported'"""
    if rate < 1 or (1 << bits) >= p or (1 << log2_limit) >= p:
        return "invalid"
    if bits > 40 or log2_limit > 40 or seed_len > 4096:
        return "unsupported"
    return 0


def default_limit(p, bits):
    """callers.py's default: bits + 6, capped by the library's 40 and by the field"""
    lam = min(bits + 6, 40)
    while (1 << lam) >= p:
        lam -= 1
    return lam


# ---------------------------------------------------------------------------------------------------- FRI
class Pow:
    def __init__(self, bits, log2_limit):
        self.bits, self.log2_limit = bits, log2_limit


def proof_words(F, W):
    return F.proof_words() + (1 if W.bits else 0)


def workspace_words(F, W):
    return F.workspace_words() + (WORK_WORDS if W.bits else 0)


def _u(F, seed, roots, final_words):
    """the transcript up to u, as fri_ref.transcript and fri_ext_ref.transcript compute it before they draw the indices"""
    c = [int(v) for v in seed]
    assert len(c) == F.D
    for root in roots:
        c = PR.sponge(F.P, c + list(root), F.D)
    return PR.sponge(F.P, c + list(final_words), F.D)


def _indices(F, u):
    idx = []
    for q in range(F.Q):
        j0 = PR.sponge(F.P, list(u) + [q], 1)[0] & (F.leaves(0) - 1)
        idx.append([j0 % F.leaves(l) for l in range(F.L)])
    return idx


def reseed(F, u, nonce):
    """u' = sponge(u || [nonce]) squeezing D words; the nonce is a word as it stands (the sponge reduces it)"""
    return PR.sponge(F.P, list(u) + [int(nonce)], F.D)


def fri_transcript_pow(F, W, seed, roots, final_words, nonce=None):
    """-> (u, nonce, u', [[j_l for l < L] for every query]).  nonce None: the prover's side, the grind of u; else the verifier's,
    the proof's word.  With W.bits == 0 there is no nonce and u' is u."""
    u = _u(F, seed, roots, final_words)
    if not W.bits:
        return u, None, u, _indices(F, u)
    if nonce is None:
        nonce = grind(F.P, u, W.bits, W.log2_limit)
    u2 = reseed(F, u, nonce)
    return u, nonce, u2, _indices(F, u2)


def _ext(F):
    return isinstance(F, FX.FriExt)


def _final_words(F, layers):
    return ER.planar(layers[F.L]) if _ext(F) else list(layers[F.L])


def fri_prove_pow(F, W, evals, seed):
    """the proof as a flat list of canonical words, the nonce last (NONE when the search finds nothing); base or extension by
    the kind of F"""
    X = FX if _ext(F) else FR
    layers, trees, roots, _ = X.commit_phase(F, evals, seed)
    final = _final_words(F, layers)
    _, nonce, _, idx = fri_transcript_pow(F, W, seed, roots, final)
    proof = [w for r in roots for w in r] + final
    for l in range(F.L):
        for q in range(F.Q):
            proof += FX.leaf_words(F, layers[l], l, idx[q][l]) if _ext(F) else [v % F.p for v in FR.leaf(F, layers[l], l, idx[q][l])]
        for q in range(F.Q):
            proof += [w for sib, _ in trees[l].get_proof(idx[q][l]) for w in sib]
    if W.bits:
        proof.append(nonce)
    assert len(proof) == proof_words(F, W)
    return proof


def fri_split_pow(F, W, proof):
    """-> (the proof without the nonce, the nonce word or None)"""
    proof = [int(w) for w in proof]
    assert len(proof) == proof_words(F, W)
    return (proof[:-1], proof[-1]) if W.bits else (proof, None)


def fri_indices_pow(F, W, proof, seed):
    """j_0 of every query, what ronk_fri_query_indices_dev writes"""
    body, nonce = fri_split_pow(F, W, proof)
    roots, final = (FX if _ext(F) else FR).split(F, body)[:2]
    return [i[0] for i in fri_transcript_pow(F, W, seed, roots, final, nonce)[3]]


def _merkle_ok(F, leaf, j, path, root):
    h = PR.sponge(F.P, leaf, F.D)
    for sib in path:
        h = PR.sponge(F.P, (sib + h) if j & 1 else (h + sib), F.D)
        j >>= 1
    return h == root


def fri_verify_pow(F, W, proof, seed):
    """0, or bits: 1 / 2 / 4 as fri_ref.verify / fri_ext_ref.verify define them, under the indices drawn from u', and 64: the
    nonce word is >= 2^log2_limit or fails the condition.  Every check runs."""
    p, A = F.p, F.A
    ext = _ext(F)
    body, nonce = fri_split_pow(F, W, proof)
    roots, final, vals, paths = (FX if ext else FR).split(F, body)
    u, _, _, idx = fri_transcript_pow(F, W, seed, roots, final, nonce)
    betas = (FX if ext else FR).transcript(F, seed, roots, final)[0]   # the challenges do not depend on the nonce
    status = 0
    if W.bits and not verify(F.P, u, W.bits, W.log2_limit, nonce):
        status |= 64
    nl = F.size(F.L)
    for q in range(F.Q):
        for l in range(F.L):
            j = idx[q][l]
            if not _merkle_ok(F, vals[l][q], j, paths[l][q], roots[l]):
                status |= 1
            x = F.layer_shift(l) * pow(F.root(F.size(l)), j, p) % p
            words, b, w = vals[l][q], betas[l], F.root(A)
            if not ext:
                f = list(words)
                while len(f) > 1:
                    f = FR.fold2(p, f, b, x, w)
                    x, w, b = x * x % p, w * w % p, b * b % p
                want = vals[l + 1][q][j // F.leaves(l + 1)] if l + 1 < F.L else final[j]
            else:
                f = [(v % p, 0) for v in words] if F.vw(l) == 1 else [(words[t] % p, words[A + t] % p) for t in range(A)]
                while len(f) > 1:
                    f = FX.fold2(F.E, f, b, x, w)
                    x, w, b = x * x % p, w * w % p, F.E.mul(b, b)
                if l + 1 < F.L:
                    s = j // F.leaves(l + 1)
                    want = (vals[l + 1][q][s], vals[l + 1][q][A + s])
                else:
                    want = (final[j], final[nl + j])
            if f[0] != want:
                status |= 2
    for plane in ((final[:nl], final[nl:]) if ext else (final,)):
        if any(FR.final_coefficients(F, [v % p for v in plane])[nl >> F.log2_blowup:]):
            status |= 4
    return status


# ---------------------------------------------------------------------------------------------------- the batched commitment
def pcs_proof_words(S, W):
    return S.proof_words() + (1 if W.bits else 0)


def pcs_workspace_words(S, W):
    return S.workspace_words() + (WORK_WORDS if W.bits else 0)


def pcs_section_offsets(S, W):
    """deep_ref.section_offsets with the embedded FRI proof one word longer"""
    fri = 2 * S.K * S.C
    leaves = fri + proof_words(S.F, W)
    return {"claims": 0, "fri": fri, "nonce": leaves - 1 if W.bits else None, "leaves": leaves, "paths": leaves + S.Q * S.leaf_len()}


def pcs_open_pow(S, W, M, tree, coef, zs, seed):
    """-> (the proof, status 0 or 32): deep_ref.open_ with FRI's grinding, the matrix openings at FRI's indices"""
    ys = DR.claims(S, coef, zs)
    a = DR.challenge(S, seed, tree.root_hash(), zs, ys)
    G, status = DR.combine_sy(S, M, ys, zs, (a[0], a[1]))
    fri = fri_prove_pow(S.F, W, ER.planar(G), a)
    j0 = fri_indices_pow(S.F, W, fri, a)
    proof = DR.claim_words(S, ys) + fri
    for q in range(S.Q):
        proof += DR.leaf_words(S, M, j0[q])
    for q in range(S.Q):
        proof += [w for sib, _ in tree.get_proof(j0[q]) for w in sib]
    assert len(proof) == pcs_proof_words(S, W)
    return proof, status


def pcs_verify_pow(S, W, root, zs, seed, proof):
    """0, or bits: 1 / 2 / 4 / 64 as FRI reports them, 8 / 16 / 32 as deep_ref.verify defines them, at FRI's indices"""
    E, p, A = S.E, S.p, S.A
    proof = [int(w) for w in proof]
    assert len(proof) == pcs_proof_words(S, W)
    off = pcs_section_offsets(S, W)
    kc, D, Q, ll, dp = S.K * S.C, S.D, S.Q, S.leaf_len(), S.F.depth(0)
    ys = [[(proof[k * S.C + c], proof[kc + k * S.C + c]) for c in range(S.C)] for k in range(S.K)]
    fri = proof[off["fri"]:off["leaves"]]
    leaves = [proof[off["leaves"] + q * ll: off["leaves"] + (q + 1) * ll] for q in range(Q)]
    paths = [[proof[off["paths"] + (q * dp + l) * D: off["paths"] + (q * dp + l + 1) * D] for l in range(dp)] for q in range(Q)]
    a = DR.challenge(S, seed, root, zs, ys)
    status = fri_verify_pow(S.F, W, fri, a)
    if any(DR.on_domain(S, z) for z in zs):
        status |= 32
    vals = FX.split(S.F, fri_split_pow(S.F, W, fri)[0])[2]
    j0 = fri_indices_pow(S.F, W, fri, a)
    for q in range(Q):
        j = j0[q]
        if not _merkle_ok(S.F, leaves[q], j, paths[q], list(root)):
            status |= 8
        for t in range(A):
            col = [leaves[q][c * A + t] % p for c in range(S.C)]
            g = DR.combine_point(S, col, S.point(j + t * S.m), ys, zs, E.el((a[0], a[1])))
            if g != (vals[0][q][t], vals[0][q][A + t]):
                status |= 16
    return status
