"""Pure-Python restatement of the library's multi-matrix polynomial commitment (include/ronk_ntt.h "multi-matrix polynomial
commitment") on Python integers, on top of tests/deep_ref.py, tests/ext2_ref.py, tests/fri_ext_ref.py and tests/poseidon_ref.py:
R committed matrices, round r opened at the points whose bits are set in masks[r], one DEEP codeword, one FRI.  Matrices are a
list of R matrices (each a list of C_r rows of N words), coefficients likewise, points are pairs, claims are ys[r][k][c] with
ys[r][k] None where mask_r lacks k.  A test helper, not product code; it shares nothing with the library."""
import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import poseidon_ref as PR

MAX_C, MAX_K, MAX_R = 1024, 8, 8


def check_shape(n_points, columns, masks, log2_n=2):
    """the part of ronk_mpcs_check after the FRI codes: 0, 'invalid' or 'unsupported', in the library's order"""
    if columns is None or masks is None or n_points == 0 or len(columns) == 0:
        return "invalid"
    if any(c == 0 for c in columns) or any(m == 0 or m >= (1 << n_points) for m in masks):
        return "invalid"
    seen = 0
    for m in masks:
        seen |= m
    if seen != (1 << n_points) - 1:
        return "invalid"
    if n_points > MAX_K or len(columns) > MAX_R or sum(columns) > MAX_C or log2_n < 2:
        return "unsupported"
    return 0


class PlainFri:
    """the embedded FRI as fri_ext_ref states it; a test with grinding passes an object of the same five methods"""

    def proof_words(self, F):
        return F.proof_words()

    def workspace_words(self, F):
        return F.workspace_words()

    def prove(self, F, evals, seed):
        return FX.prove(F, evals, seed)

    def verify(self, F, proof, seed):
        return FX.verify(F, proof, seed)

    def opened(self, F, proof, seed):
        """-> (j_0 of every query, the layer-0 leaf words of every query as they stand)"""
        roots, final, vals, _ = FX.split(F, proof)
        _, idx = FX.transcript(F, seed, roots, final)
        return [idx[q][0] for q in range(F.Q)], vals[0]


class Mpcs:
    def __init__(self, P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, n_points, columns, masks, fri=None):
        assert check_shape(n_points, columns, masks, log2_n) == 0 and len(columns) == len(masks)
        self.F = FX.FriExt(P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, 1)
        self.P, self.p, self.E = P, P.p, self.F.E
        self.K, self.R, self.Cs, self.masks = n_points, len(columns), list(columns), list(masks)
        self.off = [sum(columns[:r]) for r in range(self.R)]
        self.Ctot = sum(columns)
        self.Y = sum(len(self.points_of(r)) * columns[r] for r in range(self.R))
        self.N, self.A, self.m = self.F.size(0), self.F.A, self.F.leaves(0)
        self.d = self.N >> log2_blowup
        self.Q, self.D = n_queries, digest_len
        self.fri = PlainFri() if fri is None else fri
        # the batched commitment of one round: its tree, its leaves, its domain
        self.rounds = [DR.Pcs(P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, c, n_points) for c in columns]

    def points_of(self, r):
        return [k for k in range(self.K) if (self.masks[r] >> k) & 1]

    def point(self, i):
        return self.rounds[0].point(i)

    def domain(self):
        return self.rounds[0].domain()

    def leaf_len(self, r):
        return self.Cs[r] * self.A

    def round_words(self, r):
        return self.Q * self.leaf_len(r) + self.Q * self.F.depth(0) * self.D

    def proof_words(self):
        return 2 * self.Y + self.fri.proof_words(self.F) + sum(self.round_words(r) for r in range(self.R))

    def workspace_words(self):
        """a [D], open status [Q], G [2][N], the FRI workspace: that of deep_ref.Pcs, whatever R"""
        return self.D + self.Q + 2 * self.N + self.fri.workspace_words(self.F)


# ---------------------------------------------------------------------------------------------------- claims
def claims(S, coefs, zs):
    """ys[r][k][c] = f_(r,c)(z_k) for k in mask_r, None elsewhere"""
    assert len(coefs) == S.R and len(zs) == S.K
    return [[[DR.evaluate_ext(S.E, coefs[r][c], zs[k]) for c in range(S.Cs[r])] if k in S.points_of(r) else None for k in range(S.K)]
            for r in range(S.R)]


def claim_list(S, ys):
    """the claims in proof order: by round, by the set bits of the mask ascending, by column"""
    return [S.E.el(ys[r][k][c]) for r in range(S.R) for k in S.points_of(r) for c in range(S.Cs[r])]


def claim_words(S, ys):
    """planar [2][Y]"""
    return ER.planar(claim_list(S, ys))


def claims_from_words(S, words):
    """planar [2][Y] words as they stand -> ys[r][k][c]"""
    assert len(words) == 2 * S.Y
    ys, at = [], 0
    for r in range(S.R):
        row = [None] * S.K
        for k in S.points_of(r):
            row[k] = [(words[at + c], words[S.Y + at + c]) for c in range(S.Cs[r])]
            at += S.Cs[r]
        ys.append(row)
    return ys


def columns(S, coefs):
    return [DR.columns(S.rounds[r], coefs[r]) for r in range(S.R)]


# ---------------------------------------------------------------------------------------------------- the codeword
def on_domain(S, z):
    return DR.on_domain(S.rounds[0], z)


def combine_point(S, cols, x, ys, zs, alpha):
    """G at the point x from the values cols[r][c] there: the triple sum of the definition, every term with its own power"""
    E = S.E
    alpha = E.el(alpha)
    if getattr(S, "_powers", (None,))[0] != alpha:      # alpha^j, j < K C_tot, by repeated products; kept for the next point
        ap = [E.one]
        for _ in range(S.K * S.Ctot):
            ap.append(E.mul(ap[-1], alpha))
        S._powers = (alpha, ap)
    ap = S._powers[1]
    g = E.zero
    for r in range(S.R):
        for k in S.points_of(r):
            q = DR.inv_or_zero(E, E.sub(E.embed(x), E.el(zs[k])))
            for c in range(S.Cs[r]):
                a = ap[k * S.Ctot + S.off[r] + c]
                g = E.add(g, E.mul(a, E.mul(E.sub(E.embed(cols[r][c]), E.el(ys[r][k][c])), q)))
    return g


def combine(S, Ms, ys, zs, alpha):
    """-> (G as pairs, status 0 or 32), term by term as defined"""
    alpha = S.E.el(alpha)
    xs = S.domain()
    G = [combine_point(S, [[Ms[r][c][i] for c in range(S.Cs[r])] for r in range(S.R)], xs[i], ys, zs, alpha) for i in range(S.N)]
    return G, 32 if any(on_domain(S, z) for z in zs) else 0


def combine_sy(S, Ms, ys, zs, alpha):
    """the same through S_r,i = sum_c alpha^(o_r + c) M_r[c][i], Y_r,k = sum_c alpha^(o_r + c) y[r][k][c] and
    B_k = alpha^(k C_tot): G[i] = sum_r sum_(k in mask_r) B_k (S_r,i - Y_r,k) / (x_i - z_k), a zero norm giving a zero term"""
    E, p = S.E, S.p
    alpha = E.el(alpha)
    ap = [E.one]
    for _ in range(S.Ctot):
        ap.append(E.mul(ap[-1], alpha))
    B = [E.pow(ap[S.Ctot], k) for k in range(S.K)]
    zz = [E.el(z) for z in zs]
    Y = {}
    for r in range(S.R):
        for k in S.points_of(r):
            acc = E.zero
            for c in range(S.Cs[r]):
                acc = E.add(acc, E.mul(ap[S.off[r] + c], E.el(ys[r][k][c])))
            Y[r, k] = acc
    G = []
    for i, x in enumerate(S.domain()):
        g = E.zero
        ninv = []
        for k in range(S.K):
            d = (x - zz[k][0]) % p
            n = (d * d - E.w * zz[k][1] * zz[k][1]) % p
            ninv.append((d, pow(n, -1, p) if n else 0))
        for r in range(S.R):
            s = (sum(ap[S.off[r] + c][0] * int(Ms[r][c][i]) for c in range(S.Cs[r])) % p,
                 sum(ap[S.off[r] + c][1] * int(Ms[r][c][i]) for c in range(S.Cs[r])) % p)
            for k in S.points_of(r):
                d, ni = ninv[k]
                g = E.add(g, E.mul(B[k], E.mul(E.sub(s, Y[r, k]), E.mul_base((d, zz[k][1]), ni))))
        G.append(g)
    return G, 32 if any(on_domain(S, z) for z in zs) else 0


# ---------------------------------------------------------------------------------------------------- commitment, transcript
def commit(S, r, M):
    """the tree of round r: that of the batched commitment with C = C_r"""
    return DR.commit(S.rounds[r], M)


def challenge(S, seed, roots, zs, y_words):
    """a = sponge(seed || root_0 || .. || root_(R-1) || z planes || y planes); alpha = (a[0], a[1]) and a is the FRI seed"""
    z_words = ER.planar([(int(z[0]), int(z[1])) for z in zs])
    return PR.sponge(S.P, [int(v) for v in seed] + [int(w) for root in roots for w in root] + z_words + [int(w) for w in y_words], S.D)


# ---------------------------------------------------------------------------------------------------- prover, verifier
def open_(S, Ms, trees, coefs, zs, seed, ys=None, tweak=None):
    """-> (the proof as a flat list of canonical words, status 0 or 32); ys: claims to prove in the place of the true ones;
    tweak: a dishonest prover's change of the codeword, G -> tweak(G), before FRI runs on it"""
    ys = claims(S, coefs, zs) if ys is None else ys
    yw = claim_words(S, ys)
    a = challenge(S, seed, [t.root_hash() for t in trees], zs, yw)
    G, status = combine_sy(S, Ms, ys, zs, (a[0], a[1]))
    if tweak is not None:
        G = tweak(G)
    fri = S.fri.prove(S.F, ER.planar(G), a)
    idx, _ = S.fri.opened(S.F, fri, a)
    proof = yw + fri
    for r in range(S.R):
        for q in range(S.Q):
            proof += DR.leaf_words(S.rounds[r], Ms[r], idx[q])
        for q in range(S.Q):
            proof += [w for sib, _ in trees[r].get_proof(idx[q]) for w in sib]
    assert len(proof) == S.proof_words()
    return proof, status


def section_offsets(S):
    """word offsets: claims, the FRI proof, then per round its leaves and its paths"""
    fri = 2 * S.Y
    off = {"claims": 0, "fri": fri, "leaves": [], "paths": []}
    at = fri + S.fri.proof_words(S.F)
    for r in range(S.R):
        off["leaves"].append(at)
        off["paths"].append(at + S.Q * S.leaf_len(r))
        at += S.round_words(r)
    assert at == S.proof_words()
    return off


def split(S, proof):
    """-> (claim words as they stand, the FRI proof, leaves [r][q], paths [r][q][level])"""
    proof = [int(w) for w in proof]
    assert len(proof) == S.proof_words()
    off = section_offsets(S)
    D, Q, dp = S.D, S.Q, S.F.depth(0)
    yw = proof[:off["fri"]]
    fri = proof[off["fri"]:off["fri"] + S.fri.proof_words(S.F)]
    leaves, paths = [], []
    for r in range(S.R):
        ll, lo, po = S.leaf_len(r), off["leaves"][r], off["paths"][r]
        leaves.append([proof[lo + q * ll: lo + (q + 1) * ll] for q in range(Q)])
        paths.append([[proof[po + (q * dp + l) * D: po + (q * dp + l + 1) * D] for l in range(dp)] for q in range(Q)])
    return yw, fri, leaves, paths


def verify(S, roots, zs, seed, proof):
    """0, or bits: 1 / 2 / 4 (64) as FRI reports them, 8 a matrix path of any round fails, 16 a DEEP mismatch, 32 a point on the
    domain; every check runs.  roots: [R][D]"""
    E, p, A = S.E, S.p, S.A
    yw, fri, leaves, paths = split(S, proof)
    ys = claims_from_words(S, yw)
    a = challenge(S, seed, roots, zs, yw)
    alpha = E.el((a[0], a[1]))
    status = S.fri.verify(S.F, fri, a)
    if any(on_domain(S, z) for z in zs):
        status |= 32
    idx, vals = S.fri.opened(S.F, fri, a)
    for q in range(S.Q):
        j = idx[q]
        for r in range(S.R):
            h = PR.sponge(S.P, leaves[r][q], S.D)
            i = j
            for sib in paths[r][q]:
                h = PR.sponge(S.P, (sib + h) if i & 1 else (h + sib), S.D)
                i >>= 1
            if h != [int(w) for w in roots[r]]:
                status |= 8
        for t in range(A):
            cols = [[leaves[r][q][c * A + t] % p for c in range(S.Cs[r])] for r in range(S.R)]
            g = combine_point(S, cols, S.point(j + t * S.m), ys, zs, alpha)
            if g != (vals[q][t], vals[q][A + t]):      # the proof's words as they stand
                status |= 16
    return status
