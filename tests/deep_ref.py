"""Pure-Python restatement of the library's batched FRI polynomial commitment with DEEP quotients (include/ronk_ntt.h "batched FRI
polynomial commitment") on Python integers, on top of tests/ext2_ref.py, tests/fri_ext_ref.py and tests/poseidon_ref.py: the
evaluation of the columns at extension points, the codeword G, the transcript step, the prover, the verifier and the proof
layout.  A matrix is a list of C rows of N words, coefficients a list of C rows of d words, points and claims are pairs (claims as
ys[k][c]).  A test helper, not product code; it shares nothing with the library."""
import ext2_ref as ER
import fri_ext_ref as FX
import poseidon_ref as PR

MAX_C, MAX_K = 1024, 8


class Pcs:
    def __init__(self, P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, n_columns, n_points):
        assert 1 <= n_columns <= MAX_C and 1 <= n_points <= MAX_K and log2_n >= 2
        self.F = FX.FriExt(P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, 1)
        self.P, self.p, self.E = P, P.p, self.F.E
        self.C, self.K = n_columns, n_points
        self.N, self.A, self.m = self.F.size(0), self.F.A, self.F.leaves(0)
        self.d = self.N >> log2_blowup
        self.Q, self.D = n_queries, digest_len

    def point(self, i):
        return self.F.shift * pow(self.F.root(self.N), i, self.p) % self.p

    def domain(self):
        x, w, out = self.F.shift, self.F.root(self.N), []
        for _ in range(self.N):
            out.append(x)
            x = x * w % self.p
        return out

    def leaf_len(self):
        return self.C * self.A

    def proof_words(self):
        return 2 * self.K * self.C + self.F.proof_words() + self.Q * self.leaf_len() + self.Q * self.F.depth(0) * self.D

    def workspace_words(self):
        return self.D + self.Q + 2 * self.N + self.F.workspace_words()


# ---------------------------------------------------------------------------------------------------- evaluation
def evaluate_ext(E, coeffs, z):
    """sum_j coeffs[j] z^j for base coefficients and an extension point, by Horner's rule"""
    acc, z = E.zero, E.el(z)
    for c in reversed(list(coeffs)):
        acc = E.add(E.mul(acc, z), E.embed(c))
    return acc


def claims(S, coef, zs):
    """ys[k][c] = f_c(z_k)"""
    assert len(coef) == S.C and len(zs) == S.K
    return [[evaluate_ext(S.E, coef[c], z) for c in range(S.C)] for z in zs]


def claim_words(S, ys):
    """planar [2][K C], element k C + c"""
    return ER.planar([S.E.el(ys[k][c]) for k in range(S.K) for c in range(S.C)])


def columns(S, coef):
    """the matrix of the columns: M[c][i] = f_c(x_i)"""
    import fri_ref as FR
    return [FR.evaluate(S.F, [int(v) % S.p for v in row]) for row in coef]


# ---------------------------------------------------------------------------------------------------- the codeword
def on_domain(S, z):
    z = S.E.el(z)
    return z[1] == 0 and pow(z[0] * pow(S.F.shift, -1, S.p), S.N, S.p) == 1


def inv_or_zero(E, a):
    """the inverse with the convention of ronk_ext2_vec_inv_dev: zero for the zero element"""
    r = E.inv(a)
    return E.zero if r is None else r


def combine_point(S, col, x, ys, zs, alpha):
    """G at the point x from the C values col[c] there: the double sum of the definition"""
    E = S.E
    g, apow = E.zero, E.one
    for k in range(S.K):
        q = inv_or_zero(E, E.sub(E.embed(x), E.el(zs[k])))
        for c in range(S.C):
            g = E.add(g, E.mul(apow, E.mul(E.sub(E.embed(col[c]), E.el(ys[k][c])), q)))
            apow = E.mul(apow, alpha)
    return g


def combine(S, M, ys, zs, alpha):
    """-> (G as pairs, status 0 or 32), term by term as defined"""
    alpha = S.E.el(alpha)
    xs = S.domain()
    G = [combine_point(S, [M[c][i] for c in range(S.C)], xs[i], ys, zs, alpha) for i in range(S.N)]
    return G, 32 if any(on_domain(S, z) for z in zs) else 0


def combine_sy(S, M, ys, zs, alpha):
    """the same through S_i = sum_c alpha^c M[c][i] and Y_k = sum_c alpha^c y[k][c]: G[i] = sum_k alpha^(k C) (S_i - Y_k) / (x_i - z_k)"""
    E, p = S.E, S.p
    alpha = E.el(alpha)
    ap = [E.one]
    for _ in range(S.C):
        ap.append(E.mul(ap[-1], alpha))
    B = [E.pow(ap[S.C], k) for k in range(S.K)]
    Y = [(sum(ap[c][0] * E.el(ys[k][c])[0] + E.w * ap[c][1] * E.el(ys[k][c])[1] for c in range(S.C)) % p,
          sum(ap[c][0] * E.el(ys[k][c])[1] + ap[c][1] * E.el(ys[k][c])[0] for c in range(S.C)) % p) for k in range(S.K)]
    zz = [E.el(z) for z in zs]
    G = []
    for i, x in enumerate(S.domain()):
        s = (sum(ap[c][0] * int(M[c][i]) for c in range(S.C)) % p, sum(ap[c][1] * int(M[c][i]) for c in range(S.C)) % p)
        g = E.zero
        for k in range(S.K):
            d = (x - zz[k][0]) % p
            n = (d * d - E.w * zz[k][1] * zz[k][1]) % p
            if n:
                g = E.add(g, E.mul(B[k], E.mul(E.sub(s, Y[k]), E.mul_base((d, zz[k][1]), pow(n, -1, p)))))
        G.append(g)
    return G, 32 if any(on_domain(S, z) for z in zs) else 0


# ---------------------------------------------------------------------------------------------------- commitment, transcript
def leaf_words(S, M, j):
    """leaf j of the matrix tree: word c A + t = M[c][j + t m]"""
    return [int(M[c][j + t * S.m]) % S.p for c in range(S.C) for t in range(S.A)]


def leaf_address(S, j, q):
    """the offset in the flat [C][N] matrix of word q of leaf j"""
    return j + q * S.m


def commit(S, M):
    return PR.MerkleTree(S.P, [leaf_words(S, M, j) for j in range(S.m)], S.D)


def challenge(S, seed, root, zs, ys):
    """a = sponge(seed || root_M || z planes || y planes); alpha = (a[0], a[1]) and a is the FRI seed"""
    z_words = ER.planar([(int(z[0]), int(z[1])) for z in zs])
    y_words = ER.planar([(int(ys[k][c][0]), int(ys[k][c][1])) for k in range(S.K) for c in range(S.C)])
    return PR.sponge(S.P, [int(v) for v in seed] + list(root) + z_words + y_words, S.D)


# ---------------------------------------------------------------------------------------------------- prover, verifier
def open_(S, M, tree, coef, zs, seed, ys=None, tweak=None):
    """-> (the proof as a flat list of canonical words, status 0 or 32); ys: claims to prove in the place of the true ones;
    tweak: a dishonest prover's change of the codeword, G -> tweak(G), before FRI runs on it"""
    ys = claims(S, coef, zs) if ys is None else [[S.E.el(y) for y in row] for row in ys]
    a = challenge(S, seed, tree.root_hash(), zs, ys)
    G, status = combine_sy(S, M, ys, zs, (a[0], a[1]))
    if tweak is not None:
        G = tweak(G)
    fri = FX.prove(S.F, ER.planar(G), a)
    roots, final, _, _ = FX.split(S.F, fri)
    _, idx = FX.transcript(S.F, a, roots, final)
    proof = claim_words(S, ys) + fri
    for q in range(S.Q):
        proof += leaf_words(S, M, idx[q][0])
    for q in range(S.Q):
        proof += [w for sib, _ in tree.get_proof(idx[q][0]) for w in sib]
    assert len(proof) == S.proof_words()
    return proof, status


def split(S, proof):
    """-> (claims ys[k][c] as they stand, the FRI proof, matrix leaves [q], matrix paths [q][level])"""
    proof = [int(w) for w in proof]
    assert len(proof) == S.proof_words()
    kc, D, Q, ll, dp = S.K * S.C, S.D, S.Q, S.leaf_len(), S.F.depth(0)
    ys = [[(proof[k * S.C + c], proof[kc + k * S.C + c]) for c in range(S.C)] for k in range(S.K)]
    off = 2 * kc
    fri = proof[off:off + S.F.proof_words()]
    off += S.F.proof_words()
    leaves = [proof[off + q * ll: off + (q + 1) * ll] for q in range(Q)]
    off += Q * ll
    paths = [[proof[off + (q * dp + l) * D: off + (q * dp + l + 1) * D] for l in range(dp)] for q in range(Q)]
    return ys, fri, leaves, paths


def section_offsets(S):
    """word offsets of the proof's sections: claims, the FRI proof, the matrix leaves, the matrix paths"""
    fri = 2 * S.K * S.C
    leaves = fri + S.F.proof_words()
    return {"claims": 0, "fri": fri, "leaves": leaves, "paths": leaves + S.Q * S.leaf_len()}


def verify(S, root, zs, seed, proof):
    """0, or bits: 1 / 2 / 4 as FRI reports them, 8 a matrix path fails, 16 a DEEP mismatch, 32 a point on the domain; every
    check runs"""
    E, p, A = S.E, S.p, S.A
    ys, fri, leaves, paths = split(S, proof)
    a = challenge(S, seed, root, zs, ys)
    alpha = (a[0], a[1])
    status = FX.verify(S.F, fri, a)
    if any(on_domain(S, z) for z in zs):
        status |= 32
    roots, final, vals, _ = FX.split(S.F, fri)
    _, idx = FX.transcript(S.F, a, roots, final)
    for q in range(S.Q):
        j = idx[q][0]
        h = PR.sponge(S.P, leaves[q], S.D)
        i = j
        for sib in paths[q]:
            h = PR.sponge(S.P, (sib + h) if i & 1 else (h + sib), S.D)
            i >>= 1
        if h != list(root):
            status |= 8
        for t in range(A):
            col = [leaves[q][c * A + t] % p for c in range(S.C)]
            g = combine_point(S, col, S.point(j + t * S.m), ys, zs, E.el(alpha))
            if g != (vals[0][q][t], vals[0][q][A + t]):      # the proof's words as they stand
                status |= 16
    return status
