"""Pure-Python restatement of the library's FRI with extension challenges (include/ronk_ntt.h "FRI with extension challenges") on
Python integers, on top of tests/fri_ref.py, tests/ext2_ref.py and tests/poseidon_ref.py: the fold with beta in F_p[t] / (t^2 - w),
planar layers, the transcript with beta_l = (t_l[0], t_l[1]), the prover and the verifier.  A layer is a list of pairs here and
[2][N] planar words in a proof.  A test helper, not product code; it shares nothing with the library."""
import ext2_ref as ER
import fri_ref as FR
import poseidon_ref as PR


class FriExt(FR.Fri):
    def __init__(self, P, g, w, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len, input_ext):
        super().__init__(P, g, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len)
        assert digest_len >= 2 and input_ext in (0, 1)
        self.E = ER.Ext2(P.p, w)
        self.input_ext = input_ext

    def vw(self, l):
        """words per value of layer l"""
        return 2 if l > 0 or self.input_ext else 1

    def leaf_len(self, l):
        return self.vw(l) * self.A

    def proof_words(self):
        return (self.L * self.D + 2 * self.size(self.L)
                + sum(self.Q * self.leaf_len(l) + self.Q * self.depth(l) * self.D for l in range(self.L)))

    def workspace_words(self):
        L, D, Q = self.L, self.D, self.Q
        return (sum(2 * self.size(l + 1) + (2 * self.leaves(l) - 1) * D for l in range(L)) + 2 * L + (L + 2) * D + L * Q + Q)


def layer0(F, evals):
    """the caller's layer 0 as pairs: [N_0] base words embedded as (x, 0), or [2][N_0] planar words"""
    p, n = F.p, F.size(0)
    v = [int(x) for x in evals]
    if F.input_ext:
        assert len(v) == 2 * n
        return [(v[i] % p, v[n + i] % p) for i in range(n)]
    assert len(v) == n
    return [(x % p, 0) for x in v]


def fold2(E, f, beta, s, w):
    """f'[i] = (a + b) / 2 + beta (a - b) / (2 x_i), x_i = s w^i in the base field, a = f[i], b = f[i + N/2] pairs"""
    p = E.p
    h = len(f) // 2
    inv2 = pow(2, p - 2, p)
    xinv, winv = pow(s, p - 2, p), pow(w, p - 2, p)
    out = []
    for i in range(h):
        a, b = f[i], f[i + h]
        out.append(E.add(E.mul_base(E.add(a, b), inv2), E.mul(beta, E.mul_base(E.sub(a, b), inv2 * xinv % p))))
        xinv = xinv * winv % p
    return out


def fold(F, values, beta, layer):
    """one layer of arity 2^eta on pairs: eta arity-2 folds with beta, beta^2, beta^4"""
    E = F.E
    f = [E.el(v) for v in values]
    assert len(f) == F.size(layer)
    s, w, b = F.layer_shift(layer), F.root(len(f)), E.el(beta)
    for _ in range(F.eta):
        f = fold2(E, f, b, s, w)
        s, w, b = s * s % F.p, w * w % F.p, E.mul(b, b)
    return f


def leaf_words(F, f, l, j):
    """the words of Merkle leaf j of layer l (pairs f): a base layer 0 has A words, a planar layer its A c0 values then its A c1"""
    m = F.leaves(l)
    vals = [f[j + t * m] for t in range(F.A)]
    if F.vw(l) == 1:
        return [v[0] for v in vals]
    return [v[0] for v in vals] + [v[1] for v in vals]


def planar_address(F, l, i, j):
    """the offset in the planar layer l of word j = c A + t of leaf i"""
    return i + j * F.leaves(l)


def transcript(F, seed, roots, final_words):
    """-> (betas as pairs, [[j_l for l < L] for every query]); final_words: the c0 plane then the c1 plane"""
    c = [int(v) for v in seed]
    assert len(c) == F.D
    betas = []
    for root in roots:
        c = PR.sponge(F.P, c + list(root), F.D)
        betas.append((c[0], c[1]))
    u = PR.sponge(F.P, c + list(final_words), F.D)
    idx = []
    for q in range(F.Q):
        j0 = PR.sponge(F.P, u + [q], 1)[0] & (F.leaves(0) - 1)
        idx.append([j0 % F.leaves(l) for l in range(F.L)])
    return betas, idx


def commit_phase(F, evals, seed):
    """-> (layers f_0 .. f_L as pairs, trees, roots, betas)"""
    c = [int(v) for v in seed]
    f = layer0(F, evals)
    layers, trees, roots, betas = [f], [], [], []
    for l in range(F.L):
        t = PR.MerkleTree(F.P, [leaf_words(F, f, l, j) for j in range(F.leaves(l))], F.D)
        trees.append(t)
        roots.append(t.root_hash())
        c = PR.sponge(F.P, c + t.root_hash(), F.D)
        betas.append((c[0], c[1]))
        f = fold(F, f, betas[-1], l)
        layers.append(f)
    return layers, trees, roots, betas


def prove(F, evals, seed):
    """the proof as a flat list of canonical words"""
    layers, trees, roots, betas = commit_phase(F, evals, seed)
    final = ER.planar(layers[F.L])
    betas2, idx = transcript(F, seed, roots, final)
    assert betas2 == betas
    proof = [w for r in roots for w in r] + final
    for l in range(F.L):
        for q in range(F.Q):
            proof += leaf_words(F, layers[l], l, idx[q][l])
        for q in range(F.Q):
            proof += [w for sib, _ in trees[l].get_proof(idx[q][l]) for w in sib]
    assert len(proof) == F.proof_words()
    return proof


def split(F, proof):
    """-> (roots, final words [2 N_L], leaf words [l][q], paths [l][q][level])"""
    proof = [int(w) for w in proof]
    assert len(proof) == F.proof_words()
    D, Q = F.D, F.Q
    roots = [proof[l * D:(l + 1) * D] for l in range(F.L)]
    off = F.L * D
    final = proof[off:off + 2 * F.size(F.L)]
    off += 2 * F.size(F.L)
    vals, paths = [], []
    for l in range(F.L):
        ll = F.leaf_len(l)
        vals.append([proof[off + q * ll: off + (q + 1) * ll] for q in range(Q)])
        off += Q * ll
        dp = F.depth(l)
        paths.append([[proof[off + (q * dp + k) * D: off + (q * dp + k + 1) * D] for k in range(dp)] for q in range(Q)])
        off += Q * dp * D
    return roots, final, vals, paths


def verify(F, proof, seed):
    """0, or bits: 1 a Merkle path fails, 2 a fold mismatch, 4 a plane of the final layer is not of low degree; every check runs"""
    p, E, A = F.p, F.E, F.A
    roots, final, vals, paths = split(F, proof)
    betas, idx = transcript(F, seed, roots, final)
    nl = F.size(F.L)
    status = 0
    for q in range(F.Q):
        for l in range(F.L):
            j = idx[q][l]
            h = PR.sponge(F.P, vals[l][q], F.D)
            i = j
            for sib in paths[l][q]:
                h = PR.sponge(F.P, (sib + h) if i & 1 else (h + sib), F.D)
                i >>= 1
            if h != roots[l]:
                status |= 1
            # the fold of the opened coset: a one-leaf layer of its own
            x = F.layer_shift(l) * pow(F.root(F.size(l)), j, p) % p
            words = vals[l][q]
            if F.vw(l) == 1:
                f = [(v % p, 0) for v in words]
            else:
                f = [(words[t] % p, words[A + t] % p) for t in range(A)]
            b, w = betas[l], F.root(A)
            while len(f) > 1:
                f = fold2(E, f, b, x, w)
                x, w, b = x * x % p, w * w % p, E.mul(b, b)
            if l + 1 < F.L:
                s = j // F.leaves(l + 1)
                want = (vals[l + 1][q][s], vals[l + 1][q][A + s])
            else:
                want = (final[j], final[nl + j])
            if f[0] != want:      # the proof's words as they stand: a word >= p never matches
                status |= 2
    for plane in (final[:nl], final[nl:]):
        coeffs = FR.final_coefficients(F, [v % p for v in plane])
        if any(coeffs[nl >> F.log2_blowup:]):
            status |= 4
    return status
