"""Pure-Python restatement of the library's FRI (include/ronk_ntt.h "FRI") on Python integers, on top of tests/poseidon_ref.py:
the arity-2 fold, a layer of arity 2^eta, the Poseidon transcript, the prover and the verifier.  A test helper, not product code;
it shares nothing with the library."""
import poseidon_ref as PR


class Fri:
    def __init__(self, P, g, log2_n, shift, eta, log2_final, log2_blowup, n_queries, digest_len):
        p = P.p
        assert 1 <= eta <= 3 and log2_blowup <= log2_final <= 8 and (p - 1) % (1 << log2_n) == 0 and shift % p != 0
        assert log2_n >= log2_final + eta and (log2_n - log2_final) % eta == 0 and n_queries >= 1 and 1 <= digest_len <= P.rate
        self.P, self.p, self.g, self.n, self.shift, self.eta = P, p, g % p, log2_n, shift % p, eta
        self.log2_final, self.log2_blowup, self.Q, self.D = log2_final, log2_blowup, n_queries, digest_len
        self.A = 1 << eta
        self.L = (log2_n - log2_final) // eta

    def size(self, l):
        return 1 << (self.n - self.eta * l)

    def leaves(self, l):
        return self.size(l) // self.A

    def depth(self, l):
        return self.n - self.eta * (l + 1)

    def root(self, n):
        return pow(self.g, (self.p - 1) // n, self.p)

    def layer_shift(self, l):
        return pow(self.shift, self.A ** l, self.p)

    def proof_words(self):
        return self.L * self.D + self.size(self.L) + sum(self.Q * self.A + self.Q * self.depth(l) * self.D for l in range(self.L))

    def workspace_words(self):
        L, D, Q = self.L, self.D, self.Q
        return (sum(self.size(l + 1) + (2 * self.leaves(l) - 1) * D for l in range(L)) + L + (L + 2) * D + L * Q + Q)


def fft(p, a, w):
    """[sum_k a[k] w^(i k) for i < len(a)], len(a) a power of two, w of that order"""
    n = len(a)
    if n == 1:
        return list(a)
    ev, od = fft(p, a[0::2], w * w % p), fft(p, a[1::2], w * w % p)
    out, x = [0] * n, 1
    for i in range(n // 2):
        t = x * od[i] % p
        out[i], out[i + n // 2] = (ev[i] + t) % p, (ev[i] - t) % p
        x = x * w % p
    return out


def evaluate(F, coeffs, layer=0):
    """the values of sum_k coeffs[k] x^k on the domain of `layer`, natural order"""
    p, n = F.p, F.size(layer)
    assert len(coeffs) <= n
    s, x, a = F.layer_shift(layer), 1, []
    for c in list(coeffs) + [0] * (n - len(coeffs)):
        a.append(c * x % p)
        x = x * s % p
    return fft(p, a, F.root(n))


def fold2(p, f, beta, s, w):
    """f'[i] = (a + b) / 2 + beta (a - b) / (2 x_i), x_i = s w^i, a = f[i], b = f[i + N/2]"""
    h = len(f) // 2
    inv2 = pow(2, p - 2, p)
    xinv, winv = pow(s, p - 2, p), pow(w, p - 2, p)
    out = []
    for i in range(h):
        a, b = f[i], f[i + h]
        out.append(((a + b) * inv2 + beta * (a - b) * inv2 * xinv) % p)
        xinv = xinv * winv % p
    return out


def fold(F, values, beta, layer):
    """one layer of arity 2^eta: eta arity-2 folds with beta, beta^2, beta^4"""
    p = F.p
    f = [int(v) for v in values]
    assert len(f) == F.size(layer)
    s, w, b = F.layer_shift(layer), F.root(len(f)), int(beta) % p
    for _ in range(F.eta):
        f = fold2(p, f, b, s, w)
        s, w, b = s * s % p, w * w % p, b * b % p
    return f


def leaf(F, f, l, j):
    m = F.leaves(l)
    return [f[j + t * m] for t in range(F.A)]


def transcript(F, seed, roots, final):
    """-> (betas, [[j_l for l < L] for every query])"""
    c = [int(v) for v in seed]
    assert len(c) == F.D
    betas = []
    for root in roots:
        c = PR.sponge(F.P, c + list(root), F.D)
        betas.append(c[0])
    u = PR.sponge(F.P, c + list(final), F.D)
    idx = []
    for q in range(F.Q):
        j0 = PR.sponge(F.P, u + [q], 1)[0] & (F.leaves(0) - 1)
        idx.append([j0 % F.leaves(l) for l in range(F.L)])
    return betas, idx


def commit_phase(F, evals, seed):
    """-> (layers f_0 .. f_L, trees, roots, betas)"""
    c = [int(v) for v in seed]
    f = [int(v) for v in evals]
    layers, trees, roots, betas = [f], [], [], []
    for l in range(F.L):
        t = PR.MerkleTree(F.P, [leaf(F, f, l, j) for j in range(F.leaves(l))], F.D)
        trees.append(t)
        roots.append(t.root_hash())
        c = PR.sponge(F.P, c + t.root_hash(), F.D)
        betas.append(c[0])
        f = fold(F, f, c[0], l)
        layers.append(f)
    return layers, trees, roots, betas


def prove(F, evals, seed):
    """the proof as a flat list of canonical words"""
    p = F.p
    layers, trees, roots, betas = commit_phase(F, evals, seed)
    final = layers[F.L]
    betas2, idx = transcript(F, seed, roots, final)
    assert betas2 == betas
    proof = [w for r in roots for w in r] + list(final)
    for l in range(F.L):
        for q in range(F.Q):
            proof += [v % p for v in leaf(F, layers[l], l, idx[q][l])]
        for q in range(F.Q):
            proof += [w for sib, _ in trees[l].get_proof(idx[q][l]) for w in sib]
    assert len(proof) == F.proof_words()
    return proof


def split(F, proof):
    """-> (roots, final, leaf values [l][q], paths [l][q][level])"""
    proof = [int(w) for w in proof]
    assert len(proof) == F.proof_words()
    D, Q, A = F.D, F.Q, F.A
    roots = [proof[l * D:(l + 1) * D] for l in range(F.L)]
    off = F.L * D
    final = proof[off:off + F.size(F.L)]
    off += F.size(F.L)
    vals, paths = [], []
    for l in range(F.L):
        vals.append([proof[off + q * A: off + (q + 1) * A] for q in range(Q)])
        off += Q * A
        dp = F.depth(l)
        paths.append([[proof[off + (q * dp + k) * D: off + (q * dp + k + 1) * D] for k in range(dp)] for q in range(Q)])
        off += Q * dp * D
    return roots, final, vals, paths


def final_coefficients(F, final):
    """the interpolant of the final layer on s^(A^L) <w_(N_L)>"""
    p = F.p
    n = len(final)
    winv = pow(F.root(n), p - 2, p)
    sinv = pow(F.layer_shift(F.L), p - 2, p)
    ninv = pow(n, p - 2, p)
    return [ninv * pow(sinv, k, p) * sum(final[i] * pow(winv, i * k, p) for i in range(n)) % p for k in range(n)]


def verify(F, proof, seed):
    """0, or bits: 1 a Merkle path fails, 2 a fold mismatch, 4 the final layer is not of low degree; every check runs"""
    p = F.p
    roots, final, vals, paths = split(F, proof)
    betas, idx = transcript(F, seed, roots, final)
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
            f, b, w = list(vals[l][q]), betas[l], F.root(F.A)
            while len(f) > 1:
                f = fold2(p, f, b, x, w)
                x, w, b = x * x % p, w * w % p, b * b % p
            if l + 1 < F.L:
                want = vals[l + 1][q][j // F.leaves(l + 1)]
            else:
                want = final[j]
            if f[0] != want:      # the proof's word as it stands: a word >= p never matches
                status |= 2
    coeffs = final_coefficients(F, [v % p for v in final])
    if any(coeffs[len(final) >> F.log2_blowup:]):
        status |= 4
    return status
