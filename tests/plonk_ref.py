"""Pure-Python restatement of the PLONK quotient on the evaluation coset (include/ronk_ntt.h "PLONK quotient") on Python integers,
with what a test needs around it: a small circuit generator, the witness, the grand product Z (tests/accum_ref.py), the extension
of a column to the coset by plain integer evaluation and the way back to coefficients.  The reference has no prover, so this file
is the normative restatement of those semantics; the extension field is that of tests/ext2_ref.py.  A test helper, not product
code; it shares nothing with the library."""
import accum_ref as AR
from ext2_ref import Ext2, pairs, planar  # noqa: F401  (re-exported for the tests)

LABELS = (1, 2, 3)      # the reference's Cell::label multipliers


class Domain:
    """N = 2^log2_n trace rows, B = 2^log2_blowup, M = N B; x_i = s w_M^i"""

    def __init__(self, p, g, log2_n, log2_blowup, shift):
        self.p, self.N, self.B = p, 1 << log2_n, 1 << log2_blowup
        self.M = self.N * self.B
        assert (p - 1) % self.M == 0 and shift % p != 0 and pow(shift, self.M, p) != 1
        self.s = shift % p
        self.wM = pow(g, (p - 1) // self.M, p)
        self.wN = pow(self.wM, self.B, p)
        # x^N - 1 takes B values: s^N w_B^(i mod B) - 1
        sN, wB = pow(self.s, self.N, p), pow(self.wM, self.N, p)
        self.vanish_inv = [pow((sN * pow(wB, j, p) - 1) % p, -1, p) for j in range(self.B)]
        self.n_inv = pow(self.N, -1, p)

    def x(self, i):
        return self.s * pow(self.wM, i, self.p) % self.p

    def points(self):
        out, x = [], self.s
        for _ in range(self.M):
            out.append(x)
            x = x * self.wM % self.p
        return out


class Columns:
    """the inputs of one call, all on the coset: wires [3][M], sel [5][M] (ql, qr, qm, qo, qc), sigma [3][M], pi [M] or None,
    Z as two planes [2][M]; any integers"""

    def __init__(self, wires, sel, sigma, pi, Z):
        self.wires, self.sel, self.sigma, self.pi, self.Z = wires, sel, sigma, pi, Z


def row_terms(E, dom, cols, beta, gamma, i, x=None, k=LABELS):
    """-> (G_i, P1_i, Z_i) at row i: the gate value as a base integer, the first permutation constraint and Z as pairs"""
    p = E.p
    x = dom.x(i) if x is None else x
    a, b, o = (int(c[i]) % p for c in cols.wires)
    ql, qr, qm, qo, qc = (int(c[i]) % p for c in cols.sel)
    pi = 0 if cols.pi is None else int(cols.pi[i]) % p
    G = (a * ql + b * qr + a * b * qm + o * qo + qc + pi) % p
    j = (i + dom.B) % dom.M
    Z = E.el((cols.Z[0][i], cols.Z[1][i]))
    num, den = Z, E.el((cols.Z[0][j], cols.Z[1][j]))
    for c, wv in enumerate((a, b, o)):
        num = E.mul(num, E.add(E.add(E.embed(wv), E.mul_base(beta, k[c] % p * x % p)), gamma))
        den = E.mul(den, E.add(E.add(E.embed(wv), E.mul_base(beta, int(cols.sigma[c][i]) % p)), gamma))
    return G, E.sub(num, den), Z


def quotient_row(E, dom, cols, alpha, beta, gamma, i, x=None, k=LABELS):
    """T_i = (G_i + alpha P1_i + alpha^2 P2_i) / (x_i^N - 1), P2_i = (Z_i - 1) L1(x_i), L1(x) = (x^N - 1) / (N (x - 1))"""
    p = E.p
    alpha, beta, gamma = E.el(alpha), E.el(beta), E.el(gamma)
    x = dom.x(i) if x is None else x
    G, P1, Z = row_terms(E, dom, cols, beta, gamma, i, x, k)
    vinv = dom.vanish_inv[i % dom.B]
    vanish = pow(vinv, -1, p)
    L1 = vanish * dom.n_inv % p * pow((x - 1) % p, -1, p) % p
    P2 = E.mul_base(E.sub(Z, E.one), L1)
    total = E.add(E.add(E.embed(G), E.mul(alpha, P1)), E.mul(E.mul(alpha, alpha), P2))
    return E.mul_base(total, vinv)


def quotient(E, dom, cols, alpha, beta, gamma, k=LABELS):
    """every row -> M pairs"""
    return [quotient_row(E, dom, cols, alpha, beta, gamma, i, x, k) for i, x in enumerate(dom.points())]


# ------------------------------------------------------------------------------------------------ polynomials by plain evaluation
def interpolate(p, w, vals):
    """the coefficients of the polynomial of degree < n with f(w^i) = vals[i]; w of order n = len(vals).  O(n^2)."""
    n = len(vals)
    winv, ninv = pow(w, -1, p), pow(n, -1, p)
    pw = [pow(winv, j, p) for j in range(n)]
    return [sum(int(v) * pw[i * j % n] for i, v in enumerate(vals)) % p * ninv % p for j in range(n)]


def evaluate(p, coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % p
    return acc


def evaluate_ext(E, coef, z):
    """a polynomial with base coefficients at the extension point z"""
    acc = E.zero
    for c in reversed(coef):
        acc = E.add(E.mul(acc, z), E.embed(c))
    return acc


def extend(dom, vals):
    """N values on <w_N> -> the M values of the same polynomial on the coset"""
    coef = interpolate(dom.p, dom.wN, vals)
    return [evaluate(dom.p, coef, x) for x in dom.points()]


def coset_coefficients(dom, vals):
    """M values on the coset -> the M coefficients (the inverse coset transform)"""
    c = interpolate(dom.p, dom.wM, vals)
    sinv = pow(dom.s, -1, dom.p)
    return [v * pow(sinv, j, dom.p) % dom.p for j, v in enumerate(c)]


# ------------------------------------------------------------------------------------------------ a small circuit
class Circuit:
    """rows of (kind, a, b, o) over a pool of variables; sel [5][N], pi [N], var [3][N] the variable of every cell, value[v]"""


def circuit(rng, p, log2_n, n_gates=None, seed_vars=2):
    """random add / mul / constant / public-input gates, then padding rows with zero selectors whose cells repeat variables of the
    pool.  rng: numpy Generator.  Every variable's value follows from the gates, so the witness satisfies them all."""
    N = 1 << log2_n
    n_gates = N - max(1, N // 4) if n_gates is None else n_gates
    assert seed_vars <= n_gates <= N
    c = Circuit()
    c.p, c.N = p, N
    c.sel, c.pi, c.var, c.value = [[0] * N for _ in range(5)], [0] * N, [[0] * N for _ in range(3)], []
    ql, qr, qm, qo, qc = c.sel

    def any_var():
        return int(rng.integers(0, len(c.value)))

    for i in range(N):
        if i < seed_vars or (seed_vars < i < n_gates and int(rng.integers(0, 4)) == 0):     # row seed_vars is an add / mul gate
            # a = v by a constant (qc = -v) or by a public input (pi = -v): a new variable
            v = int(rng.integers(0, 2**62)) % p
            c.value.append(v)
            ql[i] = 1
            if int(rng.integers(0, 2)):
                qc[i] = -v % p
            else:
                c.pi[i] = -v % p
            c.var[0][i] = len(c.value) - 1
            c.var[1][i], c.var[2][i] = any_var(), any_var()
        elif i < n_gates:
            a, b = any_var(), any_var()
            if int(rng.integers(0, 2)):
                ql[i], qr[i], v = 1, 1, (c.value[a] + c.value[b]) % p
            else:
                qm[i], v = 1, c.value[a] * c.value[b] % p
            qo[i] = p - 1
            c.value.append(v)
            c.var[0][i], c.var[1][i], c.var[2][i] = a, b, len(c.value) - 1
        else:
            c.var[0][i], c.var[1][i], c.var[2][i] = any_var(), any_var(), any_var()
    return c


def witness(c):
    return [[c.value[v] for v in col] for col in c.var]


def labels(dom, k=LABELS):
    """ids[c][i] = k_c w_N^i"""
    out = []
    for kc in k:
        col, x = [], kc % dom.p
        for _ in range(dom.N):
            col.append(x)
            x = x * dom.wN % dom.p
        out.append(col)
    return out


def sigma_of(c, ids):
    """the cells of every variable form one cycle: sigma of a cell is the label of the next cell of its variable"""
    cells = {}
    for col in range(3):
        for i in range(c.N):
            cells.setdefault(c.var[col][i], []).append((col, i))
    sigma = [[0] * c.N for _ in range(3)]
    for group in cells.values():
        for (col, i), (ncol, ni) in zip(group, group[1:] + group[:1]):
            sigma[col][i] = ids[ncol][ni]
    return sigma


def trace_columns(E, dom, c, wires, sigma, beta, gamma, k=LABELS):
    """the N-row columns of a call and the grand product: -> (Columns on <w_N>, Z[N])"""
    Z, last, status = AR.perm_product(E, wires, labels(dom, k), sigma, beta, gamma)
    assert status == 0
    return Columns(wires, c.sel, sigma, c.pi, [[z[0] for z in Z], [z[1] for z in Z]]), last


def on_coset(dom, t):
    """every column of a trace-domain Columns extended to the coset"""
    ext = lambda cols: [extend(dom, col) for col in cols]      # noqa: E731
    return Columns(ext(t.wires), ext(t.sel), ext(t.sigma), None if t.pi is None else extend(dom, t.pi), ext(t.Z))


def high_coefficients(E, dom, T):
    """the coefficients of both planes of T from index 3N - 3 upward"""
    lo = 3 * dom.N - 3
    return [coset_coefficients(dom, [t[plane] for t in T])[lo:] for plane in (0, 1)]
