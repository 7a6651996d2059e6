"""Pure-Python restatement of the STARK layer (include/ronk_ntt.h "STARK") on Python integers, on top of tests/air_ref.py,
tests/mpcs_ref.py, tests/poseidon_ref.py and tests/plonk_ref.py (Domain): the points and masks a program implies, the transcript, the
quotient split, the prover, the verifier and the proof layout.  A trace round is a list of C_r rows of N words on <w_N>; a round
may also be a function of the challenge pairs drawn so far (an accumulator column built from them).  This file is the normative
restatement of those semantics.  A test helper, not product code; it shares nothing with the library."""
import air_ref as AR
import deep_ref as DR
import ext2_ref as ER
import mpcs_ref as MR
import plonk_ref as PL
import poseidon_ref as PR

MAX_R, MAX_K = 4, 8
ZETA_BASE, OOD = 128, 256      # the status bits of this layer


def rotations(ops, N):
    """[0] and then every distinct non-zero rot mod N in the order of the program's cells: point k is zeta w_N^rots[k]"""
    rots = [0]
    for o in AR.cells(ops):
        rot = AR.decode(o)[2] % N
        if rot not in rots:
            rots.append(rot)
    return rots


def layout(columns, n_ext):
    """-> (base columns per round, first flat base index per round, first extension index per round)"""
    base = [c - 2 * e for c, e in zip(columns, n_ext)]
    return base, [sum(base[:r]) for r in range(len(base))], [sum(n_ext[:r]) for r in range(len(base))]


def where(columns, n_ext, kind, index):
    """the round of a column cell and its first row there (an extension column has two: c0, c1)"""
    base, boff, eoff = layout(columns, n_ext)
    for r in range(len(columns)):
        if kind == AR.BASE and boff[r] <= index < boff[r] + base[r]:
            return r, index - boff[r]
        if kind == AR.EXT and eoff[r] <= index < eoff[r] + n_ext[r]:
            return r, base[r] + 2 * (index - eoff[r])
    raise IndexError("a cell outside the rounds")


def masks(ops, N, columns, n_ext):
    """the trace rounds' masks: bit 0, and the bit of every rotation at which one of the round's columns is read"""
    rots = rotations(ops, N)
    out = [1] * len(columns)
    for o in AR.cells(ops):
        kind, index, rot = AR.decode(o)
        out[where(columns, n_ext, kind, index)[0]] |= 1 << rots.index(rot % N)
    return out


def check_shape(columns, n_ext, n_pub, n_draw, n_chal, n_points):
    """this family's own codes, after those of ronk_air_check, ronk_mpcs_check and ronk_plonk_check: 0, 'invalid' or 'unsupported'"""
    if columns is None or n_ext is None or n_draw is None or len(columns) == 0:
        return "invalid"
    R = min(len(columns), MAX_R)
    if any(2 * n_ext[r] > columns[r] for r in range(R)) or n_pub + sum(n_draw[:R]) != n_chal:
        return "invalid"
    if len(columns) > MAX_R or n_points > MAX_K:
        return "unsupported"
    return 0


class Stark:
    def __init__(self, P, g, w, log2_n, log2_b, shift, eta, log2_final, n_queries, digest_len, columns, n_ext, n_pub, n_draw, n_chal, prog,
                 fri=None):
        self.P, self.p, self.prog = P, P.p, prog
        self.dom = PL.Domain(P.p, g, log2_n, log2_b, shift)
        self.E = ER.Ext2(P.p, w)
        self.N, self.B, self.M = self.dom.N, self.dom.B, self.dom.M
        self.R, self.Cs, self.Es, self.n_pub, self.n_draw = len(columns), list(columns), list(n_ext), n_pub, list(n_draw)
        self.rots = rotations(prog.ops, self.N)
        self.K, self.D, self.J = len(self.rots), digest_len, prog.n_constraints
        assert check_shape(columns, n_ext, n_pub, n_draw, n_chal, self.K) == 0
        self.masks = masks(prog.ops, self.N, columns, n_ext) + [1]
        self.S = MR.Mpcs(P, g, w, log2_n + log2_b, shift, eta, log2_final, log2_b, n_queries, digest_len, self.K,
                         self.Cs + [2 * self.B], self.masks, fri=fri)

    def proof_words(self):
        return (self.R + 1) * self.D + self.S.proof_words()

    def inner_offset(self):
        return (self.R + 1) * self.D


# ---------------------------------------------------------------------------------------------------- transcript
def begin(st, seed, pub):
    """t = sponge(seed || pub as [n_pub][2] words)"""
    assert len(seed) == st.D and len(pub) == st.n_pub
    return PR.sponge(st.P, [int(v) for v in seed] + [int(c) for pair in pub for c in pair], st.D)


def after_round(st, t, r, root):
    """-> (t, the pairs drawn after round r, lambda or None)"""
    extra = 1 if r == st.R - 1 else 0
    out = PR.sponge(st.P, list(t) + [int(v) for v in root], st.D + 2 * (st.n_draw[r] + extra))
    draws = [(out[st.D + 2 * k], out[st.D + 2 * k + 1]) for k in range(st.n_draw[r] + extra)]
    return out[:st.D], draws[:st.n_draw[r]], draws[-1] if extra else None


def after_quotient(st, t, root):
    """-> (t, zeta)"""
    out = PR.sponge(st.P, list(t) + [int(v) for v in root], st.D + 2)
    return out[:st.D], (out[st.D], out[st.D + 1])


def weights(st, lam):
    """lambda_j = lambda^j, j < J, by repeated products"""
    out = [st.E.one]
    for _ in range(st.J - 1):
        out.append(st.E.mul(out[-1], st.E.el(lam)))
    return out


def points(st, zeta):
    return [st.E.mul_base(st.E.el(zeta), pow(st.dom.wN, rot, st.p)) for rot in st.rots]


# ---------------------------------------------------------------------------------------------------- the quotient split
def split_quotient(st, T):
    """T as M pairs on the coset -> the [2B][N] coefficient matrix of the pieces: row 2 i + pl = plane pl of
    q_i(x) = sum_(k < N) c_(i N + k) x^k, c_j the monomial coefficients of T"""
    planes = [PL.coset_coefficients(st.dom, [v[pl] for v in T]) for pl in (0, 1)]
    return [planes[pl][i * st.N:(i + 1) * st.N] for i in range(st.B) for pl in (0, 1)]


def air_columns(st, Ms):
    """the extended rounds as the AIR's inputs: the flat base columns and the extension columns (two planes each)"""
    base, ext = [], []
    for r in range(st.R):
        nb = st.Cs[r] - 2 * st.Es[r]
        base += Ms[r][:nb]
        ext += [[Ms[r][nb + 2 * e], Ms[r][nb + 2 * e + 1]] for e in range(st.Es[r])]
    return base, ext


# ---------------------------------------------------------------------------------------------------- prover, verifier
def prove(st, seed, pub, rounds, tweak=None):
    """-> (the proof as a flat list of canonical words, status, the challenge table); rounds[r]: C_r rows of N words, or a function
    of the challenge pairs known after round r - 1 that returns them; tweak: passed on to mpcs_ref.open_"""
    S, E, p = st.S, st.E, st.p
    t = begin(st, seed, pub)
    chal = [E.el(c) for c in pub]
    coefs, Ms, trees, lam = [], [], [], None
    for r in range(st.R):
        rows = rounds[r](list(chal)) if callable(rounds[r]) else rounds[r]
        assert len(rows) == st.Cs[r] and all(len(row) == st.N for row in rows)
        coefs.append([PL.interpolate(p, st.dom.wN, [int(v) % p for v in row]) for row in rows])
        Ms.append(DR.columns(S.rounds[r], coefs[r]))
        trees.append(MR.commit(S, r, Ms[r]))
        t, draws, lam = after_round(st, t, r, trees[r].root_hash())
        chal += draws
    base, ext = air_columns(st, Ms)
    T = AR.quotient(E, st.dom, st.prog, base, ext, chal, weights(st, lam))
    coefs.append(split_quotient(st, T))
    Ms.append(DR.columns(S.rounds[st.R], coefs[st.R]))
    trees.append(MR.commit(S, st.R, Ms[st.R]))
    t, zeta = after_quotient(st, t, trees[st.R].root_hash())
    inner, status = MR.open_(S, Ms, trees, coefs, points(st, zeta), t, tweak=tweak)
    if zeta[1] == 0:
        status |= ZETA_BASE
    proof = [w for tree in trees for w in tree.root_hash()] + inner
    assert len(proof) == st.proof_words()
    return proof, status, chal


def replay(st, seed, pub, proof):
    """the verifier's transcript: -> (roots, t, the challenge table, lambda, zeta)"""
    D = st.D
    roots = [[int(w) for w in proof[r * D:(r + 1) * D]] for r in range(st.R + 1)]
    t = begin(st, seed, pub)
    chal, lam = [st.E.el(c) for c in pub], None
    for r in range(st.R):
        t, draws, lam = after_round(st, t, r, roots[r])
        chal += draws
    t, zeta = after_quotient(st, t, roots[st.R])
    return roots, t, chal, lam, zeta


def cell_values(st, ys):
    """the pair of every cell of the program from the claims: a base column's claim at the point of its rot, an extension column's
    c0-claim + t c1-claim"""
    E, out = st.E, []
    for o in AR.cells(st.prog.ops):
        kind, index, rot = AR.decode(o)
        r, row = where(st.Cs, st.Es, kind, index)
        y = ys[r][st.rots.index(rot % st.N)]
        out.append(E.el(y[row]) if kind == AR.BASE else E.add(E.el(y[row]), E.mul((0, 1), E.el(y[row + 1]))))
    return out


def quotient_at(st, ys, zeta):
    """sum_i zeta^(i N) (y_Q[2 i] + t y_Q[2 i + 1]) from the quotient round's claims at zeta"""
    E = st.E
    zN, acc = E.pow(E.el(zeta), st.N), E.zero
    for i in reversed(range(st.B)):
        y = ys[st.R][0]
        acc = E.add(E.mul(acc, zN), E.add(E.el(y[2 * i]), E.mul((0, 1), E.el(y[2 * i + 1]))))
    return acc


def verify(st, seed, pub, proof):
    """0, or bits: 1 / 2 / 4 / 8 / 16 / 32 / 64 as mpcs_ref.verify reports them, 128 zeta has a zero second word, 256 the
    out-of-domain identity fails (or cannot be evaluated: zeta^N = 1); every check runs"""
    proof = [int(w) for w in proof]
    assert len(proof) == st.proof_words()
    roots, t, chal, lam, zeta = replay(st, seed, pub, proof)
    inner = proof[st.inner_offset():]
    status = MR.verify(st.S, roots, points(st, zeta), t, inner)
    if zeta[1] == 0:
        status |= ZETA_BASE
    ys = MR.claims_from_words(st.S, inner[:2 * st.S.Y])
    want = AR.eval_point(st.E, st.dom, st.prog, zeta, cell_values(st, ys), chal, weights(st, lam))
    if want is None or quotient_at(st, ys, zeta) != want:
        status |= OOD
    return status
