"""Pure-Python restatement of the STARK layer with a fixed round and periodic columns (include/ronk_ntt.h "STARK": fixed) on
Python integers, on top of tests/stark_ref.py and tests/air_per_ref.py: the fixed round and its commitment, the transcript step
that binds its root, the shifted numbering of the inner commitment's rounds, the prover, and a verifier that takes the verifier's
own root.  With no fixed round and no periodic column every word is that of stark_ref.  This file is the normative restatement of
those words.  A test helper, not product code; it shares nothing with the library."""
from collections import namedtuple

import air_per_ref as APR
import air_ref as AR
import deep_ref as DR
import ext2_ref as ER
import mpcs_ref as MR
import plonk_ref as PL
import poseidon_ref as PR
import stark_ref as SR
from stark_ref import OOD, ZETA_BASE  # noqa: F401  (re-exported for the tests)

# what the preprocessing leaves: the coefficients [C_F][N], the extended matrix [C_F][M] and its tree
Fixed = namedtuple("Fixed", "coef M tree")


class Stark(SR.Stark):
    """stark_ref.Stark with n_fixed columns in a fixed round and the values of the periodic columns.  R, Cs, Es count the TRACE rounds
    as there; the inner commitment S has the fixed round (when there is one) in front of them: trace round r is its round fo + r"""

    def __init__(self, P, g, w, log2_n, log2_b, shift, eta, log2_final, n_queries, digest_len, columns, n_ext, n_pub, n_draw, n_chal, prog,
                 n_fixed=0, periodic=(), fri=None):
        self.P, self.p, self.prog = P, P.p, prog
        self.dom = PL.Domain(P.p, g, log2_n, log2_b, shift)
        self.E = ER.Ext2(P.p, w)
        self.N, self.B, self.M = self.dom.N, self.dom.B, self.dom.M
        self.R, self.Cs, self.Es, self.n_pub, self.n_draw = len(columns), list(columns), list(n_ext), n_pub, list(n_draw)
        self.F, self.fo, self.periodic = n_fixed, 1 if n_fixed else 0, [list(v) for v in periodic]
        assert len(self.periodic) <= 16 and all(self.N % len(v) == 0 for v in self.periodic)
        # the fixed round is laid out as a trace round without extension columns in front of the others: group 0, the first indices
        self.all_Cs, self.all_Es = [n_fixed] * self.fo + self.Cs, [0] * self.fo + self.Es
        self.rots = SR.rotations(prog.ops, self.N)
        self.K, self.D, self.J = len(self.rots), digest_len, prog.n_constraints
        assert SR.check_shape(columns, n_ext, n_pub, n_draw, n_chal, self.K) == 0
        self.masks = SR.masks(prog.ops, self.N, self.all_Cs, self.all_Es) + [1]
        self.S = MR.Mpcs(P, g, w, log2_n + log2_b, shift, eta, log2_final, log2_b, n_queries, digest_len, self.K,
                         self.all_Cs + [2 * self.B], self.masks, fri=fri)

    # proof_words and inner_offset are stark_ref's: the proof does not carry the fixed root


# ---------------------------------------------------------------------------------------------------- the fixed round
def fixed_commit(st, rows):
    """the preprocessing, once and outside any proof: C_F rows of N words on <w_N> -> Fixed"""
    assert st.F and len(rows) == st.F and all(len(row) == st.N for row in rows)
    coef = [PL.interpolate(st.p, st.dom.wN, [int(v) % st.p for v in row]) for row in rows]
    M = DR.columns(st.S.rounds[0], coef)
    return Fixed(coef, M, MR.commit(st.S, 0, M))


def fixed_root(fixed):
    return fixed.tree.root_hash()


def after_fixed(st, t, root):
    """t = sponge(t || root_F) squeezing D words: the step of a round without a draw"""
    return PR.sponge(st.P, list(t) + [int(v) for v in root], st.D)


def begin(st, seed, pub, root):
    t = SR.begin(st, seed, pub)
    return after_fixed(st, t, root) if st.F else t


def air_columns(st, Ms):
    """the AIR's inputs from the inner commitment's extended rounds: the fixed columns first, then stark_ref's"""
    base, ext = SR.air_columns(st, Ms[st.fo:])
    return (Ms[0] if st.F else []) + base, ext


# ---------------------------------------------------------------------------------------------------- prover, verifier
def prove(st, seed, pub, rounds, fixed=None, tweak=None):
    """-> (the proof as a flat list of canonical words, status, the challenge table); fixed: what fixed_commit returned"""
    S, E, p, fo = st.S, st.E, st.p, st.fo
    assert (fixed is not None) == bool(st.F)
    t = begin(st, seed, pub, fixed_root(fixed) if st.F else None)
    chal = [E.el(c) for c in pub]
    coefs, Ms, trees, lam = ([fixed.coef], [fixed.M], [fixed.tree], None) if st.F else ([], [], [], None)
    for r in range(st.R):
        rows = rounds[r](list(chal)) if callable(rounds[r]) else rounds[r]
        assert len(rows) == st.Cs[r] and all(len(row) == st.N for row in rows)
        coefs.append([PL.interpolate(p, st.dom.wN, [int(v) % p for v in row]) for row in rows])
        Ms.append(DR.columns(S.rounds[fo + r], coefs[fo + r]))
        trees.append(MR.commit(S, fo + r, Ms[fo + r]))
        t, draws, lam = SR.after_round(st, t, r, trees[fo + r].root_hash())
        chal += draws
    base, ext = air_columns(st, Ms)
    T = APR.quotient(E, st.dom, st.prog, base, ext, chal, SR.weights(st, lam), st.periodic)
    RQ = fo + st.R
    coefs.append(SR.split_quotient(st, T))
    Ms.append(DR.columns(S.rounds[RQ], coefs[RQ]))
    trees.append(MR.commit(S, RQ, Ms[RQ]))
    t, zeta = SR.after_quotient(st, t, trees[RQ].root_hash())
    inner, status = MR.open_(S, Ms, trees, coefs, SR.points(st, zeta), t, tweak=tweak)
    if zeta[1] == 0:
        status |= ZETA_BASE
    proof = [w for tree in trees[fo:] for w in tree.root_hash()] + inner
    assert len(proof) == st.proof_words()
    return proof, status, chal


def replay(st, seed, pub, proof, root=None):
    """the verifier's transcript: -> (the inner commitment's roots, its own first, t, the challenge table, lambda, zeta)"""
    D = st.D
    roots = [[int(w) for w in proof[r * D:(r + 1) * D]] for r in range(st.R + 1)]
    t = begin(st, seed, pub, root)
    chal, lam = [st.E.el(c) for c in pub], None
    for r in range(st.R):
        t, draws, lam = SR.after_round(st, t, r, roots[r])
        chal += draws
    t, zeta = SR.after_quotient(st, t, roots[st.R])
    return ([[int(w) for w in root]] if st.F else []) + roots, t, chal, lam, zeta


def cell_values(st, ys):
    """stark_ref.cell_values on the inner commitment's rounds: a cell (BASE, index < C_F, rot) is the fixed round's claim"""
    E, out = st.E, []
    for o in AR.cells(st.prog.ops):
        kind, index, rot = AR.decode(o)
        r, row = SR.where(st.all_Cs, st.all_Es, kind, index)
        y = ys[r][st.rots.index(rot % st.N)]
        out.append(E.el(y[row]) if kind == AR.BASE else E.add(E.el(y[row]), E.mul((0, 1), E.el(y[row + 1]))))
    return out


def quotient_at(st, ys, zeta):
    """stark_ref.quotient_at with the quotient's claims in the inner commitment's last round"""
    E = st.E
    zN, acc, y = E.pow(E.el(zeta), st.N), E.zero, ys[st.fo + st.R][0]
    for i in reversed(range(st.B)):
        acc = E.add(E.mul(acc, zN), E.add(E.el(y[2 * i]), E.mul((0, 1), E.el(y[2 * i + 1]))))
    return acc


def verify(st, seed, pub, proof, root=None):
    """stark_ref.verify's status with `root` the VERIFIER'S root of the fixed round (D words; None without one): the proof carries
    none, so a proof made for another fixed round fails wherever that root enters -- the transcript, the inner opening's list"""
    proof = [int(w) for w in proof]
    assert len(proof) == st.proof_words() and (root is not None) == bool(st.F)
    roots, t, chal, lam, zeta = replay(st, seed, pub, proof, root)
    inner = proof[st.inner_offset():]
    status = MR.verify(st.S, roots, SR.points(st, zeta), t, inner)
    if zeta[1] == 0:
        status |= ZETA_BASE
    ys = MR.claims_from_words(st.S, inner[:2 * st.S.Y])
    want = APR.eval_point(st.E, st.dom, st.prog, zeta, cell_values(st, ys), chal, SR.weights(st, lam), st.periodic)
    if want is None or quotient_at(st, ys, zeta) != want:
        status |= OOD
    return status
