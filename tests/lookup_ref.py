"""Pure-Python restatement of the lookup multiplicities and the logUp quotient on the evaluation coset (include/ronk_ntt.h "lookup
multiplicities and the logUp quotient") on Python integers.  The reference has no prover, so this file is the normative
restatement of those semantics; the domain is that of tests/plonk_ref.py, the extension that of tests/ext2_ref.py.  A test helper,
not product code; it shares nothing with the library."""
from ext2_ref import Ext2, pairs, planar  # noqa: F401  (re-exported for the tests)

NONE_MISSING = 2**64 - 1


def multiplicities(p, table, vals, negate=False):
    """table: T words; vals: C columns of n words; any integers, compared mod p.  -> (mult[T], missing_count, first_missing):
    mult[j] = #{(c, i): vals[c][i] = table[j]} mod p (p minus that, 0 staying 0, with negate) at the smallest index j of each
    table value and 0 at every other; missing_count the cells whose value the table lacks, first_missing the smallest c n + i
    among them or 2^64 - 1"""
    first = {}
    for j, t in enumerate(table):
        first.setdefault(int(t) % p, j)
    count = [0] * len(table)
    missing, where = 0, NONE_MISSING
    n = len(vals[0])
    for c, col in enumerate(vals):
        assert len(col) == n
        for i, v in enumerate(col):
            j = first.get(int(v) % p)
            if j is None:
                missing += 1
                where = min(where, c * n + i)
            else:
                count[j] += 1
    mult = [k % p for k in count]
    if negate:
        mult = [(p - k) % p for k in mult]
    return mult, missing, where


def quotient_row(E, dom, vals, mult, S, alpha, lam, T_in, i, x=None):
    """T_out_i = T_in_i + lambda0 R / (x_i^N - 1) + lambda1 S_i L1(x_i) / (x_i^N - 1) with L1(x) = (x^N - 1) / (N (x - 1)),
    R = (S_((i+B) mod M) - S_i) P - Q, P = prod_c D_c, Q = sum_c m_c[i] prod_(c' != c) D_c', D_c = alpha + v_c[i].
    vals, mult (or None: all ones): C columns of M words; S, T_in (or None: zero): two planes of M words; lam = (lambda0, lambda1)"""
    p = E.p
    alpha, l0, l1 = E.el(alpha), E.el(lam[0]), E.el(lam[1])
    x = dom.x(i) if x is None else x
    D = [E.add(alpha, E.embed(int(col[i]) % p)) for col in vals]
    P = E.one
    for d in D:
        P = E.mul(P, d)
    Q = E.zero
    for c in range(len(D)):
        term = E.embed(1 if mult is None else int(mult[c][i]) % p)
        for k, d in enumerate(D):
            if k != c:
                term = E.mul(term, d)
        Q = E.add(Q, term)
    j = (i + dom.B) % dom.M
    Si, Sn = E.el((S[0][i], S[1][i])), E.el((S[0][j], S[1][j]))
    R = E.sub(E.mul(E.sub(Sn, Si), P), Q)
    vinv = dom.vanish_inv[i % dom.B]
    L1 = pow(vinv, -1, p) * dom.n_inv % p * pow((x - 1) % p, -1, p) % p
    total = E.add(E.mul(l0, R), E.mul(l1, E.mul_base(Si, L1)))
    out = E.mul_base(total, vinv)
    if T_in is not None:
        out = E.add(out, E.el((T_in[0][i], T_in[1][i])))
    return out


def quotient(E, dom, vals, mult, S, alpha, lam, T_in=None):
    """every row -> M pairs"""
    return [quotient_row(E, dom, vals, mult, S, alpha, lam, T_in, i, x) for i, x in enumerate(dom.points())]


# ------------------------------------------------------------------------------------------------ the same values, faster
# quotient_row above is the definition.  The GPU suite compares every row of up to 2^13 rows and 16 columns against it; this form
# computes the same pairs with the arithmetic written out on local integers, P and Q by the streaming recurrence
# Q <- Q D_c + m_c P, P <- P D_c, and ONE modular inversion for all the differences x_i - 1 (Montgomery's trick);
# tests/test_lookup_ref.py holds it to the definition.
def quotient_fast(E, dom, vals, mult, S, alpha, lam, T_in=None):
    """columns as lists of Python integers -> M pairs"""
    from accum_ref import _batch_inverse_norms
    p, w, M, B = E.p, E.w, dom.M, dom.B
    a0, a1 = E.el(alpha)
    (l00, l01), (l10, l11) = E.el(lam[0]), E.el(lam[1])
    l10, l11 = l10 * dom.n_inv % p, l11 * dom.n_inv % p
    dinv = _batch_inverse_norms(p, [(x - 1) % p for x in dom.points()])
    wa1 = w * a1 % p
    out = []
    for i in range(M):
        P0, P1, Q0, Q1 = 1, 0, 0, 0
        for c, col in enumerate(vals):
            d0 = (a0 + col[i]) % p
            m = 1 if mult is None else mult[c][i] % p
            Q0, Q1 = (Q0 * d0 + Q1 * wa1 + m * P0) % p, (Q0 * a1 + Q1 * d0 + m * P1) % p
            P0, P1 = (P0 * d0 + P1 * wa1) % p, (P0 * a1 + P1 * d0) % p
        j = (i + B) % M
        s0, s1 = S[0][i] % p, S[1][i] % p
        e0, e1 = (S[0][j] - s0) % p, (S[1][j] - s1) % p
        r0, r1 = (e0 * P0 + w * e1 * P1 - Q0) % p, (e0 * P1 + e1 * P0 - Q1) % p
        v, d = dom.vanish_inv[i % B], dinv[i]
        t0 = (l00 * r0 + w * l01 * r1) * v + (l10 * s0 + w * l11 * s1) * d
        t1 = (l00 * r1 + l01 * r0) * v + (l10 * s1 + l11 * s0) * d
        if T_in is not None:
            t0, t1 = t0 + T_in[0][i], t1 + T_in[1][i]
        out.append((t0 % p, t1 % p))
    return out
