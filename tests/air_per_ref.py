"""Pure-Python restatement of the periodic columns of a constraint program (include/ronk_ntt.h "constraint programs", operand kind
6 PER) on Python integers, on top of tests/air_ref.py: the polynomial of a periodic column, its table on the evaluation coset, the
operand at a row and at an out-of-domain point, and the quotient and the evaluation at a point of a program that reads periodic
columns.  This file is the normative restatement of those words.  A test helper, not product code; it shares nothing with the
library."""
import air_ref as AR
from air_ref import ALL, EXCEPT_LAST, FIRST, LAST, Program, pairs_of, planar  # noqa: F401  (re-exported for the tests)

PER = 6


def log2(n):
    assert n > 0 and n & (n - 1) == 0, "a period is a power of two"
    return n.bit_length() - 1


def coefficients(dom, vals):
    """q of degree below P = len(vals) with q(w_P^k) = vals[k], w_P = w_N^(N/P): the inverse DFT written out as its P^2 products,
    so that nothing here leans on a transform"""
    p, P = dom.p, len(vals)
    assert dom.N % P == 0 and log2(P) >= 0
    wP_inv = pow(pow(dom.wN, dom.N // P, p), -1, p)
    power = [pow(wP_inv, t, p) for t in range(P)]
    P_inv = pow(P, -1, p)
    vals = [int(v) % p for v in vals]
    return [sum(v * power[j * k % P] for k, v in enumerate(vals)) * P_inv % p for j in range(P)]


def evaluate(p, q, y):
    r = 0
    for c in reversed(q):
        r = (r * y + c) % p
    return r


def table(dom, vals):
    """tab[j] = q(s^(N/P) w_M^(j N/P)), j < P B: the values of c(x) = q(x^(N/P)) on the coset, which repeat after P B rows because
    w_M^(N/P) has the order P B"""
    p, P = dom.p, len(vals)
    q, e, PB = coefficients(dom, vals), dom.N // P, len(vals) * dom.B
    sP, step = pow(dom.s, e, p), pow(dom.wM, e, p)
    assert pow(step, PB, p) == 1
    scaled = [c * pow(sP, k, p) % p for k, c in enumerate(q)]
    power = [pow(step, t, p) for t in range(PB)]
    return [sum(c * power[j * k % PB] for k, c in enumerate(scaled)) % p for j in range(PB)]


def tables(dom, periodic):
    return [table(dom, vals) for vals in periodic]


def on_coset(dom, tabs, o, i):
    """the PER operand o at row i: a base word"""
    kind, index, rot = AR.decode(o)
    assert kind == PER and abs(rot) < dom.N
    return tabs[index][(i + rot * dom.B) % len(tabs[index])]


def at_point(E, dom, periodic, o, z):
    """the PER operand o at the pair z: q((z w_N^rot)^(N/P)) in the extension"""
    kind, index, rot = AR.decode(o)
    assert kind == PER and abs(rot) < dom.N
    q = coefficients(dom, periodic[index])
    y = E.pow(E.mul_base(E.el(z), pow(dom.wN, rot % dom.N, dom.p)), dom.N // len(q))
    r = E.zero
    for c in reversed(q):
        r = E.add(E.mul(r, y), E.embed(c))
    return r


def cells(ops):
    """as air_ref.cells: a PER operand is no cell, the verifier evaluates it itself"""
    return AR.cells(ops)


def run(E, prog, cell, per, chal, x):
    """air_ref.run with per(o) the pair of a PER operand, which may carry a rotation"""
    reg = [None] * 256
    out = [None] * prog.n_constraints

    def read(o):
        kind, index, rot = AR.decode(o)
        if kind == AR.REG:
            assert reg[index] is not None, "a register is read before it is written"
            return reg[index]
        if kind in (AR.BASE, AR.EXT):
            return cell(o)
        if kind == PER:
            return per(o)
        assert rot == 0 and kind in (AR.CHAL, AR.IMM, AR.X)
        return E.el(chal[index]) if kind == AR.CHAL else E.embed(prog.imm[index]) if kind == AR.IMM else x

    for w in prog.ops:
        code, dst, a = w & 0xFF, (w >> 8) & 0xFF, read((w >> 16) & 0xFFFFFF)
        if code == AR.EMIT:
            j = (w >> 40) & 0xFFFFFF
            assert out[j] is None and dst <= AR.EXCEPT_LAST
            out[j] = (dst, a)
        elif code == AR.MOV:
            reg[dst] = a
        elif code == AR.NEG:
            reg[dst] = E.neg(a)
        else:
            b = read((w >> 40) & 0xFFFFFF)
            reg[dst] = {AR.ADD: E.add, AR.SUB: E.sub, AR.MUL: E.mul}[code](a, b)
    assert all(v is not None for v in out), "a constraint is never emitted"
    return out


def quotient(E, dom, prog, base, ext, chal, lam, periodic, T_in=None):
    """every row -> M pairs; periodic: one list of values per periodic column (its length the period)"""
    p, M = E.p, dom.M
    tabs = tables(dom, periodic)
    out = []
    for i, x in enumerate(dom.points()):
        def cell(o):
            kind, index, rot = AR.decode(o)
            r = (i + rot * dom.B) % M
            return E.embed(int(base[index][r])) if kind == AR.BASE else E.el((ext[index][0][r], ext[index][1][r]))

        xN = pow(dom.vanish_inv[i % dom.B], -1, p) + 1
        v = AR.combine(E, dom, run(E, prog, cell, lambda o: E.embed(on_coset(dom, tabs, o, i)), chal, E.embed(x)), lam, E.embed(x),
                       E.embed(xN))
        out.append(v if T_in is None else E.add(v, E.el((T_in[0][i], T_in[1][i]))))
    return out


def eval_point(E, dom, prog, z, cell_values, chal, lam, periodic):
    """the program at the pair z from the opened values, cell_values[k] the pair of cells(prog.ops)[k]; None when z^N = 1"""
    z = E.el(z)
    zN = E.pow(z, dom.N)
    if zN == E.one:
        return None
    where = {o: E.el(v) for o, v in zip(cells(prog.ops), cell_values)}
    return AR.combine(E, dom, run(E, prog, where.__getitem__, lambda o: at_point(E, dom, periodic, o, z), chal, z), lam, z, zN)
