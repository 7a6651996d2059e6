"""Pure-Python restatement of the constraint programs on the evaluation coset (include/ronk_ntt.h "constraint programs") on Python
integers: the op and operand words, the interpreter, the row formula of the four kinds, the cells a program reads and its
evaluation at one out-of-domain point.  The domain is that of tests/plonk_ref.py, the extension that of tests/ext2_ref.py.  This file
is the normative restatement of those semantics.  A test helper, not product code; it shares nothing with the library."""
from collections import namedtuple

from ext2_ref import Ext2, pairs, planar  # noqa: F401  (re-exported for the tests)

MOV, ADD, SUB, MUL, NEG, EMIT = range(6)
REG, BASE, EXT, CHAL, IMM, X = range(6)
ALL, FIRST, LAST, EXCEPT_LAST = range(4)

Program = namedtuple("Program", "ops imm n_regs n_constraints")


def operand(kind, index=0, rot=0):
    assert 0 <= index < 256 and -2048 <= rot < 2048
    return kind | index << 4 | (rot & 0xFFF) << 12


def op(code, dst, a, b=0):
    return code | dst << 8 | a << 16 | b << 40


def decode(o):
    """a 24-bit operand -> (kind, index, rot)"""
    rot = (o >> 12) & 0xFFF
    return o & 0xF, (o >> 4) & 0xFF, rot - 4096 if rot >= 2048 else rot


def cells(ops):
    """the distinct BASE and EXT operands in first-use order"""
    out = []
    for w in ops:
        code = w & 0xFF
        for o in ((w >> 16) & 0xFFFFFF,) + (((w >> 40) & 0xFFFFFF,) if code in (ADD, SUB, MUL) else ()):
            if o & 0xF in (BASE, EXT) and o not in out:
                out.append(o)
    return out


def run(E, prog, cell, chal, x):
    """the tape with cell(o) the pair of a column operand, chal the challenge pairs and x the pair that X reads: -> the J
    (kind, value) of the constraints.  Every value is a pair."""
    reg = [None] * 256
    out = [None] * prog.n_constraints

    def read(o):
        kind, index, rot = decode(o)
        if kind == REG:
            assert reg[index] is not None, "a register is read before it is written"
            return reg[index]
        if kind in (BASE, EXT):
            return cell(o)
        assert rot == 0
        return E.el(chal[index]) if kind == CHAL else E.embed(prog.imm[index]) if kind == IMM else x

    for w in prog.ops:
        code, dst, a = w & 0xFF, (w >> 8) & 0xFF, read((w >> 16) & 0xFFFFFF)
        if code == EMIT:
            j = (w >> 40) & 0xFFFFFF
            assert out[j] is None and dst <= EXCEPT_LAST
            out[j] = (dst, a)
        elif code == MOV:
            reg[dst] = a
        elif code == NEG:
            reg[dst] = E.neg(a)
        else:
            b = read((w >> 40) & 0xFFFFFF)
            reg[dst] = {ADD: E.add, SUB: E.sub, MUL: E.mul}[code](a, b)
    assert all(v is not None for v in out), "a constraint is never emitted"
    return out


def combine(E, dom, constraints, lam, x, xN):
    """sum_j lambda_j C_j (divisor of its kind) at the pair x, xN = x^N"""
    p = E.p
    wl = pow(dom.wN, -1, p)
    vinv = E.inv(E.sub(xN, E.one))
    xl = E.sub(x, E.embed(wl))
    div = {ALL: vinv, FIRST: E.mul_base(E.inv(E.sub(x, E.one)), dom.n_inv),
           LAST: E.mul_base(E.inv(xl), wl * dom.n_inv % p), EXCEPT_LAST: E.mul(xl, vinv)}
    total = E.zero
    for (kind, value), l in zip(constraints, lam):
        total = E.add(total, E.mul(E.mul(E.el(l), value), div[kind]))
    return total


def quotient_row(E, dom, prog, base, ext, chal, lam, T_in, i, x=None):
    """row i: base the flat list of base columns (M words each), ext the extension columns (two planes of M words each), T_in two
    planes or None"""
    p, M = E.p, dom.M
    x = dom.x(i) if x is None else x

    def cell(o):
        kind, index, rot = decode(o)
        r = (i + rot * dom.B) % M
        return E.embed(int(base[index][r])) if kind == BASE else E.el((ext[index][0][r], ext[index][1][r]))

    xN = pow(dom.vanish_inv[i % dom.B], -1, p) + 1
    out = combine(E, dom, run(E, prog, cell, chal, E.embed(x)), lam, E.embed(x), E.embed(xN))
    return out if T_in is None else E.add(out, E.el((T_in[0][i], T_in[1][i])))


def quotient(E, dom, prog, base, ext, chal, lam, T_in=None):
    """every row -> M pairs"""
    return [quotient_row(E, dom, prog, base, ext, chal, lam, T_in, i, x) for i, x in enumerate(dom.points())]


def eval_point(E, dom, prog, z, cell_values, chal, lam):
    """the same program at the pair z from the opened values, cell_values[k] the pair of cells(prog.ops)[k]; None when z^N = 1"""
    z = E.el(z)
    zN = E.pow(z, dom.N)
    if zN == E.one:
        return None
    where = {o: E.el(v) for o, v in zip(cells(prog.ops), cell_values)}
    return combine(E, dom, run(E, prog, where.__getitem__, chal, z), lam, z, zN)


def pairs_of(words):
    """[n][2] words as the library takes challenges and weights -> n pairs"""
    return [(int(words[2 * k]), int(words[2 * k + 1])) for k in range(len(words) // 2)]
