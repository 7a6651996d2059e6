"""The constraint programs the AIR tests share, written with ronkathon_amd.air.AirBuilder: the PLONK quotient and the logUp pair as
programs (what ronk_plonk_quotient_dev and ronk_logup_quotient_dev hard-wire), a Fibonacci AIR with all four kinds, a width-3 x^7
S-box row, and seeded random programs.  A test helper, not product code."""
import air_ref as AR
from ronkathon_amd.air import ALL, EXCEPT_LAST, FIRST, LAST, AirBuilder


def program(b):
    return AR.Program(*b.assemble())


def plonk():
    """base: wires 0-2, selectors 3-7 (ql, qr, qm, qo, qc), sigma 8-10, pi 11; ext 0: Z; chal 0, 1: beta, gamma; the identity labels
    from X and the immediates 1, 2, 3.  Constraints: the gate (ALL), P1 (ALL), Z - 1 (FIRST); lambda = 1, alpha, alpha^2."""
    b = AirBuilder()
    w = [b.base(c) for c in range(3)]
    ql, qr, qm, qo, qc = (b.base(3 + c) for c in range(5))
    sigma = [b.base(8 + c) for c in range(3)]
    beta, gamma = b.chal(0), b.chal(1)
    b.constrain(w[0] * ql + w[1] * qr + w[0] * w[1] * qm + w[2] * qo + qc + b.base(11), ALL)
    num, den = b.ext(0), b.ext(0, rot=1)
    for c in range(3):
        num = num * (w[c] + beta * (b.imm(c + 1) * b.x) + gamma)
        den = den * (w[c] + beta * sigma[c] + gamma)
    b.constrain(num - den, ALL)
    b.constrain(b.ext(0) - 1, FIRST)
    return program(b)


def logup(C, with_mult):
    """base: the C value columns, then the C multiplicity columns when with_mult; ext 0: S; chal 0: alpha.  Constraints: R (ALL) and
    S (FIRST); lambda = lambda0, lambda1."""
    b = AirBuilder()
    P, Q = None, None
    for c in range(C):
        D = b.chal(0) + b.base(c)
        m = b.base(C + c) if with_mult else b.imm(1)
        Q = m if P is None else Q * D + m * P
        P = D if P is None else P * D
    b.constrain((b.ext(0, rot=1) - b.ext(0)) * P - Q, ALL)
    b.constrain(b.ext(0), FIRST)
    return program(b)


def fibonacci():
    """base 0, 1, 2: a, b, c with a' = b, b' = a + b on every row but the last, c = a b on every row, a = chal 0 on the first row and
    b = chal 1 on the last.  Five constraints; T has degree N - 2."""
    b = AirBuilder()
    a, bb, c = b.base(0), b.base(1), b.base(2)
    b.constrain(c - a * bb, ALL)
    b.constrain(b.base(0, rot=1) - bb, EXCEPT_LAST)
    b.constrain(b.base(1, rot=1) - a - bb, EXCEPT_LAST)
    b.constrain(a - b.chal(0), FIRST)
    b.constrain(bb - b.chal(1), LAST)
    return program(b)


def fibonacci_trace(p, N, a0=1, b0=1):
    a, b = [a0 % p], [b0 % p]
    for _ in range(N - 1):
        a, b = a + [b[-1]], b + [(a[-1] + b[-1]) % p]
    return [a, b, [u * v % p for u, v in zip(a, b)]]


MDS3 = ((2, 1, 1), (1, 2, 1), (1, 1, 2))


def sbox_row(round_constants=(5, 6, 7)):
    """base 0-2: the state.  next_r = sum_c MDS[r][c] (state_c + rc_c)^7 on every row but the last, state_0 = chal 0 on the first row,
    state_0 = chal 1 on the last"""
    b = AirBuilder()
    s7 = []
    for c in range(3):
        t = b.base(c) + b.imm(round_constants[c])
        t2 = t * t
        s7.append(t2 * t2 * t2 * t)
    for r in range(3):
        b.constrain(b.base(r, rot=1) - (MDS3[r][0] * s7[0] + MDS3[r][1] * s7[1] + MDS3[r][2] * s7[2]), EXCEPT_LAST)
    b.constrain(b.base(0) - b.chal(0), FIRST)
    b.constrain(b.base(0) - b.chal(1), LAST)
    return program(b)


def random_program(rng, n_base, n_ext, n_chal, rots, kinds, n_constraints, depth=4, n_regs_min=0):
    """a seeded random program over the given leaves; -> (Program, trees): trees[j] = (nested tuple, kind) for direct evaluation.
    A tree is ("leaf", operand word), ("imm", v), ("x",) or (op, left[, right]) with op in "+-*n"."""
    b = AirBuilder()
    pool = []

    def leaf():
        k = int(rng.integers(0, 6))
        if k == 0 and n_base:
            c, r = int(rng.integers(0, n_base)), int(rots[int(rng.integers(0, len(rots)))])
            return b.base(c, r), ("leaf", AR.operand(AR.BASE, c, r))
        if k == 1 and n_ext:
            c, r = int(rng.integers(0, n_ext)), int(rots[int(rng.integers(0, len(rots)))])
            return b.ext(c, r), ("leaf", AR.operand(AR.EXT, c, r))
        if k == 2 and n_chal:
            c = int(rng.integers(0, n_chal))
            return b.chal(c), ("chal", c)
        if k == 3:
            v = int(rng.integers(0, 2**63))
            return b.imm(v), ("imm", v)
        if k == 4 and pool:
            return pool[int(rng.integers(0, len(pool)))]
        return b.x, ("x",)

    def tree(d):
        if d == 0 or (d <= depth - 2 and int(rng.integers(0, 5)) == 0):      # the two levels below a root are always operations
            return leaf()
        o = "+-*n"[int(rng.integers(0, 4))]
        le, lt = tree(d - 1)
        if o == "n":
            out = (-le, ("n", lt))
        else:
            re, rt = tree(d - 1)
            out = ({"+": le + re, "-": le - re, "*": le * re}[o], (o, lt, rt))
        if int(rng.integers(0, 3)) == 0:
            pool.append(out)
        return out

    trees = []
    for j in range(n_constraints):
        e, t = tree(depth)
        kind = int(kinds[j % len(kinds)])
        b.constrain(e, kind)
        trees.append((t, kind))
    ops, imm, n_regs, J = b.assemble()
    return AR.Program(ops, imm, max(n_regs, n_regs_min), J), trees


def evaluate_tree(E, t, cell, chal, x):
    """a tree of random_program directly on pairs"""
    if t[0] == "leaf":
        return cell(t[1])
    if t[0] == "chal":
        return E.el(chal[t[1]])
    if t[0] == "imm":
        return E.embed(t[1])
    if t[0] == "x":
        return x
    a = evaluate_tree(E, t[1], cell, chal, x)
    if t[0] == "n":
        return E.neg(a)
    b = evaluate_tree(E, t[2], cell, chal, x)
    return {"+": E.add, "-": E.sub, "*": E.mul}[t[0]](a, b)


def long_program(n_ops, n_constraints, n_base, n_ext, n_chal, n_imm, rots, n_regs=16):
    """a deterministic tape of exactly n_ops ops written word by word: every register is written before the chain reads it, the
    operands cycle through every leaf kind and rotation, so registers hold base values at one op and extension values at another;
    the last n_constraints ops emit the registers with the kinds in turn"""
    O, OP = AR.operand, AR.op
    leaves = [O(AR.X)]
    for k in range(max(n_base, n_ext, n_chal, n_imm)):
        r = rots[k % len(rots)]
        leaves += ([O(AR.BASE, k, r)] if k < n_base else []) + ([O(AR.EXT, k, -r if abs(r) < 2048 else r)] if k < n_ext else [])
        leaves += ([O(AR.CHAL, k)] if k < n_chal else []) + ([O(AR.IMM, k)] if k < n_imm else [])
    ops = []
    for k in range(n_ops - n_constraints):
        dst, leaf = k % n_regs, leaves[k % len(leaves)]
        if k < n_regs:
            ops.append(OP(AR.MOV if k % 2 else AR.NEG, dst, leaf))
        else:
            prev = O(AR.REG, (k - 1) % n_regs)
            code = (AR.MUL, AR.ADD, AR.SUB, AR.MUL, AR.MOV, AR.ADD, AR.NEG)[k % 7]
            if code in (AR.MOV, AR.NEG):
                ops.append(OP(code, dst, prev if k % 3 else leaf))
            else:
                ops.append(OP(code, dst, *((prev, leaf) if k % 2 else (leaf, prev))))
    written = min(n_regs, n_ops - n_constraints)
    for j in range(n_constraints):
        ops.append(OP(AR.EMIT, j % 4, O(AR.REG, j % written) if written else leaves[j % len(leaves)], j))
    return AR.Program(ops, [3 + 5 * k for k in range(n_imm)], n_regs, n_constraints)
