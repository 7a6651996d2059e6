"""The STARK instances with a fixed round or periodic columns that the tests share (include/ronk_ntt.h "STARK": fixed): the
program, its round shapes, a valid trace with its public inputs, the fixed columns and the periodic values.  A test helper, not
product code."""
from collections import namedtuple

import air_programs as AP
import air_ref as AR
from ronkathon_amd.air import ALL, EXCEPT_LAST, FIRST, LAST, AirBuilder

# as stark_programs.Shape, and: n_fixed columns of the fixed round (the first flat base indices), periodic = one list of values per
# periodic column
Shape = namedtuple("Shape", "prog columns n_ext n_pub n_draw n_chal n_fixed periodic")
Instance = namedtuple("Instance", "shape pub rounds fixed")


def gate_program():
    """fixed 0-4: the selectors qL, qR, qM, qO, qC; base 5-7: the wires a, b, c.  qL a + qR b + qM a b + qO c + qC = 0 on every
    row, the next row's a is this row's c on every row but the last, and a = chal 0 on the first row"""
    b = AirBuilder()
    ql, qr, qm, qo, qc = (b.base(c) for c in range(5))
    wa, wb, wc = (b.base(5 + c) for c in range(3))
    b.constrain(ql * wa + qr * wb + qm * wa * wb + qo * wc + qc, ALL)
    b.constrain(b.base(5, rot=1) - wc, EXCEPT_LAST)
    b.constrain(wa - b.chal(0), FIRST)
    return AR.Program(*b.assemble())


def gate_selectors(p, N, variant=0):
    """a circuit of N gates, the kind of gate i from (i + variant) mod 3: c = a + b, c = a b, c = 3 a + 5.  Another variant is
    another circuit of the same shape"""
    rows = {0: (1, 1, 0, p - 1, 0), 1: (0, 0, 1, p - 1, 0), 2: (3, 0, 0, p - 1, 5)}
    sel = [rows[(i + variant) % 3] for i in range(N)]
    return [[row[c] for row in sel] for c in range(5)]


def gate(p, N, variant=0, first=2):
    """the fixed round is the five selector columns, the one trace round the three wires; T has degree below 2 N"""
    sel = gate_selectors(p, N, variant)
    a, bs, cs = [first % p], [], []
    for i in range(N):
        bs.append((7 * i * i + 3) % p)
        ql, qr, qm, _, qc = (sel[c][i] for c in range(5))
        cs.append((ql * a[i] + qr * bs[i] + qm * a[i] * bs[i] + qc) % p)
        a.append(cs[i])
    return Instance(Shape(gate_program(), (3,), (0,), 1, (0,), 1, 5, ()), [(a[0], 0)], [[a[:N], bs, cs]], sel)


def sbox_periodic_program():
    """the S-box row of air_programs.sbox_row with its round constants as the periodic columns 0-2, read at rot 0; and periodic
    column 1 is column 0 one row on, which the last constraint states at rot 1"""
    b = AirBuilder()
    s7 = []
    for c in range(3):
        t = b.base(c) + b.periodic(c)
        t2 = t * t
        s7.append(t2 * t2 * t2 * t)
    for r in range(3):
        b.constrain(b.base(r, rot=1) - (AP.MDS3[r][0] * s7[0] + AP.MDS3[r][1] * s7[1] + AP.MDS3[r][2] * s7[2]), EXCEPT_LAST)
    b.constrain(b.base(0) - b.chal(0), FIRST)
    b.constrain(b.base(0) - b.chal(1), LAST)
    b.constrain(b.periodic(0, rot=1) - b.periodic(1), ALL)
    return AR.Program(*b.assemble())


def round_constants(p, period=8):
    """three columns of `period` values; column 1 is column 0 rotated by one row"""
    rc0 = [(5 + 11 * k * k + k) % p for k in range(period)]
    return [rc0, rc0[1:] + rc0[:1], [(7 + 13 * k) % p for k in range(period)]]


def sbox_periodic_trace(p, N, periodic, state=(1, 2, 3)):
    rows = [[int(v) % p for v in state]]
    for i in range(N - 1):
        s7 = [pow((v + rc[i % len(rc)]) % p, 7, p) for v, rc in zip(rows[-1], periodic)]
        rows.append([sum(m * s for m, s in zip(AP.MDS3[r], s7)) % p for r in range(3)])
    return [[row[c] for row in rows] for c in range(3)]


def sbox_periodic(p, N):
    """one round of three base columns, no fixed round, three periodic columns of period 8; degree-7 transitions, so B = 8"""
    periodic = round_constants(p)
    trace = sbox_periodic_trace(p, N, periodic)
    return Instance(Shape(sbox_periodic_program(), (3,), (0,), 2, (0,), 2, 0, periodic), [(trace[0][0], 0), (trace[0][-1], 0)], [trace], None)
