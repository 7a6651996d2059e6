"""ronkathon_amd.air.AirBuilder: the tape it assembles, run by tests/air_ref.py, equals the direct evaluation of the expression trees;
equal subexpressions are computed once; a program with seventeen live values is refused; the limits of the op word."""
import numpy as np
import pytest

import air_programs as AP
import air_ref as AR
import plonk_ref as PR
import prime_classes as PC
from ronkathon_amd import air

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_random_trees_against_direct_evaluation(p, w, seed):
    rng = np.random.default_rng(seed)
    E = PR.Ext2(p, w)
    prog, trees = AP.random_program(rng, 5, 2, 3, (0, 1, -1, 2), (0, 1, 2, 3), 1 + seed % 6, depth=3 + seed % 3)
    chal = [tuple(int(v) for v in rng.integers(0, 2**62, size=2)) for _ in range(3)]
    x = E.embed(int(rng.integers(1, 2**62)))
    values = {}

    def cell(o):
        if o not in values:
            kind = AR.decode(o)[0]
            values[o] = E.el((int(rng.integers(0, 2**62)), int(rng.integers(0, 2**62)) if kind == AR.EXT else 0))
        return values[o]

    got = AR.run(E, prog, cell, chal, x)
    assert got == [(kind, AP.evaluate_tree(E, t, cell, chal, x)) for t, kind in trees]
    assert prog.n_regs <= 16 and all((v >> 8) & 0xFF < prog.n_regs for v in prog.ops if v & 0xFF != AR.EMIT)
    assert set(AR.cells(prog.ops)) == set(values)


def test_shared_subexpressions_appear_once():
    b = air.AirBuilder()
    s = b.base(0) * b.base(1)
    t = b.base(1) * b.base(0)                 # the same product
    assert s is t and b.base(0) is b.base(0) and b.imm(5) is b.imm(5) and b.x is b.x
    b.constrain(s + b.chal(0), air.ALL)
    b.constrain(t - b.ext(0), air.FIRST)
    b.constrain((b.base(0) * b.base(1) + b.chal(0)) * s, air.LAST)
    ops, imm, n_regs, J = b.assemble()
    codes = [w & 0xFF for w in ops]
    assert codes.count(air.MUL) == 2 and codes.count(air.ADD) == 1 and codes.count(air.SUB) == 1 and codes.count(air.EMIT) == 3
    assert J == 3 and imm == [5] and n_regs == 3


def test_registers_are_reused():
    b = air.AirBuilder()
    e = b.base(0)
    for c in range(1, 40):
        e = e * b.base(c) + b.imm(c)
    b.constrain(e)
    ops, imm, n_regs, J = b.assemble()
    assert n_regs == 1 and len(ops) == 2 * 39 + 1 and len(imm) == 39


def test_seventeen_live_values_raise():
    def build(k):
        b = air.AirBuilder()
        t = [b.base(c) * b.base(c + 1) for c in range(k)]
        b.constrain(t[0], air.ALL)
        for v in t[1:]:                       # every product is computed here and is read again below
            b.constrain(v + t[0], air.ALL)
        total = t[0]
        for v in t[1:]:
            total = total * v
        b.constrain(total, air.ALL)
        return b
    ops, _, n_regs, _ = build(15).assemble()                 # fifteen products and the sum being formed
    assert n_regs == 16
    with pytest.raises(air.AirError, match="more than 16 live registers"):
        build(16).assemble()


def test_limits_of_the_op_word():
    b = air.AirBuilder()
    with pytest.raises(air.AirError):
        b.base(0, rot=2048)
    with pytest.raises(air.AirError):
        b.base(256)
    with pytest.raises(air.AirError):
        b.assemble()                          # no constraint
    with pytest.raises(air.AirError):
        b.constrain(b.x, 4)
    with pytest.raises(air.AirError):
        b.constrain(air.AirBuilder().x)       # another builder's expression
    assert AR.decode(b.base(3, rot=-2048).leaf) == (AR.BASE, 3, -2048)
    assert (air.MOV, air.ADD, air.SUB, air.MUL, air.NEG, air.EMIT) == (AR.MOV, AR.ADD, AR.SUB, AR.MUL, AR.NEG, AR.EMIT)
    assert (air.REG, air.BASE, air.EXT, air.CHAL, air.IMM, air.X) == (AR.REG, AR.BASE, AR.EXT, AR.CHAL, AR.IMM, AR.X)
