"""Periodic columns of a constraint program on the device (ronk_air_create_per, then ronk_air_quotient_dev) bit for bit against the
Python restatement tests/air_per_ref.py: Goldilocks with W = 7, MONT_P and P_MID; M = 4, 8 (one row per lane), 2^6 and 2^12 (more
than one workgroup); periods 1, 2 and N, so that a table is shorter than M or all of it; rotations 0, 1 and -1, whose rot B
crosses a table's end in both directions; values at and above p; T_in absent, present and in place; pre-filled outputs and
unchanged inputs.  The kernel's table reads are pointwise, so the columns are random words."""
import ctypes as C

import numpy as np
import pytest

import air_per_ref as APR
import air_ref as AR
import prime_classes as PC
import stark_fixed_programs as FP
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from ronkathon_amd.air import ALL, EXCEPT_LAST, FIRST, LAST, AirBuilder
from test_gpu_air import GEN, Air, Data, garbage
from test_gpu_fri import _Field, host, words

pytestmark = pytest.mark.gpu

GL, MONT, MID = 0xFFFFFFFF00000001, PC.MONT_P, PC.P_MID
FIELDS = [(GL, 7), (MONT, 10), (MID, PC.GEN[MID])]
# (log2_n, log2_b): M = 4, 8, 2^6, 2^12
SHAPES = [(1, 1), (2, 1), (4, 2), (10, 2)]
_WANT = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class AirPer(Air):
    """test_gpu_air.Air through ronk_air_create_per"""

    def __init__(self, p, w, log2_n, log2_b, prog, groups, n_ext, n_chal, periodic):
        import plonk_ref as PR
        self.p, self.M, self.prog, self.groups, self.n_ext = p, 1 << (log2_n + log2_b), prog, groups, n_ext
        self.E, self.dom, self.periodic = PR.Ext2(p, w), PR.Domain(p, GEN[p], log2_n, log2_b, GEN[p]), periodic
        self.d, self.h = C.c_void_p(), C.c_void_p()
        L.check(L.lib.ronk_plonk_create(C.byref(self.d), p, GEN[p], w, log2_n, log2_b, GEN[p], (C.c_uint64 * 3)(1, 2, 3)))
        ops, imm = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * max(1, len(prog.imm)))(*[v % p for v in prog.imm])
        n_per, log2_period, values = callers.periodic_arrays(periodic)
        L.check(L.lib.ronk_air_create_per(C.byref(self.h), self.d, len(groups), (C.c_uint32 * max(1, len(groups)))(*groups), n_ext, n_chal,
                                          len(prog.imm), prog.n_regs, prog.n_constraints, ops, len(prog.ops), imm, n_per, log2_period,
                                          L.ptr(values)))


def program(n_per):
    """two base columns, one extension column, one challenge; every periodic column at rot 0, 1 and -1, multiplied and added into a
    base chain and an extension chain, under the four kinds"""
    b = AirBuilder()
    acc, mixed = b.base(0), b.ext(0, rot=1)
    for k in range(n_per):
        for r in (0, 1, -1):
            acc = acc * b.periodic(k, r) + b.base(1, rot=r)
            mixed = mixed * b.periodic(k, -r) - b.periodic((k + 1) % n_per, r)
    b.constrain(acc, ALL)
    b.constrain(mixed + b.chal(0), EXCEPT_LAST)
    b.constrain(b.periodic(0) * b.x - b.base(0), FIRST)
    b.constrain(b.periodic(n_per - 1, 1), LAST)
    return AR.Program(*b.assemble())


def case(torch, p, w, shape):
    """the handle, its data and the restatement's T without T_in, once per (field, shape): the three T_in forms share them"""
    log2_n, log2_b = shape
    N = 1 << log2_n
    periods = sorted({1, 2, N})
    periodic = [[int(v) for v in words(900 + P + log2_n, P, p)] for P in periods]      # 0, p - 1 and words >= p among them
    air = AirPer(p, w, log2_n, log2_b, program(len(periods)), (2,), 1, 1, periodic)
    data = Data(torch, air, 1, 50 + log2_n)
    key = (p, w, shape)
    if key not in _WANT:
        _WANT[key] = APR.quotient(air.E, air.dom, air.prog, data.columns, data.planes, AR.pairs_of(data.chal), AR.pairs_of(data.lam), periodic)
    return air, data, _WANT[key]


@pytest.mark.parametrize("mode", ["no T_in", "T_in", "in place"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p,w", FIELDS)
def test_every_row_against_the_restatement(torch, p, w, shape, mode):
    air, data, T = case(torch, p, w, shape)
    E, M = air.E, air.M
    d_T = garbage(torch, 2 * M)
    if mode == "in place":
        d_T.copy_(data.d_T_in)
    air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, {"no T_in": None, "T_in": data.d_T_in, "in place": d_T}[mode], d_T)
    T_in = data.T_in.reshape(2, M).tolist()
    want = T if mode == "no T_in" else [E.add(v, E.el((T_in[0][i], T_in[1][i]))) for i, v in enumerate(T)]
    assert np.array_equal(host(torch, d_T), np.array(AR.planar(want), dtype=np.uint64)), (p, w, shape, mode)
    assert data.unchanged(torch) and np.array_equal(host(torch, data.d_T_in), data.T_in)
    air.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_sbox_periodic_and_the_host_form(torch, p, w):
    """the shared instance's program at N = 2^6, B = 8 (P = 8 < N: P B < M) through callers.air_quotient, and the old S-box row
    through the same caller with no periodic column against tests/air_ref.py"""
    log2_n, log2_b = 6, 3
    M = 1 << (log2_n + log2_b)
    inst = FP.sbox_periodic(p, 1 << log2_n)
    prog, g = inst.shape.prog, GEN[p]
    import plonk_ref as PR
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, log2_n, log2_b, g)
    base = words(7, 3 * M, p).reshape(3, M)
    chal, lam = [(3, 4), (5, 6)], [(11 + j, 13 * j) for j in range(prog.n_constraints)]
    got = callers.air_quotient(_Field(p), g, w, log2_n, log2_b, g, tuple(prog), [base], [], chal, lam, periodic=inst.shape.periodic)
    want = APR.quotient(E, dom, prog, base.tolist(), [], chal, lam, inst.shape.periodic)
    assert got.tolist() == AR.planar(want)
    import air_programs as AP
    old = AP.sbox_row()
    a = callers.air_quotient(_Field(p), g, w, log2_n, log2_b, g, tuple(old), [base], [], chal, lam[:5], periodic=())
    assert a.tolist() == AR.planar(AR.quotient(E, dom, old, base.tolist(), [], chal, lam[:5]))
