"""Argument errors of the constraint programs (ronk_air_check, ronk_air_create, ronk_air_quotient*, ronk_air_cells,
ronk_air_eval_point, ronk_air_destroy): all of them are settled by host-side integer logic before any device work, so this runs
without a GPU.  A handle lives on a ronk_plonk domain, which needs a device: where there is none, creation says so, and the values
of ronk_air_eval_point are held to tests/air_ref.py by tests/test_gpu_air.py; where there is one, here as well."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import air_programs as AP
import air_ref as AR
import plonk_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL = 0xFFFFFFFF00000001
NAMES = ("ronk_air_check", "ronk_air_create", "ronk_air_destroy", "ronk_air_quotient_dev", "ronk_air_quotient", "ronk_air_cells",
         "ronk_air_eval_point")
O, OP = AR.operand, AR.op


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def check(L, ops, log2_n=4, columns=(3, 2), n_ext=2, n_chal=2, n_imm=2, n_regs=4, J=1, n_ops=None, null_ops=False, null_columns=False):
    a = (C.c_uint64 * max(1, len(ops)))(*ops)
    c = (C.c_uint32 * max(1, len(columns)))(*columns)
    return L.lib.ronk_air_check(log2_n, len(columns), None if null_columns else c, n_ext, n_chal, n_imm, n_regs, J,
                                None if null_ops else a, len(ops) if n_ops is None else n_ops)


def test_exported_and_declared(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ronk_ntt.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ronk_[a-z0-9_]+)\s*\(", hdr)) if n.startswith("ronk_air_"))
    assert declared == sorted(NAMES)
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_check_codes_in_their_order(L):
    ok = [OP(AR.EMIT, AR.ALL, O(AR.BASE, 0))]
    assert check(L, ok) == L.OK
    # 1. RONK_ERR_INVALID: NULL pointers and zero counts, whatever else is wrong
    assert check(L, ok, null_ops=True) == L.ERR_INVALID and check(L, ok, null_ops=True, n_regs=99) == L.ERR_INVALID
    assert check(L, ok, null_columns=True) == L.ERR_INVALID and check(L, ok, null_columns=True, n_ext=99) == L.ERR_INVALID
    assert check(L, ok, n_ops=0, n_chal=99) == L.ERR_INVALID and check(L, ok, J=0, n_imm=999) == L.ERR_INVALID
    assert check(L, ok, columns=(3, 0)) == L.ERR_INVALID
    assert check(L, [OP(AR.EMIT, AR.ALL, O(AR.EXT, 0))], columns=()) == L.OK                  # no base group at all
    # 2. RONK_ERR_UNSUPPORTED: the limits, before anything of the program is read
    bad = [OP(9, 0, 0)]
    for kw in (dict(columns=(1,) * 9), dict(columns=(65,)), dict(columns=(33, 32)), dict(n_ext=9), dict(n_chal=33), dict(n_imm=257),
               dict(n_regs=17), dict(J=65), dict(log2_n=0), dict(log2_n=29)):
        assert check(L, bad, **kw) == L.ERR_UNSUPPORTED, kw
    assert check(L, bad * 4097) == L.ERR_UNSUPPORTED
    # ... and at the limits the program is read
    assert check(L, ok, columns=(8,) * 8, n_ext=8, n_chal=32, n_imm=256, n_regs=16, log2_n=28) == L.OK
    assert check(L, ok, columns=(64,), log2_n=1) == L.OK and check(L, bad, columns=(64,), n_regs=16) == L.ERR_INVALID
    # 3. RONK_ERR_INVALID: the program, op by op
    emit = OP(AR.EMIT, AR.ALL, O(AR.REG, 0))
    mov = OP(AR.MOV, 0, O(AR.X))
    assert check(L, [mov, emit]) == L.OK
    assert check(L, [OP(6, 0, O(AR.X)), emit]) == L.ERR_INVALID                                 # an unknown opcode
    assert check(L, [OP(AR.MOV, 0, O(6)), emit]) == L.ERR_INVALID                               # an unknown operand kind
    for o in (O(AR.REG, 4), O(AR.BASE, 5), O(AR.EXT, 2), O(AR.CHAL, 2), O(AR.IMM, 2), O(AR.X, 1)):
        assert check(L, [OP(AR.MOV, 0, o), emit]) == L.ERR_INVALID, AR.decode(o)                # an index out of range
        assert check(L, [OP(AR.ADD, 0, O(AR.X), o), emit]) == L.ERR_INVALID, AR.decode(o)
    for o in (O(AR.BASE, 4), O(AR.EXT, 1), O(AR.CHAL, 1), O(AR.IMM, 1), O(AR.X)):
        assert check(L, [OP(AR.MOV, 0, o), emit]) == L.OK, AR.decode(o)
    assert check(L, [OP(AR.MOV, 4, O(AR.X)), emit]) == L.ERR_INVALID                            # dst >= n_regs
    assert check(L, [OP(AR.EMIT, 4, O(AR.X))]) == L.ERR_INVALID                                 # an EMIT kind above 3
    for kind in (AR.REG, AR.CHAL, AR.IMM, AR.X):                                                # rot on what is no column
        assert check(L, [mov, OP(AR.MOV, 1, O(kind, 0, 1)), emit]) == L.ERR_INVALID, kind
    for rot, code in ((15, L.OK), (-15, L.OK), (16, L.ERR_INVALID), (-16, L.ERR_INVALID), (-2048, L.ERR_INVALID)):   # |rot| < N = 16
        assert check(L, [OP(AR.MOV, 0, O(AR.BASE, 1, rot)), emit]) == code, rot
        assert check(L, [OP(AR.MUL, 0, O(AR.X), O(AR.EXT, 1, rot)), emit]) == code, rot
    assert check(L, [OP(AR.MOV, 0, O(AR.BASE, 1, 2047)), emit], log2_n=11) == L.OK
    assert check(L, [OP(AR.MOV, 0, O(AR.BASE, 1, 1)), emit], log2_n=1) == L.OK and check(L, [OP(AR.MOV, 0, O(AR.BASE, 1, 2)), emit], log2_n=1) == L.ERR_INVALID
    assert check(L, [OP(AR.MOV, 0, O(AR.X), O(AR.X)), emit]) == L.ERR_INVALID                   # b on MOV / NEG
    assert check(L, [OP(AR.NEG, 0, O(AR.X), 1), emit]) == L.ERR_INVALID
    assert check(L, [emit]) == L.ERR_INVALID                                                    # read before written
    assert check(L, [OP(AR.ADD, 1, O(AR.X), O(AR.REG, 1)), emit]) == L.ERR_INVALID
    assert check(L, [mov, OP(AR.ADD, 1, O(AR.REG, 0), O(AR.REG, 1)), emit]) == L.ERR_INVALID
    assert check(L, [mov, OP(AR.ADD, 0, O(AR.REG, 0), O(AR.REG, 0)), emit]) == L.OK             # dst may be an operand
    assert check(L, [mov, OP(AR.EMIT, AR.ALL, O(AR.REG, 0), 1)]) == L.ERR_INVALID               # j >= J
    assert check(L, [mov, emit, emit]) == L.ERR_INVALID and check(L, [mov, emit, emit], J=2) == L.ERR_INVALID   # j twice
    assert check(L, [mov, emit], J=2) == L.ERR_INVALID and check(L, [mov]) == L.ERR_INVALID     # j never
    assert check(L, [mov, OP(AR.EMIT, AR.LAST, O(AR.REG, 0), 1), emit], J=2) == L.OK
    # the first offending op decides, and nothing after it is read as more than words
    assert check(L, [mov, emit] + [2**64 - 1] * 5) == L.ERR_INVALID


def test_the_shared_programs_pass_the_check(L):
    for prog, columns, n_ext, n_chal in ((AP.plonk(), (3, 5, 3, 1), 1, 2), (AP.logup(5, True), (5, 5), 1, 1), (AP.fibonacci(), (3,), 0, 2),
                                         (AP.sbox_row(), (3,), 0, 2)):
        assert check(L, prog.ops, 4, columns, n_ext, n_chal, len(prog.imm), prog.n_regs, prog.n_constraints) == L.OK
        assert check(L, prog.ops, 4, columns, n_ext, n_chal, len(prog.imm), prog.n_regs - 1, prog.n_constraints) == L.ERR_INVALID


def test_null_pointers(L):
    d, h = C.c_void_p(16), C.c_void_p(32)   # never dereferenced: refused first
    assert L.lib.ronk_air_destroy(None) == L.ERR_INVALID
    ops = (C.c_uint64 * 1)(OP(AR.EMIT, AR.ALL, O(AR.BASE, 0)))
    cols = (C.c_uint32 * 1)(1)
    assert L.lib.ronk_air_create(None, h, 1, cols, 0, 0, 0, 1, 1, ops, 1, None) == L.ERR_INVALID
    out = C.c_void_p(99)
    assert L.lib.ronk_air_create(C.byref(out), None, 1, cols, 0, 0, 0, 1, 1, ops, 1, None) == L.ERR_INVALID and not out.value
    assert L.lib.ronk_air_quotient_dev(None, d, d, d, d, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_air_quotient(None, d, d, d, d, d, d) == L.ERR_INVALID
    assert L.lib.ronk_air_eval_point(None, d, d, d, d, d) == L.ERR_INVALID
    assert L.lib.ronk_air_cells(None, None, 0) == 0


def test_handle_cells_and_eval_point(L):
    """with a device: the codes of creation, the cells and ronk_air_eval_point against air_ref, z on H included; without one:
    RONK_ERR_NO_DEVICE after the argument checks"""
    p, g, w = GL, 7, 7
    dom = C.c_void_p()
    rc = L.lib.ronk_plonk_create(C.byref(dom), p, g, w, 4, 2, g, (C.c_uint64 * 3)(1, 2, 3))
    if L.device_count() == 0:
        assert rc == L.ERR_NO_DEVICE
        return
    assert rc == L.OK
    prog = AP.fibonacci()
    ops, imm, cols = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(3)
    h = C.c_void_p(99)
    assert L.lib.ronk_air_create(C.byref(h), dom, 1, cols, 0, 1, 0, prog.n_regs, 5, ops, len(prog.ops), imm) == L.ERR_INVALID and not h.value
    assert L.lib.ronk_air_create(C.byref(h), dom, 1, cols, 0, 2, 0, 17, 5, ops, len(prog.ops), imm) == L.ERR_UNSUPPORTED and not h.value
    assert L.lib.ronk_air_create(C.byref(h), dom, 1, cols, 0, 2, 1, prog.n_regs, 5, ops, len(prog.ops), None) == L.ERR_INVALID
    assert L.lib.ronk_air_create(C.byref(h), dom, 1, cols, 0, 2, 0, prog.n_regs, 5, ops, len(prog.ops), None) == L.OK and h.value
    want_cells = AR.cells(prog.ops)
    assert L.lib.ronk_air_cells(h, None, 0) == len(want_cells)
    got = (C.c_uint32 * 8)()
    assert L.lib.ronk_air_cells(h, got, 2) == len(want_cells) and list(got)[:3] == want_cells[:2] + [0]
    assert L.lib.ronk_air_cells(h, got, 8) == len(want_cells) and list(got)[:len(want_cells)] == want_cells
    rng = np.random.default_rng(3)
    E, D = PR.Ext2(p, w), PR.Domain(p, g, 4, 2, g)
    u64 = lambda n: rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)      # noqa: E731
    values, chal, lam = u64(2 * len(want_cells)), u64(4), u64(10)
    pairs = lambda a: [tuple(int(v) for v in a[2 * k:2 * k + 2]) for k in range(len(a) // 2)]           # noqa: E731
    out = (C.c_uint64 * 2)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                                        # noqa: E731
    for z in ([5, 9], [2**64 - 1, 2**64 - 2], [3, 0], [1, 0], [D.wN, 0], [pow(D.wN, -1, p), 0], [p - 1, 0]):
        za = (C.c_uint64 * 2)(*z)
        want = AR.eval_point(E, D, prog, z, pairs(values), pairs(chal), pairs(lam))
        rc = L.lib.ronk_air_eval_point(h, za, ptr(values), ptr(chal), ptr(lam), out)
        assert (rc, None if rc else (out[0], out[1])) == ((L.ERR_INVALID, None) if want is None else (L.OK, want)), z
    assert L.lib.ronk_air_eval_point(h, None, ptr(values), ptr(chal), ptr(lam), out) == L.ERR_INVALID
    assert L.lib.ronk_air_destroy(h) == L.OK and L.lib.ronk_plonk_destroy(dom) == L.OK
