"""Argument errors of the periodic columns of a constraint program (ronk_air_check_per, ronk_air_create_per): host-side integer
logic before any device work, so this runs without a GPU.  The codes in their order and at their bounds, NULL pointers, the
prototypes of include/ronk_ntt_fixed.h against the library's exports, and ronk_air_check against ronk_air_check_per with no
periodic column on the shapes tests/test_cabi_air_cpu.py checks.  With a device: creation and ronk_air_eval_point against
tests/air_per_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import air_per_ref as APR
import air_programs as AP
import air_ref as AR
import plonk_ref as PR
import stark_fixed_programs as FP
import test_cabi_air_cpu as OLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL = 0xFFFFFFFF00000001
NAMES = ("ronk_air_check_per", "ronk_air_create_per")
O, OP = AR.operand, AR.op
PER = APR.PER


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def check(L, ops, periods=(), log2_n=4, columns=(3, 2), n_ext=2, n_chal=2, n_imm=2, n_regs=4, J=1, n_ops=None, null_ops=False,
          null_periods=False, n_per=None):
    a = (C.c_uint64 * max(1, len(ops)))(*ops)
    c = (C.c_uint32 * max(1, len(columns)))(*columns)
    lp = (C.c_uint32 * max(1, len(periods)))(*periods)
    return L.lib.ronk_air_check_per(log2_n, len(columns), c, n_ext, n_chal, n_imm, n_regs, J, None if null_ops else a,
                                    len(ops) if n_ops is None else n_ops, len(periods) if n_per is None else n_per,
                                    None if null_periods else lp)


def declared(prefix):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ronk_ntt_fixed.h")).read(), flags=re.S)
    return hdr, sorted(n for n in set(re.findall(r"\b(ronk_[a-z0-9_]+)\s*\(", hdr)) if n.startswith(prefix))


def test_exported_and_declared(L):
    hdr, names = declared("ronk_air_")
    assert names == sorted(NAMES)
    lib = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert name in L.EXPORTS_FIXED and hasattr(lib, name)
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(L._SIG_FIXED[name][1]) == len([a for a in params.split(",") if a.strip()]), name
    # the header of the family includes the new one, and every name the new one declares is in the ctypes table
    assert '#include "ronk_ntt_fixed.h"' in open(os.path.join(ROOT, "include", "ronk_ntt.h")).read()
    assert sorted(set(re.findall(r"\b(ronk_[a-z0-9_]+)\s*\(", hdr))) == L.EXPORTS_FIXED
    # the new forms take the arguments of the old ones and then their own
    assert L._SIG_FIXED["ronk_air_check_per"][1][:10] == L._SIG["ronk_air_check"][1]
    assert L._SIG_FIXED["ronk_air_create_per"][1][:12] == L._SIG["ronk_air_create"][1]


def test_the_new_codes_in_their_order(L):
    emit = OP(AR.EMIT, AR.ALL, O(AR.REG, 0))
    ok = [OP(AR.MOV, 0, O(PER, 1, -15)), emit]
    assert check(L, ok, (4, 0)) == L.OK
    # step 1 of the old order still comes first
    assert check(L, ok, (9,) * 17, null_ops=True) == L.ERR_INVALID and check(L, ok, (9,) * 17, J=0) == L.ERR_INVALID
    # step 2, the old limits, before the new ones
    assert check(L, ok, (4, 0), n_regs=17, null_periods=True) == L.ERR_UNSUPPORTED
    # 2a. more than sixteen periodic columns, whatever the array
    assert check(L, ok, (0,) * 17) == L.ERR_UNSUPPORTED and check(L, ok, (9,) * 17) == L.ERR_UNSUPPORTED
    assert check(L, ok, null_periods=True, n_per=17) == L.ERR_UNSUPPORTED
    assert check(L, ok, (4,) * 16) == L.OK                                                          # sixteen are read
    # 2b. a period above N
    assert check(L, ok, (4, 5)) == L.ERR_UNSUPPORTED and check(L, ok, (5, 0)) == L.ERR_UNSUPPORTED
    assert check(L, ok, (0, 1), log2_n=1) == L.ERR_INVALID                                          # the period fits; rot -15 does not
    assert check(L, [OP(AR.MOV, 0, O(PER, 1, 1)), emit], (0, 1), log2_n=1) == L.OK
    assert check(L, [OP(AR.MOV, 0, O(PER, 1, 1)), emit], (0, 2), log2_n=1) == L.ERR_UNSUPPORTED
    assert check(L, [OP(AR.MOV, 0, O(PER, 0)), emit], (28,), log2_n=28) == L.OK
    # 2c. no array
    assert check(L, ok, null_periods=True, n_per=2) == L.ERR_INVALID and check(L, ok, null_periods=True, n_per=16) == L.ERR_INVALID
    # ... before the program is read
    assert check(L, [OP(9, 0, 0)], (5,)) == L.ERR_UNSUPPORTED and check(L, [OP(9, 0, 0)], null_periods=True, n_per=1) == L.ERR_INVALID
    # 3. a periodic index at and past n_per, as either operand
    for o, code in ((O(PER, 1), L.OK), (O(PER, 2), L.ERR_INVALID), (O(PER, 255), L.ERR_INVALID)):
        assert check(L, [OP(AR.MOV, 0, o), emit], (4, 0)) == code
        assert check(L, [OP(AR.MUL, 0, O(AR.X), o), emit], (4, 0)) == code
    assert check(L, [OP(AR.MOV, 0, O(PER, 0)), emit]) == L.ERR_INVALID                              # no periodic column at all
    assert check(L, [OP(AR.MOV, 0, O(PER, 0)), emit], null_periods=True) == L.ERR_INVALID
    assert check(L, [OP(AR.MOV, 0, O(7)), emit], (4,)) == L.ERR_INVALID                             # kind 7 is still unknown
    # rot on a periodic operand: |rot| < N = 16
    for rot, code in ((15, L.OK), (-15, L.OK), (16, L.ERR_INVALID), (-16, L.ERR_INVALID), (-2048, L.ERR_INVALID)):
        assert check(L, [OP(AR.MOV, 0, O(PER, 0, rot)), emit], (0,)) == code, rot
    # a periodic operand is a base value: a program of periodic columns alone, emitted directly
    assert check(L, [OP(AR.EMIT, AR.LAST, O(PER, 0, 3))], (2,), columns=(), n_ext=0, n_chal=0, n_imm=0, n_regs=0) == L.OK


def test_the_old_check_is_the_new_one_without_periodic_columns(L):
    """the shapes and programs of tests/test_cabi_air_cpu.py, code by code"""
    emit, mov = OP(AR.EMIT, AR.ALL, O(AR.REG, 0)), OP(AR.MOV, 0, O(AR.X))
    cases = [([OP(AR.EMIT, AR.ALL, O(AR.BASE, 0))], {}), ([mov, emit], {}), ([emit], {}), ([OP(9, 0, 0)], dict(n_regs=17)),
             ([OP(9, 0, 0)], dict(columns=(65,))), ([mov, emit], dict(J=2)), ([OP(AR.MOV, 0, O(6)), emit], {}),
             ([OP(AR.MOV, 0, O(AR.BASE, 1, 16)), emit], {}), ([OP(AR.MOV, 0, O(AR.BASE, 1, -15)), emit], {}), ([mov, emit], dict(log2_n=29)),
             ([mov, emit], dict(n_ops=0)), ([mov, emit], dict(null_ops=True))]
    for prog, columns, n_ext, n_chal in ((AP.plonk(), (3, 5, 3, 1), 1, 2), (AP.logup(5, True), (5, 5), 1, 1), (AP.fibonacci(), (3,), 0, 2),
                                         (AP.sbox_row(), (3,), 0, 2)):
        for regs in (prog.n_regs, prog.n_regs - 1):
            cases.append((prog.ops, dict(columns=columns, n_ext=n_ext, n_chal=n_chal, n_imm=len(prog.imm), n_regs=regs, J=prog.n_constraints)))
    seen = set()
    for ops, kw in cases:
        want = OLD.check(L, ops, **kw)
        assert check(L, ops, **kw) == want and check(L, ops, null_periods=True, **kw) == want, kw
        seen.add(want)
    assert seen == {L.OK, L.ERR_INVALID, L.ERR_UNSUPPORTED}
    # kind 6 was unknown to ronk_air_check and still is a refused operand there: no periodic column exists
    assert OLD.check(L, [OP(AR.MOV, 0, O(PER, 0)), emit]) == L.ERR_INVALID


def test_the_shared_instance_passes_the_check(L):
    prog = FP.sbox_periodic_program()
    kw = dict(columns=(3,), n_ext=0, n_chal=2, n_imm=len(prog.imm), n_regs=prog.n_regs, J=prog.n_constraints)
    assert check(L, prog.ops, (3, 3, 3), **kw) == L.OK
    assert check(L, prog.ops, (3, 3), **kw) == L.ERR_INVALID and check(L, prog.ops, (3, 3, 3), log2_n=2, **kw) == L.ERR_UNSUPPORTED


def test_null_pointers(L):
    d, h = C.c_void_p(16), C.c_void_p(32)   # never dereferenced: refused first
    ops = (C.c_uint64 * 1)(OP(AR.EMIT, AR.ALL, O(PER, 0)))
    cols, lp, vals = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(0), (C.c_uint64 * 1)(5)
    assert L.lib.ronk_air_create_per(None, h, 1, cols, 0, 0, 0, 1, 1, ops, 1, None, 1, lp, vals) == L.ERR_INVALID
    out = C.c_void_p(99)
    assert L.lib.ronk_air_create_per(C.byref(out), None, 1, cols, 0, 0, 0, 1, 1, ops, 1, None, 1, lp, vals) == L.ERR_INVALID and not out.value


def test_creation_and_eval_point(L):
    """with a device: the codes of creation in their order, the cells without the periodic operands, and ronk_air_eval_point
    against air_per_ref at points off and on H; without one: RONK_ERR_NO_DEVICE after the argument checks"""
    p, g, w = GL, 7, 7
    dom = C.c_void_p()
    rc = L.lib.ronk_plonk_create(C.byref(dom), p, g, w, 4, 3, g, (C.c_uint64 * 3)(1, 2, 3))
    if L.device_count() == 0:
        assert rc == L.ERR_NO_DEVICE
        return
    assert rc == L.OK
    inst = FP.sbox_periodic(p, 16)
    prog, periodic = inst.shape.prog, inst.shape.periodic
    ops, imm, cols = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * len(prog.imm))(*prog.imm), (C.c_uint32 * 1)(3)
    lp, big = (C.c_uint32 * 3)(3, 3, 3), (C.c_uint32 * 3)(3, 5, 3)
    flat = [v + (p if k % 3 == 0 and v + p < 2**64 else 0) for k, v in enumerate(v for vals in periodic for v in vals)]      # words >= p
    vals = (C.c_uint64 * len(flat))(*flat)
    h = C.c_void_p(99)
    create = lambda n_per, periods, values: L.lib.ronk_air_create_per(C.byref(h), dom, 1, cols, 0, 2, len(prog.imm), prog.n_regs,      # noqa: E731
                                                                      prog.n_constraints, ops, len(prog.ops), imm, n_per, periods, values)
    assert create(17, lp, vals) == L.ERR_UNSUPPORTED and not h.value
    assert create(3, big, vals) == L.ERR_UNSUPPORTED and create(3, None, vals) == L.ERR_INVALID and create(2, lp, vals) == L.ERR_INVALID
    assert create(3, lp, None) == L.ERR_INVALID and not h.value            # after the codes of the check
    assert create(3, big, None) == L.ERR_UNSUPPORTED
    assert create(3, lp, vals) == L.OK and h.value
    want_cells = APR.cells(prog.ops)
    got = (C.c_uint32 * 16)()
    assert L.lib.ronk_air_cells(h, got, 16) == len(want_cells) and list(got)[:len(want_cells)] == want_cells
    assert all(o & 0xF != PER for o in want_cells)
    rng = np.random.default_rng(3)
    E, D = PR.Ext2(p, w), PR.Domain(p, g, 4, 3, g)
    u64 = lambda n: rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)      # noqa: E731
    values, chal, lam = u64(2 * len(want_cells)), u64(4), u64(2 * prog.n_constraints)
    pairs = lambda a: [tuple(int(v) for v in a[2 * k:2 * k + 2]) for k in range(len(a) // 2)]           # noqa: E731
    out = (C.c_uint64 * 2)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                                        # noqa: E731
    for z in ([5, 9], [2**64 - 1, 2**64 - 2], [3, 0], [1, 0], [D.wN, 0]):
        za = (C.c_uint64 * 2)(*z)
        want = APR.eval_point(E, D, prog, z, pairs(values), pairs(chal), pairs(lam), periodic)
        rc = L.lib.ronk_air_eval_point(h, za, ptr(values), ptr(chal), ptr(lam), out)
        assert (rc, None if rc else (out[0], out[1])) == ((L.ERR_INVALID, None) if want is None else (L.OK, want)), z
    assert L.lib.ronk_air_destroy(h) == L.OK and L.lib.ronk_plonk_destroy(dom) == L.OK
