"""Argument errors of the STARK layer (ronk_stark_check and the entry points around a handle): all of them are settled by host-side
integer logic before any device work, so this runs without a GPU.  A handle needs a device: where there is none, creation says
so after the argument checks, and the proofs are held to tests/stark_ref.py by tests/test_gpu_stark.py."""
import ctypes as C
import os
import re

import pytest

import air_programs as AP
import air_ref as AR
import stark_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL = 0xFFFFFFFF00000001
NAMES = ("ronk_stark_check", "ronk_stark_create", "ronk_stark_destroy", "ronk_stark_set_pow", "ronk_stark_proof_words",
         "ronk_stark_workspace_words", "ronk_stark_begin_dev", "ronk_stark_commit_round_dev", "ronk_stark_challenges_dev",
         "ronk_stark_finish_dev", "ronk_stark_split_dev", "ronk_stark_prove_dev", "ronk_stark_verify_dev", "ronk_stark_prove", "ronk_stark_verify")
O, OP = AR.operand, AR.op
FIB = AP.fibonacci()


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def u32(values):
    return None if values is None else (C.c_uint32 * max(1, len(values)))(*values)


def check(L, prog=FIB, p=GL, rate=7, g=7, w=7, log2_n=4, log2_b=2, shift=7, eta=1, log2_final=2, Q=8, D=2, columns=(3,), n_ext=(0,), n_pub=2,
          n_draw=(0,), n_chal=2, R=None, n_regs=None, J=None, n_imm=None, null_ops=False):
    ops = (C.c_uint64 * max(1, len(prog.ops)))(*prog.ops)
    R = (0 if columns is None else len(columns)) if R is None else R
    return L.lib.ronk_stark_check(p, rate, g, w, log2_n, log2_b, shift, eta, log2_final, Q, D, R, u32(columns), u32(n_ext), n_pub, u32(n_draw),
                                  n_chal, len(prog.imm) if n_imm is None else n_imm, prog.n_regs if n_regs is None else n_regs,
                                  prog.n_constraints if J is None else J, None if null_ops else ops, len(prog.ops))


def test_exported_and_declared(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ronk_ntt.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ronk_[a-z0-9_]+)\s*\(", hdr)) if n.startswith("ronk_stark_"))
    assert declared == sorted(NAMES)
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)
    # the prototypes of the ctypes table have the header's parameter counts
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(L._SIG[name][1]) == len([a for a in params.split(",") if a.strip()]), name


def test_the_shared_programs_pass_the_check(L):
    assert check(L) == L.OK
    assert check(L, AP.sbox_row(), log2_b=3, log2_final=3) == L.OK
    assert check(L, AP.logup(2, True), columns=(4, 2), n_ext=(0, 1), n_pub=0, n_draw=(1, 0), n_chal=1) == L.OK
    # a round without base columns is no AIR group; the draws may come after any round
    assert check(L, AP.logup(2, True), columns=(2, 2, 2), n_ext=(0, 0, 1), n_pub=0, n_draw=(0, 1, 0), n_chal=1) == L.OK
    assert check(L, AP.plonk(), columns=(3, 5, 3, 3), n_ext=(0, 0, 0, 1), n_pub=1, n_draw=(1, 0, 0, 0), n_chal=2, log2_b=2) == L.OK


def test_check_codes_in_their_order(L):
    # 1. the codes of ronk_air_check come first, whatever else is wrong
    for kw in (dict(null_ops=True), dict(J=0)):
        assert check(L, **kw) == L.ERR_INVALID and check(L, p=15, **kw) == L.ERR_INVALID and check(L, columns=None, **kw) == L.ERR_INVALID
    for kw in (dict(n_regs=17), dict(J=65), dict(n_imm=257), dict(n_chal=33, n_pub=33), dict(log2_n=0)):
        assert check(L, **kw) == L.ERR_UNSUPPORTED and check(L, p=15, R=0, **kw) == L.ERR_UNSUPPORTED, kw
    assert check(L, columns=(65,)) == L.ERR_UNSUPPORTED and check(L, columns=(65,), p=15, n_pub=0) == L.ERR_UNSUPPORTED
    assert check(L, columns=(33, 32), n_ext=(0, 0), n_draw=(0, 0)) == L.ERR_UNSUPPORTED              # more than 64 base columns
    assert check(L, columns=(19,), n_ext=(9,)) == L.ERR_UNSUPPORTED and check(L, columns=(19,), n_ext=(8,)) == L.OK   # sum E_r <= 8
    assert check(L, columns=(2,)) == L.ERR_INVALID and check(L, columns=(2,), p=15) == L.ERR_INVALID   # the program reads column 2
    assert check(L, columns=(3,), n_ext=(1,)) == L.ERR_INVALID                                         # one base column is left
    assert check(L, n_chal=1, n_pub=1) == L.ERR_INVALID                                                # the program reads challenge 1
    assert check(L, n_regs=FIB.n_regs - 1) == L.ERR_INVALID
    # 2. then those of ronk_mpcs_check on the derived shape: the FRI codes, then the shape
    assert check(L, p=65, g=2) == L.ERR_NOT_PRIME and check(L, p=65, g=2, n_pub=3) == L.ERR_NOT_PRIME   # 65 = 5 * 13, 64 | p - 1
    assert check(L, p=97, g=5, w=5, shift=5) == L.ERR_NO_ROOT                                         # 2^6 does not divide 96
    assert check(L, w=49) == L.ERR_INVALID and check(L, shift=0) == L.ERR_INVALID
    assert check(L, log2_final=1) != L.OK and check(L, D=8) != L.OK and check(L, Q=0) != L.OK          # final < blowup, D > rate, no query
    assert check(L, columns=(3, 0), n_ext=(0, 0), n_draw=(0, 0)) == L.ERR_INVALID                      # an empty round
    assert check(L, columns=None) == L.ERR_INVALID and check(L, n_ext=None) == L.ERR_INVALID and check(L, n_draw=None) == L.ERR_INVALID
    assert check(L, columns=(3, 1000, 25), n_ext=(0, 0, 0), n_draw=(0, 0, 0)) == L.ERR_UNSUPPORTED     # AIR: more than 64 base columns
    # 3. the domain: s^M = 1
    assert check(L, shift=1) == L.ERR_UNSUPPORTED and check(L, shift=GL - 1) == L.ERR_UNSUPPORTED
    assert check(L, shift=1, n_pub=1) == L.ERR_UNSUPPORTED                                            # before this family's own
    # 4. this family's own: INVALID before UNSUPPORTED
    assert check(L, R=0) == L.ERR_INVALID
    assert check(L, columns=(3,), n_ext=(2,)) == L.ERR_INVALID                                         # 2 E_r > C_r
    assert check(L, n_pub=1) == L.ERR_INVALID and check(L, n_pub=3) == L.ERR_INVALID and check(L, n_draw=(1,)) == L.ERR_INVALID
    assert check(L, n_pub=1, n_draw=(1,)) == L.OK and check(L, n_pub=0, n_draw=(2,)) == L.OK
    five = dict(columns=(3, 1, 1, 1, 1), n_ext=(0,) * 5, n_draw=(0,) * 5)
    assert check(L, **five) == L.ERR_UNSUPPORTED and check(L, n_pub=1, **five) == L.ERR_INVALID
    assert check(L, columns=(3, 1, 1, 1), n_ext=(0,) * 4, n_draw=(0,) * 4) == L.OK                     # R = 4


def points_program(n_rots):
    """one constraint that reads column 0 at the rotations 0 .. n_rots - 1"""
    ops = [OP(AR.MOV, 0, O(AR.BASE, 0, 0))] + [OP(AR.ADD, 0, O(AR.REG, 0), O(AR.BASE, 0, r)) for r in range(1, n_rots)]
    return AR.Program(ops + [OP(AR.EMIT, AR.ALL, O(AR.REG, 0), 0)], [], 1, 1)


def test_the_number_of_points_at_and_past_its_bound(L):
    kw = dict(columns=(1,), n_pub=0, n_chal=0)
    assert SR.rotations(points_program(8).ops, 16) == list(range(8))
    assert check(L, points_program(8), **kw) == L.OK and check(L, points_program(9), **kw) == L.ERR_UNSUPPORTED
    assert check(L, points_program(12), **kw) == L.ERR_UNSUPPORTED and check(L, points_program(9), n_pub=1, columns=(1,), n_chal=0) == L.ERR_INVALID
    # rot -1 and rot N - 1 are one point: eight points again
    prog = points_program(8)
    prog = AR.Program(prog.ops[:-1] + [OP(AR.ADD, 0, O(AR.REG, 0), O(AR.BASE, 0, -9)), prog.ops[-1]], [], 1, 1)
    assert check(L, prog, **kw) == L.OK


def test_null_pointers_and_sizes(L):
    d = C.c_void_p(16)      # never dereferenced: refused first
    lib = L.lib
    assert lib.ronk_stark_destroy(None) == L.ERR_INVALID and lib.ronk_stark_set_pow(None, 4, 10) == L.ERR_INVALID
    assert lib.ronk_stark_proof_words(None) == 0 and lib.ronk_stark_workspace_words(None) == 0
    assert lib.ronk_stark_challenges_dev(None, d) is None
    assert lib.ronk_stark_begin_dev(None, d, d, d, None) == L.ERR_INVALID
    assert lib.ronk_stark_commit_round_dev(None, 0, d, d, None) == L.ERR_INVALID
    assert lib.ronk_stark_finish_dev(None, d, d, d, None) == L.ERR_INVALID and lib.ronk_stark_split_dev(None, d, d, d, None) == L.ERR_INVALID
    assert lib.ronk_stark_prove_dev(None, d, d, d, d, d, d, None) == L.ERR_INVALID
    st = C.c_int(5)
    assert lib.ronk_stark_verify_dev(None, d, d, d, C.byref(st), None) == L.ERR_INVALID
    assert lib.ronk_stark_prove(None, d, d, d, d, C.byref(st)) == L.ERR_INVALID
    assert lib.ronk_stark_verify(None, d, d, d, C.byref(st)) == L.ERR_INVALID and st.value == 5
    ops, cols, zero = (C.c_uint64 * len(FIB.ops))(*FIB.ops), u32((3,)), u32((0,))
    args = (7, 7, 4, 2, 7, 1, 2, 8, 2, 1, cols, zero, 2, zero, 2, 0, FIB.n_regs, 5, ops, len(FIB.ops), None)
    out = C.c_void_p(99)
    assert lib.ronk_stark_create(None, d, *args) == L.ERR_INVALID
    assert lib.ronk_stark_create(C.byref(out), None, *args) == L.ERR_INVALID and not out.value
    out = C.c_void_p(99)
    assert lib.ronk_stark_create(C.byref(out), d, *(args[:15] + (1,) + args[16:])) == L.ERR_INVALID and not out.value   # n_imm without imm


def test_create_with_and_without_a_device(L):
    """with a device: the codes of the check through creation, the sizes against the restatement's, NULL arguments of the stages;
    without one: RONK_ERR_NO_DEVICE after the argument checks"""
    import poseidon_ref as PR
    from ronkathon_amd.stark import Stark

    class F:
        ORDER = GL
    P = PR.derive_params(GL, 8, 7, 2, 4, 4)
    sponge = (F,) + P.create_args()[1:]
    make = lambda **kw: Stark(sponge, 7, 7, 4, 2, kw.pop("shift", 7), 1, 2, 8, 2, kw.pop("columns", (3,)), (0,), kw.pop("n_pub", 2), (0,),     # noqa: E731
                              tuple(FIB), **kw)
    if L.device_count() == 0:
        with pytest.raises(L.RonkPanic) as e:
            L.PoseidonHandle(*P.create_args())
        assert e.value.code == L.ERR_NO_DEVICE
        return
    for kw, code in ((dict(columns=(2,)), L.ERR_INVALID), (dict(shift=1), L.ERR_UNSUPPORTED), (dict(n_pub=1), L.ERR_INVALID)):
        with pytest.raises(L.RonkPanic) as e:
            make(**kw)
        assert e.value.code == code, kw
    h = make()
    ref = SR.Stark(P, 7, 7, 4, 2, 7, 1, 2, 8, 2, (3,), (0,), 2, (0,), 2, FIB)
    assert h.proof_words == ref.proof_words() and h.workspace_words > ref.S.workspace_words() + 3 * 80 + 8 * 80
    plain = h.proof_words
    assert L.lib.ronk_stark_set_pow(h.h, 6, 12) == L.OK and h.proof_words == plain + 1
    d = C.c_void_p(16)
    assert L.lib.ronk_stark_begin_dev(h.h, None, d, d, None) == L.ERR_INVALID and L.lib.ronk_stark_begin_dev(h.h, d, None, d, None) == L.ERR_INVALID
    assert L.lib.ronk_stark_commit_round_dev(h.h, 0, d, d, None) == L.ERR_INVALID          # before begin
    assert L.lib.ronk_stark_finish_dev(h.h, d, None, d, None) == L.ERR_INVALID
    st = C.c_int(5)
    assert L.lib.ronk_stark_verify_dev(h.h, d, d, None, C.byref(st), None) == L.ERR_INVALID and L.lib.ronk_stark_verify_dev(h.h, d, d, d, None, None) == L.ERR_INVALID
    assert L.lib.ronk_stark_challenges_dev(h.h, None) is None and L.lib.ronk_stark_challenges_dev(h.h, d) == 16 + 8 * 2
    h.close()
