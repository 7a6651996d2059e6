"""The STARK restatement tests/stark_ref.py against itself and against its parts (CPU only): honest proofs of the three shared
instances verify; a changed trace word, a wrong public value and a program whose degree the blowup cannot hold are rejected by
the out-of-domain identity alone; a changed word of every proof section raises that section's bit; and for one round with the
rotations {0, 1} the inner proof is what mpcs_ref.open_ gives on the derived shape."""
import pytest

import air_ref as AR
import deep_ref as DR
import mpcs_ref as MR
import plonk_ref as PL
import poseidon_ref as PR
import stark_programs as SP
import stark_ref as SR

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
GEN = {GL: 7, MONT: 10}
Q, D, SEED = 8, 2, [3, 4]
_REF = {}


def params(p):
    return PR.derive_params(p, 8, 7, 2, 4, 4)


def make(p, name, log2_n, log2_b, eta=1, log2_final=None):
    """(the Stark object, the instance, its honest proof, status and challenge table), computed once; FRI stops at 2^2 points, or
    at the blowup where that is larger"""
    log2_final = max(2, log2_b) if log2_final is None else log2_final
    key = (p, name, log2_n, log2_b, eta, log2_final)
    if key not in _REF:
        g = GEN[p]
        E = PL.Ext2(p, g)
        inst = SP.logup(p, 1 << log2_n, E) if name == "logup" else getattr(SP, name)(p, 1 << log2_n)
        sh = inst.shape
        st = SR.Stark(params(p), g, g, log2_n, log2_b, g, eta, log2_final, Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw, sh.n_chal, sh.prog)
        _REF[key] = (st, inst) + SR.prove(st, SEED, inst.pub, inst.rounds)
    return _REF[key]


CASES = [("fibonacci", 3, 2), ("sbox_row", 3, 3), ("logup", 3, 2)]


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("name,log2_n,log2_b", CASES)
def test_honest_proofs_verify(p, name, log2_n, log2_b):
    st, inst, proof, status, chal = make(p, name, log2_n, log2_b)
    assert status == 0 and len(proof) == st.proof_words() and len(chal) == inst.shape.n_chal
    assert all(0 <= w < p for w in proof)
    assert SR.verify(st, SEED, inst.pub, proof) == 0


def test_points_and_masks():
    st, inst, _, _, _ = make(GL, "fibonacci", 3, 2)
    assert st.rots == [0, 1] and st.masks == [0b11, 1] and st.S.Cs == [3, 8]
    st, inst, _, _, _ = make(GL, "logup", 3, 2)
    assert st.rots == [0, 1] and st.masks == [0b01, 0b11, 1] and st.S.Cs == [4, 2, 8]
    assert SR.where(st.Cs, st.Es, AR.EXT, 0) == (1, 0) and SR.where(st.Cs, st.Es, AR.BASE, 3) == (0, 3)
    # rot -1 and rot N - 1 are one point
    prog = AR.Program([AR.op(AR.SUB, 0, AR.operand(AR.BASE, 0, -1), AR.operand(AR.BASE, 0, 7)), AR.op(AR.EMIT, AR.ALL, AR.operand(AR.REG, 0))], [], 1, 1)
    assert SR.rotations(prog.ops, 8) == [0, 7] and SR.masks(prog.ops, 8, (1,), (0,)) == [0b11]


def test_the_pieces_of_the_quotient():
    """Fibonacci: every piece but q_0 is zero; the S-box row at B = 8: pieces 0 .. 5 are non-zero and the last two are zero"""
    st, _, proof, _, _ = make(GL, "fibonacci", 3, 2)
    ys = MR.claims_from_words(st.S, proof[st.inner_offset():][:2 * st.S.Y])
    assert all(y == (0, 0) for y in ys[1][0][2:]) and ys[1][0][0] != (0, 0)
    st, _, proof, _, _ = make(GL, "sbox_row", 3, 3)
    ys = MR.claims_from_words(st.S, proof[st.inner_offset():][:2 * st.S.Y])
    nonzero = [i for i in range(st.B) if ys[1][0][2 * i] != (0, 0) or ys[1][0][2 * i + 1] != (0, 0)]
    assert nonzero == list(range(6))


@pytest.mark.parametrize("p", [GL, MONT])
def test_rejected_by_the_identity_alone(p):
    """one trace word changed; a wrong public value; sbox_row at B = 4, whose degree is too high: the openings verify, bit 256 alone"""
    st, inst, _, _, _ = make(p, "fibonacci", 3, 2)
    bad = [list(col) for col in inst.rounds[0]]
    bad[1][4] = (bad[1][4] + 1) % p
    proof, status, _ = SR.prove(st, SEED, inst.pub, [bad])
    assert status == 0 and SR.verify(st, SEED, inst.pub, proof) == SR.OOD
    wrong = [inst.pub[0], (inst.pub[1][0] + 1, 0)]
    proof, status, _ = SR.prove(st, SEED, wrong, inst.rounds)
    assert status == 0 and SR.verify(st, SEED, wrong, proof) == SR.OOD
    # an honest proof under another public value: the transcript differs, so more than the identity fails
    _, _, honest, _, _ = make(p, "fibonacci", 3, 2)
    assert SR.verify(st, SEED, wrong, honest) & SR.OOD
    st, inst, proof, status, _ = make(p, "sbox_row", 3, 2)
    assert status == 0 and SR.verify(st, SEED, inst.pub, proof) == SR.OOD


def sections(st):
    """a word of every section of the proof: its offset and the bits a change there must raise"""
    S, F = st.S, st.S.F
    off, base = MR.section_offsets(S), st.inner_offset()
    fri_leaves = off["fri"] + F.L * D + 2 * F.size(F.L)
    out = {"trace root": (1, 8), "quotient root": (st.R * D, 8), "claim": (base + off["claims"] + 1, 16),
           "quotient claim": (base + off["claims"] + S.Y - 1, 16 | SR.OOD), "fri root": (base + off["fri"] + 1, 1),
           "final": (base + fri_leaves - 1, 4), "fri leaf": (base + fri_leaves + 3 * F.leaf_len(0) + 1, 2),
           "fri path": (base + fri_leaves + Q * F.leaf_len(0) + 1, 1)}
    for r in range(S.R):
        out["matrix leaf %d" % r] = (base + off["leaves"][r] + 5 * S.leaf_len(r) + 1, 8 | 16)
        out["matrix path %d" % r] = (base + off["paths"][r] + 6 * F.depth(0) * D + 1, 8)
    return out


@pytest.mark.parametrize("name,log2_n,log2_b", CASES)
def test_a_changed_word_of_every_section(name, log2_n, log2_b):
    st, inst, proof, _, _ = make(GL, name, log2_n, log2_b)
    for what, (at, bits) in sections(st).items():
        t = list(proof)
        t[at] ^= 1 << 9
        got = SR.verify(st, SEED, inst.pub, t)
        assert got & bits == bits, (name, what, got)
    # matrix paths and FRI paths change nothing else
    for what in ("fri path", "matrix path 0", "matrix path %d" % st.R):
        t = list(proof)
        t[sections(st)[what][0]] ^= 1 << 9
        assert SR.verify(st, SEED, inst.pub, t) == sections(st)[what][1], what
    assert SR.verify(st, [SEED[0] + 1, SEED[1]], inst.pub, proof) != 0


@pytest.mark.parametrize("p", [GL, MONT])
def test_one_round_is_the_multi_matrix_opening_on_the_derived_shape(p):
    """R = 1, rotations {0, 1}: the roots are those of the two committed matrices, and the inner proof is mpcs_ref.open_ on the
    shape (K = 2, columns (3, 2 B), masks (0b11, 0b01)) at zeta, zeta w_N under the transcript's last state"""
    st, inst, proof, _, chal = make(p, "fibonacci", 3, 2)
    g, E, dom = GEN[p], st.E, st.dom
    S = MR.Mpcs(params(p), g, g, 5, g, 1, 2, 2, Q, D, 2, (3, 8), (0b11, 0b01))
    coef0 = [PL.interpolate(p, dom.wN, col) for col in inst.rounds[0]]
    M0 = [[PL.evaluate(p, f, x) for x in dom.points()] for f in coef0]
    tree0 = MR.commit(S, 0, M0)
    t = PR.sponge(st.P, SEED + [c for pair in inst.pub for c in pair], D)
    out = PR.sponge(st.P, t + tree0.root_hash(), D + 2)
    t, lam = out[:D], (out[D], out[D + 1])
    lams = [E.pow(lam, j) for j in range(5)]
    T = AR.quotient(E, dom, inst.shape.prog, M0, [], inst.pub, lams)
    planes = [PL.coset_coefficients(dom, [v[pl] for v in T]) for pl in (0, 1)]
    coefQ = [planes[pl][i * 8:(i + 1) * 8] for i in range(4) for pl in (0, 1)]
    MQ = [[PL.evaluate(p, f, x) for x in dom.points()] for f in coefQ]
    assert MQ == DR.columns(S.rounds[1], coefQ)
    treeQ = MR.commit(S, 1, MQ)
    out = PR.sponge(st.P, t + treeQ.root_hash(), D + 2)
    t, zeta = out[:D], (out[D], out[D + 1])
    inner, status = MR.open_(S, [M0, MQ], [tree0, treeQ], [coef0, coefQ], [zeta, E.mul_base(zeta, dom.wN)], t)
    assert status == 0 and proof == tree0.root_hash() + treeQ.root_hash() + inner
    assert chal == [E.el(c) for c in inst.pub]


def test_check_shape_codes():
    ok = ((3,), (0,), 2, (0,), 2, 2)
    assert SR.check_shape(*ok) == 0
    assert SR.check_shape(None, (0,), 2, (0,), 2, 2) == "invalid" and SR.check_shape((), (), 2, (), 2, 2) == "invalid"
    assert SR.check_shape((3,), (2,), 2, (0,), 2, 2) == "invalid" and SR.check_shape((3,), (0,), 2, (1,), 2, 2) == "invalid"
    assert SR.check_shape((4,), (2,), 1, (1,), 2, 8) == 0
    assert SR.check_shape((1,) * 5, (0,) * 5, 2, (0,) * 5, 2, 2) == "unsupported" and SR.check_shape((3,), (0,), 2, (0,), 2, 9) == "unsupported"
    assert SR.check_shape((1,) * 5, (1,) * 5, 2, (0,) * 5, 2, 9) == "invalid"      # invalid before unsupported
