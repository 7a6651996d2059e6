"""The restatement of the STARK with a fixed round and periodic columns tests/stark_fixed_ref.py against itself and against
tests/stark_ref.py (CPU only): honest proofs of the two shared instances verify; a verifier built from other selectors, or with
one changed periodic value, rejects; a changed word of every proof section raises that section's bit; and without a fixed round
and periodic columns the proof is stark_ref's word for word."""
import pytest

import poseidon_ref as PR
import stark_fixed_programs as FP
import stark_fixed_ref as FR
import stark_ref as SR
import test_stark_ref as TS

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
GEN = TS.GEN
Q, D, SEED = TS.Q, TS.D, TS.SEED
_REF = {}
CASES = [("gate", 3, 2), ("sbox_periodic", 3, 3)]


def stark_of(p, shape, log2_n, log2_b, eta=1, log2_final=None, periodic=None, fri=None):
    g = GEN[p]
    return FR.Stark(TS.params(p), g, g, log2_n, log2_b, g, eta, max(2, log2_b) if log2_final is None else log2_final, Q, D, shape.columns,
                    shape.n_ext, shape.n_pub, shape.n_draw, shape.n_chal, shape.prog, n_fixed=shape.n_fixed,
                    periodic=shape.periodic if periodic is None else periodic, fri=fri)


def make(p, name, log2_n, log2_b):
    """(the Stark object, the instance, the committed fixed round or None, the honest proof, status, challenge table), once"""
    key = (p, name, log2_n, log2_b)
    if key not in _REF:
        inst = getattr(FP, name)(p, 1 << log2_n)
        st = stark_of(p, inst.shape, log2_n, log2_b)
        fixed = FR.fixed_commit(st, inst.fixed) if inst.fixed else None
        _REF[key] = (st, inst, fixed) + FR.prove(st, SEED, inst.pub, inst.rounds, fixed)
    return _REF[key]


def root_of(fixed):
    return None if fixed is None else FR.fixed_root(fixed)


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("name,log2_n,log2_b", CASES)
def test_honest_proofs_verify(p, name, log2_n, log2_b):
    st, inst, fixed, proof, status, chal = make(p, name, log2_n, log2_b)
    assert status == 0 and len(proof) == st.proof_words() and all(0 <= w < p for w in proof)
    assert FR.verify(st, SEED, inst.pub, proof, root_of(fixed)) == 0


def test_the_shape_of_the_inner_commitment():
    """gate: the fixed round is round 0 and is opened at zeta only (no selector is read at a rotation), the wires at zeta and
    zeta w_N; the proof carries two roots, not three.  sbox_periodic: the periodic columns add no point and no round"""
    st, inst, fixed, proof, _, _ = make(GL, "gate", 3, 2)
    assert st.rots == [0, 1] and st.masks == [0b01, 0b11, 1] and st.S.Cs == [5, 3, 8] and st.S.R == 3
    assert st.inner_offset() == 2 * D and proof[:D] != FR.fixed_root(fixed)
    st, inst, fixed, proof, _, _ = make(GL, "sbox_periodic", 3, 3)
    assert fixed is None and st.rots == [0, 1] and st.masks == [0b11, 1] and st.S.Cs == [3, 16]


@pytest.mark.parametrize("p", [GL, MONT])
def test_a_verifier_with_other_selectors_rejects(p):
    """the verifier commits ITS selectors: another circuit of the same shape has another root, and the proof fails with it"""
    st, inst, fixed, proof, _, _ = make(p, "gate", 3, 2)
    other = FR.fixed_commit(st, FP.gate_selectors(p, st.N, variant=1))
    assert FR.fixed_root(other) != FR.fixed_root(fixed)
    got = FR.verify(st, SEED, inst.pub, proof, FR.fixed_root(other))
    assert got != 0 and got & 8        # at least the fixed round's paths do not lead to that root
    # one changed word of one selector is enough
    sel = [list(col) for col in inst.fixed]
    sel[4][3] = (sel[4][3] + 1) % p
    assert FR.verify(st, SEED, inst.pub, proof, FR.fixed_root(FR.fixed_commit(st, sel))) != 0
    # a prover that commits other selectors and proves ITS circuit honestly is rejected by the verifier that holds the right root
    theirs = FP.gate(p, st.N, variant=1)
    cheat, status, _ = FR.prove(st, SEED, theirs.pub, theirs.rounds, other)
    assert status == 0 and FR.verify(st, SEED, theirs.pub, cheat, FR.fixed_root(other)) == 0
    assert FR.verify(st, SEED, theirs.pub, cheat, FR.fixed_root(fixed)) != 0


@pytest.mark.parametrize("p", [GL, MONT])
def test_a_verifier_with_another_periodic_value_rejects(p):
    """nothing of a periodic column is in the proof: the verifier evaluates its own, and the identity fails alone"""
    st, inst, _, proof, _, _ = make(p, "sbox_periodic", 3, 3)
    bad = [list(v) for v in inst.shape.periodic]
    bad[1][6] = (bad[1][6] + 1) % p
    assert FR.verify(stark_of(p, inst.shape, 3, 3, periodic=bad), SEED, inst.pub, proof, None) == FR.OOD
    # and a trace made with other constants does not satisfy the verifier's program
    trace = FP.sbox_periodic_trace(p, st.N, bad)
    cheat, status, _ = FR.prove(st, SEED, [(trace[0][0], 0), (trace[0][-1], 0)], [trace])
    assert status == 0 and FR.verify(st, SEED, [(trace[0][0], 0), (trace[0][-1], 0)], cheat, None) == FR.OOD


@pytest.mark.parametrize("name,log2_n,log2_b", CASES)
def test_a_changed_word_of_every_section(name, log2_n, log2_b):
    """the sections of test_stark_ref on the inner commitment's rounds, the fixed round among them"""
    st, inst, fixed, proof, _, _ = make(GL, name, log2_n, log2_b)
    flips = TS.sections(st)
    assert len(flips) == 8 + 2 * (st.R + 1 + st.fo)
    for what, (at, bits) in flips.items():
        t = list(proof)
        t[at] ^= 1 << 9
        got = FR.verify(st, SEED, inst.pub, t, root_of(fixed))
        assert got & bits == bits, (name, what, got)
    for what in ("fri path", "matrix path 0", "matrix path %d" % (st.S.R - 1)):
        t = list(proof)
        t[flips[what][0]] ^= 1 << 9
        assert FR.verify(st, SEED, inst.pub, t, root_of(fixed)) == flips[what][1], what
    assert FR.verify(st, [SEED[0] + 1, SEED[1]], inst.pub, proof, root_of(fixed)) != 0
    if fixed:
        root = list(FR.fixed_root(fixed))
        root[0] ^= 1 << 9
        assert FR.verify(st, SEED, inst.pub, proof, root) & 8


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("name,log2_n,log2_b", TS.CASES)
def test_without_fixed_and_periodic_it_is_stark_ref(p, name, log2_n, log2_b):
    st, inst, want, status, chal = TS.make(p, name, log2_n, log2_b)
    sh = inst.shape
    mine = FR.Stark(TS.params(p), GEN[p], GEN[p], log2_n, log2_b, GEN[p], 1, max(2, log2_b), Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw,
                    sh.n_chal, sh.prog)
    assert mine.proof_words() == st.proof_words() and mine.masks == st.masks
    assert FR.prove(mine, SEED, inst.pub, inst.rounds) == (want, status, chal)
    assert FR.verify(mine, SEED, inst.pub, want) == 0
    t = list(want)
    t[-1] ^= 1
    assert FR.verify(mine, SEED, inst.pub, t) == SR.verify(st, SEED, inst.pub, t) != 0
