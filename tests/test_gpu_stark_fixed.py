"""The STARK with a fixed round and periodic columns on the device (ronk_stark_create_fixed and the entry points around the fixed
round, ronkathon_amd.stark.Stark) word for word against the Python restatement tests/stark_fixed_ref.py: proofs of the two shared
instances (tests/stark_fixed_programs.py) over Goldilocks, MONT_P and P_MID at N = 2^3, 2^4, 2^6 with B = 2, 4, 8, one of them
with grinding; the root of the preprocessing; one fixed buffer under two proofs; a verifier that holds the root alone; a verifier
with other selectors or another periodic value; tampered proofs; the order of the calls; the host forms and the callers; and one
N = 2^14 run checked for status 0 and determinism only.  Poseidon parameters, Q and D are those of tests/test_gpu_mpcs.py."""
import ctypes as C

import numpy as np
import pytest

import pow_ref as PW
import prime_classes as PC
import stark_fixed_programs as FP
import stark_fixed_ref as FR
import test_stark_ref as TS
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from ronkathon_amd.stark import Stark
from test_gpu_fri import D, GEN, Q, _Field, dev, host, params
from test_gpu_mpcs import PowFri
from test_gpu_stark import flat_pairs, garbage, matrix

pytestmark = pytest.mark.gpu

GL, MONT, MID = 0xFFFFFFFF00000001, PC.MONT_P, PC.P_MID
SEED = [3, 4]
# (instance, log2_n, log2_blowup, log2_arity, log2_final, grinding bits); sbox_periodic has degree-7 transitions: B = 8
CASES = [("gate", 3, 3, 1, 3, 0), ("gate", 4, 2, 1, 2, 6), ("gate", 6, 1, 2, 3, 0), ("sbox_periodic", 3, 3, 1, 3, 0),
         ("sbox_periodic", 4, 3, 2, 3, 0)]
_REF = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def reference(p, case):
    """(the restatement's object, the instance, its committed fixed round or None, the proof, status, challenge table), once"""
    key = (p, case)
    if key not in _REF:
        name, log2_n, log2_b, eta, log2_final, bits = case
        g, inst = GEN[p], getattr(FP, name)(p, 1 << log2_n)
        sh = inst.shape
        fri = PowFri(PW.Pow(bits, PW.default_limit(p, bits))) if bits else None
        st = FR.Stark(params(p), g, g, log2_n, log2_b, g, eta, log2_final, Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw, sh.n_chal, sh.prog,
                      n_fixed=sh.n_fixed, periodic=sh.periodic, fri=fri)
        fixed = FR.fixed_commit(st, inst.fixed) if inst.fixed else None
        _REF[key] = (st, inst, fixed) + FR.prove(st, SEED, inst.pub, inst.rounds, fixed)
    return _REF[key]


def handle_of(p, case, shape, periodic=None):
    _, log2_n, log2_b, eta, log2_final, bits = case
    g = GEN[p]
    return Stark((_Field(p),) + params(p).create_args()[1:], g, g, log2_n, log2_b, g, eta, log2_final, Q, D, shape.columns, shape.n_ext,
                 shape.n_pub, shape.n_draw, tuple(shape.prog), pow_bits=bits, n_fixed=shape.n_fixed,
                 periodic=shape.periodic if periodic is None else periodic)


def commit_fixed(torch, h, rows, fill=-1):
    """the preprocessing on the device: -> d_fixed, with the input unchanged"""
    d_rows, d_fixed = dev(torch, matrix(rows)), garbage(torch, h.fixed_words, fill)
    h.fixed_commit_dev(d_rows, d_fixed)
    assert np.array_equal(host(torch, d_rows), matrix(rows))
    return d_fixed


def root_words(torch, h, d_fixed):
    at = h.fixed_root_offset
    assert h.fixed_root(d_fixed) == d_fixed.data_ptr() + 8 * at
    return host(torch, d_fixed)[at:at + D].tolist()


def prove(torch, h, pub, trace, seed=SEED, fill=-1):
    d_seed, d_pub, d_trace = dev(torch, np.array(seed, dtype=np.uint64)), dev(torch, flat_pairs(pub)), dev(torch, matrix(trace))
    d_work, d_proof = garbage(torch, h.workspace_words, fill), garbage(torch, h.proof_words, fill)
    d_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    h.prove_dev(d_seed, d_pub, d_trace, d_work, d_proof, d_status)
    assert np.array_equal(host(torch, d_trace), matrix(trace))
    return host(torch, d_proof), int(d_status.item())


def verify(torch, h, pub, proof, seed=SEED):
    return h.verify_dev(dev(torch, np.array(seed, dtype=np.uint64)), dev(torch, flat_pairs(pub)), dev(torch, np.array(proof, dtype=np.uint64)))


# ------------------------------------------------------------------------------------------------ proofs
def check_proof(torch, p, case):
    st, inst, fixed, want, want_status, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    assert h.proof_words == st.proof_words()
    d_fixed = None
    if fixed:
        d_fixed = commit_fixed(torch, h, inst.fixed)
        assert root_words(torch, h, d_fixed) == FR.fixed_root(fixed)
        before = host(torch, d_fixed)
        h.set_fixed(d_fixed)
    else:
        assert h.fixed_words == 0
    got, status = prove(torch, h, inst.pub, inst.rounds[0])
    assert status == want_status == 0 and got.tolist() == want, (p, case)
    assert verify(torch, h, inst.pub, got) == 0
    # buffers poisoned with another pattern and another seed: the same fixed buffer under a second proof, untouched by both
    other = [SEED[0] + 5, SEED[1]]
    again, status = prove(torch, h, inst.pub, inst.rounds[0], seed=other, fill=0x55)
    want2, status2, _ = FR.prove(st, other, inst.pub, inst.rounds, fixed)
    assert status == status2 == 0 and again.tolist() == want2 and want2 != want
    assert verify(torch, h, inst.pub, again, seed=other) == 0 and verify(torch, h, inst.pub, again) != 0
    if fixed:
        assert np.array_equal(host(torch, d_fixed), before)
        # a second commit into a buffer poisoned differently gives the same extension, coefficients and tree
        twice = host(torch, commit_fixed(torch, h, inst.fixed, fill=0x33))
        assert np.array_equal(twice[:h.fixed_root_offset + D], before[:h.fixed_root_offset + D])
    h.close()


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("case", CASES)
def test_proof_word_for_word(torch, p, case):
    check_proof(torch, p, case)


@pytest.mark.parametrize("case", [CASES[1], CASES[3]])
def test_proof_word_for_word_prime_class(torch, case):
    """P_MID of tests/prime_classes.py, where every outcome of mont64::add is common: one case of each instance"""
    check_proof(torch, MID, case)


# ------------------------------------------------------------------------------------------------ the verifier
@pytest.mark.parametrize("p", [GL, MONT])
def test_a_verifier_that_holds_the_root_alone(torch, p):
    """a second handle is given D words: it accepts the proof, refuses to prove, and with the root of other selectors, or of one
    changed selector word, answers what the restatement answers"""
    case = CASES[1]
    st, inst, fixed, proof, _, _ = reference(p, case)
    prover, verifier = handle_of(p, case, inst.shape), handle_of(p, case, inst.shape)
    d_fixed = commit_fixed(torch, prover, inst.fixed)
    d_root = dev(torch, np.array(FR.fixed_root(fixed), dtype=np.uint64))
    verifier.set_fixed(d_root, root_only=True)
    assert verify(torch, verifier, inst.pub, proof) == 0
    d = garbage(torch, 8)
    assert L.lib.ronk_stark_begin_dev(verifier.h, d.data_ptr(), d.data_ptr(), d.data_ptr(), 0) == L.ERR_INVALID
    # the verifier's own preprocessing of other selectors
    sel = [list(col) for col in inst.fixed]
    sel[4][3] = (sel[4][3] + 1) % p
    for rows in (FP.gate_selectors(p, st.N, variant=1), sel):
        theirs = FR.fixed_commit(st, rows)
        want = FR.verify(st, SEED, inst.pub, proof, FR.fixed_root(theirs))
        d_other = commit_fixed(torch, verifier, rows)
        assert root_words(torch, verifier, d_other) == FR.fixed_root(theirs) != FR.fixed_root(fixed)
        verifier.set_fixed(verifier.fixed_root(d_other), root_only=True)
        assert want != 0 and want & 8 and verify(torch, verifier, inst.pub, proof) == want
        verifier.set_fixed(d_other)           # the whole buffer serves a verifier as well
        assert verify(torch, verifier, inst.pub, proof) == want
    verifier.set_fixed(d_fixed)
    assert verify(torch, verifier, inst.pub, proof) == 0
    prover.close()
    verifier.close()


@pytest.mark.parametrize("p", [GL, MONT])
def test_a_verifier_with_another_periodic_value(torch, p):
    case = CASES[3]
    st, inst, _, proof, _, _ = reference(p, case)
    bad = [list(v) for v in inst.shape.periodic]
    bad[2][6] = (bad[2][6] + 1) % p           # column 2: the program ties column 1 to column 0
    h = handle_of(p, case, inst.shape, periodic=bad)
    assert verify(torch, h, inst.pub, proof) == FR.OOD
    # and its prover on a trace made with those constants is the restatement's with them, rejected by the right verifier
    trace = FP.sbox_periodic_trace(p, st.N, bad)
    pub = [(trace[0][0], 0), (trace[0][-1], 0)]
    _, log2_n, log2_b, eta, log2_final, _ = case
    sh = inst.shape
    theirs = FR.Stark(params(p), GEN[p], GEN[p], log2_n, log2_b, GEN[p], eta, log2_final, Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw,
                      sh.n_chal, sh.prog, periodic=bad)
    want, _, _ = FR.prove(theirs, SEED, pub, [trace])
    assert FR.verify(theirs, SEED, pub, want) == 0
    got, status = prove(torch, h, pub, trace)
    assert status == 0 and got.tolist() == want and verify(torch, h, pub, got) == 0
    h.close()
    h = handle_of(p, case, inst.shape)
    assert verify(torch, h, pub, got) == FR.verify(st, SEED, pub, want) == FR.OOD
    h.close()


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]])
def test_verifier_statuses_of_tampered_proofs(torch, p, case):
    """a changed word of every section (the fixed round's leaves and paths among them), all at once, another seed, another public
    value, a changed word of the verifier's root: the restatement's status"""
    st, inst, fixed, proof, _, _ = reference(p, case)
    root = FR.fixed_root(fixed) if fixed else None
    h = handle_of(p, case, inst.shape)
    if fixed:
        h.set_fixed(np.array(root, dtype=np.uint64), root_only=True)      # the host form: the handle owns its copy
    flips = TS.sections(st)
    assert len(flips) == 8 + 2 * st.S.R
    for what, (at, bits) in flips.items():
        t = list(proof)
        t[at] ^= 1 << 9
        want = FR.verify(st, SEED, inst.pub, t, root)
        assert want & bits == bits and verify(torch, h, inst.pub, t) == want, (p, case, what)
    t = list(proof)
    for at, _ in flips.values():
        t[at] ^= 1 << 9
    assert verify(torch, h, inst.pub, t) == FR.verify(st, SEED, inst.pub, t, root)
    other = [SEED[0] + 1, SEED[1]]
    want = FR.verify(st, other, inst.pub, proof, root)
    assert want != 0 and verify(torch, h, inst.pub, proof, seed=other) == want
    wrong = [(inst.pub[0][0] + 1, 0)] + inst.pub[1:]
    want = FR.verify(st, SEED, wrong, proof, root)
    assert want & FR.OOD and verify(torch, h, wrong, proof) == want
    if fixed:
        flipped = list(root)
        flipped[1] ^= 1 << 9
        h.set_fixed(np.array(flipped, dtype=np.uint64), root_only=True)
        want = FR.verify(st, SEED, inst.pub, proof, flipped)
        assert want & 8 and verify(torch, h, inst.pub, proof) == want
    h.close()


# ------------------------------------------------------------------------------------------------ order, host forms, callers
def test_stages_before_set_fixed_are_refused(torch):
    p, case = GL, CASES[0]
    st, inst, fixed, want, _, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    lib = L.lib
    d_seed, d_pub, d_trace = dev(torch, np.array(SEED, dtype=np.uint64)), dev(torch, flat_pairs(inst.pub)), dev(torch, matrix(inst.rounds[0]))
    d_work, d_proof = garbage(torch, h.workspace_words), garbage(torch, h.proof_words)
    d_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    args = (d_seed.data_ptr(), d_pub.data_ptr(), d_trace.data_ptr(), d_work.data_ptr(), d_proof.data_ptr(), d_status.data_ptr(), 0)
    status = C.c_int(5)
    assert lib.ronk_stark_begin_dev(h.h, args[0], args[1], args[3], 0) == L.ERR_INVALID                # nothing set
    assert lib.ronk_stark_prove_dev(h.h, *args) == L.ERR_INVALID
    assert lib.ronk_stark_verify_dev(h.h, args[0], args[1], args[4], C.byref(status), 0) == L.ERR_INVALID and status.value == 5
    assert int(d_status.item()) == 99
    d_fixed = commit_fixed(torch, h, inst.fixed)                                                       # the commit needs nothing set
    h.set_fixed(h.fixed_root(d_fixed), root_only=True)
    assert lib.ronk_stark_begin_dev(h.h, args[0], args[1], args[3], 0) == L.ERR_INVALID                # a verifier's handle
    assert lib.ronk_stark_prove_dev(h.h, *args) == L.ERR_INVALID
    assert verify(torch, h, inst.pub, want) == 0
    h.set_fixed(d_fixed)
    h.begin(d_seed, d_pub, d_work)
    h.set_fixed(d_fixed)                                                                               # a setter ends the sequence in flight
    assert lib.ronk_stark_commit_round_dev(h.h, 0, args[2], args[3], 0) == L.ERR_INVALID
    h.begin(d_seed, d_pub, d_work)
    h.commit_round(0, d_trace, d_work)
    h.finish(d_work, d_proof, d_status)
    assert int(d_status.item()) == 0 and host(torch, d_proof).tolist() == want
    h.close()


@pytest.mark.parametrize("p", [GL, MONT])
def test_host_forms_and_callers(torch, p):
    case = CASES[1]
    st, inst, fixed, want, _, _ = reference(p, case)
    _, log2_n, log2_b, eta, log2_final, bits = case
    h = handle_of(p, case, inst.shape)
    buf = h.fixed_commit(inst.fixed)
    at = h.fixed_root_offset
    assert buf.size == h.fixed_words and buf[at:at + D].tolist() == FR.fixed_root(fixed)
    assert buf[:5 * st.M].tolist() == [v for col in fixed.M for v in col] and buf[5 * st.M:5 * (st.M + st.N)].tolist() == [v for c in fixed.coef for v in c]
    h.set_fixed(buf)
    proof, status = h.prove(SEED, inst.pub, inst.rounds[0])
    assert status == 0 and proof.tolist() == want and h.verify(SEED, inst.pub, proof) == 0
    h.set_fixed(buf[at:at + D], root_only=True)
    assert h.verify(SEED, inst.pub, proof) == 0
    with pytest.raises(L.RonkPanic):
        h.prove(SEED, inst.pub, inst.rounds[0])
    with pytest.raises(L.RonkPanic):
        h.set_fixed(buf[:-1])
    h.close()
    g, sponge = GEN[p], (_Field(p),) + params(p).create_args()[1:]
    args = (sponge, g, g, log2_n, log2_b, g, eta, log2_final, Q, D, tuple(inst.shape.prog))
    proof, status = callers.stark_prove(*args, inst.rounds[0], inst.pub, SEED, pow_bits=bits, fixed=inst.fixed)
    assert status == 0 and proof.tolist() == want
    assert callers.stark_verify(*args, 3, inst.pub, SEED, proof, pow_bits=bits, fixed=inst.fixed) == 0
    other = FP.gate_selectors(p, st.N, variant=1)
    assert callers.stark_verify(*args, 3, inst.pub, SEED, proof, pow_bits=bits, fixed=other) == \
        FR.verify(st, SEED, inst.pub, want, FR.fixed_root(FR.fixed_commit(st, other))) != 0
    # the periodic instance through the callers
    case = CASES[3]
    st, inst, _, want, _, _ = reference(p, case)
    _, log2_n, log2_b, eta, log2_final, bits = case
    args = (sponge, g, g, log2_n, log2_b, g, eta, log2_final, Q, D, tuple(inst.shape.prog))
    proof, status = callers.stark_prove(*args, inst.rounds[0], inst.pub, SEED, periodic=inst.shape.periodic)
    assert status == 0 and proof.tolist() == want
    assert callers.stark_verify(*args, 3, inst.pub, SEED, proof, periodic=inst.shape.periodic) == 0


# ------------------------------------------------------------------------------------------------ a large trace
def test_2_to_the_14_rows_status_and_determinism(torch):
    """gate at N = 2^14, B = 4 (M = 2^16: tiled plans, several workgroups of every kernel): no restatement at this size; status 0
    from prover and verifier, and two runs give equal words; another circuit's verifier rejects"""
    p, log2_n = GL, 14
    inst = FP.gate(p, 1 << log2_n)
    case = ("gate", log2_n, 2, 2, 4, 0)
    h = handle_of(p, case, inst.shape)
    d_fixed = commit_fixed(torch, h, inst.fixed)
    h.set_fixed(d_fixed)
    one, s1 = prove(torch, h, inst.pub, inst.rounds[0])
    two, s2 = prove(torch, h, inst.pub, inst.rounds[0], fill=0x33)
    assert s1 == s2 == 0 and np.array_equal(one, two)
    assert verify(torch, h, inst.pub, one) == 0
    bad = [list(col) for col in inst.rounds[0]]
    bad[1][12345] = (bad[1][12345] + 1) % p
    got, s3 = prove(torch, h, inst.pub, bad)
    assert s3 == 0 and verify(torch, h, inst.pub, got) == FR.OOD
    d_other = commit_fixed(torch, h, FP.gate_selectors(p, 1 << log2_n, variant=1))
    h.set_fixed(h.fixed_root(d_other), root_only=True)
    assert verify(torch, h, inst.pub, one) & 8
    h.close()
