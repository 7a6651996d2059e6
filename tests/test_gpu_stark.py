"""The STARK layer on the device (ronk_stark_*, ronkathon_amd.stark.Stark) word for word against the Python restatement
tests/stark_ref.py: proofs of the three shared instances (tests/stark_programs.py) over Goldilocks, MONT_P and P_MID, with and
without grinding, the staged two-round logUp proof with its columns built on the device from the handle's challenge pointer, the
verifier's status for honest and tampered proofs, an independent ronk_mpcs handle on the embedded proof, the host-pointer forms
and the callers, the order of the stages, and one N = 2^16 run checked for status 0 and determinism only.  Poseidon parameters,
Q and D are those of tests/test_gpu_mpcs.py.

The sizes: N = 2^3 (the radix-2 plans), 2^4 (the first tiled plan) and 2^6; B = 2, 4, 8; M <= 2^8 against the restatement."""
import ctypes as C

import numpy as np
import pytest

import mpcs_ref as MR
import plonk_ref as PL
import pow_ref as PW
import prime_classes as PC
import stark_programs as SP
import stark_ref as SR
import test_stark_ref as TS
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from ronkathon_amd.stark import Stark
from test_gpu_fri import D, GEN, Q, _Field, dev, host, params
from test_gpu_mpcs import PowFri

pytestmark = pytest.mark.gpu

GL, MONT, MID = 0xFFFFFFFF00000001, PC.MONT_P, PC.P_MID
SEED = [3, 4]
# (instance, log2_n, log2_blowup, log2_arity, log2_final, grinding bits)
CASES = [("fibonacci", 3, 1, 1, 2, 0), ("fibonacci", 4, 2, 1, 2, 6), ("fibonacci", 6, 2, 2, 4, 0), ("sbox_row", 3, 3, 1, 3, 0),
         ("sbox_row", 4, 3, 2, 3, 5), ("logup", 3, 2, 1, 2, 0), ("logup", 4, 1, 3, 2, 0)]
_REF = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def garbage(torch, n, fill=-1):
    return torch.full((n,), fill, dtype=torch.int64, device="cuda")


def reference(p, case):
    """(the restatement's object, the instance, its proof, status and challenge table), computed once per case"""
    key = (p, case)
    if key not in _REF:
        name, log2_n, log2_b, eta, log2_final, bits = case
        g = GEN[p]
        inst = SP.logup(p, 1 << log2_n, PL.Ext2(p, g)) if name == "logup" else getattr(SP, name)(p, 1 << log2_n)
        sh = inst.shape
        fri = PowFri(PW.Pow(bits, PW.default_limit(p, bits))) if bits else None
        st = SR.Stark(params(p), g, g, log2_n, log2_b, g, eta, log2_final, Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw, sh.n_chal, sh.prog,
                      fri=fri)
        _REF[key] = (st, inst) + SR.prove(st, SEED, inst.pub, inst.rounds)
    return _REF[key]


def handle_of(p, case, shape):
    _, log2_n, log2_b, eta, log2_final, bits = case
    g = GEN[p]
    return Stark((_Field(p),) + params(p).create_args()[1:], g, g, log2_n, log2_b, g, eta, log2_final, Q, D, shape.columns, shape.n_ext,
                 shape.n_pub, shape.n_draw, tuple(shape.prog), pow_bits=bits)


def flat_pairs(pairs):
    return np.array([int(c) for pair in pairs for c in pair], dtype=np.uint64)


def matrix(rows):
    return np.array(rows, dtype=np.uint64).ravel()


class Run:
    """one prover run on the device: the buffers, pre-filled with a pattern"""

    def __init__(self, torch, h, pub, fill=-1):
        self.torch, self.h = torch, h
        self.d_seed, self.d_pub = dev(torch, np.array(SEED, dtype=np.uint64)), dev(torch, flat_pairs(pub)) if pub else None
        self.d_work, self.d_proof = garbage(torch, h.workspace_words, fill), garbage(torch, h.proof_words, fill)
        self.d_status = torch.full((1,), 99, dtype=torch.int32, device="cuda")

    def result(self):
        return host(self.torch, self.d_proof), int(self.d_status.item())


def prove_one_round(torch, h, pub, trace, fill=-1):
    run = Run(torch, h, pub, fill)
    d_trace = dev(torch, matrix(trace))
    h.prove_dev(run.d_seed, run.d_pub, d_trace, run.d_work, run.d_proof, run.d_status)
    proof, status = run.result()
    assert np.array_equal(host(torch, d_trace), matrix(trace))
    return proof, status


def prove_logup(torch, h, p, w, N, fill=-1):
    """the staged proof with the columns built on the device: the multiplicities of round 0 by ronk_lookup_mult_dev (negated), S of
    round 1 by ronk_logup_sum_dev on the handle's challenge pointer"""
    f, table = SP.lookup_columns(p, N)
    run = Run(torch, h, [], fill)
    d_f, d_t = dev(torch, np.array(f, dtype=np.uint64)), dev(torch, np.array(table, dtype=np.uint64))
    d_mult, d_missing = garbage(torch, N), garbage(torch, 2)
    d_lw = garbage(torch, L.lib.ronk_lookup_workspace_words(N))
    L.check(L.lib.ronk_lookup_mult_dev(p, d_t.data_ptr(), N, d_f.data_ptr(), 1, N, 1, d_mult.data_ptr(), d_missing.data_ptr(), d_lw.data_ptr(), 0))
    d_round0 = torch.cat([d_f, d_t, torch.ones(N, dtype=torch.int64, device="cuda"), d_mult])
    h.begin(run.d_seed, None, run.d_work)
    h.commit_round(0, d_round0, run.d_work)
    d_S, d_last, d_sw = garbage(torch, 2 * N), garbage(torch, 2), garbage(torch, L.lib.ronk_scan_workspace_words(N))
    d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    alpha = h.challenges(run.d_work)
    assert alpha == run.d_work.data_ptr() + 8 * D
    L.check(L.lib.ronk_logup_sum_dev(p, w, d_round0.data_ptr(), d_round0.data_ptr() + 8 * 2 * N, 2, N, alpha, d_S.data_ptr(), d_last.data_ptr(),
                                     d_sw.data_ptr(), d_st.data_ptr(), 0))
    h.commit_round(1, d_S, run.d_work)
    h.finish(run.d_work, run.d_proof, run.d_status)
    proof, status = run.result()
    assert int(d_st.item()) == 0 and host(torch, d_last).tolist() == [0, 0] and host(torch, d_missing)[0] == 0
    return proof, status


def prove_on_device(torch, h, p, case, inst, fill=-1):
    if case[0] == "logup":
        return prove_logup(torch, h, p, GEN[p], 1 << case[1], fill)
    return prove_one_round(torch, h, inst.pub, inst.rounds[0], fill)


def verify_on_device(torch, h, pub, proof, seed=SEED):
    return h.verify_dev(dev(torch, np.array(seed, dtype=np.uint64)), dev(torch, flat_pairs(pub)) if pub else None,
                        dev(torch, np.array(proof, dtype=np.uint64)))


# ------------------------------------------------------------------------------------------------ proofs
def check_proof(torch, p, case):
    st, inst, want, want_status, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    assert h.proof_words == st.proof_words()
    got, status = prove_on_device(torch, h, p, case, inst)
    assert status == want_status == 0 and got.tolist() == want, (p, case)
    assert verify_on_device(torch, h, inst.pub, got) == 0
    # buffers poisoned with another pattern: no word the proof depends on is left unwritten; a second sequence on the same handle
    again, _ = prove_on_device(torch, h, p, case, inst, fill=0x55)
    assert np.array_equal(again, got)
    # an independent ronk_mpcs handle of the derived shape accepts the embedded proof at the transcript's points and seed
    _, log2_n, log2_b, eta, log2_final, bits = case
    roots, t, _, _, zeta = SR.replay(st, SEED, inst.pub, want)
    pos = L.PoseidonHandle(*params(p).create_args())
    inner = L.MpcsHandle(pos, GEN[p], GEN[p], log2_n + log2_b, GEN[p], eta, log2_final, log2_b, Q, D, st.K, st.S.Cs, st.masks)
    if bits:
        inner.set_pow(bits)
    assert inner.proof_words == st.S.proof_words() == h.proof_words - st.inner_offset()
    d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    d_roots, d_z = dev(torch, matrix(roots)), dev(torch, np.array(MR.ER.planar(SR.points(st, zeta)), dtype=np.uint64))
    d_t, d_inner = dev(torch, np.array(t, dtype=np.uint64)), dev(torch, got[st.inner_offset():])
    inner.verify_dev(d_roots.data_ptr(), d_z.data_ptr(), d_t.data_ptr(), d_inner.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert int(d_st.item()) == 0
    inner.close()
    pos.close()
    h.close()


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("case", CASES)
def test_proof_word_for_word(torch, p, case):
    check_proof(torch, p, case)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]])
def test_proof_word_for_word_prime_class(torch, case):
    """P_MID of tests/prime_classes.py, where every outcome of mont64::add is common: one case of each instance"""
    check_proof(torch, MID, case)


# ------------------------------------------------------------------------------------------------ the verifier
@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5]])
def test_verifier_statuses_of_tampered_proofs(torch, p, case):
    """a changed word of every section, all of them at once, another seed and another public value: the restatement's status"""
    st, inst, proof, _, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    flips = TS.sections(st)
    for what, (at, _) in flips.items():
        t = list(proof)
        t[at] ^= 1 << 9
        want = SR.verify(st, SEED, inst.pub, t)
        assert want != 0 and verify_on_device(torch, h, inst.pub, t) == want, (p, case, what)
    t = list(proof)
    for at, _ in flips.values():
        t[at] ^= 1 << 9
    assert verify_on_device(torch, h, inst.pub, t) == SR.verify(st, SEED, inst.pub, t)
    other = [SEED[0] + 1, SEED[1]]
    want = SR.verify(st, other, inst.pub, proof)
    assert want != 0 and verify_on_device(torch, h, inst.pub, proof, seed=other) == want
    if inst.pub:
        wrong = [inst.pub[0], (inst.pub[1][0] + 1, 0)]
        want = SR.verify(st, SEED, wrong, proof)
        assert want & SR.OOD and verify_on_device(torch, h, wrong, proof) == want
    # a claim word >= p in the place of its residue: the same value everywhere
    at = st.inner_offset() + 1
    if proof[at] + p < 2**64:
        t = list(proof)
        t[at] += p
        assert verify_on_device(torch, h, inst.pub, t) == SR.verify(st, SEED, inst.pub, t)
    h.close()


@pytest.mark.parametrize("p", [GL, MONT])
def test_rejected_by_the_identity_alone(torch, p):
    """one trace word changed, a wrong public value, and sbox_row at B = 4 whose degree is too high: the device proves them as the
    restatement does, the openings verify, and the verifier answers 256"""
    case = CASES[1]
    st, inst, _, _, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    bad = [list(col) for col in inst.rounds[0]]
    bad[1][4] = (bad[1][4] + 1) % p
    wrong = [inst.pub[0], (inst.pub[1][0] + 1, 0)]
    for pub, trace in ((inst.pub, bad), (wrong, inst.rounds[0])):
        want, want_status, _ = SR.prove(st, SEED, pub, [trace])
        got, status = prove_one_round(torch, h, pub, trace)
        assert status == want_status == 0 and got.tolist() == want
        assert SR.verify(st, SEED, pub, want) == SR.OOD == verify_on_device(torch, h, pub, got)
    h.close()
    case = ("sbox_row", 3, 2, 1, 2, 0)
    st, inst, want, _, _ = reference(p, case)
    h = handle_of(p, case, inst.shape)
    got, status = prove_one_round(torch, h, inst.pub, inst.rounds[0])
    assert status == 0 and got.tolist() == want
    assert SR.verify(st, SEED, inst.pub, want) == SR.OOD == verify_on_device(torch, h, inst.pub, got)
    h.close()


# ------------------------------------------------------------------------------------------------ host forms, callers, order
@pytest.mark.parametrize("p", [GL, MONT])
def test_host_forms_and_callers(torch, p):
    case = CASES[1]
    st, inst, want, _, _ = reference(p, case)
    _, log2_n, log2_b, eta, log2_final, bits = case
    h = handle_of(p, case, inst.shape)
    proof, status = h.prove(SEED, inst.pub, inst.rounds[0])
    assert status == 0 and proof.tolist() == want
    assert h.verify(SEED, inst.pub, proof) == 0
    bad = proof.copy()
    bad[-1] ^= np.uint64(1)
    assert h.verify(SEED, inst.pub, bad) == SR.verify(st, SEED, inst.pub, bad.tolist()) == 8
    with pytest.raises(L.RonkPanic):
        h.prove(SEED, inst.pub[:1], inst.rounds[0])
    h.close()
    g, sponge = GEN[p], (_Field(p),) + params(p).create_args()[1:]
    args = (sponge, g, g, log2_n, log2_b, g, eta, log2_final, Q, D, tuple(inst.shape.prog))
    proof, status = callers.stark_prove(*args, inst.rounds[0], inst.pub, SEED, pow_bits=bits)
    assert status == 0 and proof.tolist() == want
    assert callers.stark_verify(*args, 3, inst.pub, SEED, proof, pow_bits=bits) == 0
    assert callers.stark_verify(*args, 3, inst.pub, SEED, bad, pow_bits=bits) == 8


def test_stages_out_of_order_are_refused(torch):
    p = GL
    st, inst, want, _, _ = reference(p, CASES[5])
    h = handle_of(p, CASES[5], inst.shape)
    N = 1 << CASES[5][1]
    run, other = Run(torch, h, []), garbage(torch, h.workspace_words)
    d_r0, d_r1 = dev(torch, matrix(inst.rounds[0])), garbage(torch, 2 * N)
    lib, s = L.lib, 0
    work, proof, status = run.d_work.data_ptr(), run.d_proof.data_ptr(), run.d_status.data_ptr()
    assert lib.ronk_stark_commit_round_dev(h.h, 0, d_r0.data_ptr(), work, s) == L.ERR_INVALID          # before begin
    assert lib.ronk_stark_finish_dev(h.h, work, proof, status, s) == L.ERR_INVALID
    assert lib.ronk_stark_prove_dev(h.h, run.d_seed.data_ptr(), None, d_r0.data_ptr(), work, proof, status, s) == L.ERR_INVALID   # R = 2
    h.begin(run.d_seed, None, run.d_work)
    assert lib.ronk_stark_commit_round_dev(h.h, 1, d_r1.data_ptr(), work, s) == L.ERR_INVALID          # round 1 before round 0
    assert lib.ronk_stark_commit_round_dev(h.h, 2, d_r1.data_ptr(), work, s) == L.ERR_INVALID          # no such round
    assert lib.ronk_stark_commit_round_dev(h.h, 0, d_r0.data_ptr(), other.data_ptr(), s) == L.ERR_INVALID   # another workspace
    assert lib.ronk_stark_finish_dev(h.h, work, proof, status, s) == L.ERR_INVALID                     # rounds missing
    h.commit_round(0, d_r0, run.d_work)
    assert lib.ronk_stark_commit_round_dev(h.h, 0, d_r0.data_ptr(), work, s) == L.ERR_INVALID          # twice
    assert lib.ronk_stark_finish_dev(h.h, work, proof, status, s) == L.ERR_INVALID
    assert lib.ronk_stark_begin_dev(h.h, None, None, work, s) == L.ERR_INVALID
    # the refused calls changed nothing: the sequence, started again, gives the proof
    got, st_dev = prove_logup(torch, h, p, GEN[p], N)
    assert st_dev == 0 and got.tolist() == want
    assert lib.ronk_stark_finish_dev(h.h, work, proof, status, s) == L.ERR_INVALID                     # after the end
    h.close()


# ------------------------------------------------------------------------------------------------ a large trace
def test_2_to_the_16_rows_status_and_determinism(torch):
    """Fibonacci at N = 2^16, B = 4 (M = 2^18, multi-pass plans, several workgroups of the split): no restatement at this size;
    status 0 from prover and verifier, and two runs give equal words"""
    p, log2_n = GL, 16
    inst = SP.fibonacci(p, 1 << log2_n)
    case = ("fibonacci", log2_n, 2, 3, 3, 0)
    h = handle_of(p, case, inst.shape)
    one, s1 = prove_one_round(torch, h, inst.pub, inst.rounds[0])
    two, s2 = prove_one_round(torch, h, inst.pub, inst.rounds[0], fill=0x33)
    assert s1 == s2 == 0 and np.array_equal(one, two)
    assert verify_on_device(torch, h, inst.pub, one) == 0
    bad = [list(col) for col in inst.rounds[0]]
    bad[2][12345] = (bad[2][12345] + 1) % p
    got, s3 = prove_one_round(torch, h, inst.pub, bad)
    assert s3 == 0 and verify_on_device(torch, h, inst.pub, got) == SR.OOD
    h.close()


# ------------------------------------------------------------------------------------------------ the split alone
@pytest.mark.parametrize("p", [GL, MONT])
def test_the_split_as_a_building_block(torch, p):
    """ronk_stark_split_dev at N = 2^11, B = 4: more residues than one workgroup has lanes, words >= p among the inputs, every word
    of both outputs against Python integers"""
    from test_gpu_fri import words
    log2_n, log2_b = 11, 2
    N, B, M = 1 << log2_n, 1 << log2_b, 1 << (log2_n + log2_b)
    inst = SP.fibonacci(p, 8)
    h = handle_of(p, ("fibonacci", log2_n, log2_b, 1, 3, 0), inst.shape)
    c = words(77, 2 * M, p)
    d_c, d_coef, d_msg = dev(torch, c), garbage(torch, 2 * M), garbage(torch, 2 * M)
    h.split(d_c, d_coef, d_msg)
    sinv = pow(GEN[p], -1, p)
    pw = [1]
    for _ in range(M - 1):
        pw.append(pw[-1] * sinv % p)
    want_coef, want_msg = [0] * (2 * M), [0] * (2 * M)
    for pl in range(2):
        for j in range(M):
            i, k, v = j >> log2_n, j & (N - 1), int(c[pl * M + j]) % p
            want_coef[(2 * i + pl) * N + k] = v * pw[j] % p
            want_msg[(2 * i + pl) * N + k] = v * pw[i * N] % p
    assert host(torch, d_coef).tolist() == want_coef and host(torch, d_msg).tolist() == want_msg
    assert np.array_equal(host(torch, d_c), c)
    assert L.lib.ronk_stark_split_dev(h.h, None, d_coef.data_ptr(), d_msg.data_ptr(), 0) == L.ERR_INVALID
    h.close()
