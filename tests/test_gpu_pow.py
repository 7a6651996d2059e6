"""Proof-of-work grinding on the device: the stand-alone search and check (ronk_pow_*) against the Python restatement
(tests/pow_ref.py) over the emulator test's grid, under a captured graph, and at b = 20 against the library's own sponge entry point;
FRI (base and extension) and the batched commitment with grinding switched on, word for word against the restatement, with the
verifier's bit 64, the query indices, the handle size functions against canaried buffers, and a handle without grinding against
fri_ref.  The 64-bit primes run with TEST Poseidon parameters derived in poseidon_ref.py (not a standard instance)."""
import random

import numpy as np
import pytest

import deep_ref as DR
import ext2_ref as ER
import fri_ext_ref as FX
import fri_ref as FR
import poseidon_ref as PR
import pow_ref as PW
from ronkathon_amd import _lib as L
from ronkathon_amd import callers
from test_emu_pow import BITS, FIELDS, FRI_SET, OTHER_SETS, SEED_LENS, reference
from test_gpu_fri import GEN, _Field, dev, host, params

pytestmark = pytest.mark.gpu

GL, MONT = PR.GOLDILOCKS, PR.MONT_P
Q = 5
CANARY = 0x5AA55AA55AA55AA5
MAX_LANES = (64, 512, 0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def poseidon(p, pset=FRI_SET):
    return L.PoseidonHandle(*PR.derive_params(p, *pset).create_args())


def grind_dev(torch, pos, seed, bits, lam, max_lanes, stream=0, bufs=None):
    """-> the nonce; bufs: (d_seed, d_work, d_nonce) to reuse"""
    if bufs is None:
        bufs = (dev(torch, seed), torch.full((L.lib.ronk_pow_workspace_words(),), -1, dtype=torch.int64, device="cuda"),
                torch.full((1,), 77, dtype=torch.int64, device="cuda"))
    d_seed, d_work, d_nonce = bufs
    pos.pow_grind_dev(d_seed.data_ptr() if len(seed) else None, len(seed), bits, lam, max_lanes, d_work.data_ptr(), d_nonce.data_ptr(), stream)
    return int(host(torch, d_nonce)[0])


def verify_dev(torch, pos, seed, bits, lam, nonce):
    d_seed, d_nonce = dev(torch, seed), dev(torch, [nonce])
    d_ok = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    pos.pow_verify_dev(d_seed.data_ptr() if len(seed) else None, len(seed), bits, lam, d_nonce.data_ptr(), d_ok.data_ptr())
    torch.cuda.synchronize()
    return int(d_ok.item())


# ------------------------------------------------------------------------------------------------ (a) stand-alone grinding
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("seed_len", SEED_LENS)
def test_grind_against_restatement(torch, p, seed_len):
    pos = poseidon(p)
    for bits in BITS:
        seed, lam, want = reference(p, FRI_SET, seed_len, bits)
        for max_lanes in MAX_LANES:
            assert grind_dev(torch, pos, seed, bits, lam, max_lanes) == want, (p, seed_len, bits, max_lanes)
        assert verify_dev(torch, pos, seed, bits, lam, want) == 1
    pos.close()


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("pset", OTHER_SETS)
def test_grind_other_register_widths(torch, p, pset):
    pos = poseidon(p, pset)
    rate = pset[4]
    for seed_len in (1, rate, rate + 1):
        for bits in (1, 10):
            seed, lam, want = reference(p, pset, seed_len, bits)
            for max_lanes in MAX_LANES:
                assert grind_dev(torch, pos, seed, bits, lam, max_lanes) == want, (p, pset, seed_len, bits, max_lanes)
    pos.close()


@pytest.mark.parametrize("p", FIELDS)
def test_not_found_and_verify(torch, p):
    P = PR.derive_params(p, *FRI_SET)
    pos = poseidon(p)
    rng = random.Random(p % 1009)
    while True:
        seed = [rng.randrange(p) for _ in range(2)]
        if PW.grind(P, seed, 10, 4) == PW.NONE:
            break
    for max_lanes in MAX_LANES:
        assert grind_dev(torch, pos, seed, 10, 4, max_lanes) == PW.NONE
    assert verify_dev(torch, pos, seed, 10, 4, PW.NONE) == 0
    # the honest nonce, a failing nonce + 1, the same residue out of range, 2^64 - 1
    for seed_len in (1, 5):
        seed, lam, nonce = reference(p, FRI_SET, seed_len, 6)
        bad = next(n for n in range(nonce + 1, 1 << lam) if not PW.meets(P, seed, n, 6))
        assert verify_dev(torch, pos, seed, 6, lam, nonce) == 1
        assert verify_dev(torch, pos, seed, 6, lam, bad) == 0
        assert verify_dev(torch, pos, seed, 6, lam, PW.NONE) == int(PW.verify(P, seed, 6, lam, PW.NONE)) == 0
        if nonce + p < 2**64:
            assert verify_dev(torch, pos, seed, 6, lam, nonce + p) == 0
        assert verify_dev(torch, pos, seed, 6, 1, nonce) == int(nonce < 2)      # the limit alone
    with pytest.raises(L.RonkPanic) as e:
        pos.pow_grind_dev(16, 2, 64, 12, 0, 16, 16)
    assert e.value.code == L.ERR_INVALID
    pos.close()


@pytest.mark.parametrize("p", [GL, MONT])
def test_captured_graph(torch, p):
    """(grind, verify) captured once and replayed on two seeds written into the same buffer"""
    pos = poseidon(p)
    P = PR.derive_params(p, *FRI_SET)
    first, lam, want = reference(p, FRI_SET, 5, 10)
    second = [v ^ 1 for v in first]
    seeds = [(first, want), (second, PW.grind(P, second, 10, lam))]
    d_seed = dev(torch, first)
    d_work = torch.full((L.lib.ronk_pow_workspace_words(),), -1, dtype=torch.int64, device="cuda")
    d_nonce = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    d_ok = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    pos.pow_grind_dev(d_seed.data_ptr(), 5, 10, lam, 0, d_work.data_ptr(), d_nonce.data_ptr(), s.cuda_stream)   # outside the capture first
    s.synchronize()
    assert int(host(torch, d_nonce)[0]) == want
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        pos.pow_grind_dev(d_seed.data_ptr(), 5, 10, lam, 0, d_work.data_ptr(), d_nonce.data_ptr(), st)
        pos.pow_verify_dev(d_seed.data_ptr(), 5, 10, lam, d_nonce.data_ptr(), d_ok.data_ptr(), st)
    assert seeds[0][1] != seeds[1][1] and PW.NONE not in (seeds[0][1], seeds[1][1])
    for rep in range(2):
        for seed, nonce in seeds:
            d_seed.copy_(dev(torch, seed))
            d_nonce.fill_(77); d_ok.fill_(99)
            gr.replay()
            torch.cuda.synchronize()
            assert int(host(torch, d_nonce)[0]) == nonce and int(d_ok.item()) == 1
    del gr
    pos.close()


@pytest.mark.parametrize("p", [GL, MONT])
def test_twenty_bits_against_the_sponge_entry_point(torch, p):
    """b = 20 below 2^26: Python cannot check minimality there, ronk_poseidon_sponge_dev (other code: the ordinary sponge kernel)
    can: over every seed || [n], n <= nonce, the only word with 20 low zero bits is the last"""
    pos = poseidon(p)
    seed = [random.Random(p % 1009 + 20).randrange(p) for _ in range(3)]
    nonce = grind_dev(torch, pos, seed, 20, 26, 0)
    assert nonce < (1 << 26)
    assert grind_dev(torch, pos, seed, 20, 26, 512) == nonce
    chunk, zeros, last = 1 << 18, 0, None
    d_seed = dev(torch, seed)
    for n0 in range(0, nonce + 1, chunk):
        cnt = min(chunk, nonce + 1 - n0)
        items = torch.empty((cnt, 4), dtype=torch.int64, device="cuda")
        items[:, :3] = d_seed
        items[:, 3] = torch.arange(n0, n0 + cnt, dtype=torch.int64, device="cuda")
        out = torch.full((cnt,), -1, dtype=torch.int64, device="cuda")
        pos.sponge_dev(items.data_ptr(), cnt, 4, 4, 1, out.data_ptr(), 1)
        torch.cuda.synchronize()
        hits = torch.nonzero((out & ((1 << 20) - 1)) == 0).flatten().tolist()
        zeros += len(hits)
        if hits:
            last = n0 + hits[-1]
    assert zeros == 1 and last == nonce
    assert verify_dev(torch, pos, seed, 20, 26, nonce) == 1
    pos.close()


# ------------------------------------------------------------------------------------------------ (b) FRI with grinding
# ((log2_n, eta, log2_final), D, bits): D = 4 = rate takes the prefix-permutation path
FRI_CASES = [((6, 1, 2), 2, 6), ((6, 1, 2), 4, 10), ((9, 3, 3), 4, 6), ((9, 3, 3), 2, 10)]
_REF = {}


def fri_objects(p, case, D, ext):
    n, eta, log2_final = case
    if ext:
        return FX.FriExt(params(p), GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, 0)
    return FR.Fri(params(p), GEN[p], n, GEN[p], eta, log2_final, 1, Q, D)


def fri_reference(p, case, D, bits, ext):
    """(the restatement's object, Pow, codeword, seed, proof), computed once"""
    key = (p, case, D, bits, ext)
    if key not in _REF:
        F = fri_objects(p, case, D, ext)
        W = PW.Pow(bits, PW.default_limit(p, bits))
        rng = random.Random(case[0] * 100 + D + bits)
        f = FR.evaluate(F, [rng.randrange(p) for _ in range(F.size(0) >> 1)])
        seed = [3, 4, 5, 6][:D]
        _REF[key] = (F, W, f, seed, PW.fri_prove_pow(F, W, f, seed))
    return _REF[key]


def fri_handle(pos, p, case, D, ext, **kw):
    n, eta, log2_final = case
    return L.FriHandle(pos, GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, w=GEN[p] if ext else None, **kw)


def canaried(torch, words, pad=8):
    return torch.full((words + pad,), CANARY, dtype=torch.int64, device="cuda")


def fri_prove_dev(torch, h, f, seed):
    """-> (proof words, workspace words), both buffers canaried past the handle's sizes"""
    d_ev, d_seed = dev(torch, f), dev(torch, seed)
    d_work, d_proof = canaried(torch, h.workspace_words), canaried(torch, h.proof_words)
    h.prove_dev(d_ev.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr())
    proof, work = host(torch, d_proof), host(torch, d_work)
    assert (proof[h.proof_words:] == np.uint64(CANARY)).all() and (work[h.workspace_words:] == np.uint64(CANARY)).all()
    return proof[:h.proof_words], work[:h.workspace_words]


def fri_verify_dev(torch, h, proof, seed):
    d_proof, d_seed = dev(torch, proof), dev(torch, seed)
    d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    h.verify_dev(d_proof.data_ptr(), d_seed.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return int(d_st.item())


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("fc", FRI_CASES)
def test_fri_proof_word_for_word(torch, p, ext, fc):
    case, D, bits = fc
    F, W, f, seed, want = fri_reference(p, case, D, bits, ext)
    pos = poseidon(p)
    h = fri_handle(pos, p, case, D, ext, pow_bits=bits)
    assert h.pow_log2_limit == W.log2_limit
    assert (h.proof_words, h.workspace_words) == (PW.proof_words(F, W), PW.workspace_words(F, W))
    got, work = fri_prove_dev(torch, h, f, seed)
    assert got.tolist() == want, (p, ext, fc)
    # the buffers are written up to the handle's sizes: the nonce is the last proof word, the prefix state the workspace's tail
    assert int(got[-1]) != CANARY and int(work[h.workspace_words - PW.WORK_WORDS]) != CANARY
    assert fri_verify_dev(torch, h, got, seed) == 0
    # the indices the transcript implies
    def indices_dev(proof):
        d_proof, d_seed = dev(torch, proof), dev(torch, seed)      # held until the call has run
        d_idx = torch.full((Q,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.ronk_fri_query_indices_dev(h.h, d_proof.data_ptr(), d_seed.data_ptr(), d_idx.data_ptr(), None))
        return host(torch, d_idx).tolist()

    assert indices_dev(got) == PW.fri_indices_pow(F, W, want, seed)
    # the nonce word tampered: out of range with the same residue is bit 64 alone; nonce + 1 and 2^64 - 1 as the restatement says
    nonce = want[-1]
    if nonce + p < 2**64:
        assert fri_verify_dev(torch, h, want[:-1] + [nonce + p], seed) == 64
    for word in (nonce + 1, PW.NONE):
        bad = want[:-1] + [word]
        st = PW.fri_verify_pow(F, W, bad, seed)
        assert fri_verify_dev(torch, h, bad, seed) == st and (st & 64 or word == nonce + 1)
        assert indices_dev(bad) == PW.fri_indices_pow(F, W, bad, seed)
    # a tampered leaf gives its own bit beside a clean bit 64
    bad = list(want)
    bad[F.L * D + len(FR.split(F, want[:-1])[1] if not ext else FX.split(F, want[:-1])[1]) + 1] ^= 1 << 7
    st = PW.fri_verify_pow(F, W, bad, seed)
    assert st != 0 and not st & 64 and fri_verify_dev(torch, h, bad, seed) == st
    h.close()
    pos.close()


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("ext", [False, True])
def test_fri_without_grinding_is_unchanged(torch, p, ext):
    """a handle with set_pow(0, 0), and one never set: fri_ref's (fri_ext_ref's) words and the sizes of the shape functions"""
    case, D = (9, 3, 3), 2
    F = fri_objects(p, case, D, ext)
    rng = random.Random(9)
    f = FR.evaluate(F, [rng.randrange(p) for _ in range(F.size(0) >> 1)])
    seed = [3, 4]
    want = (FX if ext else FR).prove(F, f, seed)
    pos = poseidon(p)
    for mode in ("never", "zero", "on then off"):
        h = fri_handle(pos, p, case, D, ext)
        if mode == "zero":
            h.set_pow(0, 0)
        elif mode == "on then off":
            h.set_pow(6)
            h.set_pow(0, 0)
        shape = (case[0], case[1], case[2], Q, D)
        sizes = ((L.lib.ronk_fri_proof_words_ext(*shape, 0), L.lib.ronk_fri_workspace_words_ext(*shape, 0)) if ext else
                 (L.lib.ronk_fri_proof_words(*shape), L.lib.ronk_fri_workspace_words(*shape)))
        assert (h.proof_words, h.workspace_words) == sizes == (F.proof_words(), F.workspace_words())
        assert (L.lib.ronk_fri_handle_proof_words(h.h), L.lib.ronk_fri_handle_workspace_words(h.h)) == sizes
        got, _ = fri_prove_dev(torch, h, f, seed)
        assert got.tolist() == want, (p, ext, mode)
        assert fri_verify_dev(torch, h, got, seed) == 0
        h.close()
    pos.close()


# ------------------------------------------------------------------------------------------------ (c) the batched commitment
@pytest.mark.parametrize("p,D,bits", [(GL, 2, 6), (MONT, 4, 10)])
def test_pcs_with_grinding(torch, p, D, bits):
    n, eta, log2_final, C, K = 6, 1, 2, 3, 2
    P = params(p)
    S = DR.Pcs(P, GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, C, K)
    W = PW.Pow(bits, PW.default_limit(p, bits))
    rng = random.Random(60 + D)
    coef = [[rng.randrange(p) for _ in range(S.d)] for _ in range(C)]
    zs = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(K)]
    M = DR.columns(S, coef)
    tree = DR.commit(S, M)
    seed = [3, 4, 5, 6][:D]
    want, wst = PW.pcs_open_pow(S, W, M, tree, coef, zs, seed)
    pos = poseidon(p)
    h = L.PcsHandle(pos, GEN[p], GEN[p], n, GEN[p], eta, log2_final, 1, Q, D, C, K)
    plain = (h.proof_words, h.workspace_words)
    assert plain == (S.proof_words(), S.workspace_words())
    h.set_pow(bits)
    assert (h.proof_words, h.workspace_words) == (PW.pcs_proof_words(S, W), PW.pcs_workspace_words(S, W))
    d_M = dev(torch, np.array(M, dtype=np.uint64).ravel())
    d_tree = torch.full((h.tree_words,), -1, dtype=torch.int64, device="cuda")
    h.commit_dev(d_M.data_ptr(), d_tree.data_ptr())
    d_coef, d_seed = dev(torch, np.array(coef, dtype=np.uint64).ravel()), dev(torch, seed)
    d_z = dev(torch, np.array(ER.planar(zs), dtype=np.uint64))
    d_work, d_proof = canaried(torch, h.workspace_words), canaried(torch, h.proof_words)
    d_st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    h.open_dev(d_M.data_ptr(), d_tree.data_ptr(), d_coef.data_ptr(), d_z.data_ptr(), d_seed.data_ptr(), d_work.data_ptr(), d_proof.data_ptr(),
               d_st.data_ptr())
    got, work = host(torch, d_proof), host(torch, d_work)
    assert int(d_st.item()) == wst == 0
    assert (got[h.proof_words:] == np.uint64(CANARY)).all() and (work[h.workspace_words:] == np.uint64(CANARY)).all()
    assert got[:h.proof_words].tolist() == want
    assert int(work[h.workspace_words - PW.WORK_WORDS]) != CANARY

    def verify(proof):
        d_root, d_p = dev(torch, tree.root_hash()), dev(torch, proof)
        st = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        h.verify_dev(d_root.data_ptr(), d_z.data_ptr(), d_seed.data_ptr(), d_p.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
        return int(st.item())

    assert verify(want) == 0
    off = PW.pcs_section_offsets(S, W)
    bad = list(want)
    bad[off["nonce"]] += p
    assert verify(bad) == 64 == PW.pcs_verify_pow(S, W, tree.root_hash(), zs, seed, bad)
    bad = list(want)
    bad[off["nonce"]] += 1
    st = PW.pcs_verify_pow(S, W, tree.root_hash(), zs, seed, bad)
    assert st != 0 and verify(bad) == st
    bad = list(want)
    bad[off["leaves"] + 2] ^= 1 << 9
    st = PW.pcs_verify_pow(S, W, tree.root_hash(), zs, seed, bad)
    assert st & 8 and not st & 64 and verify(bad) == st
    # switched off again: today's proof
    h.set_pow(0)
    assert (h.proof_words, h.workspace_words) == plain
    proof0, st0 = h.open(np.array(M, dtype=np.uint64).ravel(), np.array(tree.flat(), dtype=np.uint64), np.array(coef, dtype=np.uint64).ravel(),
                         np.array(ER.planar(zs), dtype=np.uint64), seed)
    assert (proof0.tolist(), st0) == DR.open_(S, M, tree, coef, zs, seed)
    h.close()
    pos.close()


# ------------------------------------------------------------------------------------------------ (d) host forms
@pytest.mark.parametrize("p", [GL, MONT])
def test_host_forms(torch, p):
    sp = (_Field(p),) + params(p).create_args()[1:]
    seed, lam, nonce = reference(p, FRI_SET, 5, 10)
    assert callers.pow_grind(sp, seed, 10) == nonce == callers.pow_grind(sp, seed, 10, log2_limit=lam, max_lanes=64)
    assert callers.pow_verify(sp, seed, 10, nonce) and not callers.pow_verify(sp, seed, 10, nonce, log2_limit=1)
    assert callers.pow_grind(sp, [], 0) == 0
    with pytest.raises(L.RonkPanic) as e:
        callers.pow_grind(sp, seed, 10, log2_limit=max(1, nonce.bit_length() - 1))     # 2^limit <= nonce: nothing below it
    assert e.value.code == L.ERR_INDEX
    case, D, bits = FRI_CASES[0]
    F, W, f, fseed, want = fri_reference(p, case, D, bits, False)
    fri = callers.Fri(sp, case[0], GEN[p], case[1], case[2], 1, Q, D, pow_bits=bits)
    proof = fri.prove(f, fseed)
    assert proof.tolist() == want and fri.verify(proof, fseed) == 0
    bad = proof.copy()
    bad[-1] += np.uint64(1)
    assert fri.verify(bad, fseed) == PW.fri_verify_pow(F, W, bad.tolist(), fseed)
    # a limit under which the restatement finds nothing: the prover's host form reports it
    roots, final = FR.split(F, want[:-1])[:2]
    u = PW.fri_transcript_pow(F, W, fseed, roots, final, want[-1])[0]
    lam = 1
    if PW.grind(F.P, u, 10, lam) == PW.NONE:
        none = callers.Fri(sp, case[0], GEN[p], case[1], case[2], 1, Q, D, pow_bits=10, pow_log2_limit=lam)
        with pytest.raises(L.RonkPanic) as e:
            none.prove(f, fseed)
        assert e.value.code == L.ERR_INDEX
