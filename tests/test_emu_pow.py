"""The proof-of-work bodies of csrc/pow_kernels.h compiled for the host (tests/emu/emu_pow.cpp) and run over the search kernel's
grid for T lanes in three execution orders -- every lane to completion in forward order, in reverse order, and all lanes stepped
round-robin one candidate at a time -- against the Python restatement (tests/pow_ref.py): the nonce must be the restatement's in
every order.  The emulator derives the Poseidon constants of poseidon_ref.derive_params itself, and also compares with a sequential
search on the `unsigned __int128 % p` sponge of emu_poseidon.cpp.  Test infrastructure only."""
import os
import random
import subprocess

import pytest

import emu_cxx
import poseidon_ref as PR
import pow_ref as PW
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT, P_MID = PR.GOLDILOCKS, PR.MONT_P, PC.P_MID
FIELDS = [GL, MONT, P_MID]
SEED_LENS = [0, 1, 3, 4, 5, 8, 11]    # rate 4: every seed_len mod rate that matters, and 0, 1 and 2 prefix permutations
BITS = [0, 1, 6, 10]
LANES = [64, 256, 512]
# (width, alpha, num_p, num_f, rate): the FRI tests' set, then the other register widths; width 3 and 16 have rate = width - 1
FRI_SET = (8, 7, 2, 4, 4)
OTHER_SETS = [(3, 7, 2, 4, 2), (12, 7, 2, 4, 8), (16, 7, 2, 4, 15)]
DEPS = [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_pow.cpp", "emu_poseidon.cpp", "emu_ref.h")]
DEPS += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("pow_kernels.h", "poseidon_kernels.h", "gl64.h", "mont64.h")]


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_pow"), DEPS[:1], DEPS[1:])


@pytest.fixture(scope="module")
def emu_device_form():
    """the same emulator built with the HIP toolchain's clang++: the `__clang__` carry chains, the form the device compiles"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_pow_clang"), DEPS[:1], DEPS[1:], opt="-O1")


def run(exe, p, pset, bits, log2_limit, T, seed):
    out = subprocess.run([exe, str(p)] + [str(v) for v in pset] + [str(bits), str(log2_limit), str(T)] + [str(v) for v in seed],
                         capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK nonce="), out.stdout[-800:] + out.stderr[-400:]
    return int(last.split()[1].split("=")[1])


_REF = {}


def draw_seed(p, pset, seed_len):
    rng = random.Random(p % 1009 + 31 * pset[0] + seed_len)
    return [rng.randrange(p) for _ in range(seed_len)]


def reference(p, pset, seed_len, bits):
    """(seed, log2_limit, the restatement's nonce), computed once"""
    key = (p, pset, seed_len, bits)
    if key not in _REF:
        seed = draw_seed(p, pset, seed_len)
        lam = PW.default_limit(p, bits)
        _REF[key] = (seed, lam, PW.grind(PR.derive_params(p, *pset), seed, bits, lam))
    return _REF[key]


def check(exe, p, pset, seed_len, bits, lanes):
    seed, lam, want = reference(p, pset, seed_len, bits)
    assert want != PW.NONE
    for T in lanes:
        assert run(exe, p, pset, bits, lam, T, seed) == want, (p, pset, seed_len, bits, T)
    return want


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("seed_len", SEED_LENS)
def test_nonce_in_every_order(emu, p, seed_len):
    for bits in BITS:
        want = check(emu, p, FRI_SET, seed_len, bits, LANES)
        assert bits or want == 0


@pytest.mark.parametrize("p", FIELDS)
def test_later_strides_are_reached(emu, p):
    """with T = 512 some b = 10 nonce lies in the third stride or later, so a lane's second and third candidates, and the second
    workgroup, decide the result"""
    nonces = [reference(p, FRI_SET, seed_len, 10)[2] for seed_len in SEED_LENS]
    assert max(nonces) >= 2 * 512, nonces
    assert all(n < (1 << 16) for n in nonces)


@pytest.mark.parametrize("p", [GL, MONT])
@pytest.mark.parametrize("pset", OTHER_SETS)
def test_other_register_widths(emu, p, pset):
    rate = pset[4]
    for seed_len in (1, rate, rate + 1):
        for bits in (1, 10):
            check(emu, p, pset, seed_len, bits, (64, 512))


@pytest.mark.parametrize("p", FIELDS)
def test_not_found(emu, p):
    """b = 10 below 2^4: nothing, whatever the order; T above the limit leaves the lanes past it idle"""
    P = PR.derive_params(p, *FRI_SET)
    rng = random.Random(p % 1009)
    while True:
        seed = [rng.randrange(p) for _ in range(2)]
        if PW.grind(P, seed, 10, 4) == PW.NONE:
            break
    for T in (16, 64):
        assert run(emu, p, FRI_SET, 10, 4, T, seed) == PW.NONE


@pytest.mark.parametrize("p,pset", [(GL, FRI_SET), (MONT, FRI_SET), (P_MID, (12, 7, 2, 4, 8))])
def test_device_form_of_the_carry_chains(emu_device_form, p, pset):
    check(emu_device_form, p, pset, 5, 10, (256,))
    check(emu_device_form, p, pset, 4, 6, (64,))
