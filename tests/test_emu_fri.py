"""The FRI bodies of csrc/fri_kernels.h compiled for the host (tests/emu/emu_fri.cpp) against the plain `unsigned __int128 % p`
restatement in the same file: the fold of every arity on every layer of a chain (inputs 0, p - 1 and >= p; beta 0, 1, p - 1 and
>= p; shifts 1, g, p - 1), the transcript in one go and layer by layer, the query indices, the verifier's per-query check on an honest
and on a tampered proof, and the final-degree sum.  Goldilocks under g = 7 runs the shift roots and the Montgomery policy; another
generator must fall back to the Montgomery policy.  Test infrastructure only."""
import os
import subprocess

import pytest

import emu_cxx
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT, SMALL = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001, 0xC0000001
P_MID = PC.P_MID     # sums take every outcome of mont64::add's select (tests/prime_classes.py); MONT all but never has p <= s < 2^64


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "emu_fri")
    src = os.path.join(ROOT, "tests", "emu", "emu_fri.cpp")
    deps = [src, os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp"),
            os.path.join(ROOT, "tests", "emu", "emu_ref.h")]
    deps += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("fri_kernels.h", "poseidon_kernels.h", "field_policy.h", "gl64.h",
                                                                     "mont64.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = "%s.tmp.%d" % (exe, os.getpid())   # pytest-xdist workers may rebuild at once
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", tmp, src])
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def emu_device_form(emu):
    """the same emulator built with the HIP toolchain's clang++: mont64.h's `__clang__` branches, the device form of the carry
    chains (g++ compiles the portable form only)"""
    src = os.path.join(ROOT, "tests", "emu", "emu_fri.cpp")
    deps = [os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp"),
            os.path.join(ROOT, "tests", "emu", "emu_ref.h")]
    deps += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("fri_kernels.h", "poseidon_kernels.h", "field_policy.h", "gl64.h",
                                                                     "mont64.h")]
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_fri_clang"), [src], deps)


def run(exe, p, g):
    out = subprocess.run([exe, str(p), str(g)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last


@pytest.mark.parametrize("p,g", [(GL, 7), (MONT, 10), (SMALL, 5)])
def test_bodies_against_restatement(emu, p, g):
    assert ("shift_policy=%d" % (p == GL)) in run(emu, p, g)


def test_p_mid_portable_form(emu):
    assert "shift_policy=0" in run(emu, P_MID, PC.GEN[P_MID])


@pytest.mark.parametrize("p,g", [(GL, 7), (MONT, 10), (P_MID, 7), (PC.P_62, 3)])
def test_device_form_of_the_carry_chains(emu_device_form, p, g):
    assert ("shift_policy=%d" % (p == GL)) in run(emu_device_form, p, g)


def test_goldilocks_under_another_generator(emu):
    """w_8 is then no power of two: the handle must choose the Montgomery policy, and that policy computes the same function"""
    assert "shift_policy=0" in run(emu, GL, 11)
