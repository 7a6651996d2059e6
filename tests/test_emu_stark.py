"""The bodies of csrc/stark_kernels.h compiled for the host (tests/emu/emu_stark.cpp) and run lane by lane against the emulator's
own `unsigned __int128` restatement: the quotient split and the coset scaling at M = 2 .. 2^12 with B = 1, 2, 8, the shift s = g and
an s of order two, words >= p among the inputs, grids in which a lane owns one residue and several; the weights, the points, and
(fields above 2^32) the transcript steps against the sponge restatement.  Goldilocks runs its own arithmetic, the W = 7 form and
the Montgomery policy; F_17 and F_97 run the Montgomery policy at every size.  Test infrastructure only."""
import os
import subprocess

import pytest

import emu_cxx
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
SRC = os.path.join(ROOT, "tests", "emu", "emu_stark.cpp")
DEPS = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("stark_kernels.h", "ext2_kernels.h", "ext2.h", "fri_kernels.h",
                                                                 "poseidon_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
DEPS += [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_ref.h", "emu_fri.cpp", "emu_poseidon.cpp")]
SIZES = 12 * 3 - 2        # log2 M = 1 .. 12 with log2 B in (0, 1, 3) where B <= M
# p, g, the policies that serve the field
FIELDS = [(GL, 7, 3), (GL, 11, 2), (MONT, 10, 1), (PC.P_MID, PC.GEN[PC.P_MID], 1), (97, 5, 1), (17, 3, 1)]


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_stark"), [SRC], DEPS)


@pytest.fixture(scope="module")
def emu_device_form():
    """the same emulator built with the HIP toolchain's clang++: the `__clang__` branches of the carry chains"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_stark_clang"), [SRC], DEPS, opt="-O1")


def run(exe, p, g, policies):
    out = subprocess.run([exe, str(p), str(g)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    assert "policies=%d " % policies in last and int(last.split("cases=")[1]) == 2 * SIZES * policies, last


@pytest.mark.parametrize("p,g,policies", FIELDS)
def test_split_shift_and_transcript_bodies(emu, p, g, policies):
    run(emu, p, g, policies)


@pytest.mark.parametrize("p,g,policies", [FIELDS[0], FIELDS[2], FIELDS[5]])
def test_device_form_of_the_carry_chains(emu_device_form, p, g, policies):
    run(emu_device_form, p, g, policies)
