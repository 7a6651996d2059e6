"""The bodies of csrc/accum_kernels.h compiled for the host (tests/emu/emu_accum.cpp), run lane by lane, against the plain
`unsigned __int128 % p` restatement in the same file: the three phases of the scans over base words and pairs at sizes that cross
every lane (8), wavefront (512) and workgroup (2048) boundary and the point where phase 2 gives a lane two totals, the chunk
inversion with a zero in the first, a middle and the last slot and two zeros in one chunk, and the permutation and logUp terms.
Goldilocks runs its own arithmetic (and the W = 7 form when W = 7) and the Montgomery policy.  Test infrastructure only."""
import os
import subprocess

import pytest

import emu_cxx
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT, SMALL = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001, 0xC0000001
P_MID = PC.P_MID
SRC = os.path.join(ROOT, "tests", "emu", "emu_accum.cpp")
DEPS = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("accum_kernels.h", "deep_kernels.h", "ext2_kernels.h", "ext2.h",
                                                                 "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
DEPS.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_accum"), [SRC], DEPS)


@pytest.fixture(scope="module")
def emu_device_form():
    """the same emulator built with the HIP toolchain's clang++: the `__clang__` branches of the carry chains"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_accum_clang"), [SRC], DEPS, opt="-O1")


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last


@pytest.mark.parametrize("p,w,policies", [(GL, 7, 7), (GL, 11, 5), (MONT, 10, 4), (SMALL, 5, 4), (P_MID, PC.GEN[P_MID], 4),
                                          (PC.P_62, PC.GEN[PC.P_62], 4), (17, 3, 4)])
def test_bodies_against_restatement(emu, p, w, policies):
    """policies: 1 Goldilocks, 2 its W = 7 form, 4 Montgomery"""
    assert ("policies=%d" % policies) in run(emu, p, w)


@pytest.mark.parametrize("p,w,policies", [(GL, 7, 7), (MONT, 10, 4), (P_MID, 7, 4), (PC.P_62, 3, 4), (17, 3, 4)])
def test_device_form_of_the_carry_chains(emu_device_form, p, w, policies):
    assert ("policies=%d" % policies) in run(emu_device_form, p, w)
