"""The bodies of csrc/mpcs_kernels.h compiled for the host (tests/emu/emu_mpcs.cpp) against the plain `unsigned __int128 % p`
restatement in the same file: the table of a call (the alpha^j, the point records, the Y_r,k of every round and point) and the
combination of R matrices at per-matrix points as the combine kernel's lanes (four points) and the check kernel's lanes (one
point) compute it, with the on-domain status bit and the zero-inverse convention; R = 1, 2, 3, masks full, disjoint (01, 10),
nested (11, 01, 11), and K = 8 with (0xFF, 0x80).  Goldilocks runs its own arithmetic (and the W = 7 form when W = 7) and the
Montgomery policy.  Test infrastructure only."""
import os
import subprocess

import pytest

import emu_cxx
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT, SMALL = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001, 0xC0000001
P_MID = PC.P_MID
SRC = os.path.join(ROOT, "tests", "emu", "emu_mpcs.cpp")
DEPS = [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_fri.cpp", "emu_poseidon.cpp", "emu_ref.h")]
DEPS += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("mpcs_kernels.h", "deep_kernels.h", "ext2_kernels.h", "ext2.h",
                                                                  "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "emu_mpcs")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in [SRC] + DEPS):
        tmp = "%s.tmp.%d" % (exe, os.getpid())   # pytest-xdist workers may rebuild at once
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", tmp, SRC])
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def emu_device_form(emu):
    """the same emulator built with the HIP toolchain's clang++: mont64.h's `__clang__` branches, the device form of the carry
    chains (g++ compiles the portable form only)"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_mpcs_clang"), [SRC], DEPS)


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last


@pytest.mark.parametrize("p,g,w,policies", [(GL, 7, 7, 7), (GL, 7, 11, 5), (MONT, 10, 10, 4), (SMALL, 5, 5, 4)])
def test_bodies_against_restatement(emu, p, g, w, policies):
    """policies: 1 Goldilocks, 2 its W = 7 form, 4 Montgomery"""
    assert ("policies=%d" % policies) in run(emu, p, g, w)


def test_p_mid_portable_form(emu):
    assert "policies=4" in run(emu, P_MID, PC.GEN[P_MID], PC.GEN[P_MID])


@pytest.mark.parametrize("p,g,w,policies", [(GL, 7, 7, 7), (MONT, 10, 10, 4)])
def test_device_form_of_the_carry_chains(emu_device_form, p, g, w, policies):
    assert ("policies=%d" % policies) in run(emu_device_form, p, g, w)
