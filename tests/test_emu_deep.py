"""The bodies that ronk_pcs_* runs (csrc/deep_kernels.h and the one-round case of csrc/mpcs_kernels.h) compiled for the host
(tests/emu/emu_deep.cpp) against the plain `unsigned __int128 % p`
restatement in the same file: the table of a call, the DEEP combination as the combine kernel's lanes (four points) and as the
check kernel's lanes (one point) compute it, the on-domain status bit and the zero-inverse convention, and the evaluation at
extension points, for K = 1, 2, 3, 8 points.  Goldilocks runs its own arithmetic (and the W = 7 form when W = 7) and the Montgomery
policy.  Test infrastructure only."""
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
    exe = os.path.join(ROOT, "build", "emu_deep")
    src = os.path.join(ROOT, "tests", "emu", "emu_deep.cpp")
    deps = [src, os.path.join(ROOT, "tests", "emu", "emu_fri.cpp"), os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp"),
            os.path.join(ROOT, "tests", "emu", "emu_ref.h")]
    deps += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("deep_kernels.h", "mpcs_kernels.h", "ext2_kernels.h", "ext2.h",
                                                                     "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = "%s.tmp.%d" % (exe, os.getpid())   # pytest-xdist workers may rebuild at once
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", tmp, src])
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def emu_device_form(emu):
    """the same emulator built with the HIP toolchain's clang++: mont64.h's `__clang__` branches, the device form of the carry
    chains (g++ compiles the portable form only)"""
    src = os.path.join(ROOT, "tests", "emu", "emu_deep.cpp")
    deps = [os.path.join(ROOT, "tests", "emu", "emu_fri.cpp"), os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp"),
            os.path.join(ROOT, "tests", "emu", "emu_ref.h")]
    deps += [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("deep_kernels.h", "mpcs_kernels.h", "ext2_kernels.h", "ext2.h",
                                                                     "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_deep_clang"), [src], deps)


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


@pytest.mark.parametrize("p,g,w,policies", [(GL, 7, 7, 7), (MONT, 10, 10, 4), (P_MID, 7, 7, 4), (PC.P_62, 3, 3, 4)])
def test_device_form_of_the_carry_chains(emu_device_form, p, g, w, policies):
    assert ("policies=%d" % policies) in run(emu_device_form, p, g, w)
