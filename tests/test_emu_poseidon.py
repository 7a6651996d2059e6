"""The Poseidon, sponge and Merkle bodies of csrc/poseidon_kernels.h compiled for the host (tests/emu/emu_poseidon.cpp) against the
plain `unsigned __int128 % p` restatement in the same file: Goldilocks, a Montgomery prime above 2^63 and F_101; the register widths
and their zero padding; the fixed and the generic s-box; inputs p - 1, 0 and >= p; and the accumulator's worst case, an all-(p - 1)
state under an all-(p - 1) matrix, which is what the three-word bound rests on.  Test infrastructure only."""
import os
import subprocess

import pytest

import emu_cxx
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT, F101 = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001, 101
P_MID = PC.P_MID     # sums take every outcome of the conditional subtractions (tests/prime_classes.py); MONT all but never has p <= s < 2^64


def _build(cmd, out):
    """compile to a private name, then rename (pytest-xdist workers may rebuild at once)"""
    tmp = "%s.tmp.%d" % (out, os.getpid())
    subprocess.check_call(cmd[:cmd.index("-o") + 1] + [tmp] + cmd[cmd.index("-o") + 2:])
    os.replace(tmp, out)


def _exe(name, flags):
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", name)
    src = os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("poseidon_kernels.h", "gl64.h", "mont64.h")]
    deps.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        _build(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, src], exe)
    return exe


@pytest.fixture(scope="module")
def emu():
    return _exe("emu_poseidon", [])


@pytest.fixture(scope="module")
def emu_eager():
    return _exe("emu_poseidon_eager", ["-DRONK_POSEIDON_LAZY=0"])


@pytest.fixture(scope="module")
def emu_device_form(emu):
    """the same emulator built with the HIP toolchain's clang++: mont64.h's and poseidon_kernels.h's `__clang__` branches, the device form of the carry
    chains (g++ compiles the portable form only)"""
    src = os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp")
    deps = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("poseidon_kernels.h", "gl64.h", "mont64.h")]
    deps.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_poseidon_clang"), [src], deps, opt="-O1")   # 4 s a run at -O0


def run(exe, p, width, alpha, num_p, num_f, rate, seed):
    out = subprocess.run([exe] + [str(a) for a in (p, width, alpha, num_p, num_f, rate, seed)], capture_output=True, text=True,
                         timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last


@pytest.mark.parametrize("p", [GL, MONT, F101])
@pytest.mark.parametrize("width", [2, 3, 8, 12, 16])
def test_widths_and_alphas(emu, p, width):
    for k, alpha in enumerate((3, 5, 7, 11)):
        rate = (1, width - 1, max(1, width // 2), max(1, width - 4))[k] if width > 2 else 1
        assert "width=%d " % width in run(emu, p, width, alpha, 3 + k, 4 + (k & 1), rate, 100 * width + alpha)


def test_round_shape_of_the_reference_vector(emu):
    """width 16, alpha 3, 8 full and 11 partial rounds (the shape of the F_101 instance), and a width-12 shape with 8 + 22"""
    for p in (GL, MONT, F101):
        run(emu, p, 16, 3, 11, 8, 15, 7)
        run(emu, p, 12, 7, 22, 8, 8, 8)


def test_alpha_one_and_large_alpha(emu):
    run(emu, GL, 5, 1, 2, 2, 2, 3)
    run(emu, MONT, 5, 65537, 2, 2, 3, 4)
    run(emu, GL, 4, 0xFFFFFFFF00000000 - 1, 1, 2, 3, 5)


@pytest.mark.parametrize("p", [GL, MONT, F101])
def test_reduce_after_every_product_form(emu_eager, p):
    """the build-time alternative (RONK_POSEIDON_LAZY=0) computes the same function"""
    assert "lazy=0" in run(emu_eager, p, 12, 7, 5, 4, 8, 21)
    assert "lazy=0" in run(emu_eager, p, 3, 5, 2, 3, 1, 22)


def test_p_mid_portable_form(emu):
    """width 16: the lazy accumulator holds its maximum of 16 products"""
    run(emu, P_MID, 16, 3, 11, 8, 15, 7)
    run(emu, P_MID, 2, 7, 3, 4, 1, 8)


@pytest.mark.parametrize("p", [GL, MONT, P_MID, PC.P_62])
def test_device_form_of_the_carry_chains(emu_device_form, p):
    """PosGl::acc_mad's four-limb chain and PosMont::acc_mad's conditional subtraction as the device compiles them"""
    run(emu_device_form, p, 16, 3, 11, 8, 15, 7)
    run(emu_device_form, p, 12, 7, 5, 4, 8, 21)
    run(emu_device_form, p, 2, 7, 3, 4, 1, 8)
