"""The bodies of csrc/air_kernels.h compiled for the host (tests/emu/emu_air.cpp), run lane by lane over the kernel's grid with
the LDS register file as a host array, against the emulator's own `unsigned __int128` restatement (generated programs: 1 and 4096
ops, 1 and 64 constraints, 1 and 16 registers, every kind alone and all four, 8 groups and 8 extension columns, M = 2 .. 2^12,
B = 1, 2, 8, T_in absent, present and in place) and against the Python restatement tests/air_ref.py (the programs the GPU suite
runs: the PLONK quotient, the logUp pair, the Fibonacci AIR, the S-box row and seeded random trees).  Goldilocks runs its own
arithmetic, the W = 7 form and the Montgomery policy.  Test infrastructure only."""
import os
import subprocess

import numpy as np
import pytest

import air_programs as AP
import air_ref as AR
import emu_cxx
import plonk_ref as PR
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
SRC = os.path.join(ROOT, "tests", "emu", "emu_air.cpp")
DEPS = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("air_kernels.h", "plonk_kernels.h", "deep_kernels.h", "ext2_kernels.h",
                                                                 "ext2.h", "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
DEPS.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))
FIELDS = [(GL, 7, 7, 3), (GL, 7, 11, 2), (MONT, 10, 10, 1)]       # p, g, w, policies that serve it


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_air"), [SRC], DEPS)


@pytest.fixture(scope="module")
def emu_device_form():
    """the same emulator built with the HIP toolchain's clang++: the `__clang__` branches of the carry chains"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_air_clang"), [SRC], DEPS, opt="-O1")


def words(rng, size, p):
    """any 64-bit words with the edges mixed in: 0, p - 1 and values >= p"""
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    k = rng.integers(0, 8, size=size)
    v[k == 0] = np.uint64(p - 1)
    v[k == 1] = 0
    v[k == 2] = np.uint64(p) + rng.integers(0, min(5, 2**64 - p), size=int((k == 2).sum()), dtype=np.uint64)
    return v


def check(exe, tmp_path, p, g, w, policies, log2_n, log2_b, prog, groups, n_ext, n_chal, tin, seed):
    M = 1 << (log2_n + log2_b)
    rng = np.random.default_rng(seed)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, log2_n, log2_b, g)
    base, ext = [words(rng, c * M, p) for c in groups], [words(rng, 2 * M, p) for _ in range(n_ext)]
    chal, lam, T_in = words(rng, 2 * n_chal, p), words(rng, 2 * prog.n_constraints, p), words(rng, 2 * M, p)
    head = [len(groups)] + list(groups) + [0] * (8 - len(groups)) + [n_ext, n_chal, len(prog.imm), prog.n_regs, prog.n_constraints,
                                                                     len(prog.ops), tin]
    u = lambda a: np.array([int(v) % 2**64 for v in a], dtype=np.uint64)      # noqa: E731
    blob = np.concatenate([u(head), u(prog.ops), u([v % p for v in prog.imm])] + base + ext + [chal, lam] + ([T_in] if tin else []))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    blob.tofile(src)
    out = subprocess.run([exe] + [str(a) for a in (p, g, w, log2_n, log2_b, src, dst)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK") and ("results=%d" % policies) in last, out.stdout[-800:] + out.stderr[-400:]
    got = np.fromfile(dst, dtype=np.uint64).reshape(policies, 2 * M)
    columns = [col.tolist() for a, c in zip(base, groups) for col in a.reshape(c, M)]
    want = AR.quotient(E, dom, prog, columns, [a.reshape(2, M).tolist() for a in ext], AR.pairs_of(chal), AR.pairs_of(lam),
                       T_in.reshape(2, M).tolist() if tin else None)
    for r in range(policies):
        assert np.array_equal(got[r], np.array(AR.planar(want), dtype=np.uint64)), (p, w, log2_n, log2_b, "policy %d" % r)


PROGRAMS = {"plonk": (AP.plonk, (3, 5, 3, 1), 1, 2), "logup": (lambda: AP.logup(5, True), (5, 5), 1, 1),
            "logup ones": (lambda: AP.logup(2, False), (2,), 1, 1), "fibonacci": (AP.fibonacci, (3,), 0, 2), "sbox": (AP.sbox_row, (1, 2), 0, 2)}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_the_shared_programs_against_air_ref(emu, tmp_path, p, g, w, policies, name):
    """M = 2^11 and 2^12 (the first sizes of two workgroups of the two row counts), B = 2 and 8, the three T_in forms in turn"""
    make, groups, n_ext, n_chal = PROGRAMS[name]
    k = sorted(PROGRAMS).index(name)
    for j, (log2_m, log2_b) in enumerate(((11, 1), (12, 3))):
        check(emu, tmp_path, p, g, w, policies, log2_m - log2_b, log2_b, make(), groups, n_ext, n_chal, (k + j) % 3, 10 * k + j)


@pytest.mark.parametrize("variant", range(6))
@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_random_programs_against_air_ref(emu, tmp_path, p, g, w, policies, variant):
    """seeded random trees with the rotations 0, 1, -1, 2, N - 1, -(N - 1): each kind alone, all four, none of the boundary kinds;
    the registers the program needs and sixteen; M = 2^4 and 2^9"""
    kinds = [(AR.ALL,), (AR.FIRST,), (AR.LAST,), (AR.EXCEPT_LAST,), (0, 1, 2, 3), (AR.EXCEPT_LAST, AR.ALL)][variant]
    for log2_n, log2_b in ((3, 1), (7, 2)):
        N = 1 << log2_n
        rng = np.random.default_rng(100 * variant + log2_n)
        prog, _ = AP.random_program(rng, 5, 2, 3, (0, 1, -1, 2, N - 1, 1 - N), kinds, 1 + variant, depth=4, n_regs_min=16 * (variant % 2))
        check(emu, tmp_path, p, g, w, policies, log2_n, log2_b, prog, ((5,), (2, 3), (1, 1, 1, 1, 1))[variant % 3], 2, 3, variant % 3, variant)


@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_device_form_of_the_carry_chains(emu_device_form, tmp_path, p, g, w, policies):
    check(emu_device_form, tmp_path, p, g, w, policies, 4, 2, AP.plonk(), (3, 5, 3, 1), 1, 2, 1, 3)
    out = subprocess.run([emu_device_form] + [str(a) for a in (p, g, w)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("OK"), out.stdout[-800:] + out.stderr[-400:]


@pytest.mark.parametrize("p,g,w", [(GL, 7, 7), (GL, 7, 11), (MONT, 10, 10), (PC.P_MID, PC.GEN[PC.P_MID], PC.GEN[PC.P_MID]), (97, 5, 5),
                                   (17, 3, 3)])
def test_own_restatement_over_the_generated_cases(emu, p, g, w):
    """the emulator's generated programs and random inputs against its own `unsigned __int128` restatement; F_17 has the domains up
    to M = 8 only, F_97 up to M = 32"""
    out = subprocess.run([emu] + [str(a) for a in (p, g, w)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    cases = int(last.split("cases=")[1].split()[0])
    assert cases == (16 if p > 2**32 else 11 if p == 97 else 4)
