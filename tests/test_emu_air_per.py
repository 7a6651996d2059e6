"""The bodies of csrc/air_kernels.h with periodic columns compiled for the host (tests/emu/emu_air_per.cpp): the kernel's grid lane
by lane, the tables air_per_build makes, against the Python restatement tests/air_per_ref.py word for word and against the
emulator's own direct evaluation.  Sizes M = 2, 4, 8 (one row per lane), 2^6 (four or eight rows per lane) and 2^12 (more than one
workgroup); tables with P B < M and P B = M; rotations whose rot B crosses a table's end in both directions; values at and above
p; Goldilocks on its own arithmetic, the W = 7 form and the Montgomery policy, and the small fields F_17 and F_97.  With no
periodic column the output is that of tests/emu/emu_air.cpp on every program of tests/air_programs.py.  Test infrastructure only."""
import os
import subprocess

import numpy as np
import pytest

import air_per_ref as APR
import air_ref as AR
import emu_cxx
import plonk_ref as PR
import prime_classes as PC
import stark_fixed_programs as FP
from ronkathon_amd.air import ALL, EXCEPT_LAST, FIRST, LAST, AirBuilder
from test_emu_air import DEPS as AIR_DEPS
from test_emu_air import PROGRAMS, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
SRC = os.path.join(ROOT, "tests", "emu", "emu_air_per.cpp")
OLD = os.path.join(ROOT, "tests", "emu", "emu_air.cpp")
FIELDS = [(GL, 7, 7, 3), (GL, 7, 11, 2), (MONT, 10, 10, 1), (97, 5, 5, 1), (17, 3, 3, 1)]       # p, g, w, policies that serve it


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_air_per"), [SRC], AIR_DEPS)


@pytest.fixture(scope="module")
def emu_old():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_air"), [OLD], AIR_DEPS)


def run(exe, tmp_path, p, g, w, policies, log2_n, log2_b, prog, groups, n_ext, n_chal, tin, seed, periodic=None):
    """-> (the T of every policy, the inputs); periodic None: the header of emu_air.cpp, for the emulator without periodic columns"""
    M = 1 << (log2_n + log2_b)
    rng = np.random.default_rng(seed)
    base, ext = [words(rng, c * M, p) for c in groups], [words(rng, 2 * M, p) for _ in range(n_ext)]
    chal, lam, T_in = words(rng, 2 * n_chal, p), words(rng, 2 * prog.n_constraints, p), words(rng, 2 * M, p)
    head = [len(groups)] + list(groups) + [0] * (8 - len(groups)) + [n_ext, n_chal, len(prog.imm), prog.n_regs, prog.n_constraints,
                                                                     len(prog.ops), tin]
    per = []
    if periodic is not None:
        head += [len(periodic)] + [APR.log2(len(v)) for v in periodic] + [0] * (16 - len(periodic))
        per = [int(v) for vals in periodic for v in vals]
    u = lambda a: np.array([int(v) % 2**64 for v in a], dtype=np.uint64)      # noqa: E731
    blob = np.concatenate([u(head), u(prog.ops), u([v % p for v in prog.imm]), u(per)] + base + ext + [chal, lam] + ([T_in] if tin else []))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    blob.tofile(src)
    out = subprocess.run([exe] + [str(a) for a in (p, g, w, log2_n, log2_b, src, dst)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK") and ("results=%d" % policies) in last, out.stdout[-800:] + out.stderr[-400:]
    return np.fromfile(dst, dtype=np.uint64).reshape(policies, 2 * M), (base, ext, chal, lam, T_in)


def check(exe, tmp_path, p, g, w, policies, log2_n, log2_b, prog, groups, n_ext, n_chal, tin, seed, periodic):
    M = 1 << (log2_n + log2_b)
    got, (base, ext, chal, lam, T_in) = run(exe, tmp_path, p, g, w, policies, log2_n, log2_b, prog, groups, n_ext, n_chal, tin, seed, periodic)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, log2_n, log2_b, g)
    columns = [col.tolist() for a, c in zip(base, groups) for col in a.reshape(c, M)]
    want = APR.quotient(E, dom, prog, columns, [a.reshape(2, M).tolist() for a in ext], AR.pairs_of(chal), AR.pairs_of(lam), periodic,
                        T_in.reshape(2, M).tolist() if tin else None)
    for r in range(policies):
        assert np.array_equal(got[r], np.array(AR.planar(want), dtype=np.uint64)), (p, w, log2_n, log2_b, "policy %d" % r)


def periodic_program(n_per, rots):
    """two base columns, one extension column, one challenge; every periodic column at every rotation, in products and sums with
    the columns, under the four kinds"""
    b = AirBuilder()
    acc, mixed = b.base(0), b.ext(0, rot=rots[-1])
    for k in range(n_per):
        for r in rots:
            acc = acc * b.periodic(k, r) + b.base(1, rot=r)
            mixed = mixed * b.periodic(k, -r if r else 0) - b.periodic((k + 1) % n_per, r)
    b.constrain(acc, ALL)
    b.constrain(mixed + b.chal(0), EXCEPT_LAST)
    b.constrain(b.periodic(0) * b.x - b.base(0), FIRST)
    b.constrain(b.periodic(n_per - 1, rots[1 % len(rots)]), LAST)
    return AR.Program(*b.assemble())


def edge_values(p, P, seed):
    """values with the edges mixed in: 0, p - 1, words at and above p"""
    rng = np.random.default_rng(seed)
    return [int(v) for v in words(rng, P, p)]


# (log2_n, log2_b): M = 2, 4, 8, 2^6, 2^12, 2^12
SHAPES = [(1, 0), (1, 1), (2, 1), (4, 2), (10, 2), (9, 3)]


# F_17 has the domains up to M = 8 only, F_97 up to M = 32
@pytest.mark.parametrize("p,g,w,policies,shape", [f + (s,) for f in FIELDS for s in SHAPES if (f[0] - 1) % (1 << sum(s)) == 0])
def test_periodic_programs_against_air_per_ref(emu, tmp_path, p, g, w, policies, shape):
    """periods 1, 2, N / 2 and N where they differ, so that P B < M and P B = M both occur; rot B crosses the end of every table
    shorter than M in both directions"""
    log2_n, log2_b = shape
    N = 1 << log2_n
    periods = sorted({1, min(2, N), max(1, N // 2), N})
    rots = sorted({0, 1 % N, -(1 % N), N - 1, 1 - N}, key=lambda r: (abs(r), r))
    periodic = [edge_values(p, P, 31 * P + log2_n) for P in periods]
    prog = periodic_program(len(periods), rots if log2_n < 9 else rots[:3])
    check(emu, tmp_path, p, g, w, policies, log2_n, log2_b, prog, (2,), 1, 1, (log2_n + log2_b) % 3, log2_n, periodic)


@pytest.mark.parametrize("p,g,w,policies", FIELDS[:3])
def test_sbox_periodic_against_air_per_ref(emu, tmp_path, p, g, w, policies):
    """the shared instance's program: three columns of period 8 at rot 0 and one read at rot 1, N = 8 (P = N) and N = 2^6"""
    for log2_n, log2_b, tin in ((3, 3, 0), (6, 3, 2)):
        inst = FP.sbox_periodic(p, 1 << log2_n)
        check(emu, tmp_path, p, g, w, policies, log2_n, log2_b, inst.shape.prog, (3,), 0, 2, tin, 5, inst.shape.periodic)


@pytest.mark.parametrize("name", sorted(PROGRAMS))
@pytest.mark.parametrize("p,g,w,policies", FIELDS[:3])
def test_without_periodic_columns_it_is_the_old_emulator(emu, emu_old, tmp_path, p, g, w, policies, name):
    """every program of tests/air_programs.py through the new form of the handle with n_per = 0: the words of the old one"""
    make, groups, n_ext, n_chal = PROGRAMS[name]
    k = sorted(PROGRAMS).index(name)
    for j, (log2_m, log2_b) in enumerate(((6, 1), (12, 3))):
        args = (tmp_path, p, g, w, policies, log2_m - log2_b, log2_b, make(), groups, n_ext, n_chal, (k + j) % 3, 10 * k + j)
        new, _ = run(emu, *args, periodic=[])
        old, _ = run(emu_old, *args)
        assert np.array_equal(new, old), (name, log2_m)


@pytest.mark.parametrize("p,g,w", [(GL, 7, 7), (GL, 7, 11), (MONT, 10, 10), (PC.P_MID, PC.GEN[PC.P_MID], PC.GEN[PC.P_MID]), (97, 5, 5),
                                   (17, 3, 3)])
def test_own_restatement_over_the_generated_cases(emu, p, g, w):
    """the emulator's generated programs (sixteen periodic columns among them) against its own direct evaluation of q(x^(N/P)), and
    the check's codes in their order; F_17 has the domains up to M = 8 only, F_97 up to M = 32"""
    out = subprocess.run([emu] + [str(a) for a in (p, g, w)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    cases = int(last.split("cases=")[1].split()[0])
    assert cases == (12 if p > 2**32 else 6 if p == 97 else 5)
