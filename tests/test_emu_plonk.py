"""The bodies of csrc/plonk_kernels.h compiled for the host (tests/emu/emu_plonk.cpp), run lane by lane over the kernel's grid,
against the Python restatement tests/plonk_ref.py: Goldilocks with w = 7 and w = 11 (its own arithmetic, the W = 7 form, and the
Montgomery policy over the same prime) and MONT_P; M = 2^4, 2^11 and 2^12, B = 2 and 8, with and without the public-input
column.  A lane owns the rows i + t M / R, R = 4 over Goldilocks and 8 over a Montgomery prime, and a workgroup 256 lanes: one
workgroup's row set is the whole array up to M = 2^10 (2^11), and M = 2^11 (2^12) is the first size at which it is not.  Test
infrastructure only."""
import os
import subprocess

import numpy as np
import pytest

import emu_cxx
import plonk_ref as PR
import prime_classes as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
SRC = os.path.join(ROOT, "tests", "emu", "emu_plonk.cpp")
DEPS = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("plonk_kernels.h", "deep_kernels.h", "ext2_kernels.h", "ext2.h",
                                                                 "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
DEPS.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))
FIELDS = [(GL, 7, 7, 3), (GL, 7, 11, 2), (MONT, 10, 10, 1)]       # p, g, w, policies that serve it
LANES, ROWS_GL, ROWS_MONT = 256, 4, 8
FIRST_TWO_WORKGROUPS = (11, 12)                                  # log2 of the first M with more than LANES * rows rows, per policy
assert tuple(1 << m for m in FIRST_TWO_WORKGROUPS) == (2 * LANES * ROWS_GL, 2 * LANES * ROWS_MONT)


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_plonk"), [SRC], DEPS)


@pytest.fixture(scope="module")
def emu_device_form():
    """the same emulator built with the HIP toolchain's clang++: the `__clang__` branches of the carry chains"""
    return emu_cxx.build_device_form(os.path.join(ROOT, "build", "emu_plonk_clang"), [SRC], DEPS, opt="-O1")


def words(rng, size, p):
    """any 64-bit words with the edges mixed in: 0, p - 1 and values >= p"""
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    k = rng.integers(0, 8, size=size)
    v[k == 0] = np.uint64(p - 1)
    v[k == 1] = 0
    v[k == 2] = np.uint64(p) + rng.integers(0, min(5, 2**64 - p), size=int((k == 2).sum()), dtype=np.uint64)
    return v


def run(exe, args, tmp_path, blob, M):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    blob.tofile(src)
    out = subprocess.run([exe] + [str(a) for a in args] + [src, dst], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last, np.fromfile(dst, dtype=np.uint64).reshape(-1, 2 * M)


def check(exe, tmp_path, p, g, w, policies, log2_m, log2_b, with_pi):
    M = 1 << log2_m
    rng = np.random.default_rng(log2_m * 100 + log2_b * 10 + with_pi)
    E = PR.Ext2(p, w)
    dom = PR.Domain(p, g, log2_m - log2_b, log2_b, g)
    wires, sel, sigma, pi, Z = (words(rng, k * M, p) for k in (3, 5, 3, 1, 2))
    ch = words(rng, 6, p)
    parts = [wires, sel, sigma] + ([pi] if with_pi else []) + [Z, ch]
    last, got = run(exe, (p, g, w, log2_m - log2_b, log2_b, g, int(with_pi)), tmp_path, np.concatenate(parts), M)
    assert got.shape[0] == policies and ("results=%d" % policies) in last
    cols = PR.Columns(wires.reshape(3, M).tolist(), sel.reshape(5, M).tolist(), sigma.reshape(3, M).tolist(),
                      pi.tolist() if with_pi else None, Z.reshape(2, M).tolist())
    want = np.array(PR.planar(PR.quotient(E, dom, cols, ch[0:2].tolist(), ch[2:4].tolist(), ch[4:6].tolist())), dtype=np.uint64)
    for r in range(policies):
        assert np.array_equal(got[r], want), (p, w, log2_m, log2_b, with_pi, "policy %d" % r)


@pytest.mark.parametrize("with_pi", [False, True])
@pytest.mark.parametrize("log2_b", [1, 3])
@pytest.mark.parametrize("log2_m", (4,) + FIRST_TWO_WORKGROUPS)
@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_bodies_against_plonk_ref(emu, tmp_path, p, g, w, policies, log2_m, log2_b, with_pi):
    check(emu, tmp_path, p, g, w, policies, log2_m, log2_b, with_pi)


@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_device_form_of_the_carry_chains(emu_device_form, tmp_path, p, g, w, policies):
    check(emu_device_form, tmp_path, p, g, w, policies, 6, 2, True)


@pytest.mark.parametrize("p,g,w", [(GL, 7, 7), (MONT, 10, 10), (PC.P_MID, PC.GEN[PC.P_MID], PC.GEN[PC.P_MID]), (97, 5, 5)])
def test_own_restatement_and_the_smallest_shapes(emu, p, g, w):
    """the emulator's random inputs against its own `unsigned __int128` restatement: M = 2 (one row per lane), M = 4 and 8"""
    for log2_n, log2_b in ((1, 0), (1, 1), (2, 1), (1, 2)):
        out = subprocess.run([emu] + [str(a) for a in (p, g, w, log2_n, log2_b, g, 1)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
