"""The transform over BN254's scalar field (csrc/fr_ntt_kernels.h) under the host fiber emulator (tests/emu/emu_fr_ntt.cpp): the
pass body on host fibers with the library's own planner and table builder, forward against the naive DFT, inverse in place
against the input's residues, the multiply's pointwise middle against the schoolbook product; rows hold r, r + 1 and
2^256 - 1.  Test infrastructure only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "emu_fr_ntt")
DEFAULT_MAX = 10      # FR_LOGR_MAX: the largest single-pass transform of the default plan


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    src = os.path.join(ROOT, "tests", "emu", "emu_fr_ntt.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("fr_ntt_kernels.h", "bn254_fr.h", "bn254_consts.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", tmp, src])
        os.replace(tmp, EXE)
    return EXE


def run(emu, log2n, cap, batch, seed):
    out = subprocess.run([emu, str(log2n), str(cap), str(batch), str(seed)], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-600:] + out.stderr[-400:]
    return last


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log2n", [0, 1, 2, 3, DEFAULT_MAX])
def test_one_pass(emu, log2n, batch):
    assert "passes=1 rows=%d," % log2n in run(emu, log2n, 0, batch, 11 + log2n)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log2n,cap,rows", [(8, 4, "4,4,"), (9, 5, "5,4,")])
def test_two_passes(emu, log2n, cap, rows, batch):
    assert "passes=2 rows=%s " % rows in run(emu, log2n, cap, batch, 23 + log2n)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log2n,cap,rows", [(12, 4, "4,4,4,"), (13, 5, "5,4,4,")])
def test_three_passes(emu, log2n, cap, rows, batch):
    assert "passes=3 rows=%s " % rows in run(emu, log2n, cap, batch, 37 + log2n)


def test_default_plan_leaves_one_pass_above_its_maximum(emu):
    """the first two-pass size of the default plan, with uneven factors"""
    assert "passes=2 rows=6,5," in run(emu, DEFAULT_MAX + 1, 0, 1, 5)
