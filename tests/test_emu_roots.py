"""The product tree of ronk_poly_from_roots (csrc/roots_kernels.h) under the host fiber emulator (tests/emu/emu_roots.cpp): the
leaf body on host fibers, the level combine on the oracle's pair products, every node against the oracle's chain of products of
linear factors, the monic combine identity at each level boundary.  Test infrastructure only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "emu_roots")


def _build(cmd, out):
    """compile to a private name, then rename (pytest-xdist workers may rebuild at once)"""
    tmp = "%s.tmp.%d" % (out, os.getpid())
    subprocess.check_call(cmd[:cmd.index("-o") + 1] + [tmp] + cmd[cmd.index("-o") + 2:])
    os.replace(tmp, out)


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    src = os.path.join(ROOT, "tests", "emu", "emu_roots.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("roots_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        obj = os.path.join(ROOT, "build", "orc_emu_roots.o")
        _build(["gcc", "-O2", "-c", "-o", obj, os.path.join(ROOT, "oracle", "ronk_oracle.c")], obj)
        _build(["g++", "-O2", "-std=c++17", "-o", EXE, src, obj], EXE)
    return EXE


def run(emu, *args, env=None):
    out = subprocess.run([emu] + [str(a) for a in args], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **env) if env else None)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-600:] + out.stderr[-400:]
    return last


def _counts(G):
    return [1, 2, G - 1, G, G + 1, 2 * G, 3 * G + 5]


@pytest.mark.parametrize("G", [64, 128])
def test_tree_goldilocks(emu, G):
    for m in _counts(G):
        assert "m=%d " % m in run(emu, m, G, 0x1234 + m)


@pytest.mark.parametrize("G", [64])
def test_tree_montgomery(emu, G):
    env = {"RONK_EMU_P": str(0xFFFFFFFC00000001)}
    for m in _counts(G):
        run(emu, m, G, 77 + m, env=env)


def test_tree_small_prime_single_leaf(emu):
    """F_101: one leaf covers m <= G for any odd prime (no NTT level)"""
    run(emu, 50, 64, 5, env={"RONK_EMU_P": "101"})
    run(emu, 64, 64, 6, env={"RONK_EMU_P": "101"})
