"""Multipoint evaluation and interpolation (csrc/multipoint_kernels.h) under the host fiber emulator (tests/emu/emu_multipoint.cpp):
the leaf bodies on host fibers, the window store and the combine on the oracle's level products; at every node of the walk down
the window identity W_S * A_S == rev(f mod M_S) mod z^s with the oracle's remainder, every output against the oracle's evaluate,
and the interpolant of those values against f.  Test infrastructure only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "emu_multipoint")
G = 64


def _build(cmd, out):
    """compile to a private name, then rename (pytest-xdist workers may rebuild at once)"""
    tmp = "%s.tmp.%d" % (out, os.getpid())
    subprocess.check_call(cmd[:cmd.index("-o") + 1] + [tmp] + cmd[cmd.index("-o") + 2:])
    os.replace(tmp, out)


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    src = os.path.join(ROOT, "tests", "emu", "emu_multipoint.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f)
                    for f in ("multipoint_kernels.h", "roots_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        obj = os.path.join(ROOT, "build", "orc_emu_multipoint.o")
        _build(["gcc", "-O2", "-c", "-o", obj, os.path.join(ROOT, "oracle", "ronk_oracle.c")], obj)
        _build(["g++", "-O2", "-std=c++17", "-o", EXE, src, obj], EXE)
    return EXE


def run(emu, *args, env=None):
    out = subprocess.run([emu] + [str(a) for a in args], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **env) if env else None)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-600:] + out.stderr[-400:]
    return last


def _cases():
    for m in (1, 2, G - 1, G, G + 1, 2 * G, 3 * G + 5):
        for d in sorted({1, max(1, m - 1), m, 2 * m + 3}):
            yield m, d


def test_goldilocks_distinct_nodes(emu):
    for m, d in _cases():
        assert "repeated=0" in run(emu, m, d, 0x1234 + m + d, 1)


def test_goldilocks_repeated_point_and_zero(emu):
    """points with a repeat and the point ZERO: values still exact, interpolation reports the coincident nodes"""
    for m, d in _cases():
        last = run(emu, m, d, 0x77 + m + d, 0)
        assert ("repeated=1" in last) == (m >= 5)


def test_montgomery(emu):
    env = {"RONK_EMU_P": str(0xFFFFFFFC00000001)}
    for m, d in _cases():
        run(emu, m, d, 99 + m + d, 1, env=env)
    run(emu, 3 * G + 5, 2 * (3 * G + 5) + 3, 5, 0, env=env)


def test_small_prime_single_leaf(emu):
    """F_101: one leaf, no NTT level"""
    env = {"RONK_EMU_P": "101"}
    run(emu, 50, 49, 5, 1, env=env)
    run(emu, 50, 103, 6, 1, env=env)
    run(emu, 64, 64, 7, 1, env=env)
    run(emu, 64, 131, 8, 0, env=env)
