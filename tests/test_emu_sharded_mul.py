"""The sharded polynomial multiply (ronk_dist.hip ronk_poly_mul_sharded_dev) under the host fiber emulator
(tests/emu/emu_sharded_mul.cpp): all W ranks in one process, exchanges as memcpy, the fused middle (ntt_mul.h mul_mid_body with
the dist instantiation's arguments) and the composed one run on host fibers, every coefficient against the oracle, plus the
swapped-split layout argument.  Test infrastructure only: the product library does not contain the emulator."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "emu_sharded_mul")


def _build(cmd, out):
    """compile to a private name, then rename (pytest-xdist workers may rebuild at once; a binary being written cannot run)"""
    tmp = "%s.tmp.%d" % (out, os.getpid())
    subprocess.check_call(cmd[:cmd.index("-o") + 1] + [tmp] + cmd[cmd.index("-o") + 2:])
    os.replace(tmp, out)


@pytest.fixture(scope="module")
def emu():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    src = os.path.join(ROOT, "tests", "emu", "emu_sharded_mul.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("ntt_tile.h", "ntt_mul.h", "plan.h", "plan_dist_mul.h", "gl64.h", "field_policy.h",
                                                                               "mont64.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        obj = os.path.join(ROOT, "build", "orc_emu_smul.o")
        _build(["gcc", "-O2", "-c", "-o", obj, os.path.join(ROOT, "oracle", "ronk_oracle.c")], obj)
        _build(["g++", "-O2", "-std=c++17", "-o", EXE, src, obj], EXE)
    return EXE


def run(emu, *args, env=None):
    out = subprocess.run([emu] + [str(a) for a in args], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, **env) if env else None)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-400:] + out.stderr[-400:]
    return last


# the fused middle needs W * chunks >= 16 (ntt_mul.h mul_mid_matches_dist: received row blocks no longer than a lane's row step)
@pytest.mark.parametrize("log2n,W,chunks", [(18, 4, 4), (18, 8, 2), (18, 8, 4), (19, 4, 4), (19, 8, 2), (19, 8, 4)])
def test_fused_middle(emu, log2n, W, chunks):
    assert "middle=fused" in run(emu, log2n, W, chunks, 1)


@pytest.mark.parametrize("log2n,W,chunks", [(14, 2, 1), (18, 1, 1), (18, 2, 4), (19, 1, 2), (19, 2, 1), (19, 4, 2), (19, 8, 4)])
def test_composed_middle(emu, log2n, W, chunks):
    assert "middle=composed" in run(emu, log2n, W, chunks, 0)


@pytest.mark.parametrize("p,g", [(0xFFFFFFFC00000001, 10)])
def test_fused_middle_montgomery(emu, p, g):
    env = {"RONK_EMU_P": str(p), "RONK_EMU_G": str(g)}
    assert "middle=fused" in run(emu, 19, 8, 2, 1, env=env)
    assert "middle=composed" in run(emu, 18, 2, 1, 0, env=env)
