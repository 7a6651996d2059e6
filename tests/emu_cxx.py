"""Which compilers build the host emulators (tests/emu/*.cpp).

csrc/mont64.h, poseidon_kernels.h and gl64.h keep two forms of their carry chains: `#if defined(__clang__)` is what the device
build compiles (__builtin_addc / __builtin_subc and a select on the carry masks), the other branch is portable C++.  g++ only
ever sees the portable one, so a host leg that is to say anything about the device form has to be built with clang: the clang++
that hipcc itself drives, found beside it.  A test helper, not product code."""
import os
import shutil
import subprocess


def device_form_cxx():
    """the host clang++ of the HIP toolchain, or None"""
    cands = []
    hipcc = shutil.which("hipcc")
    if hipcc:
        root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        cands += [os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++")]
    for env in ("ROCM_PATH", "HIP_PATH"):
        if os.environ.get(env):
            cands.append(os.path.join(os.environ[env], "lib", "llvm", "bin", "clang++"))
    cands.append("/opt/rocm/lib/llvm/bin/clang++")
    for c in cands:
        if os.path.exists(c):
            return c
    return None


def build(cxx, exe, srcs, deps, opt="-O2"):
    """compile srcs to exe unless it is newer than srcs + deps; to a private name first, then renamed (pytest-xdist workers may
    rebuild at once, and a binary that is being written cannot be executed)"""
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in list(srcs) + list(deps)):
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call([cxx, opt, "-std=c++17", "-o", tmp] + list(srcs))
        os.replace(tmp, exe)
    return exe


def build_device_form(exe, srcs, deps, opt="-O0"):
    """the same with the HIP toolchain's clang++ (the `__clang__` branches); skips the test where there is none.  Unoptimised
    unless asked: these legs are about which source form is compiled, their runs are short, and clang spends minutes optimising
    the tile emulator's instantiations"""
    import pytest
    cxx = device_form_cxx()
    if cxx is None:
        pytest.skip("no clang++ beside hipcc: the device form of the carry chains cannot be built for the host")
    return build(cxx, exe, srcs, deps, opt)
