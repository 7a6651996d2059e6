"""Host-side pieces of the transform over BN254's scalar field: ronk_root_of_unity_bn254 against pow(5, (r-1) >> k, r) and the
pinned 2^28-th root, fr_pow / fr_inv (csrc/fr_ntt_kernels.h) through a host shim against Python's pow, the planner's factors
and the table budget.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

from oracle import bn254 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libfr_ntt_host.so")
W28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904
ERR_NO_ROOT, ERR_INVALID = -1, -7


@pytest.fixture(scope="module")
def H():
    src = os.path.join(ROOT, "tests", "emu", "fr_ntt_host.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("fr_ntt_kernels.h", "bn254_fr.h", "bn254_consts.h")]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = "%s.tmp.%d" % (SO, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, SO)
    h = C.CDLL(SO)
    h.h_fr_factors.restype = C.c_uint32
    h.h_fr_table_bytes.restype = C.c_uint64
    return h


def w4(v):
    return (C.c_uint64 * 4)(*[(v >> (64 * i)) & (2**64 - 1) for i in range(4)])


def rd(a):
    return sum(int(a[i]) << (64 * i) for i in range(4))


def test_root_of_unity_abi():
    from ronkathon_amd import _lib as L
    out = (C.c_uint64 * 4)()
    for k in (0, 1, 2, 28):
        assert L.lib.ronk_root_of_unity_bn254(k, out) == 0
        assert rd(out) == pow(5, (o.R - 1) >> k, o.R), k
    assert rd(out) == W28 and pow(W28, 1 << 27, o.R) == o.R - 1      # the pinned 2^28-th root: omega^(2^27) = -1
    assert L.lib.ronk_root_of_unity_bn254(29, out) == ERR_NO_ROOT
    assert L.lib.ronk_root_of_unity_bn254(3, None) == ERR_INVALID
    h = C.c_void_p()
    assert L.lib.ronk_plan_create_bn254(C.byref(h), 29, 0) == ERR_NO_ROOT
    assert L.lib.ronk_plan_create_bn254(None, 4, 0) == ERR_INVALID
    assert L.lib.ronk_poly_mul_bn254(None, 1, None, 1, None) == ERR_INVALID
    assert L.lib.ronk_poly_mul_bn254(out, 0, out, 1, out) == ERR_INVALID
    assert L.lib.ronk_ntt_forward_bn254(29, out, out) == ERR_NO_ROOT
    assert L.lib.ronk_ntt_inverse_bn254(2, None, out) == ERR_INVALID
    if L.device_count() == 0:      # no CPU path: a valid call without a GPU fails loudly
        assert L.lib.ronk_plan_create_bn254(C.byref(h), 4, 0) == L.ERR_NO_DEVICE
        assert L.lib.ronk_ntt_forward_bn254(0, out, out) == L.ERR_NO_DEVICE
        assert L.lib.ronk_poly_mul_bn254(out, 1, out, 1, out) == L.ERR_NO_DEVICE


def test_pow_and_inverse(H):
    rng = random.Random(2828)
    out = (C.c_uint64 * 4)()
    vals = [0, 1, 2, 5, o.R - 1, o.R - 2, o.R, o.R + 1, 2**256 - 1] + [rng.randrange(2**256) for _ in range(40)]
    exps = [0, 1, 2, o.R - 1, o.R - 2, (o.R - 1) >> 28, 2**256 - 1] + [rng.randrange(2**256) for _ in range(6)]
    for i, a in enumerate(vals):
        for e in exps[i % 3::3] + exps[:2]:
            H.h_fr_pow(w4(a), w4(e), out)
            assert rd(out) == pow(a % o.R, e, o.R), (a, e)
        H.h_fr_inv(w4(a), out)
        assert rd(out) == (pow(a % o.R, -1, o.R) if a % o.R else 0), a
    for k in range(0, 29):
        H.h_fr_root(k, out)
        assert rd(out) == pow(5, (o.R - 1) >> k, o.R), k


def test_planner_factors(H):
    rows = (C.c_uint32 * 4)()
    got = {}
    for k in range(0, 29):
        p = H.h_fr_factors(k, 0, rows)
        assert 1 <= p <= 3 and sum(rows[i] for i in range(p)) == k and all(rows[i] <= 10 for i in range(p)), k
        got[k] = [rows[i] for i in range(p)]
    assert got[10] == [10] and got[11] == [6, 5] and got[20] == [10, 10] and got[22] == [8, 7, 7] and got[28] == [10, 9, 9]
    for k, cap, want in ((8, 4, [4, 4]), (9, 5, [5, 4]), (12, 4, [4, 4, 4]), (13, 5, [5, 4, 4]), (16, 4, [4, 4, 4, 4])):
        p = H.h_fr_factors(k, cap, rows)
        assert [rows[i] for i in range(p)] == want
    assert H.h_fr_factors(20, 4, rows) == 0      # five passes: no plan under this cap


def test_table_budget(H):
    """no table of n entries; all tables of a transform together at most 1/8 of its data from 2^20 up"""
    m = C.c_uint64(0)
    for k in range(20, 29):
        b = H.h_fr_table_bytes(k, 0, C.byref(m))
        assert 0 < b <= (32 << k) // 8, (k, b)
        assert m.value <= (1 << k) // 16, (k, m.value)
