"""csrc/bn254.h (the arithmetic under the BN254 MSM kernels and the MSM's host tail) compiled for the host and checked
against oracle/bn254.py: Montgomery multiplication, add / sub / inverse, the XYZZ mixed addition, general addition and
doubling including their special cases (P + P, P - P, infinity operands).  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libbn254_host.so")


@pytest.fixture(scope="module")
def H():
    src = os.path.join(ROOT, "tests", "emu", "bn254_host.cpp")
    deps = [src] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("bn254.h", "bn254_probe.h", "bn254_fr.h", "bn254_consts.h", "msm_common.h")]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


def w4(v):
    return (C.c_uint64 * 4)(*[(v >> (64 * i)) & (2**64 - 1) for i in range(4)])


def w8(pt):
    x, y = (0, 0) if pt is None else pt
    return (C.c_uint64 * 8)(*[(x >> (64 * i)) & (2**64 - 1) for i in range(4)], *[(y >> (64 * i)) & (2**64 - 1) for i in range(4)])


def rd(a, off=0):
    return sum(int(a[off + i]) << (64 * i) for i in range(4))


def rdpt(a):
    x, y = rd(a), rd(a, 4)
    return None if x == 0 and y == 0 else (x, y)


def test_field_ops(H):
    from oracle import bn254 as o
    rng = random.Random(254)
    edge = [0, 1, 2, o.P - 1, o.P - 2, (1 << 253) - 1, (1 << 253), 0xFFFFFFFF, 1 << 32, (1 << 224) - 1]
    vals = edge + [rng.randrange(o.P) for _ in range(200)]
    out = (C.c_uint64 * 4)()
    for i, a in enumerate(vals):
        b = vals[(7 * i + 3) % len(vals)]
        H.h_fp_mul(w4(a), w4(b), out); assert rd(out) == a * b % o.P, (a, b)
        H.h_fp_add(w4(a), w4(b), out); assert rd(out) == (a + b) % o.P
        H.h_fp_sub(w4(a), w4(b), out); assert rd(out) == (a - b) % o.P
        if a:
            H.h_fp_inv(w4(a), out); assert rd(out) == pow(a, -1, o.P)
    for v, want in ((o.P, 1), (o.P - 1, 0), (o.P + 1, 1), (2**256 - 1, 1), (0, 0), (1 << 253, 0)):
        assert H.h_fp_geq_p(w4(v)) == want


def test_group_law(H):
    from oracle import bn254 as o
    rng = random.Random(7)
    pts = [o.mul(rng.randrange(1, o.R), o.G) for _ in range(12)] + [o.G, o.TWO_G, None]
    out = (C.c_uint64 * 8)()
    for p in pts:
        assert H.h_on_curve(w8(p)) == (0 if p is None else 1)
        for q in pts:
            for neg in (0, 1):
                qq = o.neg(q) if neg else q
                for mode in (0, 1):
                    H.h_point_op(w8(p), w8(q), neg, mode, out)
                    assert rdpt(out) == o.add(p, qq), (p, q, neg, mode)
        H.h_point_op(w8(p), w8(p), 0, 2, out)
        assert rdpt(out) == o.add(p, p)
    bad = (o.G[0], o.G[1] + 1)
    assert H.h_on_curve(w8(bad)) == 0
    for k in (0, 1, 2, o.R - 1, o.R, 2**256 - 1, rng.randrange(2**256)):
        H.h_scalar_mul(w8(pts[0]), w4(k), out)
        assert rdpt(out) == o.mul(k, pts[0]), k


def test_msm_pipeline_on_host(H):
    """the bucket-method pipeline of csrc/msm_kernels.h -- signed-digit recoding (rippled and from the per-scalar carry mask
    the sort kernels use), buckets, bit-plane reduction, host tail -- restated sequentially with the shared pieces of
    csrc/msm_common.h, for every window size, against the oracle's fold (kzg::commit, src/kzg/setup.rs:48-60)"""
    from oracle import bn254 as o
    rng = random.Random(11)
    base = o.multiples(40)
    for c in range(5, 17):
        n = 30
        pts = [base[rng.randrange(40)] if rng.random() < 0.85 else None for _ in range(n)]
        ks = [rng.choice([0, 1, (1 << (c - 1)), (1 << (c - 1)) + 1, (1 << c) - 1, o.R - 1, 2**256 - 1, rng.randrange(2**256), rng.randrange(o.R)])
              for _ in range(n)]
        pw = (C.c_uint64 * (8 * n))(); sw = (C.c_uint64 * (4 * n))()
        for i, (pt, k) in enumerate(zip(pts, ks)):
            x, y = (0, 0) if pt is None else pt
            for j in range(4):
                pw[8 * i + j] = (x >> (64 * j)) & (2**64 - 1); pw[8 * i + 4 + j] = (y >> (64 * j)) & (2**64 - 1)
                sw[4 * i + j] = (k >> (64 * j)) & (2**64 - 1)
        out = (C.c_uint64 * 8)()
        assert H.h_msm_pipeline(pw, sw, n, c, out) == 0, c
        assert rdpt(out) == o.msm(pts, ks), c


def test_scalar_field_ops(H):
    """csrc/bn254_fr.h (the field of kzg::open's division, src/kzg/setup.rs:63-78, on BN254): Montgomery product with one
    operand in Montgomery form, add / sub, canonicalisation of arbitrary 256-bit inputs, and the power table of the suffix scan"""
    from oracle import bn254 as o
    rng = random.Random(2540)
    edge = [0, 1, 2, o.R - 1, o.R - 2, (1 << 253) - 1, (1 << 253), 0xFFFFFFFF, 1 << 32, (1 << 224) - 1]
    vals = edge + [rng.randrange(o.R) for _ in range(200)]
    out = (C.c_uint64 * 4)()
    for i, a in enumerate(vals):
        b = vals[(7 * i + 3) % len(vals)]
        H.h_fr_mul(w4(a), w4(b), out); assert rd(out) == a * b % o.R, (a, b)
        H.h_fr_add(w4(a), w4(b), out); assert rd(out) == (a + b) % o.R
        H.h_fr_sub(w4(a), w4(b), out); assert rd(out) == (a - b) % o.R
    for v in (o.R, o.R + 1, 2 * o.R, 2**256 - 1, 5 * o.R + 7, 0, o.R - 1):
        H.h_fr_canon(w4(v), out); assert rd(out) == v % o.R, v
        H.h_fr_mul(w4(v), w4(3), out); assert rd(out) == v * 3 % o.R        # first operand: ANY 256-bit integer
    pw = (C.c_uint64 * (4 * 257))()
    for z in (0, 1, 2, o.R - 1, rng.randrange(o.R), 2**256 - 5):
        H.h_fr_powers(w4(z), pw)
        for k in (0, 1, 2, 3, 17, 128, 255, 256):
            assert rd(pw, 4 * k) == pow(z % o.R, 4 * k, o.R), (z, k)
    q, v = o.fr_div_linear([3, 0, 5, 7], 2)
    assert q == [(0 + 2 * (5 + 2 * 7)) % o.R, 5 + 2 * 7, 7, 0] and v == 3 + 2 * q[0]
