"""ronk_poly_mul_sharded*: the polynomial product sharded like the four-step transform (forward phase 1 of both operands,
exchange, the middle -- fused kernel or forward phase 2 + inverse phase 1 with the product on load --, exchange, phase 2 of the
swapped-split inverse).  Every coefficient against the oracle's NTT product of the zero-padded operands.  Logical ranks share
device 0 (a peer copy to the same device is a plain copy); with >= 2 visible devices the distinct-device layout runs as well."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
import prime_classes as PC
import ronkathon_amd as R
from ronkathon_amd import _lib as L
from ronkathon_amd import dist

pytestmark = pytest.mark.gpu

GP, GG = R.GOLDILOCKS_P, R.GOLDILOCKS_G
MONT = [(0xFFFFFFFC00000001, 10), (29 * 2**57 + 1, 3)]   # two of test_gpu_mont.py's primes


def field_vec(seed, size, p=GP):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    return v % np.uint64(p) if p != GP else np.where(v >= np.uint64(p), v - np.uint64(p), v)


def cyclic(p, g, a, b, n):
    """length-n cyclic convolution of the zero-padded operands = a * b when len(a) + len(b) - 1 <= n"""
    pa, pb = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pa[:a.size], pb[:b.size] = a, b
    return orc.ifft(p, g, orc.vec_mul(p, orc.fft(p, g, pa), orc.fft(p, g, pb)))


def fusable(log2n, W, chunks):
    """an instantiation of the fused middle matches: single-pass phases (log2n 18 .. 25) whose received row blocks fit a lane's
    row step (W * chunks >= 16, ntt_mul.h mul_mid_matches_dist)"""
    return 18 <= log2n <= 25 and W * chunks >= 16


def fused_expected(log2n, W, chunks):
    """the plan's default middle: fused only where it measured faster (2^24)"""
    return 1 if log2n == 24 and fusable(log2n, W, chunks) else 0


def layouts(W):
    ndev = R.device_count()
    return [[0] * W] + ([[g % ndev for g in range(W)]] if ndev >= 2 and W >= 2 else [])


# (log2n, W, chunks, d, d2): odd and even log2n across the composed (12, 16, 26) and fused (18 .. 25) ranges, ragged lengths
CASES = [
    (12, 1, 1, 1 << 11, 1 << 11), (12, 2, 0, 1000, 3001),
    (16, 2, 2, 1, 1 << 16), (16, 4, 1, 40000, 25537),
    (18, 8, 1, 1 << 17, 1 << 17), (18, 4, 2, 99999, 100000),
    (19, 2, 0, 300001, 224288), (19, 8, 4, 1, 1 << 19),
    (20, 8, 0, 1 << 19, 1 << 19), (20, 1, 1, 777777, 123),
    (22, 8, 2, 3 << 20, 1 << 20), (24, 8, 0, 1 << 23, (1 << 23) + 1),
    (25, 4, 0, 1 << 24, 1 << 24), (26, 8, 0, 1 << 25, 1 << 25),
]


@pytest.mark.parametrize("log2n,W,chunks,d,d2", CASES)
def test_sharded_mul_matches_oracle(log2n, W, chunks, d, d2):
    n = 1 << log2n
    assert d + d2 - 1 <= n
    a, b = field_vec(0x5EED7000 + log2n, d), field_vec(0x5EED7100 + log2n + W, d2)
    want = cyclic(GP, GG, a, b, n)[:d + d2 - 1]
    for devs in layouts(W):
        mp = L.ShardedMulPlan(log2n, devs, chunks=chunks)
        assert mp.R * mp.C == n and mp.per_rank * W == n
        assert mp.fused_middle == fused_expected(log2n, W, mp.chunks), (log2n, W, chunks)
        got = mp.mul(a, b)
        assert np.array_equal(got, want), (log2n, W, chunks, d, d2, devs)
        mp.close()


@pytest.mark.parametrize("log2n,W,chunks", [(18, 8, 2), (19, 4, 4), (22, 8, 0), (23, 8, 4), (25, 8, 2)])
def test_fused_and_composed_middles_agree(log2n, W, chunks):
    n = 1 << log2n
    a, b = field_vec(0x5EED7200 + log2n, n // 2), field_vec(0x5EED7300 + log2n, n // 2 + 1)
    fused = L.ShardedMulPlan(log2n, [0] * W, chunks=chunks, fused=True)
    comp = L.ShardedMulPlan(log2n, [0] * W, chunks=chunks, unfused=True)
    assert fused.fused_middle == 1 and comp.fused_middle == 0
    x, y = fused.mul(a, b), comp.mul(a, b)
    assert np.array_equal(x, y)
    if log2n <= 22:
        assert np.array_equal(x, cyclic(GP, GG, a, b, n)[:n])
    fused.close(); comp.close()


def check_sharded_mul_montgomery(p, g, log2n, W, chunks):
    n = 1 << log2n
    a, b = field_vec(0x5EED7400 + log2n, n // 2, p), field_vec(0x5EED7500 + log2n, n // 2 - 3, p)
    want = cyclic(p, g, a, b, n)[:a.size + b.size - 1]
    for unfused in (False, True):
        mp = L.ShardedMulPlan(log2n, [0] * W, chunks=chunks, p=p, g=g, unfused=unfused, fused=not unfused)
        assert mp.fused_middle == (0 if unfused else int(fusable(log2n, W, mp.chunks)))
        assert np.array_equal(mp.mul(a, b), want), (p, log2n, W, chunks, unfused)
        mp.close()


@pytest.mark.parametrize("p,g", MONT)
@pytest.mark.parametrize("log2n,W,chunks", [(16, 2, 1), (20, 8, 2), (24, 4, 4)])
def test_sharded_mul_montgomery(p, g, log2n, W, chunks):
    check_sharded_mul_montgomery(p, g, log2n, W, chunks)


def test_sharded_mul_montgomery_p_mid():
    """the fused and the composed middle at 2^20 over the prime whose sums take every outcome of mont64::add (tests/prime_classes.py)"""
    check_sharded_mul_montgomery(PC.P_MID, PC.GEN[PC.P_MID], 20, 8, 2)


class Blocks:
    """one [R][C/W] block per rank on device memory (rank g on devs[g])"""

    def __init__(self, devs, per):
        self.devs, self.per, self.ptrs = devs, per, []
        for d in devs:
            L.check(L.lib.ronk_set_device(d))
            h = C.c_void_p()
            L.check(L.lib.ronk_dev_alloc(C.byref(h), per * 8))
            self.ptrs.append(h.value)
        L.check(L.lib.ronk_set_device(0))

    def put(self, x, world):
        for g, d in enumerate(self.devs):
            blk = dist.scatter_input(x, g, world)
            L.check(L.lib.ronk_set_device(d))
            L.check(L.lib.ronk_memcpy_h2d(self.ptrs[g], L.ptr(blk), self.per * 8))
        L.check(L.lib.ronk_set_device(0))

    def get(self, n, world):
        log2n = n.bit_length() - 1
        Rr, Cc, _, Cw = dist.shape(log2n, world)
        out = np.empty(n, dtype=np.uint64)
        for g, d in enumerate(self.devs):
            blk = np.empty(self.per, dtype=np.uint64)
            L.check(L.lib.ronk_set_device(d))
            L.check(L.lib.ronk_memcpy_d2h(L.ptr(blk), self.ptrs[g], self.per * 8))
            out.reshape(Rr, Cc)[:, g * Cw:(g + 1) * Cw] = blk.reshape(Rr, Cw)
        L.check(L.lib.ronk_set_device(0))
        return out

    def free(self):
        for g, d in enumerate(self.devs):
            L.check(L.lib.ronk_set_device(d))
            L.lib.ronk_dev_free(self.ptrs[g])
        L.check(L.lib.ronk_set_device(0))


@pytest.mark.parametrize("log2n,W,chunks,unfused", [(20, 8, 2, False), (20, 8, 2, True), (22, 4, 4, False), (16, 2, 1, False)])
def test_sharded_mul_device_api(log2n, W, chunks, unfused):
    """two products back to back and one sync; a chained (a.b).c with the first call's output as an input of the second (no host
    round trip); a second use of the same plan (buffer reuse under the event guards)"""
    n = 1 << log2n
    q = n // 4
    a, b, c = field_vec(0x5EED7600 + log2n, q), field_vec(0x5EED7700 + log2n, q), field_vec(0x5EED7800 + log2n, q)
    ab, ac = cyclic(GP, GG, a, b, n), cyclic(GP, GG, a, c, n)
    abc = cyclic(GP, GG, ab[:2 * q - 1], c, n)
    for devs in layouts(W):
        mp = L.ShardedMulPlan(log2n, devs, chunks=chunks, unfused=unfused, fused=not unfused)
        bufs = {k: Blocks(devs, mp.per_rank) for k in ("a", "b", "c", "ab", "ac", "abc")}
        for k, v in (("a", a), ("b", b), ("c", c)):
            pad = np.zeros(n, dtype=np.uint64)
            pad[:v.size] = v
            bufs[k].put(pad, W)
        mp.mul_dev(bufs["a"].ptrs, bufs["b"].ptrs, bufs["ab"].ptrs)
        mp.mul_dev(bufs["a"].ptrs, bufs["c"].ptrs, bufs["ac"].ptrs)
        mp.sync()
        assert np.array_equal(bufs["ab"].get(n, W), ab), (log2n, W, devs)
        assert np.array_equal(bufs["ac"].get(n, W), ac), (log2n, W, devs)
        mp.mul_dev(bufs["a"].ptrs, bufs["b"].ptrs, bufs["ab"].ptrs)      # again, then chained without a host round trip
        mp.mul_dev(bufs["ab"].ptrs, bufs["c"].ptrs, bufs["abc"].ptrs)
        mp.sync()
        assert np.array_equal(bufs["abc"].get(n, W), abc), (log2n, W, devs)
        for v in bufs.values():
            v.free()
        mp.close()


def test_sharded_mul_rccl_exchange():
    """RONK_EXCHANGE_RCCL with one rank per visible device (a single GPU: one rank that sends to itself); fused and composed"""
    ndev = R.device_count()
    W = 1
    while W * 2 <= ndev and W < 8:
        W *= 2
    for log2n, chunks in ((16, 1), (20, 2), (22, 0)):
        n = 1 << log2n
        a, b = field_vec(0x5EED7900 + log2n, n // 2), field_vec(0x5EED7A00 + log2n, n // 2)
        want = cyclic(GP, GG, a, b, n)[:n - 1]
        for unfused in (False, True):
            mp = L.ShardedMulPlan(log2n, list(range(W)), chunks=chunks, exchange=L.EXCHANGE_RCCL, unfused=unfused, fused=not unfused)
            assert np.array_equal(mp.mul(a, b), want), (log2n, W, chunks, unfused)
            assert np.array_equal(mp.mul(a, b), want)
            mp.close()
    with pytest.raises(R.RonkPanic) as e:
        L.ShardedMulPlan(16, [0, 0], exchange=L.EXCHANGE_RCCL)
    assert e.value.code == -9


def test_sharded_mul_errors():
    mp = L.ShardedMulPlan(16, [0, 0])
    with pytest.raises(R.RonkPanic) as e:
        mp.mul(np.ones(40000, dtype=np.uint64), np.ones(30000, dtype=np.uint64))   # d + d2 - 1 > n
    assert e.value.code == -7
    mp.close()
    for log2n, W in ((10, 8), (9, 2), (16, 3)):   # fewer than 16 rows / columns per rank; not a power of two
        with pytest.raises(R.RonkPanic) as e:
            L.ShardedMulPlan(log2n, [0] * W)
        assert e.value.code == -9, (log2n, W)
    with pytest.raises(R.RonkPanic) as e:
        L.ShardedMulPlan(16, [0, 99])
    assert e.value.code == -7
    with pytest.raises(R.RonkPanic) as e:
        L.ShardedMulPlan(16, [0, 0], chunks=3)
    assert e.value.code == -9
    with pytest.raises(R.RonkPanic) as e:
        L.ShardedMulPlan(20, [0] * 8, unfused=True, fused=True)
    assert e.value.code == -7
