"""The transform and the polynomial product over BN254's scalar field on the GPU (csrc/fr_ntt_kernels.h, csrc/ronk_fr_ntt.hip)
against integer arithmetic mod oracle.bn254.R written here: a recursive radix-2 FFT, a schoolbook product and Horner."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bn254 as ob

pytestmark = pytest.mark.gpu

R = ob.R


# ---- the Python reference
def root(k):
    return pow(5, (R - 1) >> k, R)


def fft(x, w):
    n = len(x)
    if n == 1:
        return [x[0] % R]
    e, o = fft(x[0::2], w * w % R), fft(x[1::2], w * w % R)
    out = [0] * n
    t = 1
    for i in range(n // 2):
        v = t * o[i] % R
        out[i] = (e[i] + v) % R
        out[i + n // 2] = (e[i] - v) % R
        t = t * w % R
    return out


def ntt_ref(x):
    return fft(x, root(len(x).bit_length() - 1))


def intt_ref(y):
    n = len(y)
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in fft(y, pow(root(n.bit_length() - 1), -1, R))]


def schoolbook(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, u in enumerate(a):
        if u:
            for j, v in enumerate(b):
                out[i + j] += u * v
    return [v % R for v in out]


def horner(c, z):
    acc = 0
    for v in reversed(c):
        acc = (acc * z + v) % R
    return acc


# ---- device plumbing
@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("these tests need a GPU")
    return _lib


def words(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).copy()


def ints(w):
    buf = np.ascontiguousarray(w).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


class Dev:
    """a device buffer of `count` elements"""

    def __init__(self, L, count, data=None):
        self.L, self.count, self.p = L, count, C.c_void_p()
        L.check(L.lib.ronk_dev_alloc(C.byref(self.p), max(count, 1) * 32))
        if data is not None:
            self.put(data)

    def put(self, data):
        w = words(data)
        assert w.size == 4 * self.count
        self.L.check(self.L.lib.ronk_memcpy_h2d(self.p, self.L.ptr(w), w.nbytes))

    def get(self):
        w = np.empty(4 * self.count, dtype=np.uint64)
        self.L.check(self.L.lib.ronk_dev_sync())
        self.L.check(self.L.lib.ronk_memcpy_d2h(self.L.ptr(w), self.p, w.nbytes))
        return ints(w)

    def free(self):
        self.L.lib.ronk_dev_free(self.p)


def rand_vals(rng, n):
    return [rng.getrandbits(256) % R for _ in range(n)]


def transform(L, x, log2n, cap=0, inverse=False, batch=1, inplace=False):
    plan = L.FrPlan(log2n, cap)
    din = Dev(L, len(x), x)
    dout = din if inplace else Dev(L, len(x))
    (plan.inverse_dev if inverse else plan.forward_dev)(din.p, dout.p, batch)
    out = dout.get()
    plan.close(); din.free()
    if not inplace:
        dout.free()
    return out


# ---- transforms
@pytest.mark.parametrize("log2n", range(0, 13))
def test_small_transforms_full_compare(L, log2n):
    rng = random.Random(100 + log2n)
    x = rand_vals(rng, 1 << log2n)
    y = transform(L, x, log2n)
    assert y == ntt_ref(x)
    assert transform(L, y, log2n, inverse=True) == x
    assert transform(L, x, log2n, inverse=True) == intt_ref(x)


def first_two_pass_size(L):
    for k in range(1, 29):
        plan = L.FrPlan(k)
        p = len(plan.info())
        plan.close()
        if p == 2:
            return k
    raise AssertionError("no two-pass size")


def test_plan_info(L):
    k2 = first_two_pass_size(L)
    assert k2 == 11
    for k, cap, want in ((k2 - 1, 0, [k2 - 1]), (k2, 0, [6, 5]), (12, 4, [4, 4, 4]), (13, 5, [5, 4, 4]), (20, 0, [10, 10]), (9, 5, [5, 4])):
        plan = L.FrPlan(k, cap)
        assert plan.info() == want
        plan.close()
    with pytest.raises(L.RonkPanic) as e:
        L.FrPlan(29)
    assert e.value.code == L.ERR_NO_ROOT


@pytest.mark.parametrize("log2n,cap", [(16, 0), (11, 0), (12, 0), (12, 4), (13, 5)])
def test_larger_transforms_full_compare(L, log2n, cap):
    """2^16, the first default two-pass size (test_plan_info pins it at 2^11) and the next, the forced three-pass shapes"""
    rng = random.Random(200 + log2n + cap)
    x = rand_vals(rng, 1 << log2n)
    y = transform(L, x, log2n, cap)
    assert y == ntt_ref(x)
    assert transform(L, y, log2n, cap, inverse=True) == x


@pytest.fixture(scope="module")
def big(L):
    """2^20 on the default plan: two different rows, their forward transform as one batch of two"""
    k = 20
    rng = random.Random(2020)
    x = rand_vals(rng, 2 << k)
    y = transform(L, x, k, batch=2)
    return k, x, y


def test_2p20_outputs_by_horner(big):
    k, x, y = big
    n = 1 << k
    rng = random.Random(16)
    w = root(k)
    for _ in range(8):
        i = rng.randrange(n)
        assert y[i] == horner(x[:n], pow(w, i, R)), i
    for _ in range(8):
        i = rng.randrange(n)
        assert y[n + i] == horner(x[n:], pow(w, i, R)), i


def test_2p20_unit_impulse(L):
    k = 20
    n = 1 << k
    j = random.Random(77).randrange(1, n)
    x = [0] * n
    x[j] = 1
    y = transform(L, x, k)
    wj = pow(root(k), j, R)
    want, t = [], 1
    for _ in range(n):
        want.append(t)
        t = t * wj % R
    assert y == want


def test_2p20_round_trip_batch_and_in_place(L, big):
    k, x, y = big
    n = 1 << k
    assert transform(L, y, k, inverse=True, batch=2) == x
    # the rows of the batch are independent transforms
    assert transform(L, x[n:], k) == y[n:]
    assert transform(L, x[:n], k, inplace=True) == y[:n]
    assert transform(L, x, k, batch=2, inplace=True) == y


def test_batch_above_the_reserved_scratch(L):
    """a multi-pass plan holds scratch for one row until ronk_plan_reserve_bn254: a larger batch runs in slices, the same results"""
    for k, cap in ((11, 0), (12, 4)):
        n = 1 << k
        x = rand_vals(random.Random(400 + k), 3 * n)
        want = [v for b in range(3) for v in ntt_ref(x[b * n:(b + 1) * n])]
        plan = L.FrPlan(k, cap)
        din, dout = Dev(L, 3 * n, x), Dev(L, 3 * n)
        plan.forward_dev(din.p, dout.p, 3)
        assert dout.get() == want
        plan.reserve(2)                      # slices of 2 + 1
        plan.forward_dev(din.p, din.p, 3)    # in place
        assert din.get() == want
        plan.reserve(3)
        plan.inverse_dev(din.p, dout.p, 3)
        assert dout.get() == x
        plan.close(); din.free(); dout.free()


def test_non_canonical_inputs(L):
    for k, cap in ((6, 0), (12, 4), (12, 0)):
        rng = random.Random(300 + k + cap)
        n = 1 << k
        x = [rng.getrandbits(256) for _ in range(n)]
        x[0], x[n // 2], x[n - 1], x[3] = R, 2 * R, 2**256 - 1, R + 1
        want = ntt_ref([v % R for v in x])
        assert transform(L, x, k, cap) == want
        assert transform(L, x, k, cap, inverse=True) == intt_ref([v % R for v in x])


def test_against_the_linear_division(L):
    """output i of the forward transform is the remainder of the division by (x - omega^i) (csrc/fr_scan_kernels.h)"""
    k = 12
    n = 1 << k
    rng = random.Random(12)
    x = rand_vals(rng, n)
    y = transform(L, x, k)
    dc, dq, dr = Dev(L, n, x), Dev(L, n), Dev(L, 1)
    for i in (1, 1000, n - 1):
        z = words([pow(root(k), i, R)])
        L.check(L.lib.ronk_poly_div_linear_bn254_dev(dc.p, n, L.ptr(z), dq.p, dr.p, None))
        assert dr.get()[0] == y[i], i
    dc.free(); dq.free(); dr.free()


# ---- products
@pytest.mark.parametrize("d,d2", [(1, 1), (1, 7), (3, 5), (17, 17), (1025, 1021)])
def test_products_against_schoolbook(L, d, d2):
    from ronkathon_amd import callers
    rng = random.Random(d * 31 + d2)
    a, b = [rng.getrandbits(256) for _ in range(d)], [rng.getrandbits(256) for _ in range(d2)]
    got = callers.poly_mul_bn254(a, b)
    assert len(got) == d + d2 - 1
    assert got == schoolbook([v % R for v in a], [v % R for v in b])


def test_product_2p16_against_the_python_fft(L):
    from ronkathon_amd import callers
    rng = random.Random(1616)
    d, d2 = 1 << 15, (1 << 15) - 1
    a, b = rand_vals(rng, d), rand_vals(rng, d2)
    n = 1 << 16
    fa, fb = ntt_ref(a + [0] * (n - d)), ntt_ref(b + [0] * (n - d2))
    want = intt_ref([u * v % R for u, v in zip(fa, fb)])
    assert not any(want[d + d2 - 1:])
    assert callers.poly_mul_bn254(a, b) == want[:d + d2 - 1]


def test_product_of_all_r_minus_one(L):
    from ronkathon_amd import callers
    a, b = [R - 1] * 100, [R - 1] * 29
    # (-1)(-1) = 1 per term: coefficient k counts the pairs (i, j) with i + j = k
    want = [min(k, 99, 28, 127 - k) + 1 for k in range(128)]
    assert callers.poly_mul_bn254(a, b) == want == schoolbook(a, b)
    rng = random.Random(5)
    c = rand_vals(rng, 40)
    assert callers.poly_mul_bn254(a, c) == schoolbook(a, c)


def test_product_errors(L):
    a = words([1, 2])
    out = np.zeros(16, dtype=np.uint64)
    assert L.lib.ronk_poly_mul_bn254(L.ptr(a), (1 << 28) + 1, L.ptr(a), 1, L.ptr(out)) == L.ERR_UNSUPPORTED
    assert L.lib.ronk_poly_mul_bn254(L.ptr(a), 0, L.ptr(a), 1, L.ptr(out)) == L.ERR_INVALID


def test_commit_from_evaluations(L):
    from ronkathon_amd import callers
    rng = random.Random(64)
    srs = ob.multiples(64)
    c = rand_vals(rng, 64)
    ev = callers.ntt_bn254(c)
    assert ev == ntt_ref(c)
    assert callers.intt_bn254(ev) == c
    assert callers.kzg_commit_evals_bn254(ev, srs) == callers.msm_bn254(srs, c) == ob.msm(srs, c)


def test_two_plans_on_two_streams(L):
    import torch
    k = 16
    n = 1 << k
    rng = random.Random(2)
    xa, xb = rand_vals(rng, n), rand_vals(rng, n)
    pa, pb = L.FrPlan(k), L.FrPlan(k)
    da, db, oa, ob_ = Dev(L, n, xa), Dev(L, n, xb), Dev(L, n), Dev(L, n)
    # one after the other
    pa.forward_dev(da.p, oa.p)
    ya = oa.get()
    pb.inverse_dev(db.p, ob_.p)
    yb = ob_.get()
    oa.put([0] * n); ob_.put([0] * n)
    L.check(L.lib.ronk_dev_sync())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        pa.forward_dev(da.p, oa.p, 1, C.c_void_p(sa.cuda_stream))
        pb.inverse_dev(db.p, ob_.p, 1, C.c_void_p(sb.cuda_stream))
    sa.synchronize(); sb.synchronize()
    assert oa.get() == ya and ob_.get() == yb
    assert ya == ntt_ref(xa)
    pa.close(); pb.close()
    for d in (da, db, oa, ob_):
        d.free()
