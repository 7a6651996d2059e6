"""The older `Ops`-templated kernels over the prime classes of tests/prime_classes.py: P_MID (a sum lands in [p, 2^64) and carries
out of bit 63 in the same launch), P_62 (never carries), MONT_P (carries, all but never lands in [p, 2^64)), P_32 where it is
cheap, and 0xFFFFFFFFFFFFFFC5 (p - 1 has a single factor 2: no transform of any size) where a path needs a prime without roots.
Every kernel below is the MontOps instantiation, which compiles its own copy of mont64::add / sub / redc.

Entry point -> kernels reached:

    ronk_poly_eval_dev                     scan_kernels.h eval_onepass_kernel (every size here is below its chunk limit)
    ronk_poly_div_linear_dev               lindiv_kernels.h lindiv_one_kernel with 4 coefficients per lane, with 8 from 3 * 2^19
                                           coefficients on; lindiv_scan_kernel / lindiv_apply_kernel2 (the two launches) for z = 0, for a quotient
                                           written over the dividend and for a dividend 8 bytes off a 16-byte boundary
    tests/scan_subprocess_check.py         (test_gpu_parity.py::test_scan_onepass_variants) the other forms of scan_kernels.h
    ronk_poly_divrem_dev                   longdiv_kernel.h poly_divrem_kernel with 256 / 512 / 1024 work-items
    ronk_lagrange_eval_dev                 field_kernels.h lagrange_terms / lagrange_finish (general), lagrange_check,
                                           lagrange_fast_terms / lagrange_fast_finish (chosen on the device at 256 nodes, by the
                                           host above 2^16)
    ronk_lagrange_nodes                    power_table_kernel
    ronk_rs_decode / ronk_rs_decode_dev    interp_kernels.h rs_weights / master_poly / rs_accumulate / rs_finish (the only decode
                                           of a generic prime); ronk_rs_encode is nodes + transform
    ronk_dft / ronk_dft_dev                dft_naive_kernel (n no power of two)
    ronk_poly_mul                          poly_mul_schoolbook_kernel (short products, or a generator that has no tiled plan)
    L.Plan(p, g^2, 10)                     bitrev_copy / radix2_stage

References: Python integers for everything directed, O(n) or small O(n^2); the oracle (`__int128 % p`) for whole vectors.  All
comparisons are bit-exact.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import prime_classes as PC
from conftest import splitmix_field

pytestmark = pytest.mark.gpu

P_MID, P_62, MONT_P, P_32 = PC.P_MID, PC.P_62, PC.MONT_P, PC.P_32
P_NOROOT = 0xFFFFFFFFFFFFFFC5          # p - 1 = 2 * 11 * 137 * 547 * ...: wrap only, and no root of unity beyond -1
CLASSES = [(P_MID, PC.GEN[P_MID]), (P_62, PC.GEN[P_62]), (MONT_P, PC.GEN[MONT_P])]
CLASS_IDS = ["P_MID", "P_62", "MONT_P"]
WITH_32 = CLASSES + [(P_32, PC.GEN[P_32])]
WITH_32_IDS = CLASS_IDS + ["P_32"]
SENTINEL = 0x5555555555555555


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib as L
    import ronkathon_amd as R
    assert R.device_count() >= 1
    return L


@pytest.fixture(scope="module")
def orc():
    import oracle
    return oracle


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def status_word(torch):
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def full(p, v, n):
    return np.full(n, v % p, dtype=np.uint64)


def horner(p, c, z):
    acc = 0
    for v in reversed(c.tolist()):
        acc = (acc * z + v) % p
    return acc


# ------------------------------------------------------------------------------------------ evaluate and linear division
SIZES = [1, 7, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5, 70001]
BIG = 3 * 2**19 + 3                      # from 3 * 2^19 coefficients on the one-launch form takes 8 per lane


def coefficient_sets(p, d, seed):
    return [("random", splitmix_field(seed, d, p)), ("all p-1", full(p, p - 1, d))]


def points(p, seed):
    return [0, 1, p - 1, PC.T % p, int(splitmix_field(seed, 1, p)[0])]


class Divider:
    """ronk_poly_div_linear_dev / ronk_poly_eval_dev with guard words round both outputs"""

    def __init__(self, torch, L, orc, p):
        self.torch, self.L, self.orc, self.p = torch, L, orc, p

    def evaluate(self, d_c, d, z):
        t = self.torch
        out = t.full((3,), SENTINEL, dtype=t.int64, device="cuda")
        self.L.check(self.L.lib.ronk_poly_eval_dev(self.p, d_c, d, z, out.data_ptr() + 8, None))
        o = host(t, out).tolist()
        assert o[0] == SENTINEL and o[2] == SENTINEL, "evaluate wrote outside its one word"
        return o[1]

    def divide(self, d_c, d, b0, b1, d_q=None):
        """-> (quotient, remainder); d_q: write there (in place); default a fresh array, 16-byte aligned, with two guard words on
        either side"""
        t = self.torch
        rem = t.full((3,), SENTINEL, dtype=t.int64, device="cuda")
        if d_q is None:
            buf = t.full((d + 4,), SENTINEL, dtype=t.int64, device="cuda")
            assert buf.data_ptr() % 16 == 0
            self.L.check(self.L.lib.ronk_poly_div_linear_dev(self.p, d_c, d, b0, b1, buf.data_ptr() + 16, rem.data_ptr() + 8, None))
            q = host(t, buf)
            assert q[:2].tolist() == [SENTINEL] * 2 and q[d + 2:].tolist() == [SENTINEL] * 2, "quotient written outside [0, d)"
            q = q[2:d + 2]
        else:
            self.L.check(self.L.lib.ronk_poly_div_linear_dev(self.p, d_c, d, b0, b1, d_q, rem.data_ptr() + 8, None))
            q = None
        r = host(t, rem).tolist()
        assert r[0] == SENTINEL and r[2] == SENTINEL, "remainder written outside its one word"
        return q, r[1]

    def verify(self, c, q, r, b0, b1, value, what):
        """c = q * (b0 + b1 x) + r coefficient by coefficient -- with q[d-1] = 0 that is the recurrence
        q[j-1] = (c[j] - b0 q[j]) / b1 at every j, (c[j] + z q[j]) for the monic divisor x - z -- and r = c(z)"""
        p, orc, d = self.p, self.orc, c.size
        assert int(q[d - 1]) == 0, what
        assert r == value, (what, "remainder", hex(r), hex(value))
        assert int(c[0]) == (b0 * int(q[0]) + r) % p, (what, "constant coefficient")
        if d > 1:
            rhs = orc.vec_add(p, orc.vec_mul(p, q[1:], full(p, b0, d - 1)), orc.vec_mul(p, q[:-1], full(p, b1, d - 1)))
            bad = np.nonzero(rhs != c[1:])[0]
            assert bad.size == 0, (what, "recurrence fails first at j =", int(bad[0]) + 1, "of", d)


@pytest.mark.parametrize("d", SIZES)
@pytest.mark.parametrize("p,g", WITH_32, ids=WITH_32_IDS)
def test_evaluate_and_linear_division_at_the_chunk_edges(torch, L, orc, p, g, d):
    """the default forms: one-launch evaluate; lindiv_one_kernel with 4 coefficients per lane (chunks of 4096; the evaluate's
    chunks hold 2048), the two launches for z = 0.  Every coefficient set at every point with a monic, a small and a p - 1
    leading coefficient of the divisor; then one call in place and one with the dividend 8 bytes off a 16-byte boundary"""
    dv = Divider(torch, L, orc, p)
    for cname, c in coefficient_sets(p, d, 0x5C0 + d):
        d_c = dev(torch, c)
        assert d_c.data_ptr() % 16 == 0
        for z in points(p, d):
            value = horner(p, c, z)
            assert dv.evaluate(d_c.data_ptr(), d, z) == value, (hex(p), d, cname, hex(z), "evaluate")
            for b1 in (1, 5, p - 1):
                b0 = (-z * b1) % p
                q, r = dv.divide(d_c.data_ptr(), d, b0, b1)
                dv.verify(c, q, r, b0, b1, value, (hex(p), d, cname, hex(z), hex(b1)))
    # in place, and 8 bytes off: both keep the two launches (lindiv_scan_kernel / lindiv_apply_kernel2), the second without 16-byte loads
    c = splitmix_field(0x1D0 + d, d, p)
    z = int(splitmix_field(d + 1, 1, p)[0]) or 1
    b1 = p - 1
    b0 = (-z * b1) % p
    value = horner(p, c, z)
    buf = torch.full((d + 4,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[2:d + 2] = dev(torch, c)
    _, r = dv.divide(buf.data_ptr() + 16, d, b0, b1, d_q=buf.data_ptr() + 16)
    got = host(torch, buf)
    assert got[:2].tolist() == [SENTINEL] * 2 and got[d + 2:].tolist() == [SENTINEL] * 2, "in place: written outside [0, d)"
    dv.verify(c, got[2:d + 2], r, b0, b1, value, (hex(p), d, "in place"))
    off = torch.full((d + 3,), SENTINEL, dtype=torch.int64, device="cuda")
    off[1:d + 1] = dev(torch, c)
    assert (off.data_ptr() + 8) % 16 == 8
    q, r = dv.divide(off.data_ptr() + 8, d, b0, b1)
    dv.verify(c, q, r, b0, b1, value, (hex(p), d, "dividend 8 bytes off"))
    o = host(torch, off)
    assert o[0] == SENTINEL and o[d + 1:].tolist() == [SENTINEL] * 2 and np.array_equal(o[1:d + 1], c), "the dividend changed"


@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_linear_division_with_eight_coefficients_per_lane(torch, L, orc, p, g):
    """3 * 2^19 + 3 coefficients: lindiv_one_kernel's 8-per-lane form (chunks of 8192), 769 chunks of the evaluate; the value from
    the oracle's Horner"""
    d = BIG
    dv = Divider(torch, L, orc, p)
    for cname, c in coefficient_sets(p, d, 0xB16):
        d_c = dev(torch, c)
        for z, b1 in ((int(splitmix_field(0xB17, 1, p)[0]), 1), (p - 1, p - 1)):
            value = orc.poly_eval(p, c, z)
            assert dv.evaluate(d_c.data_ptr(), d, z) == value, (hex(p), cname, hex(z), "evaluate")
            b0 = (-z * b1) % p
            q, r = dv.divide(d_c.data_ptr(), d, b0, b1)
            dv.verify(c, q, r, b0, b1, value, (hex(p), cname, hex(z), hex(b1)))


# ------------------------------------------------------------------------------------------ long division
def ragged(b, zeros):
    b = b.copy()
    b[-zeros:] = 0
    return b


def divrem_cases(p):
    """(name, a, b): one shape per workgroup size (d2 <= 256 / <= 1023 / >= 1024), each with a quotient below 2048 coefficients; a
    divisor longer than the dividend; a ragged divisor (trailing zeros: the reference's early stop or index panic)"""
    out = []
    for d, d2 in ((200, 7), (700, 300), (2100, 1024), (50, 80)):
        a, b = splitmix_field(d, d, p), splitmix_field(d2 + 1, d2, p)
        a[-1] = p - 1
        b[-1] = p - 1 if d2 != 300 else 2          # leading coefficients whose inverses are p - 1 and (p + 1) / 2
        out.append(("%d/%d" % (d, d2), a, b))
    out.append(("ragged 200/7", splitmix_field(9, 200, p), ragged(splitmix_field(10, 7, p), 3)))
    out.append(("ragged 700/300", splitmix_field(11, 700, p), ragged(splitmix_field(12, 300, p), 1)))
    # both operands one short of their length: one elimination step, then the reference stops early instead of panicking
    out.append(("ragged 50/50", ragged(splitmix_field(13, 50, p), 1), ragged(splitmix_field(14, 50, p), 1)))
    return out


def check_divrem(torch, L, orc, p, name, a, b):
    try:
        wq, wr = orc.poly_divrem(p, a, b)
        code = 0
    except orc.OraclePanic as e:
        wq = wr = None
        code = e.code
    d_a, d_b = dev(torch, a), dev(torch, b)
    d_q = torch.full((a.size,), -1, dtype=torch.int64, device="cuda")
    d_r = torch.full((a.size,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 0x7777, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_poly_divrem_dev(p, d_a.data_ptr(), a.size, d_b.data_ptr(), b.size, d_q.data_ptr(), d_r.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(st.item()) == code, (hex(p), name, "status")
    if code == 0:
        assert np.array_equal(host(torch, d_q), wq), (hex(p), name, "quotient")
        assert np.array_equal(host(torch, d_r), wr), (hex(p), name, "remainder")
    return code


@pytest.mark.parametrize("p,g", WITH_32 + [(P_NOROOT, None)], ids=WITH_32_IDS + ["P_NOROOT"])
def test_long_division_kernel(torch, L, orc, p, g):
    codes = [check_divrem(torch, L, orc, p, name, a, b) for name, a, b in divrem_cases(p)]
    assert codes == [0, 0, 0, 0, L.ERR_INDEX, L.ERR_INDEX, 0], "the ragged divisors: two index panics of the reference, one early stop"
    if p == P_NOROOT:    # a shape that the primes with roots give to the O(n log n) form: here it stays with this kernel
        a, b = splitmix_field(1, 2200, p), splitmix_field(2, 64, p)
        a[-1] = b[-1] = p - 1
        assert check_divrem(torch, L, orc, p, "2200/64", a, b) == 0


# ------------------------------------------------------------------------------------------ Lagrange evaluate and the node table
def omega_table(p, g, n):
    w = pow(g, (p - 1) // n, p)
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * w % p
    return np.array(out, dtype=np.uint64)


def lagrange_dev(torch, L, p, d_c, d_nodes, n, x):
    out = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda")
    st = status_word(torch)
    L.check(L.lib.ronk_lagrange_eval_dev(p, d_c.data_ptr(), d_nodes.data_ptr(), n, x, out.data_ptr() + 8, st.data_ptr(), None))
    o = host(torch, out).tolist()
    assert o[0] == SENTINEL and o[2] == SENTINEL
    return o[1], int(st.item())


@pytest.mark.parametrize("kind,n", [("arbitrary", 255), ("arbitrary", 300), ("omega", 256)])
@pytest.mark.parametrize("p,g", WITH_32, ids=WITH_32_IDS)
def test_lagrange_evaluate_below_2_16_nodes(torch, L, orc, p, g, kind, n):
    """255 nodes: the general O(n^2) kernels alone; 300 arbitrary nodes: lagrange_check_kernel refuses the O(n) form on the device;
    256 powers of omega: it selects it.  Against the oracle's restatement of the reference (which yields ZERO at a node)"""
    if kind == "omega":
        nodes = omega_table(p, g, n)
    else:
        nodes = np.unique(splitmix_field(0x1A6 + n, n + 8, p))[:n].copy()
        nodes = nodes[np.argsort(splitmix_field(n, n, P_32), kind="stable")]       # not sorted
        assert nodes.size == n and int(nodes.min()) > 1                             # so that 0 and 1 are no nodes here
    c = splitmix_field(0x1A7 + n, n, p)
    c[0] = c[-1] = p - 1
    d_c, d_nodes = dev(torch, c), dev(torch, nodes)
    for x in (int(splitmix_field(n, 1, p)[0]), int(nodes[n // 3]), int(nodes[n - 1]), 0, 1):
        got, st = lagrange_dev(torch, L, p, d_c, d_nodes, n, x)
        assert st == 0 and got == orc.lagrange_eval(p, c, nodes, x), (hex(p), kind, n, hex(x))
        assert L.out_scalar(L.lib.ronk_lagrange_eval, p, L.ptr(c), L.ptr(nodes), n, x) == got
    dup = nodes.copy()
    dup[n - 2] = dup[7]
    _, st = lagrange_dev(torch, L, p, d_c, dev(torch, dup), n, 5)
    assert st != 0 and not st & 4, "coincident nodes"
    out = np.zeros(1, dtype=np.uint64)
    assert L.lib.ronk_lagrange_eval(p, L.ptr(c), L.ptr(dup), n, 5, out.ctypes.data_as(L.C.POINTER(L.C.c_uint64))) == L.ERR_ZERO_INVERSE


@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_lagrange_evaluate_at_2_17_nodes(torch, L, orc, p, g):
    """above 2^16 nodes the host takes the O(n) form.  Off the nodes the value is that of the interpolating polynomial: the oracle's
    inverse transform of the values, then Horner on Python integers.  At a node the reference's fold yields ZERO (the O(n^2)
    restatement says so for the same kernels at 256 nodes above)"""
    n = 1 << 17
    nodes = omega_table(p, g, n)
    c = splitmix_field(0x217, n, p)
    c[0] = c[-1] = p - 1
    coeffs = orc.ifft(p, g, c)
    d_c, d_nodes = dev(torch, c), dev(torch, nodes)
    for x in (int(splitmix_field(0x218, 1, p)[0]), 0, p - 2):
        assert pow(x, n, p) != 1
        got, st = lagrange_dev(torch, L, p, d_c, d_nodes, n, x)
        assert st == 0 and got == horner(p, coeffs, x), (hex(p), hex(x))
    for x in (1, int(nodes[12345])):
        got, st = lagrange_dev(torch, L, p, d_c, d_nodes, n, x)
        assert st == 0 and got == 0, (hex(p), hex(x), "at a node")
    dup = nodes.copy()
    dup[n - 2] = dup[7]
    _, st = lagrange_dev(torch, L, p, d_c, dev(torch, dup), n, 5)
    assert st & 4, "not the powers of an order-n element"


NON_POW2 = {P_MID: 768, P_62: 464, MONT_P: 448}        # 3 * 2^8, 29 * 16, 7 * 64: each divides p - 1 and spans a 256-lane block edge


@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_lagrange_nodes_are_the_powers_of_omega(L, p, g):
    """ronk_lagrange_nodes (power_table_kernel) against Python powers"""
    for n in (1 << 14, NON_POW2[p]):
        assert (p - 1) % n == 0
        nodes = np.full(n, SENTINEL, dtype=np.uint64)
        L.check(L.lib.ronk_lagrange_nodes(p, g, L.ptr(nodes), n))
        assert np.array_equal(nodes, omega_table(p, g, n)), (hex(p), n)


# ------------------------------------------------------------------------------------------ Reed-Solomon
def rs_decode_both(torch, L, p, xs, ys, k):
    """(host form's result, its return code, _dev form's result, its status)"""
    xs, ys = np.ascontiguousarray(xs[:k]), np.ascontiguousarray(ys[:k])
    out = np.full(k, SENTINEL, dtype=np.uint64)
    rc = L.lib.ronk_rs_decode(p, L.ptr(xs), L.ptr(ys), k, L.ptr(out))
    d_out = torch.full((k + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    st = status_word(torch)
    d_xs, d_ys = dev(torch, xs), dev(torch, ys)
    L.check(L.lib.ronk_rs_decode_dev(p, d_xs.data_ptr(), d_ys.data_ptr(), k, d_out.data_ptr(), st.data_ptr(), None))
    o = host(torch, d_out)
    assert o[k:].tolist() == [SENTINEL] * 2, "decode wrote beyond k"
    return out, rc, o[:k], int(st.item())


@pytest.fixture(scope="module")
def codewords(L, orc):
    """{p: (message of 600, xs, ys)}: ronk_rs_encode at N = 1024 against the oracle's encode, once for all decode cases"""
    out = {}
    for p, g in CLASSES:
        msg = splitmix_field(0x25, 600, p)
        msg[0] = msg[-1] = p - 1
        n = 1024
        xs, ys = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        L.check(L.lib.ronk_rs_encode(p, g, L.ptr(msg), msg.size, n, L.ptr(xs), L.ptr(ys)))
        wx, wy = orc.rs_encode(p, g, msg, n)
        assert np.array_equal(xs, wx) and np.array_equal(ys, wy), hex(p)
        out[p] = (msg, xs, ys)
    return out


@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, 600])
@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_reed_solomon_decode(torch, L, orc, codewords, p, g, k):
    """Message::decode interpolates through whichever k coordinates come first: the first k of the codeword and a random k-subset
    of it (a codeword of a 600-coefficient message, so for k < 600 the result is not the message), against the oracle's decode"""
    msg, xs, ys = codewords[p]
    pick = np.argsort(splitmix_field(k, xs.size, P_32), kind="stable")[:k]
    for what, sel in (("first k", np.arange(k)), ("random subset", pick)):
        want = orc.rs_decode(p, xs[sel], ys[sel], k)
        got, rc, got_dev, st = rs_decode_both(torch, L, p, xs[sel], ys[sel], k)
        assert rc == 0 and st == 0
        assert np.array_equal(got, want) and np.array_equal(got_dev, want), (hex(p), k, what)
        if k == 600:
            assert np.array_equal(want, msg)
    if k >= 2:
        bad = xs[pick].copy()
        bad[k - 1] = bad[0]
        _, rc, _, st = rs_decode_both(torch, L, p, bad, ys[pick], k)
        assert rc == L.ERR_ZERO_INVERSE and st != 0 and not st & 4, "coincident nodes"


@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_reed_solomon_round_trip_of_2000(torch, L, p, g):
    """K = 2000 (eight blocks of the O(K^2) kernels, master_poly's 1024 lanes with two coefficients each) from a random 2000-subset
    of 4096 coordinates, against the message itself"""
    k, n = 2000, 4096
    msg = splitmix_field(0x2000, k, p)
    msg[0] = msg[-1] = p - 1
    xs, ys = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    L.check(L.lib.ronk_rs_encode(p, g, L.ptr(msg), k, n, L.ptr(xs), L.ptr(ys)))
    pick = np.argsort(splitmix_field(k, n, P_32), kind="stable")[:k]
    got, rc, got_dev, st = rs_decode_both(torch, L, p, xs[pick], ys[pick], k)
    assert rc == 0 and st == 0
    assert np.array_equal(got, msg) and np.array_equal(got_dev, msg), hex(p)


# ------------------------------------------------------------------------------------------ naive DFT, schoolbook, radix-2
@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_naive_dft_at_a_size_that_is_no_power_of_two(torch, L, p, g):
    """Polynomial::dft by its O(n^2) definition on Python integers"""
    n = NON_POW2[p]
    x = splitmix_field(0xDF7, n, p)
    x[0] = x[-1] = p - 1
    pw = omega_table(p, g, n).tolist()
    xl = x.tolist()
    want = [sum(xl[j] * pw[j * k % n] for j in range(n)) % p for k in range(n)]
    out = np.full(n, SENTINEL, dtype=np.uint64)
    L.check(L.lib.ronk_dft(p, g, L.ptr(x), L.ptr(out), n))
    assert out.tolist() == want, (hex(p), "host")
    d_out = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    d_x = dev(torch, x)
    L.check(L.lib.ronk_dft_dev(p, g, d_x.data_ptr(), d_out.data_ptr(), n, None))
    o = host(torch, d_out).tolist()
    assert o[:n] == want and o[n] == SENTINEL, (hex(p), "dev")


def schoolbook(p, a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return [v % p for v in out]


@pytest.mark.parametrize("p,g", CLASSES, ids=CLASS_IDS)
def test_schoolbook_multiply(L, p, g):
    """poly_mul_schoolbook_kernel: products of at most 64 coefficients with the true generator; longer ones with g^2, a quadratic
    residue, under which no tiled plan exists (asserted on the plan itself)"""
    g2 = g * g % p
    for k in (7, 9):
        plan = L.Plan(p, g2, k)
        assert plan.path() == 0
        plan.close()
    for gen, d, d2 in ((g, 40, 25), (g, 64, 1), (g, 1, 1), (g2, 300, 200), (g2, 257, 1)):
        a, b = splitmix_field(d, d, p), splitmix_field(d2 + 77, d2, p)
        a[0] = a[-1] = b[-1] = p - 1
        out = np.full(d + d2 - 1, SENTINEL, dtype=np.uint64)
        L.check(L.lib.ronk_poly_mul(p, gen, L.ptr(a), d, L.ptr(b), d2, L.ptr(out)))
        assert out.tolist() == schoolbook(p, a.tolist(), b.tolist()), (hex(p), d, d2)


@pytest.mark.parametrize("p,g", CLASSES[:2], ids=CLASS_IDS[:2])
def test_radix2_plan_under_a_residue_generator(L, orc, p, g):
    """bitrev_copy / radix2_stage restate the reference's recursion for a `g` without a full 2-power subgroup: forward and inverse
    against the oracle called with that same g^2 (test_gpu_mont.py does this for MONT_P)"""
    g2 = g * g % p
    plan = L.Plan(p, g2, 10)
    assert plan.path() == 0
    x = splitmix_field(0x22D, 1 << 10, p)
    x[0] = x[-1] = p - 1
    assert np.array_equal(plan.forward(x), orc.fft(p, g2, x)), hex(p)
    assert np.array_equal(plan.inverse(x), orc.ifft(p, g2, x)), hex(p)
    plan.close()
