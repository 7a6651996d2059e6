"""The element-wise kernels (ronk_vec_add / sub / mul / neg, host and _dev forms; csrc/field_kernels.h over mont64.h) at the edges
of the modular addition's select, over every generic prime of tests/prime_classes.py, against Python integers.

mont64::add selects s - p by `c2 | !b2` (carry out of bit 63, no borrow from s - p).  The operand pairs put the sum on both sides
of p, of 2^64 and at 2 p - 2, the difference on both sides of zero, and cross the operands whose Montgomery products sit at the
edges of the reduction.  One launch per operation and kernel: the 16-byte pair kernel (even length, aligned arrays, b as long as
a) and the scalar kernel (odd length; b shorter than a through ronk_poly_add / ronk_poly_sub).

Then the kernels built on mont64::pow and the Montgomery product -- ronk_vec_pow / ronk_vec_inv (vec_pow_kernel), ronk_vec_euler
(vec_euler_kernel), ronk_vec_sqrt (vec_sqrt_kernel: Tonelli-Shanks) and their _dev forms -- over the same primes, against Python's
pow and, for the roots, their defining properties.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import prime_classes as PC
from conftest import splitmix_field
from ronkathon_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


OPS = {"add": (PC.add_pairs, lambda p, a, b: (a + b) % p),
       "sub": (PC.sub_pairs, lambda p, a, b: (a - b) % p),
       "mul": (PC.mul_pairs, lambda p, a, b: a * b % p)}


def operands(p, name, odd):
    """(a, b, want): the pairs of the operation, of even length for the pair kernel and one pair more for the scalar kernel"""
    pairs = list(OPS[name][0](p))
    if len(pairs) % 2:
        pairs.append(pairs[0])
    if odd:
        pairs.append(pairs[1])
    a = np.array([x for x, _ in pairs], dtype=np.uint64)
    b = np.array([y for _, y in pairs], dtype=np.uint64)
    want = [OPS[name][1](p, x, y) for x, y in pairs]
    assert a.size % 2 == int(odd)
    return a, b, want


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("name", ["add", "sub", "mul"])
@pytest.mark.parametrize("odd", [False, True], ids=["pair_kernel", "scalar_kernel"])
def test_binary_operations_at_the_edges(torch, p, g, name, odd):
    a, b, want = operands(p, name, odd)
    n = a.size
    # the _dev form
    d_a, d_b = dev(torch, a), dev(torch, b)
    assert (d_a.data_ptr() | d_b.data_ptr()) % 16 == 0
    d_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    L.check(getattr(L.lib, "ronk_vec_%s_dev" % name)(p, d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), n, None))
    got = host(torch, d_out).tolist()
    bad = [(hex(x), hex(y), hex(v), hex(w)) for x, y, v, w in zip(a.tolist(), b.tolist(), got, want) if v != w]
    assert not bad, (hex(p), name, "dev", bad[:4])
    # the host form
    out = np.full(n, 2**64 - 1, dtype=np.uint64)
    L.check(getattr(L.lib, "ronk_vec_%s" % name)(p, L.ptr(a), L.ptr(b), L.ptr(out), n))
    assert out.tolist() == want, (hex(p), name, "host")


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("name", ["add", "sub"])
def test_second_operand_shorter_than_the_first(p, g, name):
    """ronk_poly_add / ronk_poly_sub: b is read as zero beyond its length, which takes the scalar kernel at any length"""
    a, b, _ = operands(p, name, False)
    nb = a.size // 2 + 1
    fn = OPS[name][1]
    want = [fn(p, int(x), int(y) if i < nb else 0) for i, (x, y) in enumerate(zip(a, b))]
    out = np.full(a.size, 2**64 - 1, dtype=np.uint64)
    bs = np.ascontiguousarray(b[:nb])
    L.check(getattr(L.lib, "ronk_poly_%s" % name)(p, L.ptr(a), a.size, L.ptr(bs), nb, L.ptr(out)))
    assert out.tolist() == want, (hex(p), name)


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
def test_negation_at_the_edges(torch, p, g):
    vals = sorted(set(PC.mul_operands(p)) | {x for pair in PC.add_pairs(p) for x in pair})
    for odd in (False, True):
        a = np.array(vals[:len(vals) - (len(vals) % 2 != int(odd))], dtype=np.uint64)
        assert a.size % 2 == int(odd)
        want = [(-int(x)) % p for x in a]
        d_a = dev(torch, a)
        d_out = torch.full((a.size,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.ronk_vec_neg_dev(p, d_a.data_ptr(), d_out.data_ptr(), a.size, None))
        assert host(torch, d_out).tolist() == want, (hex(p), "dev", odd)
        out = np.full(a.size, 2**64 - 1, dtype=np.uint64)
        L.check(L.lib.ronk_vec_neg(p, L.ptr(a), L.ptr(out), a.size))
        assert out.tolist() == want, (hex(p), "host", odd)


# ------------------------------------------------------------------------------------------------ pow, inverse, Euler, square root
def pow_operands(p, n):
    """n canonical values: the operands at the edges of the Montgomery reduction, then random ones"""
    edge = PC.mul_operands(p)
    return np.array(edge + splitmix_field(0xE0 + n, n - len(edge), p).tolist(), dtype=np.uint64)


LENGTHS = [300, 301]


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("n", LENGTHS)
def test_power_at_the_edge_exponents(torch, p, g, n):
    a = pow_operands(p, n)
    d_a = dev(torch, a)
    for e in (0, 1, 2, p - 2, p - 1, 2**64 - 1):
        want = [pow(int(x), e, p) for x in a]
        d_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.ronk_vec_pow_dev(p, d_a.data_ptr(), e, d_out.data_ptr(), n, None))
        assert host(torch, d_out).tolist() == want, (hex(p), hex(e), "dev")
        out = np.full(n, 2**64 - 1, dtype=np.uint64)
        L.check(L.lib.ronk_vec_pow(p, L.ptr(a), e, L.ptr(out), n))
        assert out.tolist() == want, (hex(p), hex(e), "host")


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("n", LENGTHS)
def test_inverse_and_the_zero_among_the_inputs(torch, p, g, n):
    a = pow_operands(p, n)
    a[a == 0] = p - 3
    want = [pow(int(x), p - 2, p) for x in a]
    assert all(int(x) * w % p == 1 for x, w in zip(a, want))
    d_a = dev(torch, a)
    d_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_vec_inv_dev(p, d_a.data_ptr(), d_out.data_ptr(), n, st.data_ptr(), None))
    assert host(torch, d_out).tolist() == want and int(st.item()) == 0, (hex(p), "dev")
    out = np.full(n, 2**64 - 1, dtype=np.uint64)
    L.check(L.lib.ronk_vec_inv(p, L.ptr(a), L.ptr(out), n))
    assert out.tolist() == want, (hex(p), "host")
    a[n - 2] = 0                                  # Field::inverse of ZERO is None: the reference's unwrap panics
    d_a = dev(torch, a)
    L.check(L.lib.ronk_vec_inv_dev(p, d_a.data_ptr(), d_out.data_ptr(), n, st.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(st.item()) != 0, (hex(p), "dev: the zero went unreported")
    assert L.lib.ronk_vec_inv(p, L.ptr(a), L.ptr(out), n) == L.ERR_ZERO_INVERSE, (hex(p), "host")


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("n", LENGTHS)
def test_euler_criterion(torch, p, g, n):
    a = pow_operands(p, n)
    a[-1], a[-2] = g, g * g % p
    want = [int(pow(int(x), (p - 1) // 2, p) == 1) for x in a]
    assert want[-1] == 0 and want[-2] == 1 and want[0] == 0       # a generator is no residue, its square is; ZERO is none by this test
    d_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_a = dev(torch, a)
    L.check(L.lib.ronk_vec_euler_dev(p, d_a.data_ptr(), d_out.data_ptr(), n, None))
    assert host(torch, d_out).tolist() == want, (hex(p), "dev")
    out = np.full(n, 2**64 - 1, dtype=np.uint64)
    L.check(L.lib.ronk_vec_euler(p, L.ptr(a), L.ptr(out), n))
    assert out.tolist() == want, (hex(p), "host")


def sqrt_operands(p, g, n):
    """n squares: ZERO and ONE; g^2 and g^(2 odd), the squares of elements of maximal 2-power order, for which the Tonelli-Shanks
    loop runs its full s - 1 rounds (s the 2-adicity: 34, 57, 34, 30); the squares of the edge operands and of random values"""
    odd = [1, 3, 5, (p - 1) // 2**PC.BY_P[p].two_adicity, 0xFFFFFFFF, p - 2]
    assert all(k % 2 for k in odd)
    top = [pow(g, 2 * k, p) for k in odd]
    assert all(pow(x, (p - 1) // 4, p) == p - 1 for x in top)       # x = y^2 with y of order divisible by 2^s
    roots = PC.mul_operands(p)[2:] + splitmix_field(0x50 + n, n, p).tolist()
    sq = [0, 1] + top + [int(r) * int(r) % p for r in roots]
    return np.array(sq[:n], dtype=np.uint64)


def check_roots(p, x, r0, r1, what):
    """the two roots by their defining properties, on Python integers"""
    for xi, a, b in zip(x.tolist(), r0.tolist(), r1.tolist()):
        if xi == 0:
            assert (a, b) == (0, 0), (hex(p), what, "ZERO")
        else:
            assert a * a % p == xi and a < b and a + b == p, (hex(p), what, hex(xi), hex(a), hex(b))


@pytest.mark.parametrize("p,g", PC.GENERIC_PRIMES, ids=[e.name for e in PC.TABLE])
@pytest.mark.parametrize("n", LENGTHS)
def test_square_roots(torch, p, g, n):
    x = sqrt_operands(p, g, n)
    d_r0 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_r1 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_x = dev(torch, x)
    L.check(L.lib.ronk_vec_sqrt_dev(p, d_x.data_ptr(), d_r0.data_ptr(), d_r1.data_ptr(), n, st.data_ptr(), None))
    r0, r1 = host(torch, d_r0), host(torch, d_r1)
    assert int(st.item()) == 0
    check_roots(p, x, r0, r1, "dev")
    h0, h1 = np.full(n, 2**64 - 1, dtype=np.uint64), np.full(n, 2**64 - 1, dtype=np.uint64)
    L.check(L.lib.ronk_vec_sqrt(p, L.ptr(x), L.ptr(h0), L.ptr(h1), n))
    check_roots(p, x, h0, h1, "host")
    # a non-residue among them is the reference's assert: the flag on the device, ERR_NOT_RESIDUE from the host form
    for bad in (g, pow(g, (p - 1) // 2**PC.BY_P[p].two_adicity, p)):
        y = x.copy()
        y[n - 3] = bad
        st.zero_()
        d_y = dev(torch, y)
        L.check(L.lib.ronk_vec_sqrt_dev(p, d_y.data_ptr(), d_r0.data_ptr(), d_r1.data_ptr(), n, st.data_ptr(), None))
        r0, r1 = host(torch, d_r0), host(torch, d_r1)
        assert int(st.item()) != 0, (hex(p), hex(bad), "dev: the non-residue went unreported")
        assert (int(r0[n - 3]), int(r1[n - 3])) == (0, 0)
        keep = np.arange(n) != n - 3
        check_roots(p, y[keep], r0[keep], r1[keep], "dev, beside a non-residue")
        assert L.lib.ronk_vec_sqrt(p, L.ptr(y), L.ptr(h0), L.ptr(h1), n) == L.ERR_NOT_RESIDUE, (hex(p), hex(bad), "host")
