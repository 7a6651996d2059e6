"""The element-wise kernels (ronk_vec_add / sub / mul / neg, host and _dev forms; csrc/field_kernels.h over mont64.h) at the edges
of the modular addition's select, over every generic prime of tests/prime_classes.py, against Python integers.

mont64::add selects s - p by `c2 | !b2` (carry out of bit 63, no borrow from s - p).  The operand pairs put the sum on both sides
of p, of 2^64 and at 2 p - 2, the difference on both sides of zero, and cross the operands whose Montgomery products sit at the
edges of the reduction.  One launch per operation and kernel: the 16-byte pair kernel (even length, aligned arrays, b as long as
a) and the scalar kernel (odd length; b shorter than a through ronk_poly_add / ronk_poly_sub).  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import prime_classes as PC
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
