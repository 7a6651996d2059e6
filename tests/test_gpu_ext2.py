"""The quadratic-extension vector entry points on the device (ronk_ext2_vec_*) against the Python restatement (tests/ext2_ref.py),
over Goldilocks (its own arithmetic), a generic 64-bit prime (the Montgomery policy) and F_101 with the reference's own vectors
(tests/golden/gf101_2_vectors.json).  Arrays are planar: [2][n] words."""
import json
import os

import numpy as np
import pytest

import ext2_ref as ER
import prime_classes as PC
from ronkathon_amd import _lib as L
from ronkathon_amd import extension
from test_gpu_fri import dev, host, words

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GL, MONT = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001
FIELDS = [(GL, 7), (MONT, 10), (101, 99)]
SIZES = [1, 63, 64, 65, 4097]   # one lane, the wave boundary, several workgroups with a grid-stride tail
# MONT's sums all but never land in [p, 2^64): the primes of tests/prime_classes.py take every outcome of mont64::add; W the generator
CLASS_FIELDS = PC.CLASS_PRIMES


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "gf101_2_vectors.json")) as f:
        return json.load(f)


def planar_words(seed, n, p, golden=None, key="a"):
    """[2][n] words with the edges mixed in (0, p - 1, words >= p); over F_101 the golden operands come first"""
    v = words(seed, 2 * n, p)
    if p == 101 and golden is not None:
        ops = [c[key] for op in ("add", "sub", "mul") for c in golden[op]][:n]
        for i, c in enumerate(ops):
            v[i], v[n + i] = c[0], c[1]
    return v


def els(E, v):
    return [E.el(x) for x in ER.pairs(v.tolist())]


def run_dev(torch, fn, p, w, n, *args, out=None):
    """call a _dev entry point: array arguments are device tensors, others pass through; returns the [2][n] output words"""
    d_out = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda") if out is None else out
    ptrs = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]
    L.check(fn(p, w, *ptrs, d_out.data_ptr(), n, 0))
    return host(torch, d_out)


def check_ring_operations(torch, golden, p, w, n):
    E = ER.Ext2(p, w)
    a, b = planar_words(n, n, p, golden, "a"), planar_words(n + 1000, n, p, golden, "b")
    ea, eb = els(E, a), els(E, b)
    d_a, d_b = dev(torch, a), dev(torch, b)
    for name, op in (("add", E.add), ("sub", E.sub), ("mul", E.mul)):
        got = run_dev(torch, getattr(L.lib, "ronk_ext2_vec_%s_dev" % name), p, w, n, d_a, d_b)
        assert got.tolist() == ER.planar([op(x, y) for x, y in zip(ea, eb)]), (name, p, n)
    assert run_dev(torch, L.lib.ronk_ext2_vec_neg_dev, p, w, n, d_a).tolist() == ER.planar([E.neg(x) for x in ea])
    s = words(n + 2000, n, p)
    got = run_dev(torch, L.lib.ronk_ext2_vec_mul_base_dev, p, w, n, d_a, dev(torch, s))
    assert got.tolist() == ER.planar([E.mul_base(x, int(t) % p) for x, t in zip(ea, s)])


@pytest.mark.parametrize("p,w", FIELDS)
@pytest.mark.parametrize("n", SIZES)
def test_ring_operations(torch, golden, p, w, n):
    check_ring_operations(torch, golden, p, w, n)


@pytest.mark.parametrize("p,w", CLASS_FIELDS)
@pytest.mark.parametrize("n", SIZES)
def test_ring_operations_prime_classes(torch, golden, p, w, n):
    check_ring_operations(torch, golden, p, w, n)


def test_golden_vectors_on_the_device(torch, golden):
    p, w = golden["p"], golden["w"]
    for op in ("add", "sub", "mul"):
        cases = golden[op]
        a = np.array(ER.planar([c["a"] for c in cases]), dtype=np.uint64)
        b = np.array(ER.planar([c["b"] for c in cases]), dtype=np.uint64)
        got = run_dev(torch, getattr(L.lib, "ronk_ext2_vec_%s_dev" % op), p, w, len(cases), dev(torch, a), dev(torch, b))
        assert got.tolist() == ER.planar([c["out"] for c in cases]), op
    a = np.array(ER.planar([c["a"] for c in golden["neg"]]), dtype=np.uint64)
    assert run_dev(torch, L.lib.ronk_ext2_vec_neg_dev, p, w, len(golden["neg"]), dev(torch, a)).tolist() == ER.planar([c["out"] for c in golden["neg"]])
    g = np.array(golden["primitive_element"], dtype=np.uint64)
    d_g = dev(torch, g)
    order = golden["primitive_element_order"]
    assert run_dev(torch, L.lib.ronk_ext2_vec_pow_dev, p, w, 1, d_g, order).tolist() == [1, 0]
    for q in (2, 3, 5, 17):     # 101^2 - 1 = 2^3 * 3 * 5^2 * 17
        assert run_dev(torch, L.lib.ronk_ext2_vec_pow_dev, p, w, 1, d_g, order // q).tolist() != [1, 0]


def check_inverse(torch, p, w, n):
    E = ER.Ext2(p, w)
    a = planar_words(n + 7, n, p)
    a[0] = 1                                                     # no zero element (c0 of element 0; the others by chance never)
    ea = els(E, a)
    for i, x in enumerate(ea):
        if x == E.zero:
            a[i] = 1
    ea = els(E, a)
    d_a = dev(torch, a)
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_inv = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    L.check(L.lib.ronk_ext2_vec_inv_dev(p, w, d_a.data_ptr(), d_inv.data_ptr(), n, d_st.data_ptr(), 0))
    inv = host(torch, d_inv)
    assert int(d_st.item()) == 0
    assert inv.tolist() == ER.planar([E.inv(x) for x in ea])
    # a * a^-1 = (1, 0) through the device product
    assert run_dev(torch, L.lib.ronk_ext2_vec_mul_dev, p, w, n, d_a, d_inv).tolist() == [1] * n + [0] * n
    # a zero element at position 0 and at n - 1 (as a word >= p there) sets the status; (0, 0) is written for it, like
    # ronk_vec_inv_dev writes 0 for a zero word
    for pos, zero in ((0, 0), (n - 1, p)):
        z = a.copy()
        z[pos], z[n + pos] = zero, 0
        d_st.zero_()
        L.check(L.lib.ronk_ext2_vec_inv_dev(p, w, dev(torch, z).data_ptr(), d_inv.data_ptr(), n, d_st.data_ptr(), 0))
        got = host(torch, d_inv)
        assert int(d_st.item()) != 0 and (got[pos], got[n + pos]) == (0, 0), (p, n, pos)
        with pytest.raises(L.RonkPanic) as e:
            extension.Ext2(_Field(p), w).vec_inv(z)
        assert e.value.code == L.ERR_ZERO_INVERSE
    # the base-field call reports its zero the same way
    d_b = dev(torch, np.array([0, 5], dtype=np.uint64))
    d_bo = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    d_st.zero_()
    L.check(L.lib.ronk_vec_inv_dev(p, d_b.data_ptr(), d_bo.data_ptr(), 2, d_st.data_ptr(), 0))
    assert int(d_st.item()) != 0 and host(torch, d_bo)[0] == 0


@pytest.mark.parametrize("p,w", FIELDS)
@pytest.mark.parametrize("n", SIZES)
def test_inverse(torch, p, w, n):
    check_inverse(torch, p, w, n)


@pytest.mark.parametrize("p,w", CLASS_FIELDS)
@pytest.mark.parametrize("n", [1, 65])
def test_inverse_prime_classes(torch, p, w, n):
    check_inverse(torch, p, w, n)


class _Field:
    def __init__(self, p):
        self.ORDER = p


def check_pow(torch, p, w, n):
    E = ER.Ext2(p, w)
    a = planar_words(n + 11, n, p)
    ea = els(E, a)
    d_a = dev(torch, a)
    for e in (0, 1, 2, p, 2 ** 64 - 1):
        got = run_dev(torch, L.lib.ronk_ext2_vec_pow_dev, p, w, n, d_a, e).tolist()
        assert got == ER.planar([E.pow(x, e) for x in ea]), (p, n, e)
        if e == p:
            assert got == ER.planar([(x[0], -x[1] % p) for x in ea]), "Frobenius"


@pytest.mark.parametrize("p,w", FIELDS)
@pytest.mark.parametrize("n", SIZES)
def test_pow(torch, p, w, n):
    """every (n, e) against the restatement; a^p = (a0, -a1) (Frobenius) as an independent check"""
    check_pow(torch, p, w, n)


@pytest.mark.parametrize("p,w", CLASS_FIELDS)
@pytest.mark.parametrize("n", [1, 65])
def test_pow_prime_classes(torch, p, w, n):
    check_pow(torch, p, w, n)


@pytest.mark.parametrize("p,w", FIELDS)
def test_aliased_output_and_host_forms(torch, p, w):
    n = 4097
    E = ER.Ext2(p, w)
    X = extension.Ext2(_Field(p), w)
    a, b, s = planar_words(1, n, p), planar_words(2, n, p), words(3, n, p)
    a[0], a[n] = 1, 0
    for i, x in enumerate(els(E, a)):
        if x == E.zero:
            a[i] = 1
    host_forms = {"add": X.vec_add(a, b), "sub": X.vec_sub(a, b), "mul": X.vec_mul(a, b), "neg": X.vec_neg(a),
                  "mul_base": X.vec_mul_base(a, s), "pow": X.vec_pow(a, 12345), "inv": X.vec_inv(a)}
    d_b, d_s = dev(torch, b), dev(torch, s)
    for name, want in host_forms.items():
        fn = getattr(L.lib, "ronk_ext2_vec_%s_dev" % name)
        d_a = dev(torch, a)      # the output overwrites the first operand
        if name in ("add", "sub", "mul"):
            got = run_dev(torch, fn, p, w, n, d_a, d_b, out=d_a)
        elif name == "mul_base":
            got = run_dev(torch, fn, p, w, n, d_a, d_s, out=d_a)
        elif name == "pow":
            got = run_dev(torch, fn, p, w, n, d_a, 12345, out=d_a)
        elif name == "inv":
            L.check(fn(p, w, d_a.data_ptr(), d_a.data_ptr(), n, None, 0))
            got = host(torch, d_a)
        else:
            got = run_dev(torch, fn, p, w, n, d_a, out=d_a)
        assert np.array_equal(got, want), (name, p)
    # the second operand as the output, and a square in place
    d_a, d_b2 = dev(torch, a), dev(torch, b)
    assert np.array_equal(run_dev(torch, L.lib.ronk_ext2_vec_mul_dev, p, w, n, d_a, d_b2, out=d_b2), host_forms["mul"])
    ea = els(E, a)
    assert run_dev(torch, L.lib.ronk_ext2_vec_mul_dev, p, w, n, d_a, d_a, out=d_a).tolist() == ER.planar([E.mul(x, x) for x in ea])
    assert host_forms["mul"].tolist() == ER.planar([E.mul(x, y) for x, y in zip(ea, els(E, b))])


def test_mirror_scalars_agree_with_the_device(torch, golden):
    X = extension.PlutoBaseFieldExtension
    a, b = X((10, 20)), X((20, 10))
    assert (a * b).coeffs == (2, 96) and (a + b).coeffs == (30, 30) and (-a).coeffs == (91, 81) and (a - b).coeffs == (91, 10)
    got = X.vec_mul(X.planar([a, a.inverse()]), X.planar([b, a]))
    assert got.tolist() == X.planar([a * b, X.one()]).tolist()
    assert X.vec_pow(X.planar([a]), 77).tolist() == list(a.pow(77).coeffs)
    assert (a / b) * b == a and a * 2 == a + a and a.norm() == X.BASE(10 * 10 + 2 * 20 * 20)


@pytest.mark.parametrize("p,w", FIELDS)
def test_under_stream_capture(torch, p, w):
    """no library workspace: the calls are legal under capture, and a replay gives the same words"""
    n = 4097
    E = ER.Ext2(p, w)
    a, b = planar_words(21, n, p), planar_words(22, n, p)
    d_a, d_b = dev(torch, a), dev(torch, b)
    d_out = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    d_out2 = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        L.check(L.lib.ronk_ext2_vec_mul_dev(p, w, d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), n, s.cuda_stream))
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        L.check(L.lib.ronk_ext2_vec_mul_dev(p, w, d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), n, st))
        L.check(L.lib.ronk_ext2_vec_pow_dev(p, w, d_out.data_ptr(), 5, d_out2.data_ptr(), n, st))
    want = [E.pow(E.mul(x, y), 5) for x, y in zip(els(E, a), els(E, b))]
    for _ in range(2):
        d_out.zero_(); d_out2.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert host(torch, d_out2).tolist() == ER.planar(want)
