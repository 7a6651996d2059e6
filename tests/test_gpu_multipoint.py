"""Multipoint evaluation and interpolation at arbitrary points (ronk_poly_eval_many(_dev), ronk_poly_interpolate(_dev);
csrc/multipoint_kernels.h).  Every comparison is bit-exact.

Every output of every evaluation case is compared against the oracle's Polynomial::evaluate (orc.poly_eval), point by point; the
oracle's calls for one polynomial are spread over a pool of threads (ctypes releases the interpreter lock), which keeps the
largest case (m = 2^14 + 3 points, d = 3m + 7 coefficients: 8 * 10^8 oracle products) at about a second."""
from concurrent.futures import ThreadPoolExecutor
import json
import os

import numpy as np
import pytest

import oracle as orc
import prime_classes as PC
import ronkathon_amd as R
from ronkathon_amd import _lib as L
from ronkathon_amd.callers import poly_eval_many, poly_interpolate
from ronkathon_amd.polynomial import Polynomial

pytestmark = pytest.mark.gpu

GP = R.GOLDILOCKS_P
MONT = [0xFFFFFFFC00000001, 29 * 2**57 + 1]   # test_gpu_rs_recover.py's primes
PRIMES = [GP] + MONT
G = L.ROOTS_LEAF
SIZES = [1, 2, 63, 64, 65, 128, 197, 1000, 4096, 2**14 + 3]
POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class form:
    """RONK_MULTIPOINT_FORM for the calls inside the block (None: the library's choice)"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = os.environ.pop("RONK_MULTIPOINT_FORM", None)
        if self.name:
            os.environ["RONK_MULTIPOINT_FORM"] = self.name

    def __exit__(self, *a):
        os.environ.pop("RONK_MULTIPOINT_FORM", None)
        if self.old is not None:
            os.environ["RONK_MULTIPOINT_FORM"] = self.old


def field_vec(seed, size, p=GP):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    return v % np.uint64(p)


def points_with_repeats(seed, m, p):
    x = field_vec(seed, m, p)
    if m >= 3:
        x[1] = 0
        x[m - 1] = x[0]
    return x


def distinct_nodes(seed, m, p):
    """m distinct residues in a seeded random order, ZERO among them"""
    v = np.unique(field_vec(seed, m + m // 8 + 16, p))
    v = v[v != 0][: m - 1]
    assert v.size == m - 1
    v = np.concatenate([v, np.zeros(1, dtype=np.uint64)])
    np.random.default_rng(seed + 1).shuffle(v)
    return v


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def eval_host(p, c, x):
    out = np.empty(x.size, dtype=np.uint64)
    L.check(L.lib.ronk_poly_eval_many(p, L.ptr(c), c.size, L.ptr(x), x.size, L.ptr(out)))
    return out


def eval_dev(torch, p, c, x):
    d_c, d_x = dev(torch, c), dev(torch, x)
    d_out = torch.empty(x.size, dtype=torch.int64, device="cuda")
    L.check(L.lib.ronk_poly_eval_many_dev(p, d_c.data_ptr(), c.size, d_x.data_ptr(), x.size, d_out.data_ptr(), None))
    return host(torch, d_out)


def interp_host_rc(p, x, y):
    out = np.empty(x.size, dtype=np.uint64)
    return L.lib.ronk_poly_interpolate(p, L.ptr(x), L.ptr(y), x.size, L.ptr(out)), out


def interp_dev(torch, p, x, y):
    d_x, d_y = dev(torch, x), dev(torch, y)
    d_out = torch.empty(x.size, dtype=torch.int64, device="cuda")
    d_st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_poly_interpolate_dev(p, d_x.data_ptr(), d_y.data_ptr(), x.size, d_out.data_ptr(), d_st.data_ptr(), None))
    out = host(torch, d_out)
    return int(d_st.cpu()[0]), out


def oracle_values(p, c, x, idx=None):
    """orc.poly_eval at x[i] for every i (or for i in idx), in order"""
    idx = list(range(x.size)) if idx is None else list(idx)
    c = np.ascontiguousarray(c, dtype=np.uint64)
    pts = [int(x[i]) for i in idx]
    if len(pts) * c.size < 2**22:
        return [orc.poly_eval(p, c, v) for v in pts]
    step = max(1, len(pts) // 256)
    parts = POOL.map(lambda lo: [orc.poly_eval(p, c, v) for v in pts[lo:lo + step]], range(0, len(pts), step))
    return [v for part in parts for v in part]


def check_values(p, c, x, got):
    """every output against the oracle"""
    assert [int(v) for v in got] == oracle_values(p, c, x), (p, x.size, c.size)


def coeff_counts(m):
    return [1, m, 3 * m + 7] + ([2**16] if m == 4096 else [])


def check_eval_many_both_forms(torch, p, m):
    for d in coeff_counts(m):
        c = field_vec(m * 31 + d, d, p)
        x = points_with_repeats(m * 7 + d, m, p)
        with form("tree"):
            tree = eval_host(p, c, x)
            tree_dev = eval_dev(torch, p, c, x)
        with form("direct"):
            direct = eval_host(p, c, x)
            direct_dev = eval_dev(torch, p, c, x)
        with form(None):
            auto = eval_dev(torch, p, c, x)
        check_values(p, c, x, direct)
        for other in (tree, tree_dev, direct_dev, auto):
            assert np.array_equal(other, direct), (p, m, d)


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("p", PRIMES)
def test_eval_many_against_oracle_both_forms(torch, p, m):
    check_eval_many_both_forms(torch, p, m)


@pytest.mark.parametrize("m", [65, 4096])
def test_eval_many_both_forms_p_mid(torch, m):
    """one leaf past the first and a full tree over the prime whose sums take every outcome of mont64::add (tests/prime_classes.py)"""
    check_eval_many_both_forms(torch, PC.P_MID, m)


def test_eval_many_unreduced_points_and_python_mirrors():
    p = MONT[0]
    c = field_vec(5, 300, p)
    x = field_vec(6, 200, GP)   # values up to 2^64 - 2^32: reduced mod p by the call
    for name in ("tree", "direct"):
        with form(name):
            assert [int(v) for v in eval_host(p, c, x)] == [orc.poly_eval(p, c, int(v) % p) for v in x]
    F = R.PrimeField(p)
    f = Polynomial.new(F, c)
    assert np.array_equal(f.evaluate_many(x[:50]), poly_eval_many(F, c, [int(v) for v in x[:50]]))
    assert [int(v) for v in f.evaluate_many(x[:5])] == [f.evaluate(int(v)).value for v in x[:5]]
    g = poly_interpolate(F, [1, 2, 3], [int(f.evaluate(v).value) for v in (1, 2, 3)])
    assert [int(g.evaluate(v).value) for v in (1, 2, 3)] == [int(f.evaluate(v).value) for v in (1, 2, 3)]


@pytest.mark.parametrize("p", [101, 17])
def test_small_primes_direct_form(p):
    for m in (1, 2, 16, 17, 64, 65, 100):
        for d in (1, m, 3 * m + 7):
            c = field_vec(m + d, d, p)
            x = field_vec(m * 3 + d, m, p)
            assert [int(v) for v in eval_host(p, c, x)] == oracle_values(p, c, x), (p, m, d)
    # the tree form does not serve these fields (no 2^7 | p - 1 for the root's products)
    with form("tree"):
        one = np.ones(4, dtype=np.uint64)
        assert L.lib.ronk_poly_eval_many(p, L.ptr(one), 4, L.ptr(one), 4, L.ptr(one.copy())) == L.ERR_UNSUPPORTED
    # interpolation: distinct nodes of the field, the O(m^2) form
    m = p - 1
    x = np.arange(1, p, dtype=np.uint64)[::-1].copy()
    f = field_vec(p, m, p)
    y = np.array(oracle_values(p, f, x), dtype=np.uint64)
    rc, out = interp_host_rc(p, x, y)
    assert rc == 0 and np.array_equal(out, f)


def test_interpolate_reference_reed_solomon_vectors():
    """the reference's own Reed-Solomon vectors (tests/golden): interpolation equals the oracle's Message::decode"""
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as fh:
        d = json.load(fh)["rs_decode"]
    p = d["p"]
    g = orc.find_primitive_element(p)
    for msg in d["cases"]:
        xs, ys = orc.rs_encode(p, g, msg, d["n"])
        for sel in (list(range(len(msg))), [6, 1, 4, 0, 3][: len(msg)]):
            x, y = np.ascontiguousarray(xs[sel]), np.ascontiguousarray(ys[sel])
            rc, out = interp_host_rc(p, x, y)
            assert rc == 0 and out.tolist() == orc.rs_decode(p, x, y, len(sel)).tolist()


def py_lagrange(p, xs, ys):
    """the Lagrange sum in Python integers: sum_i y_i prod_{j != i} (x - x_j) / (x_i - x_j), ascending coefficients"""
    m = len(xs)
    z = [1]
    for r in xs:
        nx = [0] * (len(z) + 1)
        for j, v in enumerate(z):
            nx[j + 1] = (nx[j + 1] + v) % p
            nx[j] = (nx[j] - r * v) % p
        z = nx
    out = [0] * m
    for i in range(m):
        q, carry = [0] * m, 0          # z / (x - x_i) by synthetic division
        for j in range(m, 0, -1):
            carry = (z[j] + carry * xs[i]) % p
            q[j - 1] = carry
        den = 0
        for v in reversed(q):
            den = (den * xs[i] + v) % p
        w = ys[i] * pow(den, p - 2, p) % p
        for j in range(m):
            out[j] = (out[j] + w * q[j]) % p
    return out


@pytest.mark.parametrize("p", PRIMES)
def test_interpolate_small_against_python_lagrange(torch, p):
    for m in (1, 2, 63, 64, 65, 128, 197):
        x = distinct_nodes(m * 11, m, p)
        y = field_vec(m * 13, m, p)
        want = py_lagrange(p, [int(v) for v in x], [int(v) for v in y])
        for name in ("tree", "direct"):
            with form(name):
                rc, out = interp_host_rc(p, x, y)
                st, out_dev = interp_dev(torch, p, x, y)
            assert rc == 0 and st == 0 and [int(v) for v in out] == want and np.array_equal(out, out_dev), (p, m, name)


def values_of(p, f, x):
    """the values of f at x from the oracle; beyond the listed sizes (2^15 and 2^17 nodes) from the library, whose values the
    evaluation tests check, with 16 seeded indices against the oracle"""
    if x.size <= SIZES[-1]:
        return np.array(oracle_values(p, f, x), dtype=np.uint64)
    y = eval_host(p, f, x)
    idx = [int(i) for i in np.random.default_rng(x.size).integers(0, x.size, size=16)]
    assert [int(y[i]) for i in idx] == oracle_values(p, f, x, idx)
    return y


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("p", PRIMES)
def test_interpolate_recovers_polynomial(torch, p, m):
    x = distinct_nodes(m * 17 + 1, m, p)
    f = field_vec(m * 19, m, p)
    y = values_of(p, f, x)
    with form("tree"):
        rc, out = interp_host_rc(p, x, y)
        st, out_dev = interp_dev(torch, p, x, y)
    assert rc == 0 and st == 0 and np.array_equal(out, f) and np.array_equal(out_dev, f), (p, m)
    with form(None):
        rc, out = interp_host_rc(p, x, y)
    assert rc == 0 and np.array_equal(out, f)
    if m <= 2**14:
        with form("direct"):
            rc, out = interp_host_rc(p, x, y)
        assert rc == 0 and np.array_equal(out, f)
        if m <= 197:   # the same polynomial as Message::decode's, where the oracle's O(m^2) loop is affordable
            assert np.array_equal(L.arr(orc.rs_decode(p, x, y, m)), out)


@pytest.mark.parametrize("m", [2**15, 2**17])
def test_interpolate_beyond_the_decode_limit(torch, m):
    """sizes ronk_rs_decode refuses for arbitrary nodes -- and still refuses"""
    p = GP
    x = distinct_nodes(m, m, p)
    f = field_vec(m + 5, m, p)
    y = values_of(p, f, x)
    refused = np.empty(m, dtype=np.uint64)
    assert L.lib.ronk_rs_decode(p, L.ptr(x), L.ptr(y), m, L.ptr(refused)) == L.ERR_UNSUPPORTED
    rc, out = interp_host_rc(p, x, y)
    assert rc == 0 and np.array_equal(out, f)
    st, out_dev = interp_dev(torch, p, x, y)
    assert st == 0 and np.array_equal(out_dev, f)


@pytest.mark.parametrize("p", PRIMES)
def test_repeated_node_is_zero_inverse(torch, p):
    for m, name in ((5, "direct"), (5, "tree"), (300, "direct"), (300, "tree"), (5000, None)):
        x = distinct_nodes(m, m, p)
        x[m - 2] = x[m // 2]
        y = field_vec(m + 1, m, p)
        with form(name):
            rc, _ = interp_host_rc(p, x, y)
            st, _ = interp_dev(torch, p, x, y)
        assert rc == L.ERR_ZERO_INVERSE and st == L.ERR_ZERO_INVERSE, (p, m, name)
    with pytest.raises(L.RonkPanic) as e:
        poly_interpolate(R.GoldilocksField, [1, 2, 1], [3, 4, 5])
    assert e.value.code == L.ERR_ZERO_INVERSE


def test_large_goldilocks(torch):
    m = d = 2**20
    x = distinct_nodes(20, m, GP)
    f = field_vec(21, d, GP)
    d_f, d_x = dev(torch, f), dev(torch, x)
    d_y = torch.empty(m, dtype=torch.int64, device="cuda")
    L.check(L.lib.ronk_poly_eval_many_dev(GP, d_f.data_ptr(), d, d_x.data_ptr(), m, d_y.data_ptr(), None))
    y = host(torch, d_y)
    idx = sorted(set(list(range(G)) + list(range(m - G, m)) + [int(i) for i in np.random.default_rng(22).integers(0, m, size=64)]))
    assert [int(y[i]) for i in idx] == oracle_values(GP, f, x, idx)
    d_out = torch.empty(m, dtype=torch.int64, device="cuda")
    d_st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_poly_interpolate_dev(GP, d_x.data_ptr(), d_y.data_ptr(), m, d_out.data_ptr(), d_st.data_ptr(), None))
    out = host(torch, d_out)
    assert int(d_st.cpu()[0]) == 0 and np.array_equal(out, f)


def test_random_sweep():
    """seeded by the clock unless RONK_SWEEP_SEED is set; a failure prints the seed"""
    seed = int.from_bytes(os.urandom(4), "little") if os.environ.get("RONK_SWEEP_SEED") is None else int(os.environ["RONK_SWEEP_SEED"])
    rng = np.random.default_rng(seed)
    for _ in range(100):
        p = PRIMES[int(rng.integers(0, 3))]
        m, d = int(rng.integers(1, 5001)), int(rng.integers(1, 5001))
        name = ("tree", "direct", None)[int(rng.integers(0, 3))]
        tag = "seed %d: p=%d m=%d d=%d form=%s" % (seed, p, m, d, name)
        c = field_vec(int(rng.integers(0, 2**31)), d, p)
        x = points_with_repeats(int(rng.integers(0, 2**31)), m, p)
        with form(name):
            got = eval_host(p, c, x)
        idx = [int(i) for i in rng.integers(0, m, size=8)]
        assert [int(got[i]) for i in idx] == oracle_values(p, c, x, idx), tag
        xi = distinct_nodes(int(rng.integers(0, 2**31)), m, p)
        with form(name):
            yi = eval_host(p, c, xi)
            rc, out = interp_host_rc(p, xi, yi)
            assert rc == 0, tag
            if d <= m:   # the interpolant of f's values is f
                assert np.array_equal(out[:d], c) and not out[d:].any(), tag
            else:        # ... or f mod prod (x - x_i): the same values at the nodes
                assert np.array_equal(eval_host(p, out, xi), yi), tag
