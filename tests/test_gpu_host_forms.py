"""Every host-pointer entry point of the base-field half of the library against its `_dev` twin: the host form returns the same
words and the same code as uploading the input, calling the twin on a stream and downloading -- and, where the oracle covers the
entry point, the oracle's words.  Every comparison is bit-exact.  Shapes: 0 where legal, 1, 5 (odd and unaligned tails: the scalar
path of the vector kernels), 300 (more than one block), and the sizes at which an entry point changes its kernels."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
import poseidon_ref as PR
from oracle import bn254 as ob
from ronkathon_amd import _lib as L
from ronkathon_amd import callers as K

pytestmark = pytest.mark.gpu

GP, GG = L.GOLDILOCKS_P, L.GOLDILOCKS_G
MONT = 0xFFFFFFFC00000001
SIZES = (0, 1, 5, 300)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def stream(torch):
    return torch.cuda.Stream()


def vec(seed, n, p=GP):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    return v % np.uint64(p)


def nonzero(seed, n, p=GP):
    v = vec(seed, n, p)
    v[v == 0] = 1
    return v


ALIVE = []


@pytest.fixture(autouse=True)
def release_uploads():
    yield
    ALIVE.clear()


def up(torch, a):
    """a device copy (at least one word, so that an empty array still has an address), kept alive until the test ends: a call may
    be handed `up(..).data_ptr()` directly, and torch would give a dropped tensor's block to the next one while work is queued"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    ALIVE.append(torch.from_numpy((a if a.size else np.zeros(1, dtype=np.uint64)).view(np.int64).copy()).cuda())
    return ALIVE[-1]


def filled(torch, n, fill, dtype):
    t = torch.full((max(int(n), 1),), fill, dtype=dtype, device="cuda")
    torch.cuda.synchronize()       # the fill runs on torch's stream, the calls under test on their own
    return t


def blank(torch, n, fill=0x5A):
    return filled(torch, n, fill, torch.int64)


def status_word(torch, fill=0):
    return filled(torch, 2, fill, torch.int32)


def down(stream, t, n=None):
    stream.synchronize()
    a = t.cpu().numpy().view(np.uint64)
    return a if n is None else a[:n]


def sp(stream):
    return C.c_void_p(stream.cuda_stream)


def out(n):
    return np.full(max(int(n), 1), 0xA5, dtype=np.uint64)


# ------------------------------------------------------------------------------------- element-wise
@pytest.mark.parametrize("p", [GP, MONT, 101])
@pytest.mark.parametrize("n", SIZES)
def test_vector_binary_and_poly_add_sub(torch, stream, p, n):
    a, b = vec(1, n, p), vec(2, n, p)
    da, db = up(torch, a), up(torch, b)
    for name, ref in (("add", orc.vec_add), ("sub", orc.vec_sub), ("mul", orc.vec_mul)):
        h, d = out(n), blank(torch, n)
        L.check(getattr(L.lib, "ronk_vec_" + name)(p, L.ptr(a), L.ptr(b), L.ptr(h), n))
        L.check(getattr(L.lib, "ronk_vec_%s_dev" % name)(p, da.data_ptr(), db.data_ptr(), d.data_ptr(), n, sp(stream)))
        assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], ref(p, a, b)), (name, p, n)
    if n == 0:
        return
    # Polynomial + / -: the right-hand side zero-extended (shorter) or truncated (longer) to the left one's length
    for m in (max(n - 3, 1), n + 3):
        b2 = vec(3, m, p)
        ext = np.zeros(n, dtype=np.uint64)
        ext[:min(n, m)] = b2[:min(n, m)]
        dext = up(torch, ext)
        for name, ref in (("add", orc.poly_add), ("sub", orc.poly_sub)):
            h, d = out(n), blank(torch, n)
            L.check(getattr(L.lib, "ronk_poly_" + name)(p, L.ptr(a), n, L.ptr(b2), m, L.ptr(h)))
            L.check(getattr(L.lib, "ronk_vec_%s_dev" % name)(p, da.data_ptr(), dext.data_ptr(), d.data_ptr(), n, sp(stream)))
            assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], ref(p, a, b2)), (name, p, n, m)


@pytest.mark.parametrize("p", [GP, MONT, 101])
@pytest.mark.parametrize("n", SIZES)
def test_vector_unary(torch, stream, p, n):
    a = nonzero(4, n, p)
    da = up(torch, a)
    e = 0x123456789ABCDEF % (p - 1)
    h, d = out(n), blank(torch, n)
    L.check(L.lib.ronk_vec_neg(p, L.ptr(a), L.ptr(h), n))
    L.check(L.lib.ronk_vec_neg_dev(p, da.data_ptr(), d.data_ptr(), n, sp(stream)))
    assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], orc.vec_neg(p, a))
    h, d = out(n), blank(torch, n)
    L.check(L.lib.ronk_vec_pow(p, L.ptr(a), e, L.ptr(h), n))
    L.check(L.lib.ronk_vec_pow_dev(p, da.data_ptr(), e, d.data_ptr(), n, sp(stream)))
    assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], orc.vec_pow(p, a, e))
    h, d, st = out(n), blank(torch, n), status_word(torch)
    L.check(L.lib.ronk_vec_inv(p, L.ptr(a), L.ptr(h), n))
    L.check(L.lib.ronk_vec_inv_dev(p, da.data_ptr(), d.data_ptr(), n, st.data_ptr(), sp(stream)))
    assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], orc.vec_inv(p, a)) and int(st[0]) == 0
    h, d = out(n), blank(torch, n)
    L.check(L.lib.ronk_vec_euler(p, L.ptr(a), L.ptr(h), n))
    L.check(L.lib.ronk_vec_euler_dev(p, da.data_ptr(), d.data_ptr(), n, sp(stream)))
    assert np.array_equal(h[:n], down(stream, d, n)) and np.array_equal(h[:n], orc.vec_euler(p, a))
    sq = orc.vec_mul(p, a, a)      # residues
    dsq = up(torch, sq)
    h0, h1, d0, d1, st = out(n), out(n), blank(torch, n), blank(torch, n), status_word(torch)
    L.check(L.lib.ronk_vec_sqrt(p, L.ptr(sq), L.ptr(h0), L.ptr(h1), n))
    L.check(L.lib.ronk_vec_sqrt_dev(p, dsq.data_ptr(), d0.data_ptr(), d1.data_ptr(), n, st.data_ptr(), sp(stream)))
    r0, r1 = orc.vec_sqrt(p, sq)
    assert np.array_equal(h0[:n], down(stream, d0, n)) and np.array_equal(h1[:n], down(stream, d1, n)) and int(st[0]) == 0
    assert np.array_equal(h0[:n], r0) and np.array_equal(h1[:n], r1)


def test_vector_status_paths(torch, stream):
    a = nonzero(5, 300)
    a[277] = 0
    h, d, st = out(300), blank(torch, 300), status_word(torch)
    assert L.lib.ronk_vec_inv(GP, L.ptr(a), L.ptr(h), 300) == L.ERR_ZERO_INVERSE == -2
    L.check(L.lib.ronk_vec_inv_dev(GP, up(torch, a).data_ptr(), d.data_ptr(), 300, st.data_ptr(), sp(stream)))
    stream.synchronize()
    assert int(st[0]) != 0
    with pytest.raises(orc.OraclePanic):
        orc.vec_inv(GP, a)
    sq = orc.vec_mul(GP, a, a)
    sq[5] = 7                      # the generator of Goldilocks: no residue
    assert not orc.euler_criterion(GP, 7)
    h0, h1, d0, d1, st = out(300), out(300), blank(torch, 300), blank(torch, 300), status_word(torch)
    assert L.lib.ronk_vec_sqrt(GP, L.ptr(sq), L.ptr(h0), L.ptr(h1), 300) == L.ERR_NOT_RESIDUE == -13
    L.check(L.lib.ronk_vec_sqrt_dev(GP, up(torch, sq).data_ptr(), d0.data_ptr(), d1.data_ptr(), 300, st.data_ptr(), sp(stream)))
    stream.synchronize()
    assert int(st[0]) != 0


# ------------------------------------------------------------------------------------- evaluate, Lagrange, division, decode, MSM
@pytest.mark.parametrize("p", [GP, MONT, 101])
@pytest.mark.parametrize("d", SIZES)
def test_poly_eval(torch, stream, p, d):
    c, x = vec(6, d, p), int(vec(7, 1, p)[0])
    h, dv = C.c_uint64(0xA5), blank(torch, 1)
    L.check(L.lib.ronk_poly_eval(p, L.ptr(c) if d else L.ptr(out(1)), d, x, C.byref(h)))
    L.check(L.lib.ronk_poly_eval_dev(p, up(torch, c).data_ptr(), d, x, dv.data_ptr(), sp(stream)))
    assert h.value == int(down(stream, dv)[0]) == orc.poly_eval(p, c, x), (p, d)


@pytest.mark.parametrize("n", [4, 256])
def test_lagrange_eval(torch, stream, n):
    # 4: the general formula on arbitrary nodes; 256: the first size that tries the O(n) form on the device (omega^i nodes)
    nodes = orc.lagrange_nodes(GP, GG, n) if n == 256 else np.array([3, 0, GP - 1, 12345678901234567], dtype=np.uint64)
    c, x = vec(8, n), int(vec(9, 1)[0])
    h, dv, st = C.c_uint64(0xA5), blank(torch, 1), status_word(torch)
    L.check(L.lib.ronk_lagrange_eval(GP, L.ptr(c), L.ptr(nodes), n, x, C.byref(h)))
    L.check(L.lib.ronk_lagrange_eval_dev(GP, up(torch, c).data_ptr(), up(torch, nodes).data_ptr(), n, x, dv.data_ptr(), st.data_ptr(), sp(stream)))
    assert h.value == int(down(stream, dv)[0]) == orc.lagrange_eval(GP, c, nodes, x) and int(st[0]) == 0
    nodes = nodes.copy()
    nodes[n - 1] = nodes[1]        # coincident nodes
    st = status_word(torch)
    assert L.lib.ronk_lagrange_eval(GP, L.ptr(c), L.ptr(nodes), n, x, C.byref(h)) == L.ERR_ZERO_INVERSE == -2
    L.check(L.lib.ronk_lagrange_eval_dev(GP, up(torch, c).data_ptr(), up(torch, nodes).data_ptr(), n, x, dv.data_ptr(), st.data_ptr(), sp(stream)))
    stream.synchronize()
    assert int(st[0]) != 0 and not int(st[0]) & 4


def divrem_both(torch, stream, p, a, b):
    d, d2 = a.size, b.size
    hq, hr = out(d), out(d)
    rc = L.lib.ronk_poly_divrem(p, L.ptr(a), d, L.ptr(b), d2, L.ptr(hq), L.ptr(hr))
    dq, dr, st = blank(torch, d), blank(torch, d), status_word(torch, 77)
    L.check(L.lib.ronk_poly_divrem_dev(p, up(torch, a).data_ptr(), d, up(torch, b).data_ptr(), d2, dq.data_ptr(), dr.data_ptr(), st.data_ptr(),
                                       sp(stream)))
    q, r = down(stream, dq, d), down(stream, dr, d)
    return rc, hq, hr, int(st[0]), q, r


@pytest.mark.parametrize("p,d,d2", [(GP, 40, 7), (MONT, 40, 7), (101, 40, 7), (GP, 4096, 65)])
def test_poly_divrem_general(torch, stream, p, d, d2):
    """(40, 7): the long division; (4096, 65) over Goldilocks with full-length operands: the Newton window"""
    a, b = vec(10, d, p), vec(11, d2, p)
    a[d - 1] = b[d2 - 1] = 1
    rc, hq, hr, st, q, r = divrem_both(torch, stream, p, a, b)
    oq, orr = orc.poly_divrem(p, a, b)
    assert rc == 0 and st == 0
    assert np.array_equal(hq, q) and np.array_equal(hr, r) and np.array_equal(hq, oq) and np.array_equal(hr, orr)


@pytest.mark.parametrize("p", [GP, 101])
def test_poly_divrem_linear(torch, stream, p):
    """a divisor b0 + b1 x with d = 9: the host form takes the Horner scan (ronk_poly_div_linear_dev is its twin: the quotient and the
    ONE remainder word), the general _dev entry point the long division; both equal the oracle"""
    a, b = vec(12, 9, p), np.array([5, 3], dtype=np.uint64)
    rc, hq, hr, st, q, r = divrem_both(torch, stream, p, a, b)
    oq, orr = orc.poly_divrem(p, a, b)
    assert rc == 0 and st == 0
    assert np.array_equal(hq, q) and np.array_equal(hr, r) and np.array_equal(hq, oq) and np.array_equal(hr, orr)
    dq, dr = blank(torch, 9), blank(torch, 1)
    L.check(L.lib.ronk_poly_div_linear_dev(p, up(torch, a).data_ptr(), 9, 5, 3, dq.data_ptr(), dr.data_ptr(), sp(stream)))
    assert np.array_equal(hq, down(stream, dq, 9)) and hr[0] == down(stream, dr)[0] and not hr[1:].any()


def test_poly_divrem_zero_divisor(torch, stream):
    a, b = vec(13, 40), np.zeros(7, dtype=np.uint64)
    with pytest.raises(orc.OraclePanic) as e:
        orc.poly_divrem(GP, a, b)
    rc, _hq, _hr, st, _q, _r = divrem_both(torch, stream, GP, a, b)
    assert rc == st == e.value.code != 0


@pytest.mark.parametrize("k", [5, 1024])
def test_rs_decode(torch, stream, k):
    """5: the O(k^2) kernels; 1024: the first size that tries the O(k log k) form, on the geometric nodes of Message::encode.  The
    message is the oracle's input to Message::encode; its own O(k^3) decode is asked at k = 5 only."""
    msg = vec(14, k)
    xs, ys = orc.rs_encode(GP, GG, msg, 2 * k if k == 1024 else 8)
    xs, ys = xs[:k].copy(), ys[:k].copy()
    h, d, st = out(k), blank(torch, k), status_word(torch)
    L.check(L.lib.ronk_rs_decode(GP, L.ptr(xs), L.ptr(ys), k, L.ptr(h)))
    L.check(L.lib.ronk_rs_decode_dev(GP, up(torch, xs).data_ptr(), up(torch, ys).data_ptr(), k, d.data_ptr(), st.data_ptr(), sp(stream)))
    assert np.array_equal(h, down(stream, d, k)) and np.array_equal(h, msg)
    assert k > 5 or np.array_equal(h, orc.rs_decode(GP, xs, ys, k))
    assert int(st[0]) == 0
    xs[k - 1] = xs[0]              # coincident nodes
    st = status_word(torch)
    assert L.lib.ronk_rs_decode(GP, L.ptr(xs), L.ptr(ys), k, L.ptr(h)) == L.ERR_ZERO_INVERSE == -2
    L.check(L.lib.ronk_rs_decode_dev(GP, up(torch, xs).data_ptr(), up(torch, ys).data_ptr(), k, d.data_ptr(), st.data_ptr(), sp(stream)))
    stream.synchronize()
    assert int(st[0]) != 0 and not int(st[0]) & 4


@pytest.mark.parametrize("n", [1, 5, 300])
def test_curve_msm(torch, stream, refvec, n):
    v = refvec["curve"]
    cv, oc = K.Curve(v["p"], v["nr"], v["a"], v["b"]), orc.Curve(v["p"], v["nr"], v["a"], v["b"])
    pool = [orc.curve_mul(oc, v["g"], k) for k in range(0, 17)] + [orc.curve_mul(oc, v["g2"], k) for k in range(1, 12)]
    rng = np.random.default_rng(15)
    pts = [pool[i] for i in rng.integers(0, len(pool), n)]
    sc = rng.integers(0, 17, n).astype(np.uint64)
    flat = L.arr([w for pt in pts for w in pt])
    h, d, st = out(5), blank(torch, 5), status_word(torch)
    L.check(L.lib.ronk_curve_msm(C.byref(cv), L.ptr(flat), n, L.ptr(sc), n, L.ptr(h)))
    L.check(L.lib.ronk_curve_msm_dev(C.byref(cv), up(torch, flat).data_ptr(), n, up(torch, sc).data_ptr(), n, d.data_ptr(), st.data_ptr(),
                                     sp(stream)))
    assert h.tolist() == down(stream, d, 5).tolist() == orc.kzg_commit(oc, sc.tolist(), pts) and int(st[0]) == 0
    if n == 5:                     # a point off the curve
        flat[10:15] = L.arr(v["false_point"])
        st = status_word(torch)
        assert L.lib.ronk_curve_msm(C.byref(cv), L.ptr(flat), n, L.ptr(sc), n, L.ptr(h)) == L.ERR_NOT_ON_CURVE == -11
        L.check(L.lib.ronk_curve_msm_dev(C.byref(cv), up(torch, flat).data_ptr(), n, up(torch, sc).data_ptr(), n, d.data_ptr(),
                                         st.data_ptr(), sp(stream)))
        stream.synchronize()
        assert int(st[0]) & 2      # CURVE_ERR_NOT_ON_CURVE


# ------------------------------------------------------------------------------------- nodes, dft, products
@pytest.mark.parametrize("p,g,n", [(GP, GG, 1), (GP, GG, 5), (GP, GG, 320), (GP, GG, 768), (101, 2, 5), (MONT, 10, 7), (MONT, 10, 384)])
def test_lagrange_nodes_and_dft(torch, stream, p, g, n):
    """n must divide p - 1, so "odd" and "more than one block" are 5 and 320 = 64 * 5 over Goldilocks and 7 and 384 = 128 * 3 over the
    Montgomery prime: the direct kernel; 768 over Goldilocks: Bluestein (from 512 on).  The nodes have no _dev entry point: the
    oracle's."""
    h = out(n)
    L.check(L.lib.ronk_lagrange_nodes(p, g, L.ptr(h), n))
    assert np.array_equal(h, orc.lagrange_nodes(p, g, n))
    x = vec(16, n, p)
    h, d = out(n), blank(torch, n)
    L.check(L.lib.ronk_dft(p, g, L.ptr(x), L.ptr(h), n))
    L.check(L.lib.ronk_dft_dev(p, g, up(torch, x).data_ptr(), d.data_ptr(), n, sp(stream)))
    assert np.array_equal(h, down(stream, d, n)) and np.array_equal(h, orc.dft(p, g, x)), (p, n)


@pytest.mark.parametrize("p,g", [(GP, GG), (101, 2)])
@pytest.mark.parametrize("d,d2", [(1, 1), (5, 3), (300, 5), (300, 300)])
def test_poly_mul(torch, stream, p, g, d, d2):
    """products of up to 64 coefficients: the schoolbook kernel; beyond, over Goldilocks, the transforms"""
    a, b = vec(17, d, p), vec(18, d2, p)
    m = d + d2 - 1
    h, dv = out(m), blank(torch, m)
    L.check(L.lib.ronk_poly_mul(p, g, L.ptr(a), d, L.ptr(b), d2, L.ptr(h)))
    L.check(L.lib.ronk_poly_mul_dev(p, g, up(torch, a).data_ptr(), d, up(torch, b).data_ptr(), d2, dv.data_ptr(), sp(stream)))
    assert np.array_equal(h, down(stream, dv, m)) and np.array_equal(h, orc.poly_mul(p, a, b)), (p, d, d2)


# ------------------------------------------------------------------------------------- the product tree and what stands on it
def from_roots_ref(p, roots):
    acc = np.array([1], dtype=np.uint64)
    for r in roots:
        acc = orc.poly_mul(p, acc, np.array([(p - int(r)) % p, 1], dtype=np.uint64))
    return acc


@pytest.mark.parametrize("p", [GP, MONT])
@pytest.mark.parametrize("m", SIZES)
def test_poly_from_roots(torch, stream, p, m):
    r = vec(19, m, p)
    h, d = out(m + 1), blank(torch, m + 1)
    L.check(L.lib.ronk_poly_from_roots(p, L.ptr(r) if m else None, m, L.ptr(h)))
    L.check(L.lib.ronk_poly_from_roots_dev(p, up(torch, r).data_ptr() if m else None, m, d.data_ptr(), sp(stream)))
    assert np.array_equal(h, down(stream, d, m + 1)) and np.array_equal(h, from_roots_ref(p, r)), (p, m)


@pytest.mark.parametrize("p,g", [(GP, GG), (MONT, 10)])
def test_rs_recover(torch, stream, p, g):
    n, k = 64, 20
    msg = vec(20, k, p)
    _xs, ys = orc.rs_encode(p, g, msg, n)
    erased = np.array([0, 5, 63, 17, 40], dtype=np.uint64)
    got = ys.copy()
    got[erased.astype(np.int64)] = 12345
    hm, hf = out(k), out(n)
    L.check(L.lib.ronk_rs_recover(p, g, n, k, L.ptr(erased), erased.size, L.ptr(got), L.ptr(hm), L.ptr(hf)))
    plan = L.Plan(p, g, 6)
    dm, df, st = blank(torch, k), blank(torch, n), status_word(torch, 77)
    plan.rs_recover_batch_dev(k, up(torch, erased).data_ptr(), erased.size, up(torch, got).data_ptr(), dm.data_ptr(), df.data_ptr(),
                              st.data_ptr(), stream.cuda_stream)
    assert np.array_equal(hm, down(stream, dm, k)) and np.array_equal(hf, down(stream, df, n)) and int(st[0]) == 0
    assert np.array_equal(hm, msg) and np.array_equal(hf, ys)
    got[1] = (int(got[1]) + 1) % p      # a surviving value off the codeword: more than k survivors disagree
    st = status_word(torch, 77)
    assert L.lib.ronk_rs_recover(p, g, n, k, L.ptr(erased), erased.size, L.ptr(got), L.ptr(hm), None) == L.ERR_NOT_CODEWORD == -14
    plan.rs_recover_batch_dev(k, up(torch, erased).data_ptr(), erased.size, up(torch, got).data_ptr(), dm.data_ptr(), None, st.data_ptr(),
                              stream.cuda_stream)
    stream.synchronize()
    assert int(st[0]) == L.ERR_NOT_CODEWORD
    plan.close()


@pytest.mark.parametrize("p", [GP, MONT])
@pytest.mark.parametrize("m", [1, 5, 300])
def test_multipoint(torch, stream, p, m):
    c, x = vec(21, m + 2, p), np.unique(vec(22, m + 8, p))[:m].copy()
    assert x.size == m
    h, d = out(m), blank(torch, m)
    L.check(L.lib.ronk_poly_eval_many(p, L.ptr(c), c.size, L.ptr(x), m, L.ptr(h)))
    L.check(L.lib.ronk_poly_eval_many_dev(p, up(torch, c).data_ptr(), c.size, up(torch, x).data_ptr(), m, d.data_ptr(), sp(stream)))
    want = np.array([orc.poly_eval(p, c, int(v)) for v in x], dtype=np.uint64)
    assert np.array_equal(h, down(stream, d, m)) and np.array_equal(h, want), (p, m)
    y = vec(23, m, p)
    h, d, st = out(m), blank(torch, m), status_word(torch, 77)
    L.check(L.lib.ronk_poly_interpolate(p, L.ptr(x), L.ptr(y), m, L.ptr(h)))
    L.check(L.lib.ronk_poly_interpolate_dev(p, up(torch, x).data_ptr(), up(torch, y).data_ptr(), m, d.data_ptr(), st.data_ptr(), sp(stream)))
    assert np.array_equal(h, down(stream, d, m)) and int(st[0]) == 0
    assert [orc.poly_eval(p, h, int(v)) for v in x] == y.tolist(), (p, m)     # the polynomial of degree < m through the points


# ------------------------------------------------------------------------------------- Poseidon and Merkle
@pytest.mark.parametrize("p", [GP, MONT])
def test_hash_forms(torch, stream, p):
    P = PR.derive_params(p, 8, 7, 3, 4, 4)
    h = L.PoseidonHandle(*P.create_args())
    for length in (0, 1, 5, 8):
        x = vec(24, length, p)
        hs = out(8)
        L.check(L.lib.ronk_poseidon_hash(h.h, L.ptr(x) if length else None, length, L.ptr(hs)))
        state = np.zeros(8, dtype=np.uint64)
        state[:length] = x
        d = up(torch, state)
        h.permute_dev(d.data_ptr(), 1, stream.cuda_stream)
        assert hs.tolist() == down(stream, d, 8).tolist() == PR.permute(P, [int(v) for v in state]), (p, length)
    digest = 2
    for n_leaves, leaf_len in ((1, 5), (5, 3), (300, 5), (5, 0)):
        leaves = vec(25, n_leaves * leaf_len, p)
        words = L.merkle_tree_words(n_leaves, digest)
        ht, dt = out(words), blank(torch, words)
        L.check(L.lib.ronk_merkle_commit(h.h, L.ptr(leaves) if leaf_len else None, n_leaves, leaf_len, digest, L.ptr(ht)))
        h.merkle_commit_dev(up(torch, leaves).data_ptr() if leaf_len else None, n_leaves, leaf_len, leaf_len, 1, digest, dt.data_ptr(),
                            stream.cuda_stream)
        assert np.array_equal(ht, down(stream, dt, words)), (p, n_leaves, leaf_len)
        if n_leaves <= 5 and leaf_len:
            ref = PR.MerkleTree(P, [[int(v) for v in leaves[i * leaf_len:(i + 1) * leaf_len]] for i in range(n_leaves)], digest)
            assert ht.tolist() == [int(v) for v in ref.flat()]
        if n_leaves not in (5, 1) or leaf_len == 0:
            continue
        # three openings, the middle one with a wrong path word (one leaf: no path, a wrong leaf instead)
        depth = 0
        while L.merkle_level_offset(n_leaves, digest, depth + 1) < words:
            depth += 1
        idx = np.array([0, 1, 3] if n_leaves > 1 else [0, 0, 0], dtype=np.uint64)
        paths = np.zeros(max(idx.size * depth * digest, 1), dtype=np.uint64)
        stt = (C.c_int * idx.size)()
        L.check(L.lib.ronk_merkle_open(L.ptr(ht), n_leaves, digest, L.ptr(idx), idx.size, L.ptr(paths) if depth else None, stt))
        assert list(stt) == [0] * idx.size
        opened = np.concatenate([leaves[int(i) * leaf_len:(int(i) + 1) * leaf_len] for i in idx])
        if depth:
            paths[depth * digest] ^= np.uint64(1)
        else:
            opened[leaf_len] ^= np.uint64(1)
        root = ht[words - digest:].copy()
        ok = (C.c_int * idx.size)(*([9] * idx.size))
        L.check(L.lib.ronk_merkle_verify(h.h, L.ptr(opened), idx.size, leaf_len, L.ptr(idx), L.ptr(paths) if depth else None, n_leaves,
                                         digest, L.ptr(root), ok))
        dok = torch.full((idx.size,), 9, dtype=torch.int32, device="cuda")
        h.merkle_verify_dev(up(torch, opened).data_ptr(), idx.size, leaf_len, leaf_len, 1, up(torch, idx).data_ptr(),
                            up(torch, paths).data_ptr() if depth else None, n_leaves, digest, up(torch, root).data_ptr(), dok.data_ptr(),
                            stream.cuda_stream)
        stream.synchronize()
        assert list(ok) == dok.cpu().tolist() == [1, 0, 1], (p, n_leaves)
    h.close()


# ------------------------------------------------------------------------------------- BN254
def w4(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).copy()


def i4(words):
    buf = np.ascontiguousarray(words, dtype=np.uint64).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def test_bn254_forms(torch, stream):
    n = 3
    rng = np.random.default_rng(26)
    ks = [int.from_bytes(rng.bytes(32), "little") % ob.R for _ in range(n)]
    pts = ob.multiples(n)
    pw = np.concatenate([np.concatenate([w4([pt[0]]), w4([pt[1]])]) for pt in pts])
    sw = w4(ks)
    ho, do_ = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    L.check(L.lib.ronk_msm_bn254(L.ptr(pw), L.ptr(sw), n, L.ptr(ho)))
    L.check(L.lib.ronk_msm_bn254_dev(up(torch, pw).data_ptr(), up(torch, sw).data_ptr(), n, L.ptr(do_), sp(stream)))
    want = ob.msm(pts, ks)
    assert ho.tolist() == do_.tolist() and (i4(ho[:4])[0], i4(ho[4:])[0]) == want
    assert K.msm_bn254([], []) is None
    # kzg::open
    z = 12345
    zw = w4([z])
    hp, hv, dp, dv = (np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64))
    L.check(L.lib.ronk_kzg_open_bn254(L.ptr(sw), n, L.ptr(zw), L.ptr(pw), n, L.ptr(hp), L.ptr(hv)))
    dq = blank(torch, 4 * n)
    L.check(L.lib.ronk_kzg_open_bn254_dev(up(torch, sw).data_ptr(), n, L.ptr(zw), up(torch, pw).data_ptr(), dq.data_ptr(), L.ptr(dp), L.ptr(dv),
                                          sp(stream)))
    proof, value = ob.kzg_open(ks, z, pts)
    assert hp.tolist() == dp.tolist() and hv.tolist() == dv.tolist()
    assert (i4(hp[:4])[0], i4(hp[4:])[0]) == (proof or (0, 0)) and i4(hv)[0] == value
    L.check(L.lib.ronk_kzg_open_bn254(L.ptr(sw), n, L.ptr(zw), L.ptr(pw), n, L.ptr(dp), None))      # the value is optional
    assert dp.tolist() == hp.tolist()
    # transforms of 4 points (a batch of one) and the product 3 x 3
    x = w4([int.from_bytes(rng.bytes(32), "little") % ob.R for _ in range(4)])
    plan = L.FrPlan(2)
    for host_fn, dev_fn in ((L.lib.ronk_ntt_forward_bn254, plan.forward_dev), (L.lib.ronk_ntt_inverse_bn254, plan.inverse_dev)):
        h, d = out(16), blank(torch, 16)
        L.check(host_fn(2, L.ptr(x), L.ptr(h)))
        dev_fn(up(torch, x).data_ptr(), d.data_ptr(), 1, sp(stream))
        assert np.array_equal(h, down(stream, d, 16))
    assert K.intt_bn254(K.ntt_bn254(i4(x))) == i4(x)
    omega = pow(5, (ob.R - 1) // 4, ob.R)
    assert K.ntt_bn254(i4(x)) == [sum(c * pow(omega, i * j, ob.R) for j, c in enumerate(i4(x))) % ob.R for i in range(4)]
    plan.close()
    a, b = w4(ks), x[:12]
    h, d = out(20), blank(torch, 20)
    L.check(L.lib.ronk_poly_mul_bn254(L.ptr(a), 3, L.ptr(b), 3, L.ptr(h)))
    L.check(L.lib.ronk_poly_mul_bn254_dev(up(torch, a).data_ptr(), 3, up(torch, b).data_ptr(), 3, d.data_ptr(), sp(stream)))
    ai, bi = i4(a), i4(b)
    want = [sum(ai[i] * bi[t - i] for i in range(3) if 0 <= t - i < 3) % ob.R for t in range(5)]
    assert np.array_equal(h, down(stream, d, 20)) and i4(h) == want


# ------------------------------------------------------------------------------------- the workspace pool
def test_pool_across_streams_and_a_trim(torch):
    """ronk_poly_eval_dev of 5000 coefficients on stream A, on stream B (the pool goes multi-stream here), ronk_trim_workspace, and
    on A again: four times the oracle's value"""
    c, x = vec(27, 5000), int(vec(28, 1)[0])
    want = orc.poly_eval(GP, c, x)
    dc = up(torch, c)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got = []
    for s in (sa, sb, None, sa, sb):
        if s is None:
            assert L.lib.ronk_trim_workspace() == 0
            continue
        d = blank(torch, 1)
        L.check(L.lib.ronk_poly_eval_dev(GP, dc.data_ptr(), 5000, x, d.data_ptr(), sp(s)))
        got.append(int(down(s, d)[0]))
    assert got == [want] * 4
