"""The fused PLONK quotient on the device (ronk_plonk_quotient_dev, ronk_plonk_quotient) bit for bit against the Python
restatement tests/plonk_ref.py, over Goldilocks (its own arithmetic, w = 7 and w = 11), MONT_P, P_MID and P_62 (the Montgomery
policy).  The kernel is pointwise, so the rows are random words (0, p - 1 and words >= p among them) and no valid witness is
needed; the last test runs a valid circuit through ronk_perm_product_dev, ronk_lde_batch_dev and the quotient and checks that T is
a polynomial.

The blocking under test (csrc/plonk_kernels.h): a lane owns the rows i + t M / R (R = 4 over Goldilocks, 8 over a Montgomery prime;
one row below M = R), row i reads Z at row (i + B) mod M, and the vanishing inverse comes from a table indexed by i mod B."""
import ctypes as C

import numpy as np
import pytest

import plonk_ref as PR
import prime_classes as PC
from ronkathon_amd import _lib as L
from test_gpu_fri import dev, host, words

pytestmark = pytest.mark.gpu

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
GEN = {**PC.GEN, GL: 7}
FIELDS = [(GL, 7), (GL, 11), (MONT, 10), (PC.P_MID, PC.GEN[PC.P_MID]), (PC.P_62, PC.GEN[PC.P_62])]
SMALL = [3, 4, 6, 8, 11, 12, 13]       # log2 M, every row compared
LARGE = [16, 20]                       # sampled
K = PR.LABELS


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


class Handle:
    def __init__(self, p, g, w, log2_n, log2_b, shift, k=K):
        self.h = C.c_void_p()
        L.check(L.lib.ronk_plonk_create(C.byref(self.h), p, g, w, log2_n, log2_b, shift, (C.c_uint64 * 3)(*k)))

    def close(self):
        if self.h:
            L.check(L.lib.ronk_plonk_destroy(self.h))
            self.h = None


def garbage(torch, n):
    return torch.full((n,), -1, dtype=torch.int64, device="cuda")


class Case:
    """random words for one (field, M, B), on the host and on the device; or the caller's `host` arrays in their place: wires 3M,
    selectors 5M, sigma 3M, pi M, Z 2M, then alpha, beta, gamma of two words each"""

    def __init__(self, torch, p, w, log2_m, log2_b, seed=0, host=None):
        self.p, self.w, self.M, self.log2_m, self.log2_b = p, w, 1 << log2_m, log2_m, log2_b
        M = self.M
        self.E = PR.Ext2(p, w)
        self.dom = PR.Domain(p, GEN[p], log2_m - log2_b, log2_b, GEN[p])
        s = 1000 * log2_m + 10 * log2_b + seed
        self.host = host if host is not None else \
            [words(s + j, k * M, p) for j, k in enumerate((3, 5, 3, 1, 2))] + [words(s + 5 + j, 2, p) for j in range(3)]
        assert [a.size for a in self.host] == [3 * M, 5 * M, 3 * M, M, 2 * M, 2, 2, 2]
        self.dev = [dev(torch, a) for a in self.host]
        self.handle = Handle(p, GEN[p], w, log2_m - log2_b, log2_b, GEN[p])
        wires, sel, sigma, pi, Z = self.host[:5]
        self.cols = PR.Columns(wires.reshape(3, M), sel.reshape(5, M), sigma.reshape(3, M), pi, Z.reshape(2, M))
        self.ch = [a.tolist() for a in self.host[5:]]

    def call(self, torch, d_T, with_pi=True, stream=0):
        p = [t.data_ptr() for t in self.dev]
        L.check(L.lib.ronk_plonk_quotient_dev(self.handle.h, p[0], p[1], p[2], p[3] if with_pi else None, p[4], p[5], p[6], p[7],
                                              d_T.data_ptr(), stream))

    def want_rows(self, rows, with_pi=True):
        cols = self.cols if with_pi else PR.Columns(self.cols.wires, self.cols.sel, self.cols.sigma, None, self.cols.Z)
        return [PR.quotient_row(self.E, self.dom, cols, *self.ch, int(i)) for i in rows]

    def want_all(self, with_pi=True):
        cols = self.cols if with_pi else PR.Columns(self.cols.wires, self.cols.sel, self.cols.sigma, None, self.cols.Z)
        return np.array(PR.planar(PR.quotient(self.E, self.dom, cols, *self.ch)), dtype=np.uint64)

    def inputs_unchanged(self, torch):
        return all(np.array_equal(host(torch, d), h) for d, h in zip(self.dev, self.host))


@pytest.mark.parametrize("log2_m", SMALL)
@pytest.mark.parametrize("p,w", FIELDS)
def test_every_row_against_the_restatement(torch, p, w, log2_m):
    """B = 2, 4, 8 where B < M; with the public-input column and, at B = 4, without it"""
    for log2_b in (1, 2, 3):
        if log2_b >= log2_m:
            continue
        c = Case(torch, p, w, log2_m, log2_b)
        d_T = garbage(torch, 2 * c.M)
        c.call(torch, d_T)
        assert np.array_equal(host(torch, d_T), c.want_all()), (p, w, log2_m, log2_b)
        if log2_b == 2:
            d_T.fill_(-1)
            c.call(torch, d_T, with_pi=False)
            assert np.array_equal(host(torch, d_T), c.want_all(with_pi=False)), (p, w, log2_m, "no pi")
        assert c.inputs_unchanged(torch)
        c.handle.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_fewer_rows_than_a_lane_owns(torch, p, w):
    """M = 2 (B = 1) and M = 4 (B = 2): the one-row-per-lane kernel"""
    for log2_m, log2_b in ((1, 0), (2, 1)):
        c = Case(torch, p, w, log2_m, log2_b, seed=2)
        d_T = garbage(torch, 2 * c.M)
        c.call(torch, d_T)
        assert np.array_equal(host(torch, d_T), c.want_all()), (p, w, log2_m)
        c.handle.close()


@pytest.mark.parametrize("log2_m", LARGE)
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_large_sizes_at_sampled_rows(torch, p, w, log2_m):
    """B = 4: the first and last 2 B rows, the 2 B rows on either side of every eighth of M (where the rows of a lane start),
    and 4096 seeded rows, which reach every quarter of M"""
    B = 4
    c = Case(torch, p, w, log2_m, 2)
    M = c.M
    d_T = garbage(torch, 2 * M)
    c.call(torch, d_T)
    got = host(torch, d_T)
    rng = np.random.default_rng(log2_m)
    edges = np.concatenate([np.arange(q * M // 8 - 2 * B, q * M // 8 + 2 * B) for q in range(9)])
    rows = np.unique(np.concatenate([edges[(edges >= 0) & (edges < M)], rng.integers(0, M, size=4096)]))
    assert set(range(2 * B)) <= set(rows.tolist()) and set(range(M - 2 * B, M)) <= set(rows.tolist())
    assert all(((rows >= q * M // 4) & (rows < (q + 1) * M // 4)).sum() > 500 for q in range(4))
    want = c.want_rows(rows)
    assert [(int(got[i]), int(got[M + i])) for i in rows] == want, (p, log2_m)
    assert c.inputs_unchanged(torch)
    c.handle.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_null_pi_is_a_zero_column(torch, p, w):
    c = Case(torch, p, w, 11, 2, seed=3)
    d_null, d_zero = garbage(torch, 2 * c.M), garbage(torch, 2 * c.M)
    c.call(torch, d_null, with_pi=False)
    c.dev[3].zero_()
    c.call(torch, d_zero)
    assert np.array_equal(host(torch, d_null), host(torch, d_zero))
    assert np.array_equal(host(torch, d_null), c.want_all(with_pi=False))
    c.handle.close()


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_under_stream_capture(torch, p, w):
    """one launch, no library workspace and no host round trip: legal under capture, and two replays give the direct call's words"""
    c = Case(torch, p, w, 12, 2, seed=4)
    d_direct, d_T = garbage(torch, 2 * c.M), garbage(torch, 2 * c.M)
    c.call(torch, d_direct)
    direct = host(torch, d_direct)
    assert np.array_equal(direct, c.want_all())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        c.call(torch, d_T, stream=s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        c.call(torch, d_T, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        d_T.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(torch, d_T), direct)
    c.handle.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_host_pointer_form(torch, p, w):
    c = Case(torch, p, w, 8, 2, seed=5)
    T = np.full(2 * c.M, 2**64 - 1, dtype=np.uint64)
    a = c.host
    L.check(L.lib.ronk_plonk_quotient(c.handle.h, L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]), L.ptr(a[3]), L.ptr(a[4]), L.ptr(a[5]), L.ptr(a[6]),
                                      L.ptr(a[7]), L.ptr(T)))
    assert np.array_equal(T, c.want_all())
    L.check(L.lib.ronk_plonk_quotient(c.handle.h, L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]), None, L.ptr(a[4]), L.ptr(a[5]), L.ptr(a[6]),
                                      L.ptr(a[7]), L.ptr(T)))
    assert np.array_equal(T, c.want_all(with_pi=False))
    c.handle.close()
    # and the Python wrapper over it
    from ronkathon_amd import callers

    class F:
        ORDER = p
    M = c.M
    got = callers.plonk_quotient(F, GEN[p], w, 6, 2, GEN[p], a[0].reshape(3, M), a[1].reshape(5, M), a[2].reshape(3, M), a[3],
                                 a[4].reshape(2, M), *c.ch)
    assert np.array_equal(got, c.want_all())
    with pytest.raises(L.RonkPanic) as e:
        callers.plonk_quotient(F, GEN[p], w, 6, 2, 1, a[0].reshape(3, M), a[1].reshape(5, M), a[2].reshape(3, M), None, a[4].reshape(2, M),
                               *c.ch)
    assert e.value.code == L.ERR_UNSUPPORTED        # the shift 1 lies on the domain


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_end_to_end_through_the_existing_entry_points(torch, p, w):
    """a valid generated circuit: Z by ronk_perm_product_dev, the columns and the planes of Z extended by ronk_lde_batch_dev, the
    quotient, ronk_ntt_inverse_dev per plane and the un-shift by s^-i: the coefficients from 3N - 3 upward are zero, and with one
    witness cell changed they are not"""
    log2_n, log2_b = 6, 2
    g = shift = GEN[p]
    N, M = 1 << log2_n, 1 << (log2_n + log2_b)
    rng = np.random.default_rng(60)
    dom = PR.Domain(p, g, log2_n, log2_b, shift)
    c = PR.circuit(rng, p, log2_n)
    ids = PR.labels(dom)
    sigma = PR.sigma_of(c, ids)
    ch = [[int(v) % p for v in rng.integers(0, 2**62, size=2)] for _ in range(3)]
    d_ch = [dev(torch, np.array(v, dtype=np.uint64)) for v in ch]
    handle = Handle(p, g, w, log2_n, log2_b, shift)
    pk, pn = L.Plan(p, g, log2_n, 16), L.Plan(p, g, log2_n + log2_b, 16)
    inv = L.Plan(p, g, log2_n + log2_b, 1)
    sinv = pow(shift, -1, p)
    unshift = [pow(sinv, j, p) for j in range(M)]

    def high_coefficients(wires):
        d_w, d_i, d_s = (dev(torch, np.array(a, dtype=np.uint64).ravel()) for a in (wires, ids, sigma))
        d_Z, d_last, d_work = garbage(torch, 2 * N), garbage(torch, 2), garbage(torch, L.lib.ronk_scan_workspace_words(N))
        d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        L.check(L.lib.ronk_perm_product_dev(p, w, d_w.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), 3, N, d_ch[1].data_ptr(),
                                            d_ch[2].data_ptr(), d_Z.data_ptr(), d_last.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), 0))
        assert int(d_st.item()) == 0
        last = tuple(host(torch, d_last).tolist())
        # one batch of 16 columns: wires 3, selectors 5, sigma 3, pi 1, the two planes of Z as the device left them, two spare
        d_in = torch.cat([dev(torch, np.array(wires + c.sel + sigma + [c.pi], dtype=np.uint64).ravel()), d_Z,
                          torch.zeros(2 * N, dtype=torch.int64, device="cuda")])
        d_co, d_cols = garbage(torch, 16 * N), garbage(torch, 16 * M)
        L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_in.data_ptr(), d_co.data_ptr(), d_cols.data_ptr(), shift, 0))
        d_T = garbage(torch, 2 * M)
        base = d_cols.data_ptr()
        L.check(L.lib.ronk_plonk_quotient_dev(handle.h, base, base + 8 * 3 * M, base + 8 * 8 * M, base + 8 * 11 * M, base + 8 * 12 * M,
                                              d_ch[0].data_ptr(), d_ch[1].data_ptr(), d_ch[2].data_ptr(), d_T.data_ptr(), 0))
        d_c = garbage(torch, 2 * M)
        for plane in (0, 1):
            L.check(L.lib.ronk_ntt_inverse_dev(inv.h, d_T.data_ptr() + 8 * plane * M, d_c.data_ptr() + 8 * plane * M, 0))
        coef = host(torch, d_c).reshape(2, M).tolist()
        hi = [[v * u % p for v, u in zip(plane, unshift)][3 * N - 3:] for plane in coef]
        # the device's quotient is the restatement's, row for row
        x = host(torch, d_cols).reshape(16, M)
        on = PR.Columns(x[0:3], x[3:8], x[8:11], x[11], x[12:14])
        E = PR.Ext2(p, w)
        assert host(torch, d_T).tolist() == PR.planar(PR.quotient(E, dom, on, *ch))
        return hi, last

    wires = PR.witness(c)
    hi, last = high_coefficients(wires)
    assert last == (1, 0) and len(hi[0]) == M - (3 * N - 3)
    assert not any(hi[0]) and not any(hi[1])
    gate_rows = [i for i in range(N) if c.sel[3][i]]
    wires[2][gate_rows[-1]] = (wires[2][gate_rows[-1]] + 1) % p
    hi, _ = high_coefficients(wires)
    assert any(hi[0]) or any(hi[1])
    handle.close()
