"""The lookup multiplicities and the logUp quotient on the device (ronk_lookup_mult*, ronk_logup_quotient*) bit for bit against
the Python restatement tests/lookup_ref.py, and the whole lookup argument end to end through the existing entry points.

Multiplicities (csrc/lookup_kernels.h): a hash table of the power-of-two capacity >= 2 T in the caller's workspace, four launches
(clear, build, count, finalise), one lane per table entry and per lookup word, equal slots combined inside a wavefront before the
global atomic.  The shapes sit on both sides of a capacity step, below and above one workgroup of 256 lanes and one wavefront of
64, and the last lane of the last column is the one that misses.

Quotient: the lane of the PLONK quotient (rows i + t M / R, R = 4 over Goldilocks, 8 over a Montgomery prime; one row below
M = R); row i reads S at row (i + B) mod M.  The kernel is pointwise, so the rows are random words (0, p - 1 and words >= p among
them)."""
import ctypes as C

import numpy as np
import pytest

import accum_ref as AR
import lookup_ref as LR
import plonk_ref as PR
import prime_classes as PC
from ronkathon_amd import _lib as L
from test_gpu_fri import dev, host, words

pytestmark = pytest.mark.gpu

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
GEN = {**PC.GEN, GL: 7}
MULT_FIELDS = [GL, MONT, PC.P_MID, PC.P_62, PC.P_32]
FIELDS = [(GL, 7), (GL, 11), (MONT, 10), (PC.P_MID, PC.GEN[PC.P_MID]), (PC.P_62, PC.GEN[PC.P_62])]      # p, w: those of test_gpu_plonk
SMALL = [3, 4, 6, 8, 11, 12, 13]       # log2 M, every row compared
LARGE = [16, 20]                       # sampled
NONE = 2**64 - 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def garbage(torch, n):
    return torch.full((n,), -1, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ multiplicities
def instance(seed, p, T, n, C, absent=0, last_absent=False):
    """a table of T words with repeats (one of them another word of the same value) and C columns of n lookups drawn from it;
    `absent` cells hold words the table lacks, the last cell of the last column among them when asked"""
    rng = np.random.default_rng(seed)
    table = words(seed, T, p)
    if T > 2:
        k = rng.integers(0, T, size=T // 3)
        table[k] = table[rng.integers(0, T, size=k.size)]
        if int(table[0]) % p + p < 2**64:
            table[T - 1] = np.uint64(int(table[0]) % p + p)
    vals = table[rng.integers(0, T, size=C * n)]
    have = {int(t) % p for t in table}
    cells = set(int(e) for e in rng.choice(C * n, size=absent, replace=False)) if absent else set()
    if last_absent and absent and C * n - 1 not in cells:
        cells.pop()
        cells.add(C * n - 1)
    for e in cells:
        v = int(rng.integers(0, 2**62))
        while v % p in have:
            v += 1
        vals[e] = np.uint64(v)
    return table, vals


class MultCall:
    """the device buffers of one ronk_lookup_mult_dev call, outputs and workspace pre-filled with all-ones words"""

    def __init__(self, torch, p, table, vals, C):
        self.p, self.T, self.C, self.n = p, table.size, C, vals.size // C
        self.d_table, self.d_vals = dev(torch, table), dev(torch, vals)
        self.d_mult, self.d_missing = garbage(torch, self.T), garbage(torch, 2)
        words_needed = L.lib.ronk_lookup_workspace_words(self.T)
        assert words_needed >= 4 * self.T
        self.d_work = garbage(torch, words_needed)

    def run(self, negate, stream=0):
        L.check(L.lib.ronk_lookup_mult_dev(self.p, self.d_table.data_ptr(), self.T, self.d_vals.data_ptr(), self.C, self.n, int(negate),
                                           self.d_mult.data_ptr(), self.d_missing.data_ptr(), self.d_work.data_ptr(), stream))

    def result(self, torch):
        miss = host(torch, self.d_missing)
        return host(torch, self.d_mult).tolist(), int(miss[0]), int(miss[1])


def check_mult(torch, p, table, vals, C, negates=(0, 1)):
    want = {neg: LR.multiplicities(p, table.tolist(), vals.reshape(C, -1).tolist(), negate=bool(neg)) for neg in negates}
    c = MultCall(torch, p, table, vals, C)
    for neg in negates:
        c.d_mult.fill_(-1); c.d_missing.fill_(-1); c.d_work.fill_(-1)
        c.run(neg)
        assert c.result(torch) == want[neg], (p, table.size, vals.size, C, neg)
    assert np.array_equal(host(torch, c.d_table), table) and np.array_equal(host(torch, c.d_vals), vals)      # inputs unchanged
    return want


@pytest.mark.parametrize("T,n,C", [(1, 1, 1), (2, 65, 1), (255, 300, 2), (256, 4096, 3), (257, 4097, 1), (1025, 10**4, 2)])
@pytest.mark.parametrize("p", MULT_FIELDS)
def test_multiplicities_every_word(torch, p, T, n, C):
    """every word of the output with negate both ways, inputs unchanged, outputs and workspace pre-filled with all ones; 0, 1 and
    7 absent words, the last lane of the last column among them"""
    for absent in (0, 1, 7):
        if absent > C * n:
            continue
        table, vals = instance(100 * T + absent, p, T, n, C, absent, last_absent=True)
        want = check_mult(torch, p, table, vals, C)
        assert want[0][1] == absent and want[1][1:] == want[0][1:]
        if absent < 2:
            assert want[0][2] == (C * n - 1 if absent else NONE)


@pytest.mark.parametrize("p", MULT_FIELDS)
def test_all_lookups_equal_one_value(torch, p):
    """the contention path: 2^16 lookups of one table value, the count exact; and that value's other word p + v"""
    n = 1 << 16
    table = words(3, 500, p)
    table[7] = np.uint64(12345 % p)
    v = int(table[7]) % p
    first = next(j for j, t in enumerate(table.tolist()) if t % p == v)
    for word in (v, v + p if v + p < 2**64 else v):
        vals = np.full(n, np.uint64(word), dtype=np.uint64)
        want = check_mult(torch, p, table, vals, 1)
        assert want[0][0][first] == n % p and sum(1 for k in want[0][0] if k) == 1 and want[1][0][first] == (p - n % p) % p


@pytest.mark.parametrize("p", MULT_FIELDS)
def test_a_table_of_one_value_repeated(torch, p):
    table = np.full(1000, np.uint64(p - 1), dtype=np.uint64)
    vals = np.full(777, np.uint64(p - 1), dtype=np.uint64)
    want = check_mult(torch, p, table, vals, 1)
    assert want[0] == ([777 % p] + [0] * 999, 0, NONE)


def numpy_multiplicities(p, table, vals):
    """the same counts by sorting: -> (mult [T] as plain counts, missing, first missing)"""
    t, v = table % np.uint64(p), vals % np.uint64(p)
    keys, first = np.unique(t, return_index=True)                 # the first index of every value
    pos = np.searchsorted(keys, v)
    pos[pos == keys.size] = 0
    found = keys[pos] == v
    counts = np.bincount(first[pos[found]], minlength=t.size)
    miss = np.flatnonzero(~found)
    return counts.astype(np.uint64), int(miss.size), int(miss[0]) if miss.size else NONE


@pytest.mark.parametrize("p", [GL, MONT])
def test_a_large_case_against_numpy(torch, p):
    T, n, C = 1 << 16, 1 << 18, 2
    rng = np.random.default_rng(16)
    table = words(16, T, p)
    vals = table[rng.integers(0, T, size=C * n)]
    vals[rng.integers(0, C * n, size=5)] ^= np.uint64(1 << 40)     # five words the table (almost surely) lacks
    counts, missing, first = numpy_multiplicities(p, table, vals)
    assert 0 < missing <= 5
    c = MultCall(torch, p, table, vals, C)
    c.run(0)
    got = c.result(torch)
    assert np.array_equal(np.array(got[0], dtype=np.uint64), counts) and got[1:] == (missing, first)
    c.run(1)
    got = c.result(torch)
    assert np.array_equal(np.array(got[0], dtype=np.uint64), np.where(counts == 0, counts, np.uint64(p) - counts)) and got[1:] == (missing, first)


@pytest.mark.parametrize("p", [GL, MONT])
def test_skewed_columns_over_several_passes_of_a_wavefront(torch, p):
    """The count launch has at most 2048 workgroups = 2^19 lanes, so above 2^19 cells a wavefront makes several passes and carries
    what its first round retired from pass to pass.  C n = 3 (2^19 + 77) = 3 * 2^19 + 231 cells: three full passes and a fourth
    in which only 231 lanes are live (three whole wavefronts, one with 39 live lanes, every other wavefront with none: its carry
    must survive).  Even wavefronts look up one hot value in every pass (the carry accumulates), odd ones another hot value in
    each pass (the carry is added when the first slot changes); a tenth of the cells are uniform, so most wavefronts also hold
    other slots, and some cells hold words the table lacks.  Every word against numpy, negate both ways."""
    T, n, C = 1000, (1 << 19) + 77, 3
    lanes = 1 << 19
    rng = np.random.default_rng(19)
    table = words(19, T, p)
    e = np.arange(C * n)
    hot = np.where((e // 64) % 2 == 0, 3, np.array([11, 500, 999, 11])[e // lanes])
    vals = table[hot]
    spread = rng.random(C * n) < 0.1
    vals[spread] = table[rng.integers(0, T, size=int(spread.sum()))]
    absent = np.concatenate([rng.integers(0, C * n, size=40), [lanes + 5, 3 * lanes + 230]])      # the last live lane among them
    vals[absent] = vals[absent] ^ np.uint64(1 << 41)
    counts, missing, first = numpy_multiplicities(p, table, vals)
    assert 30 < missing <= 42 and counts.max() > C * n // 3
    c = MultCall(torch, p, table, vals, C)
    for neg in (0, 1):
        c.d_mult.fill_(-1); c.d_missing.fill_(-1); c.d_work.fill_(-1)
        c.run(neg)
        got = c.result(torch)
        want = counts if not neg else np.where(counts == 0, counts, np.uint64(p) - counts)
        assert np.array_equal(np.array(got[0], dtype=np.uint64), want) and got[1:] == (missing, first), (p, neg)
    assert np.array_equal(host(torch, c.d_vals), vals)


@pytest.mark.parametrize("p", [GL, MONT])
def test_multiplicities_under_stream_capture(torch, p):
    """a fixed number of launches, no library workspace and no host round trip: legal under capture; the graph is replayed on
    changed inputs and gives each input's words"""
    T, n, C = 300, 5000, 2
    inputs = [instance(40 + k, p, T, n, C, absent=k) for k in range(2)]
    c = MultCall(torch, p, *inputs[0], C)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        c.run(1, stream=s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        c.run(1, stream=torch.cuda.current_stream().cuda_stream)
    for table, vals in inputs + inputs[:1]:
        c.d_table.copy_(dev(torch, table)); c.d_vals.copy_(dev(torch, vals))
        c.d_mult.fill_(-1); c.d_missing.fill_(-1)
        graph.replay()
        assert c.result(torch) == LR.multiplicities(p, table.tolist(), vals.reshape(C, n).tolist(), negate=True)


@pytest.mark.parametrize("p", MULT_FIELDS)
def test_multiplicities_host_form_and_caller(torch, p):
    from ronkathon_amd import callers

    class F:
        ORDER = p
    T, n, C = 100, 333, 3
    table, vals = instance(7, p, T, n, C, absent=2)
    for neg in (0, 1):
        want = LR.multiplicities(p, table.tolist(), vals.reshape(C, n).tolist(), negate=bool(neg))
        mult, missing = np.full(T, NONE, dtype=np.uint64), np.full(2, 77, dtype=np.uint64)
        L.check(L.lib.ronk_lookup_mult(p, L.ptr(table), T, L.ptr(vals), C, n, neg, L.ptr(mult), L.ptr(missing)))
        assert (mult.tolist(), int(missing[0]), int(missing[1])) == want
        m, count, first = callers.lookup_multiplicities(F, table, vals.reshape(C, n), negate=bool(neg))
        assert (m.tolist(), count, first) == want
    table, vals = instance(8, p, T, n, C)
    assert callers.lookup_multiplicities(F, table, vals.reshape(C, n))[1:] == (0, None)


# ------------------------------------------------------------------------------------------------ the quotient
class Handle:
    def __init__(self, p, g, w, log2_n, log2_b, shift):
        self.h = C.c_void_p()
        L.check(L.lib.ronk_plonk_create(C.byref(self.h), p, g, w, log2_n, log2_b, shift, (C.c_uint64 * 3)(1, 2, 3)))

    def close(self):
        if self.h:
            L.check(L.lib.ronk_plonk_destroy(self.h))
            self.h = None


class Case:
    """random words for one (field, M, B, C), on the host and on the device"""

    def __init__(self, torch, p, w, log2_m, log2_b, n_cols, seed=0):
        self.p, self.w, self.M, self.log2_m, self.log2_b, self.C = p, w, 1 << log2_m, log2_m, log2_b, n_cols
        M = self.M
        self.E = LR.Ext2(p, w)
        self.dom = PR.Domain(p, GEN[p], log2_m - log2_b, log2_b, GEN[p])
        s = 1000 * log2_m + 100 * log2_b + 7 * n_cols + seed
        # vals, mult, S, T_in, alpha, lambda
        self.host = [words(s + j, k, p) for j, k in enumerate((n_cols * M, n_cols * M, 2 * M, 2 * M, 2, 4))]
        self.dev = [dev(torch, a) for a in self.host]
        self.handle = Handle(p, GEN[p], w, log2_m - log2_b, log2_b, GEN[p])
        self.lists = [self.host[0].reshape(n_cols, M).tolist(), self.host[1].reshape(n_cols, M).tolist(), self.host[2].reshape(2, M).tolist(),
                      self.host[3].reshape(2, M).tolist()]
        self.alpha, self.lam = self.host[4].tolist(), [self.host[5][0:2].tolist(), self.host[5][2:4].tolist()]

    def call(self, d_out, with_mult=True, d_T_in=None, stream=0):
        p = [t.data_ptr() for t in self.dev]
        L.check(L.lib.ronk_logup_quotient_dev(self.handle.h, p[0], p[1] if with_mult else None, self.C, p[2], p[4], p[5],
                                              None if d_T_in is None else d_T_in.data_ptr(), d_out.data_ptr(), stream))

    def want_all(self, with_mult=True, with_tin=False):
        v, m, S, T = self.lists
        out = LR.quotient_fast(self.E, self.dom, v, m if with_mult else None, S, self.alpha, self.lam, T if with_tin else None)
        return np.array(LR.planar(out), dtype=np.uint64)

    def want_rows(self, rows, with_mult=True, with_tin=False):
        v, m, S, T = self.lists
        return [LR.quotient_row(self.E, self.dom, v, m if with_mult else None, S, self.alpha, self.lam, T if with_tin else None, int(i))
                for i in rows]

    def inputs_unchanged(self, torch):
        return all(np.array_equal(host(torch, d), h) for d, h in zip(self.dev, self.host))


# with the multiplicities, onto a T_in, in place
VARIANTS = [(True, True, True), (False, False, False), (True, False, False), (False, True, False)]


@pytest.mark.parametrize("log2_m", SMALL)
@pytest.mark.parametrize("p,w", FIELDS)
def test_every_row_against_the_restatement(torch, p, w, log2_m):
    """B = 2, 4, 8 where B < M, C = 1, 2, 5, 16 at each; the four variants (with / without the multiplicities, onto a T_in in
    place / onto one elsewhere / onto none) rotate over the twelve calls, starting at another one for every M"""
    k = log2_m
    for log2_b in (1, 2, 3):
        if log2_b >= log2_m:
            continue
        for n_cols in (1, 2, 5, 16):
            with_mult, with_tin, in_place = VARIANTS[k % 4]
            k += 1
            c = Case(torch, p, w, log2_m, log2_b, n_cols)
            d_out = garbage(torch, 2 * c.M)
            if in_place:
                d_out.copy_(c.dev[3])
            c.call(d_out, with_mult, d_out if in_place else c.dev[3] if with_tin else None)
            assert np.array_equal(host(torch, d_out), c.want_all(with_mult, with_tin)), (p, w, log2_m, log2_b, n_cols, with_mult, with_tin)
            assert c.inputs_unchanged(torch)
            c.handle.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_fewer_rows_than_a_lane_owns(torch, p, w):
    """M = 2 (B = 1) and M = 4 (B = 2): the one-row-per-lane kernel"""
    for log2_m, log2_b in ((1, 0), (2, 1)):
        for n_cols, (with_mult, with_tin, _) in zip((1, 2, 5, 16), VARIANTS):
            c = Case(torch, p, w, log2_m, log2_b, n_cols, seed=2)
            d_out = garbage(torch, 2 * c.M)
            c.call(d_out, with_mult, c.dev[3] if with_tin else None)
            assert np.array_equal(host(torch, d_out), c.want_all(with_mult, with_tin)), (p, w, log2_m, n_cols)
            c.handle.close()


@pytest.mark.parametrize("log2_m", LARGE)
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_large_sizes_at_sampled_rows(torch, p, w, log2_m):
    """B = 4, C = 2, with the multiplicities, in place onto T_in: the first and last 2 B rows, the 2 B rows on either side of
    every eighth of M (where the rows of a lane start), and 4096 seeded rows, which reach every quarter of M"""
    B = 4
    c = Case(torch, p, w, log2_m, 2, 2)
    M = c.M
    d_T = c.dev[3].clone()
    c.call(d_T, True, d_T)
    got = host(torch, d_T)
    rng = np.random.default_rng(log2_m)
    edges = np.concatenate([np.arange(q * M // 8 - 2 * B, q * M // 8 + 2 * B) for q in range(9)])
    rows = np.unique(np.concatenate([edges[(edges >= 0) & (edges < M)], rng.integers(0, M, size=4096)]))
    assert set(range(2 * B)) <= set(rows.tolist()) and set(range(M - 2 * B, M)) <= set(rows.tolist())
    assert all(((rows >= q * M // 4) & (rows < (q + 1) * M // 4)).sum() > 500 for q in range(4))
    want = c.want_rows(rows, True, True)
    assert [(int(got[i]), int(got[M + i])) for i in rows] == want, (p, log2_m)
    assert c.inputs_unchanged(torch)
    c.handle.close()


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_quotient_under_stream_capture(torch, p, w):
    """one launch, no library workspace and no host round trip: legal under capture, and two replays give the direct call's words"""
    c = Case(torch, p, w, 12, 2, 3, seed=4)
    d_direct, d_T = garbage(torch, 2 * c.M), garbage(torch, 2 * c.M)
    c.call(d_direct, True, c.dev[3])
    direct = host(torch, d_direct)
    assert np.array_equal(direct, c.want_all(True, True))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        c.call(d_T, True, c.dev[3], stream=s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        c.call(d_T, True, c.dev[3], stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        d_T.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(torch, d_T), direct)
    c.handle.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_quotient_host_form_and_caller(torch, p, w):
    c = Case(torch, p, w, 8, 2, 3, seed=5)
    M, a = c.M, c.host
    T = np.full(2 * M, NONE, dtype=np.uint64)
    L.check(L.lib.ronk_logup_quotient(c.handle.h, L.ptr(a[0]), L.ptr(a[1]), 3, L.ptr(a[2]), L.ptr(a[4]), L.ptr(a[5]), L.ptr(a[3]), L.ptr(T)))
    assert np.array_equal(T, c.want_all(True, True))
    L.check(L.lib.ronk_logup_quotient(c.handle.h, L.ptr(a[0]), None, 3, L.ptr(a[2]), L.ptr(a[4]), L.ptr(a[5]), None, L.ptr(T)))
    assert np.array_equal(T, c.want_all(False, False))
    c.handle.close()
    from ronkathon_amd import callers

    class F:
        ORDER = p
    got = callers.logup_quotient(F, GEN[p], w, 6, 2, GEN[p], a[0].reshape(3, M), a[1].reshape(3, M), a[2].reshape(2, M), c.alpha, c.lam,
                                 a[3].reshape(2, M))
    assert np.array_equal(got, c.want_all(True, True))
    got = callers.logup_quotient(F, GEN[p], w, 6, 2, GEN[p], a[0].reshape(3, M), None, a[2].reshape(2, M), c.alpha, c.lam)
    assert np.array_equal(got, c.want_all(False, False))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_end_to_end_through_the_entry_points(torch, p, w):
    """two lookup columns into a table column: ronk_lookup_mult_dev (negate) -> ronk_logup_sum_dev -> ronk_lde_batch_dev of the
    columns, the multiplicities and both planes of S -> ronk_logup_quotient_dev -> ronk_ntt_inverse_dev per plane and the un-shift
    by s^-i.  The sum closes, nothing is missing and the coefficients from C N - C upward are zero; with one lookup word
    replaced by a word the table lacks they are not.  Added onto the PLONK quotient of a valid circuit, the sum is still a
    polynomial."""
    log2_n, log2_b, n_cols = 6, 2, 3
    g = shift = GEN[p]
    N, M = 1 << log2_n, 1 << (log2_n + log2_b)
    rng = np.random.default_rng(61)
    E = LR.Ext2(p, w)
    dom = PR.Domain(p, g, log2_n, log2_b, shift)
    handle = Handle(p, g, w, log2_n, log2_b, shift)
    pk, pn = L.Plan(p, g, log2_n, 16), L.Plan(p, g, log2_n + log2_b, 16)
    inv = L.Plan(p, g, log2_n + log2_b, 1)
    sinv = pow(shift, -1, p)
    unshift = [pow(sinv, j, p) for j in range(M)]
    alpha, lam = [int(v) % p for v in rng.integers(0, 2**62, size=2)], [int(v) % p for v in rng.integers(0, 2**62, size=4)]
    d_alpha, d_lam = dev(torch, np.array(alpha, dtype=np.uint64)), dev(torch, np.array(lam, dtype=np.uint64))

    def coefficients(d_T, lo):
        d_c = garbage(torch, 2 * M)
        for plane in (0, 1):
            L.check(L.lib.ronk_ntt_inverse_dev(inv.h, d_T.data_ptr() + 8 * plane * M, d_c.data_ptr() + 8 * plane * M, 0))
        coef = host(torch, d_c).reshape(2, M).tolist()
        return [[v * u % p for v, u in zip(plane, unshift)][lo:] for plane in coef]

    def lookup_quotient(table, lookups, d_T_in=None):
        """-> (T on the device, S[N], missing)"""
        d_table, d_look = dev(torch, table), dev(torch, lookups)
        d_m, d_missing = garbage(torch, N), garbage(torch, 2)
        d_lwork = garbage(torch, L.lib.ronk_lookup_workspace_words(N))
        L.check(L.lib.ronk_lookup_mult_dev(p, d_table.data_ptr(), N, d_look.data_ptr(), n_cols - 1, N, 1, d_m.data_ptr(),
                                           d_missing.data_ptr(), d_lwork.data_ptr(), 0))
        ones = torch.ones((n_cols - 1) * N, dtype=torch.int64, device="cuda")
        d_vals, d_mult = torch.cat([d_look, d_table]), torch.cat([ones, d_m])
        d_S, d_last, d_work = garbage(torch, 2 * N), garbage(torch, 2), garbage(torch, L.lib.ronk_scan_workspace_words(N))
        d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        L.check(L.lib.ronk_logup_sum_dev(p, w, d_vals.data_ptr(), d_mult.data_ptr(), n_cols, N, d_alpha.data_ptr(), d_S.data_ptr(),
                                         d_last.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), 0))
        assert int(d_st.item()) == 0
        # one batch of 16 columns: the values 3, the multiplicities 3, the two planes of S as the device left them, eight spare
        d_in = torch.cat([d_vals, d_mult, d_S, torch.zeros(8 * N, dtype=torch.int64, device="cuda")])
        d_co, d_cols = garbage(torch, 16 * N), garbage(torch, 16 * M)
        L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_in.data_ptr(), d_co.data_ptr(), d_cols.data_ptr(), shift, 0))
        base = d_cols.data_ptr()
        d_T = garbage(torch, 2 * M) if d_T_in is None else d_T_in.clone()
        L.check(L.lib.ronk_logup_quotient_dev(handle.h, base, base + 8 * 3 * M, n_cols, base + 8 * 6 * M, d_alpha.data_ptr(), d_lam.data_ptr(),
                                              None if d_T_in is None else d_T.data_ptr(), d_T.data_ptr(), 0))
        # the device's quotient is the restatement's, row for row
        x = host(torch, d_cols).reshape(16, M)
        t_in = None if d_T_in is None else host(torch, d_T_in).reshape(2, M).tolist()
        want = LR.quotient_fast(E, dom, x[0:3].tolist(), x[3:6].tolist(), x[6:8].tolist(), alpha, [lam[0:2], lam[2:4]], t_in)
        assert host(torch, d_T).tolist() == LR.planar(want)
        return d_T, tuple(host(torch, d_last).tolist()), tuple(host(torch, d_missing).tolist())

    table = words(62, N, p) % np.uint64(p)      # canonical: the transforms of ronk_lde_batch_dev take residues in [0, p)
    table[5] = table[9]
    lookups = table[rng.integers(0, N, size=(n_cols - 1) * N)]
    d_T, last, missing = lookup_quotient(table, lookups)
    assert last == (0, 0) and missing == (0, NONE)
    lo = n_cols * N - n_cols
    hi = coefficients(d_T, lo)
    assert len(hi[0]) == M - lo and not any(hi[0]) and not any(hi[1])
    # the restatement agrees on the multiplicities and the sum
    m, _, _ = LR.multiplicities(p, table.tolist(), lookups.reshape(n_cols - 1, N).tolist(), negate=True)
    _, ref_last, _ = AR.logup_sum(E, lookups.reshape(n_cols - 1, N).tolist() + [table.tolist()], [[1] * N] * (n_cols - 1) + [m], alpha)
    assert ref_last == E.zero

    # the PLONK quotient of a valid circuit as T_in: the sum is still a polynomial of degree below 3 N - 3
    c = PR.circuit(rng, p, log2_n)
    ids = PR.labels(dom)
    sigma = PR.sigma_of(c, ids)
    wires = PR.witness(c)
    ch = [[int(v) % p for v in rng.integers(0, 2**62, size=2)] for _ in range(3)]
    d_ch = [dev(torch, np.array(v, dtype=np.uint64)) for v in ch]
    d_w, d_i, d_s = (dev(torch, np.array(a, dtype=np.uint64).ravel()) for a in (wires, ids, sigma))
    d_Z, d_zlast, d_work = garbage(torch, 2 * N), garbage(torch, 2), garbage(torch, L.lib.ronk_scan_workspace_words(N))
    d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_perm_product_dev(p, w, d_w.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), 3, N, d_ch[1].data_ptr(), d_ch[2].data_ptr(),
                                        d_Z.data_ptr(), d_zlast.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), 0))
    assert int(d_st.item()) == 0 and tuple(host(torch, d_zlast).tolist()) == (1, 0)
    d_in = torch.cat([dev(torch, np.array(wires + c.sel + sigma + [c.pi], dtype=np.uint64).ravel()), d_Z,
                      torch.zeros(2 * N, dtype=torch.int64, device="cuda")])
    d_co, d_cols = garbage(torch, 16 * N), garbage(torch, 16 * M)
    L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_in.data_ptr(), d_co.data_ptr(), d_cols.data_ptr(), shift, 0))
    d_plonk = garbage(torch, 2 * M)
    base = d_cols.data_ptr()
    L.check(L.lib.ronk_plonk_quotient_dev(handle.h, base, base + 8 * 3 * M, base + 8 * 8 * M, base + 8 * 11 * M, base + 8 * 12 * M,
                                          d_ch[0].data_ptr(), d_ch[1].data_ptr(), d_ch[2].data_ptr(), d_plonk.data_ptr(), 0))
    d_sum, last, missing = lookup_quotient(table, lookups, d_plonk)
    assert last == (0, 0) and missing == (0, NONE)
    hi = coefficients(d_sum, 3 * N - 3)
    assert not any(hi[0]) and not any(hi[1])
    assert any(host(torch, d_sum) != host(torch, d_plonk))

    # one lookup word the table does not hold
    bad = lookups.copy()
    have = {int(t) % p for t in table}
    v = 12345
    while v % p in have:
        v += 1
    bad[N + 17] = np.uint64(v)
    d_T, last, missing = lookup_quotient(table, bad)
    assert missing == (1, N + 17) and last != (0, 0)
    hi = coefficients(d_T, lo)
    assert any(hi[0]) or any(hi[1])
    handle.close()
