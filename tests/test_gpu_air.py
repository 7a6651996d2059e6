"""Constraint programs on the device (ronk_air_create, ronk_air_quotient_dev, ronk_air_quotient, ronk_air_cells,
ronk_air_eval_point) bit for bit against the Python restatement tests/air_ref.py, over the five fields of tests/test_gpu_plonk.py,
and word for word against the two hard-wired quotients, ronk_plonk_quotient_dev and ronk_logup_quotient_dev, whose constraints are
written as programs (tests/air_programs.py).  The kernel is pointwise, so the rows are random words (0, p - 1 and words >= p among
them); the last test runs a valid trace through ronk_lde_batch_dev, the quotient and ronk_ntt_inverse_dev and closes the identity
at one out-of-domain point.

The blocking under test (csrc/air_kernels.h): a lane owns the rows i + t M / R (R = 4 over Goldilocks, 8 over a Montgomery prime;
one row below M = R) and runs the tape once per row; row i reads a column at row (i + rot B) mod M; the registers live in LDS, as
many as the program declares; a program with a FIRST or LAST constraint parks 2 R inverses per lane behind them, and a workgroup
has 256 lanes, or 128 where 16 registers and those inverses would pass 64 KiB."""
import ctypes as C

import numpy as np
import pytest

import air_programs as AP
import air_ref as AR
import plonk_ref as PR
import prime_classes as PC
from ronkathon_amd import _lib as L
from test_gpu_fri import dev, host, words

pytestmark = pytest.mark.gpu

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
GEN = {**PC.GEN, GL: 7}
FIELDS = [(GL, 7), (GL, 11), (MONT, 10), (PC.P_MID, PC.GEN[PC.P_MID]), (PC.P_62, PC.GEN[PC.P_62])]
KINDS = [(AR.ALL,), (AR.FIRST,), (AR.LAST,), (AR.EXCEPT_LAST,), (AR.ALL, AR.FIRST, AR.LAST, AR.EXCEPT_LAST), (AR.EXCEPT_LAST, AR.ALL)]
GROUPS = [(5,), (2, 3), (1, 1, 1, 1, 1), (4, 1)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def garbage(torch, n):
    return torch.full((n,), -1, dtype=torch.int64, device="cuda")


def pointers(tensors):
    return (C.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])


def flat(a):
    return L.arr([int(c) % 2**64 for e in a for c in e])


class Air:
    """a program on the domain (p, w, N, B, shift = the generator): both handles"""

    def __init__(self, p, w, log2_n, log2_b, prog, groups, n_ext, n_chal):
        self.p, self.M, self.prog, self.groups, self.n_ext = p, 1 << (log2_n + log2_b), prog, groups, n_ext
        self.E, self.dom = PR.Ext2(p, w), PR.Domain(p, GEN[p], log2_n, log2_b, GEN[p])
        self.d, self.h = C.c_void_p(), C.c_void_p()
        L.check(L.lib.ronk_plonk_create(C.byref(self.d), p, GEN[p], w, log2_n, log2_b, GEN[p], (C.c_uint64 * 3)(1, 2, 3)))
        ops, imm = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * max(1, len(prog.imm)))(*[v % p for v in prog.imm])
        L.check(L.lib.ronk_air_create(C.byref(self.h), self.d, len(groups), (C.c_uint32 * max(1, len(groups)))(*groups), n_ext, n_chal,
                                      len(prog.imm), prog.n_regs, prog.n_constraints, ops, len(prog.ops), imm))

    def call(self, d_base, d_ext, d_chal, d_lam, d_T_in, d_T_out, stream=0):
        L.check(L.lib.ronk_air_quotient_dev(self.h, pointers(d_base), pointers(d_ext), d_chal.data_ptr() if d_chal is not None else None,
                                            d_lam.data_ptr(), None if d_T_in is None else d_T_in.data_ptr(), d_T_out.data_ptr(), stream))

    def close(self):
        L.check(L.lib.ronk_air_destroy(self.h))
        L.check(L.lib.ronk_plonk_destroy(self.d))


class Data:
    """random words for the columns, challenges and weights of a program, on the host and on the device"""

    def __init__(self, torch, air, n_chal, seed):
        p, M = air.p, air.M
        self.base = [words(seed + 10 * g, c * M, p) for g, c in enumerate(air.groups)]
        self.ext = [words(seed + 100 + e, 2 * M, p) for e in range(air.n_ext)]
        self.chal, self.lam = words(seed + 200, 2 * max(1, n_chal), p), words(seed + 201, 2 * air.prog.n_constraints, p)
        self.T_in = words(seed + 202, 2 * M, p)
        self.d_base, self.d_ext = [dev(torch, a) for a in self.base], [dev(torch, a) for a in self.ext]
        self.d_chal, self.d_lam, self.d_T_in = dev(torch, self.chal), dev(torch, self.lam), dev(torch, self.T_in)
        self.columns = [col.tolist() for a, c in zip(self.base, air.groups) for col in a.reshape(c, M)]
        self.planes = [a.reshape(2, M).tolist() for a in self.ext]

    def want(self, air, with_T_in, rows=None):
        T_in = self.T_in.reshape(2, air.M).tolist() if with_T_in else None
        args = (air.E, air.dom, air.prog, self.columns, self.planes, AR.pairs_of(self.chal), AR.pairs_of(self.lam), T_in)
        if rows is None:
            return np.array(AR.planar(AR.quotient(*args)), dtype=np.uint64)
        return [AR.quotient_row(*args, int(i)) for i in rows]

    def unchanged(self, torch):
        pairs = list(zip(self.d_base, self.base)) + list(zip(self.d_ext, self.ext)) + [(self.d_chal, self.chal), (self.d_lam, self.lam)]
        return all(np.array_equal(host(torch, d), h) for d, h in pairs)


def rotations(N):
    far = min(N - 1, 2047)
    return tuple(r for r in (0, 1, -1, 2, far, -far) if abs(r) < N)


def check_random_program(torch, p, w, log2_m, log2_b, variant):
    """a seeded random program with the kinds, the groups, the register count and the T_in form of `variant`, every row"""
    log2_n = log2_m - log2_b
    rng = np.random.default_rng(1000 * log2_m + variant)
    kinds, groups = KINDS[variant % len(KINDS)], GROUPS[variant % len(GROUPS)]
    prog, _ = AP.random_program(rng, 5, 2, 3, rotations(1 << log2_n), kinds, 1 + variant % 5, depth=4,
                                n_regs_min=16 if variant % 2 else 0)
    air = Air(p, w, log2_n, log2_b, prog, groups, 2, 3)
    data = Data(torch, air, 3, 7 * log2_m + variant)
    mode = variant % 3                       # T_in absent, present, in place
    d_T = garbage(torch, 2 * air.M)
    if mode == 2:
        d_T.copy_(data.d_T_in)
    air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, (None, data.d_T_in, d_T)[mode], d_T)
    assert np.array_equal(host(torch, d_T), data.want(air, mode != 0)), (p, w, log2_m, log2_b, variant)
    assert data.unchanged(torch) and np.array_equal(host(torch, data.d_T_in), data.T_in)
    air.close()


@pytest.mark.parametrize("log2_m", range(3, 14))
@pytest.mark.parametrize("p,w", FIELDS)
def test_every_row_against_the_restatement(torch, p, w, log2_m):
    """M = 2^3 .. 2^13 with B = 2, 4, 8, the kinds, the groups, the register count and the three T_in forms rotating"""
    check_random_program(torch, p, w, log2_m, 1 + log2_m % 3 if log2_m > 3 else 1, log2_m)


@pytest.mark.parametrize("variant", range(6))
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_every_kind_at_the_first_size_of_two_workgroups(torch, p, w, variant):
    """each kind alone, all four, and a program without boundary kinds, at M = 2^11 (Goldilocks) and 2^12 (Montgomery)"""
    check_random_program(torch, p, w, 11 if p == GL else 12, 2, variant)


@pytest.mark.parametrize("p,w", FIELDS)
def test_fewer_rows_than_a_lane_owns(torch, p, w):
    """M = 2 (B = 1) and M = 4 (B = 2): the one-row-per-lane kernel, N = 2"""
    for log2_m, log2_b in ((1, 0), (2, 1)):
        for variant in (4, 5):
            check_random_program(torch, p, w, log2_m, log2_b, variant)


@pytest.mark.parametrize("p,w", FIELDS)
def test_the_longest_and_the_shortest_tape(torch, p, w):
    """4096 ops on 16 registers that hold base values at one op and extension values at another, 64 constraints, 8 groups of 8
    columns, 8 extension columns, 32 challenges and 256 immediates at M = 2^6; and the one-op tape, EMIT of a column, on one
    register and on none"""
    log2_n, log2_b = 4, 2
    prog = AP.long_program(4096, 64, 64, 8, 32, 256, rotations(1 << log2_n))
    air = Air(p, w, log2_n, log2_b, prog, (8,) * 8, 8, 32)
    data = Data(torch, air, 32, 5)
    d_T = garbage(torch, 2 * air.M)
    air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, data.d_T_in, d_T)
    assert np.array_equal(host(torch, d_T), data.want(air, True)), (p, w)
    assert data.unchanged(torch)
    air.close()
    for kind in range(4):
        for n_regs in (0, 1):
            prog = AR.Program([AR.op(AR.EMIT, kind, AR.operand(AR.BASE, 1, -1), 0)], [], n_regs, 1)
            air = Air(p, w, log2_n, log2_b, prog, (2,), 0, 0)
            data = Data(torch, air, 0, 6 + kind)
            d_T = garbage(torch, 2 * air.M)
            air.call(data.d_base, [], None, data.d_lam, None, d_T)
            assert np.array_equal(host(torch, d_T), data.want(air, False)), (p, w, kind, n_regs)
            air.close()


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_2_to_the_20_at_sampled_rows(torch, p, w):
    """B = 4: the first and last 2 B rows, the 2 B rows on either side of every eighth of M (where the rows of a lane start) and
    2048 seeded rows"""
    log2_m, B = 20, 4
    rng = np.random.default_rng(20)
    prog, _ = AP.random_program(rng, 5, 2, 3, rotations(1 << 18), KINDS[4], 4, depth=4)
    air = Air(p, w, log2_m - 2, 2, prog, (2, 3), 2, 3)
    data = Data(torch, air, 3, 20)
    M = air.M
    d_T = garbage(torch, 2 * M)
    air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, data.d_T_in, d_T)
    got = host(torch, d_T)
    edges = np.concatenate([np.arange(q * M // 8 - 2 * B, q * M // 8 + 2 * B) for q in range(9)])
    rows = np.unique(np.concatenate([edges[(edges >= 0) & (edges < M)], rng.integers(0, M, size=2048)]))
    assert [(int(got[i]), int(got[M + i])) for i in rows] == data.want(air, True, rows), (p, w)
    assert data.unchanged(torch)
    air.close()


# ------------------------------------------------------------------------------------------------ the two hard-wired quotients
@pytest.mark.parametrize("log2_m", [10, 11, 12, 13])
@pytest.mark.parametrize("p,w", FIELDS)
def test_word_for_word_against_the_plonk_quotient(torch, p, w, log2_m):
    """the gate, P1 and Z - 1 as a program with lambda = 1, alpha, alpha^2 and the kinds ALL, ALL, FIRST; then the logUp pair of
    C = 1, 2, 5 columns, with and without multiplicities, added onto that T by both"""
    log2_b = 1 + log2_m % 3
    M = 1 << log2_m
    air = Air(p, w, log2_m - log2_b, log2_b, AP.plonk(), (3, 5, 3, 1), 1, 2)
    E = air.E
    cols = [words(log2_m + j, k * M, p) for j, k in enumerate((3, 5, 3, 1, 2))]
    alpha, beta, gamma = (words(log2_m + 5 + j, 2, p) for j in range(3))
    a = E.el(alpha.tolist())
    d_cols, d_ch = [dev(torch, c) for c in cols], [dev(torch, c) for c in (alpha, beta, gamma)]
    d_chal, d_lam = dev(torch, np.concatenate([beta, gamma])), dev(torch, flat([E.one, a, E.mul(a, a)]))
    d_want, d_got = garbage(torch, 2 * M), garbage(torch, 2 * M)
    L.check(L.lib.ronk_plonk_quotient_dev(air.d, *[t.data_ptr() for t in d_cols], *[t.data_ptr() for t in d_ch], d_want.data_ptr(), 0))
    air.call(d_cols[:4], d_cols[4:], d_chal, d_lam, None, d_got)
    assert np.array_equal(host(torch, d_got), host(torch, d_want)), (p, w, log2_m)
    for n_cols, with_mult in ((1, True), (2, False), (5, True), (5, False)):
        lookup = Air(p, w, log2_m - log2_b, log2_b, AP.logup(n_cols, with_mult), (n_cols, n_cols) if with_mult else (n_cols,), 1, 1)
        vals, mult, S = (dev(torch, words(log2_m + 20 + n_cols + j, k * M, p)) for j, k in enumerate((n_cols, n_cols, 2)))
        d_alpha, d_l = dev(torch, words(log2_m + 30, 2, p)), dev(torch, words(log2_m + 31, 4, p))
        d_want2, d_got2 = garbage(torch, 2 * M), garbage(torch, 2 * M)
        L.check(L.lib.ronk_logup_quotient_dev(air.d, vals.data_ptr(), mult.data_ptr() if with_mult else None, n_cols, S.data_ptr(),
                                              d_alpha.data_ptr(), d_l.data_ptr(), d_want.data_ptr(), d_want2.data_ptr(), 0))
        lookup.call([vals, mult] if with_mult else [vals], [S], d_alpha, d_l, d_got, d_got2)
        assert np.array_equal(host(torch, d_got2), host(torch, d_want2)), (p, w, log2_m, n_cols, with_mult)
        lookup.close()
    air.close()


# ------------------------------------------------------------------------------------------------ capture, host form, caller
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_a_captured_graph_replayed_on_changed_columns_and_challenges(torch, p, w):
    """one launch, no library workspace and no host round trip: legal under capture; a replay reads the arrays as they are then"""
    rng = np.random.default_rng(4)
    prog, _ = AP.random_program(rng, 5, 2, 3, rotations(1 << 10), KINDS[4], 4, depth=4)
    air = Air(p, w, 10, 2, prog, (2, 3), 2, 3)
    data = Data(torch, air, 3, 40)
    d_T = garbage(torch, 2 * air.M)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, data.d_T_in, d_T, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(host(torch, d_T), data.want(air, True))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        air.call(data.d_base, data.d_ext, data.d_chal, data.d_lam, data.d_T_in, d_T, stream=torch.cuda.current_stream().cuda_stream)
    other = Data(torch, air, 3, 41)
    for d, o in zip(data.d_base + data.d_ext + [data.d_chal, data.d_lam, data.d_T_in], other.d_base + other.d_ext + [other.d_chal, other.d_lam, other.d_T_in]):
        d.copy_(o)
    for _ in range(2):
        d_T.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(torch, d_T), other.want(air, True))
    air.close()


@pytest.mark.parametrize("p,w", FIELDS)
def test_host_pointer_form_and_the_caller(torch, p, w):
    rng = np.random.default_rng(8)
    prog, _ = AP.random_program(rng, 5, 2, 3, rotations(1 << 6), KINDS[4], 4, depth=4)
    air = Air(p, w, 6, 2, prog, (2, 3), 2, 3)
    data = Data(torch, air, 3, 50)
    M = air.M
    hp = lambda arrays: (C.c_void_p * max(1, len(arrays)))(*[a.ctypes.data for a in arrays])      # noqa: E731
    for T_in in (None, data.T_in):
        T = np.full(2 * M, 2**64 - 1, dtype=np.uint64)
        L.check(L.lib.ronk_air_quotient(air.h, hp(data.base), hp(data.ext), L.ptr(data.chal), L.ptr(data.lam),
                                        None if T_in is None else L.ptr(T_in), L.ptr(T)))
        assert np.array_equal(T, data.want(air, T_in is not None))
    assert L.lib.ronk_air_quotient(air.h, hp(data.base), None, L.ptr(data.chal), L.ptr(data.lam), None, L.ptr(T)) == L.ERR_INVALID
    assert L.lib.ronk_air_quotient_dev(air.h, pointers(data.d_base), pointers(data.d_ext), None, data.d_lam.data_ptr(), None,
                                       data.d_T_in.data_ptr(), 0) == L.ERR_INVALID
    air.close()
    from ronkathon_amd import callers

    class F:
        ORDER = p
    got = callers.air_quotient(F, GEN[p], w, 6, 2, GEN[p], tuple(prog), [a.reshape(c, M) for a, c in zip(data.base, (2, 3))],
                               [a.reshape(2, M) for a in data.ext], AR.pairs_of(data.chal), AR.pairs_of(data.lam), data.T_in.reshape(2, M))
    assert np.array_equal(got, data.want(air, True))
    with pytest.raises(L.RonkPanic) as e:
        callers.air_quotient(F, GEN[p], w, 6, 2, GEN[p], (prog.ops, prog.imm, prog.n_regs, prog.n_constraints + 1),
                             [a.reshape(c, M) for a, c in zip(data.base, (2, 3))], [a.reshape(2, M) for a in data.ext],
                             AR.pairs_of(data.chal), AR.pairs_of(data.lam) + [(1, 0)])
    assert e.value.code == L.ERR_INVALID            # a constraint is never emitted


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_end_to_end_through_the_existing_entry_points(torch, p, w):
    """a Fibonacci trace of N = 2^6 rows with all four kinds: ronk_lde_batch_dev, the quotient, ronk_ntt_inverse_dev per plane and
    the un-shift by s^-i give zeros from N - 1 upward, and not with one trace word changed; ronk_air_eval_point at a random point z,
    from the columns' values at z w_N^rot (ronk_ext2_poly_eval_batch), equals T(z)"""
    log2_n, log2_b = 6, 2
    g = shift = GEN[p]
    N, M = 1 << log2_n, 1 << (log2_n + log2_b)
    rng = np.random.default_rng(61)
    prog = AP.fibonacci()
    air = Air(p, w, log2_n, log2_b, prog, (3,), 0, 2)
    E, dom = air.E, air.dom
    pk, pn, inv = L.Plan(p, g, log2_n, 4), L.Plan(p, g, log2_n + log2_b, 4), L.Plan(p, g, log2_n + log2_b, 1)
    sinv = pow(shift, -1, p)
    unshift = [pow(sinv, j, p) for j in range(M)]
    lam = [tuple(int(v) % p for v in rng.integers(0, 2**62, size=2)) for _ in range(5)]
    d_lam = dev(torch, flat(lam))

    def quotient(trace, first, last):
        chal = [(first, 0), (last, 0)]
        d_in = dev(torch, np.array(trace + [[0] * N], dtype=np.uint64).ravel())
        d_co, d_cols, d_T, d_c = garbage(torch, 4 * N), garbage(torch, 4 * M), garbage(torch, 2 * M), garbage(torch, 2 * M)
        L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_in.data_ptr(), d_co.data_ptr(), d_cols.data_ptr(), shift, 0))
        air.call([d_cols], [], dev(torch, flat(chal)), d_lam, None, d_T)
        for plane in (0, 1):
            L.check(L.lib.ronk_ntt_inverse_dev(inv.h, d_T.data_ptr() + 8 * plane * M, d_c.data_ptr() + 8 * plane * M, 0))
        coef = [[v * u % p for v, u in zip(plane, unshift)] for plane in host(torch, d_c).reshape(2, M).tolist()]
        on = host(torch, d_cols).reshape(4, M)[:3].tolist()
        assert host(torch, d_T).tolist() == AR.planar(AR.quotient(E, dom, prog, on, [], chal, lam))
        return coef, chal

    trace = AP.fibonacci_trace(p, N, 2, 3)
    coef, chal = quotient(trace, trace[0][0], trace[1][-1])
    poly = np.array([PR.interpolate(p, dom.wN, col) for col in trace], dtype=np.uint64)       # the trace polynomials
    assert not any(coef[0][N - 1:]) and not any(coef[1][N - 1:]) and coef[0][N - 2]
    # the identity at one point: the cells a verifier needs opened, their values, and T(z)
    n_cells = L.lib.ronk_air_cells(air.h, None, 0)
    cells = (C.c_uint32 * n_cells)()
    assert L.lib.ronk_air_cells(air.h, cells, n_cells) == n_cells and list(cells) == AR.cells(prog.ops)
    z = tuple(int(v) % p for v in rng.integers(0, 2**62, size=2))
    opened = []
    for o in cells:
        _, index, rot = AR.decode(o)
        y = L.ext2_poly_eval_batch(p, w, poly[index:index + 1], np.array(E.mul_base(z, pow(dom.wN, rot, p)), dtype=np.uint64))
        opened.append((int(y[0]), int(y[1])))
    Tz = E.add(PR.evaluate_ext(E, coef[0], z), E.mul(PR.evaluate_ext(E, coef[1], z), (0, 1)))
    out = (C.c_uint64 * 2)()
    L.check(L.lib.ronk_air_eval_point(air.h, (C.c_uint64 * 2)(*z), L.ptr(flat(opened)), L.ptr(flat(chal)), L.ptr(flat(lam)), out))
    assert (out[0], out[1]) == Tz == AR.eval_point(E, dom, prog, z, opened, chal, lam)
    for on_h in ((1, 0), (dom.wN, 0), (pow(dom.wN, -1, p), 0)):
        assert L.lib.ronk_air_eval_point(air.h, (C.c_uint64 * 2)(*on_h), L.ptr(flat(opened)), L.ptr(flat(chal)), L.ptr(flat(lam)), out) == L.ERR_INVALID
    # one trace word changed, a wrong first value, a wrong last value
    bad = [list(col) for col in trace]
    bad[1][N // 2] = (bad[1][N // 2] + 1) % p
    for tr, first, last in ((bad, trace[0][0], trace[1][-1]), (trace, trace[0][0] + 1, trace[1][-1]), (trace, trace[0][0], trace[1][-1] + 1)):
        coef, _ = quotient(tr, first, last)
        assert any(coef[0][N - 1:]) or any(coef[1][N - 1:])
    air.close()
