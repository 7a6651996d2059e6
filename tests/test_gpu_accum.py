"""The running products and sums, the permutation grand product and the logUp running sum on the device (ronk_vec_prefix_*_dev,
ronk_ext2_vec_prefix_*_dev, ronk_perm_product_dev, ronk_logup_sum_dev) against the Python restatement tests/accum_ref.py, over
Goldilocks (its own arithmetic, w = 7 and w = 11), MONT_P, P_MID and P_62 (the Montgomery policy) and the reference's own F_17
permutation vectors (tests/golden/plonk_f17_permutation.json).  Extension arrays are planar: [2][n] words.

The blocking under test (csrc/accum_kernels.h): a lane owns 8 elements, a wavefront 512, a workgroup 2048; phase 2 gives each of
its 256 lanes ceil(B / 256) of the B block totals, which leaves 1 at n = 2048 * 256 + 1 -- the only size-dependent switch."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import prime_classes as PC
from ronkathon_amd import _lib as L
from test_gpu_fri import dev, host, words

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
EXT_FIELDS = [(GL, 7), (GL, 11), (MONT, 10), (PC.P_MID, PC.GEN[PC.P_MID]), (PC.P_62, PC.GEN[PC.P_62])]
BASE_FIELDS = [GL, MONT, PC.P_MID, PC.P_62]
GEN = {**PC.GEN, GL: 7}
BLOCK = 2048
SIZES = sorted({1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 65535, 65537}
               | {7, 8, 9, 511, 512, 513, 2047, 2048, 2049})     # and the lane, wavefront and workgroup boundaries
SWITCH = BLOCK * 256 + 1                                          # phase 2: two totals per lane from here on
LARGE = [SWITCH, (1 << 20) + 1, 1 << 22]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def f17():
    with open(os.path.join(HERE, "golden", "plonk_f17_permutation.json")) as f:
        return json.load(f)


def garbage(torch, n):
    return torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")


def work_for(torch, n):
    return garbage(torch, L.lib.ronk_scan_workspace_words(n))


def scan_dev(torch, p, w, op, d_a, d_out, n, exclusive, with_total, d_work, stream=0):
    """one _dev call; w None: the base field.  -> the total words (or None)"""
    ew = 1 if w is None else 2
    d_total = garbage(torch, ew) if with_total else None
    tp = d_total.data_ptr() if with_total else None
    if w is None:
        fn = L.lib.ronk_vec_prefix_prod_dev if op == "prod" else L.lib.ronk_vec_prefix_sum_dev
        L.check(fn(p, d_a.data_ptr(), d_out.data_ptr(), n, exclusive, tp, d_work.data_ptr(), stream))
    else:
        fn = L.lib.ronk_ext2_vec_prefix_prod_dev if op == "prod" else L.lib.ronk_ext2_vec_prefix_sum_dev
        L.check(fn(p, w, d_a.data_ptr(), d_out.data_ptr(), n, exclusive, tp, d_work.data_ptr(), stream))
    return host(torch, d_total).tolist() if with_total else None


def scan_input(seed, n, p, ew, op):
    """words with the edges mixed in (0, p - 1, words >= p); a product keeps its zeros out so that it stays alive"""
    a = words(seed, ew * n, p)
    if op == "prod":
        a[a % np.uint64(p) == 0] = 2
    return a


def check_scans(torch, p, w, op):
    ew = 1 if w is None else 2
    E = None if w is None else AR.Ext2(p, w)
    for n in SIZES:
        a = scan_input(n, n, p, ew, op)
        if w is None:
            incl, total = AR.base_scan(p, a.tolist(), op, 0)
            excl = [1 if op == "prod" else 0] + incl[:-1]
            want = {0: np.array(incl, dtype=np.uint64), 1: np.array(excl, dtype=np.uint64)}
            total = [total]
        else:
            incl, total = AR.ext_scan(E, AR.pairs(a.tolist()), op, 0)
            excl = [E.one if op == "prod" else E.zero] + incl[:-1]
            want = {0: np.array(AR.planar(incl), dtype=np.uint64), 1: np.array(AR.planar(excl), dtype=np.uint64)}
            total = list(total)
        d_work = work_for(torch, n)
        d_src = dev(torch, a)
        for exclusive in (0, 1):
            for in_place in (False, True):
                for with_total in (False, True):
                    d_a = d_src.clone() if in_place else d_src
                    d_out = d_a if in_place else garbage(torch, ew * n)
                    got_total = scan_dev(torch, p, w, op, d_a, d_out, n, exclusive, with_total, d_work)
                    assert np.array_equal(host(torch, d_out), want[exclusive]), (p, w, op, n, exclusive, in_place, with_total)
                    assert got_total == (total if with_total else None), (p, w, op, n, "total")
        assert np.array_equal(host(torch, d_src), a), "an out-of-place scan changed its input"


@pytest.mark.parametrize("op", ["prod", "sum"])
@pytest.mark.parametrize("p", BASE_FIELDS)
def test_base_scans(torch, p, op):
    check_scans(torch, p, None, op)


@pytest.mark.parametrize("op", ["prod", "sum"])
@pytest.mark.parametrize("p,w", EXT_FIELDS)
def test_extension_scans(torch, p, w, op):
    check_scans(torch, p, w, op)


def sample_indices(rng, n):
    """every block boundary and its neighbours, the ends, and 4096 random indices"""
    edges = np.arange(0, n + 1, BLOCK)
    idx = np.concatenate([edges - 1, edges, edges + 1, [0, n - 1], rng.integers(0, n, size=4096)])
    return np.unique(idx[(idx >= 0) & (idx < n)])


@pytest.mark.parametrize("n", LARGE)
@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_large_scans_against_closed_forms(torch, p, w, n):
    """a constant g with 32 random positions overwritten by random words: out[i] = g^(i + 1 - k_i) * (the specials up to i), k_i
    the specials among the first i + 1 positions; a[i] = i + 1 for the sums.  Checked by pow at the sampled indices."""
    rng = np.random.default_rng(n ^ p & 0xFFFF)
    E = AR.Ext2(p, w)
    idx = sample_indices(rng, n)
    pos = np.sort(rng.choice(n, size=32, replace=False))
    d_work = work_for(torch, n)
    # products: the base field with the generator, the extension with (g, 1); in place, exclusive, with the total
    for ew in (1, 2):
        g = (GEN[p], 1) if ew == 2 else (GEN[p], 0)
        a = np.empty(ew * n, dtype=np.uint64)
        a[:n] = g[0]
        a[n:] = g[1]
        special = [(int(rng.integers(1, 2**63)), int(rng.integers(1, 2**63)) if ew == 2 else 0) for _ in pos]
        for k, s in zip(pos, special):
            a[k] = s[0]
            if ew == 2:
                a[n + k] = s[1]
        d_a = dev(torch, a)
        total = scan_dev(torch, p, w if ew == 2 else None, "prod", d_a, d_a, n, 1, True, d_work)
        got = host(torch, d_a)
        acc, before = [E.one], E.one                        # acc[k]: the product of the first k specials
        for s in special:
            before = E.mul(before, E.el(s))
            acc.append(before)
        count = np.searchsorted(pos, idx, side="left")      # the specials strictly before i: the exclusive form
        for i, k in zip(idx.tolist(), count.tolist()):
            want = E.mul(E.pow(g, i - k), acc[k])
            assert (int(got[i]), int(got[n + i]) if ew == 2 else 0) == want, (p, n, ew, i)
        assert tuple(total + [0])[:2] == E.mul(E.pow(g, n - 32), acc[32]), (p, n, ew, "total")
    # sums: out of place, inclusive, no total; a[i] = i + 1, and (i + 1, 3 (i + 1)) as pairs
    i1 = np.arange(1, n + 1, dtype=np.uint64)
    for ew in (1, 2):
        a = np.concatenate([i1, i1 * np.uint64(3)]) if ew == 2 else i1
        d_a, d_out = dev(torch, a), garbage(torch, ew * n)
        scan_dev(torch, p, w if ew == 2 else None, "sum", d_a, d_out, n, 0, False, d_work)
        got = host(torch, d_out)
        for i in idx.tolist():
            t = (i + 1) * (i + 2) // 2
            assert int(got[i]) == t % p and (ew == 1 or int(got[n + i]) == 3 * t % p), (p, n, ew, i)


# ------------------------------------------------------------------------------------------------ the accumulators
def perm_dev(torch, p, w, wires, ids, sigma, beta, gamma, stream=0, bufs=None):
    """-> (Z planar words, Z[N] as a pair, status); wires, ids, sigma: numpy [W][N]"""
    W, N = wires.shape
    if bufs is None:
        bufs = (dev(torch, wires.ravel()), dev(torch, ids.ravel()), dev(torch, sigma.ravel()),
                dev(torch, np.array(beta, dtype=np.uint64)), dev(torch, np.array(gamma, dtype=np.uint64)),
                garbage(torch, 2 * N), garbage(torch, 2), work_for(torch, N), torch.full((1,), 7, dtype=torch.int32, device="cuda"))
    d_a, d_i, d_s, d_b, d_g, d_Z, d_last, d_work, d_st = bufs
    L.check(L.lib.ronk_perm_product_dev(p, w, d_a.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), W, N, d_b.data_ptr(), d_g.data_ptr(),
                                        d_Z.data_ptr(), d_last.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), stream))
    return host(torch, d_Z), tuple(host(torch, d_last).tolist()), int(d_st.item())


def logup_dev(torch, p, w, vals, mult, alpha):
    C, N = vals.shape
    d_v, d_m = dev(torch, vals.ravel()), None if mult is None else dev(torch, mult.ravel())
    d_al, d_S, d_last, d_work = dev(torch, np.array(alpha, dtype=np.uint64)), garbage(torch, 2 * N), garbage(torch, 2), work_for(torch, N)
    d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.check(L.lib.ronk_logup_sum_dev(p, w, d_v.data_ptr(), None if d_m is None else d_m.data_ptr(), C, N, d_al.data_ptr(), d_S.data_ptr(),
                                     d_last.data_ptr(), d_work.data_ptr(), d_st.data_ptr(), 0))
    return host(torch, d_S), tuple(host(torch, d_last).tolist()), int(d_st.item())


def test_f17_fixture_on_the_device(torch, f17):
    p, w = f17["p"], f17["w"]
    E = AR.Ext2(p, w)
    wires, ids, sigma = (np.array(f17[k], dtype=np.uint64) for k in ("wires", "ids", "sigma"))
    for ch in f17["closing_challenges"]:
        Z, last, status = perm_dev(torch, p, w, wires, ids, sigma, ch["beta"], ch["gamma"])
        want, want_last, want_status = AR.perm_product(E, f17["wires"], f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])
        assert Z.tolist() == AR.planar(want) and last == want_last == (1, 0) and status == want_status == 0, ch
    # a challenge pair that meets a zero denominator, and words >= p
    Z, last, status = perm_dev(torch, p, w, wires + np.uint64(p), ids, sigma + np.uint64(2 * p), (1, 0), (11, 0))
    want, want_last, want_status = AR.perm_product(E, f17["wires"], f17["ids"], f17["sigma"], (1, 0), (11, 0))
    assert want_status == 1 and (Z.tolist(), last, status) == (AR.planar(want), want_last, 1)


def field_of(case):
    return EXT_FIELDS[case % len(EXT_FIELDS)]


def random_columns(seed, W, N, p):
    return words(seed, W * N, p).reshape(W, N)


def challenge(rng, p):
    return (int(rng.integers(0, 2**63)) % p, int(rng.integers(0, 2**63)) % p)


@pytest.mark.parametrize("N", [1, 5, 4097, 65537])
@pytest.mark.parametrize("W", [1, 3, 16])
def test_perm_product_random_instances(torch, W, N):
    """every row against the restatement; the small shapes over every field, the large ones over one each (Goldilocks with
    w = 7 takes W = 3 and W = 16 at N = 65537 and 4097, MONT_P the largest)"""
    fields = EXT_FIELDS if N <= 5 else [{(1, 4097): EXT_FIELDS[1], (3, 4097): EXT_FIELDS[3], (16, 4097): EXT_FIELDS[0],
                                         (1, 65537): EXT_FIELDS[4], (3, 65537): EXT_FIELDS[0], (16, 65537): EXT_FIELDS[2]}[(W, N)]]
    for p, w in fields:
        E = AR.Ext2(p, w)
        rng = np.random.default_rng(W * 100003 + N)
        wires, ids, sigma = random_columns(1 + N, W, N, p), random_columns(2 + N, W, N, p), random_columns(3 + N, W, N, p)
        beta, gamma = challenge(rng, p), challenge(rng, p)
        Z, last, status = perm_dev(torch, p, w, wires, ids, sigma, beta, gamma)
        want, want_last, want_status = AR.perm_product_fast(E, wires.tolist(), ids.tolist(), sigma.tolist(), beta, gamma)
        assert want_status == 0 and status == 0 and last == want_last, (p, w, W, N)
        assert np.array_equal(Z, np.array(AR.planar(want), dtype=np.uint64)), (p, w, W, N)


@pytest.mark.parametrize("N", [1, 5, 4097, 65537])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_logup_sum_random_instances(torch, C, N):
    fields = EXT_FIELDS if N <= 5 else [{(1, 4097): EXT_FIELDS[2], (3, 4097): EXT_FIELDS[4], (16, 4097): EXT_FIELDS[0],
                                         (1, 65537): EXT_FIELDS[3], (3, 65537): EXT_FIELDS[0], (16, 65537): EXT_FIELDS[1]}[(C, N)]]
    for p, w in fields:
        E = AR.Ext2(p, w)
        rng = np.random.default_rng(C * 100019 + N)
        vals, mult = random_columns(4 + N, C, N, p), random_columns(5 + N, C, N, p)
        alpha = challenge(rng, p)
        for m in ((mult, None) if N < 65537 else (mult,)):     # all ones: the smaller shapes
            S, last, status = logup_dev(torch, p, w, vals, m, alpha)
            want, want_last, want_status = AR.logup_sum_fast(E, vals.tolist(), None if m is None else m.tolist(), alpha)
            assert want_status == 0 and status == 0 and last == want_last, (p, w, C, N)
            assert np.array_equal(S, np.array(AR.planar(want), dtype=np.uint64)), (p, w, C, N, m is None)


@pytest.mark.parametrize("p,w", EXT_FIELDS)
def test_zero_denominator_rows(torch, p, w):
    """status 1; the product is ZERO from the row after on, the sum only loses that term.  gamma1 = -beta1 s makes
    a + beta s + gamma = 0 for the wire a = -(beta0 s + gamma0) wherever sigma = s."""
    E = AR.Ext2(p, w)
    W, N = 3, 4097
    rng = np.random.default_rng(p % 9973)
    wires, ids, sigma = random_columns(11, W, N, p), random_columns(12, W, N, p), random_columns(13, W, N, p)
    beta, s = challenge(rng, p), 12345 % p
    gamma = (int(rng.integers(0, 2**63)) % p, -beta[1] * s % p)
    for rows in ([2051], [N - 1], [8, 15], [0]):            # mid-chunk in the second block, the last row, both ends of a chunk, row 0
        a, sg = wires.copy(), sigma.copy()
        for k, r in enumerate(rows):
            sg[k % W, r], a[k % W, r] = s, -(beta[0] * s + gamma[0]) % p
        Z, last, status = perm_dev(torch, p, w, a, ids, sg, beta, gamma)
        want, want_last, want_status = AR.perm_product_fast(E, a.tolist(), ids.tolist(), sg.tolist(), beta, gamma)
        assert want_status == 1 and status == 1 and last == want_last == (0, 0), (p, rows)
        assert np.array_equal(Z, np.array(AR.planar(want), dtype=np.uint64)), (p, rows)
        r = rows[0]
        assert (Z[r], Z[N + r]) != (0, 0) and not Z[r + 1:N].any() and not Z[N + r + 1:].any()
    alpha = (int(rng.integers(0, 2**63)) % p, 0)
    for rows in ([2051], [N - 1], [8, 15]):
        v = wires.copy()
        for k, r in enumerate(rows):
            v[k % W, r] = -alpha[0] % p
        for m in (None, ids):
            S, last, status = logup_dev(torch, p, w, v, m, alpha)
            want, want_last, want_status = AR.logup_sum_fast(E, v.tolist(), None if m is None else m.tolist(), alpha)
            assert want_status == 1 and status == 1 and last == want_last != (0, 0), (p, rows)
            assert np.array_equal(S, np.array(AR.planar(want), dtype=np.uint64)), (p, rows)


def rows_to_check(rng, N):
    edges = np.arange(0, N + 1, BLOCK)
    idx = np.concatenate([edges - 1, edges, [0, N - 1], rng.integers(0, N, size=4096)])
    return np.unique(idx[(idx >= 0) & (idx < N)]).tolist()


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_perm_product_closes_at_2_20(torch, p, w):
    """3 x 2^20 cells grouped by a random variable id, sigma the cyclic shift inside each group, ids the cell numbers plus one:
    status 0, Z[0] = 1, Z[N] = 1, and Z[i+1] den_i = Z[i] num_i on Python integers at every block boundary and 4096 random rows"""
    E = AR.Ext2(p, w)
    N, W = 1 << 20, 3
    rng = np.random.default_rng(20)
    wires, ids, sigma = AR.cycle_instance(rng, N, W, N // 2)
    beta, gamma = challenge(rng, p), challenge(rng, p)
    Z, last, status = perm_dev(torch, p, w, wires, ids, sigma, beta, gamma)
    assert status == 0 and (int(Z[0]), int(Z[N])) == (1, 0) and last == (1, 0)
    z = lambda i: (int(Z[i]), int(Z[N + i])) if i < N else last          # noqa: E731
    moved = 0
    for i in rows_to_check(rng, N):
        num, den = AR.perm_factors(E, wires, ids, beta, gamma, i), AR.perm_factors(E, wires, sigma, beta, gamma, i)
        assert E.mul(z(i + 1), den) == E.mul(z(i), num), (p, i)
        moved += z(i + 1) != z(i)
    assert moved > 1000, "the product must move"
    # one altered wire value no longer closes
    cell = int(np.flatnonzero(sigma[1] != ids[1])[0])                  # a cell that is joined to another
    wires[1, cell] ^= np.uint64(1)
    assert perm_dev(torch, p, w, wires, ids, sigma, beta, gamma)[1] != (1, 0)


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_logup_multiset_identity_at_2_20(torch, p, w):
    """two witness columns whose values all lie in a table column, the table with minus the counts as its multiplicities:
    S[N] = 0 in one call over the three columns; the recurrence at the sampled rows; one foreign value breaks it"""
    E = AR.Ext2(p, w)
    N = 1 << 20
    rng = np.random.default_rng(21)
    table = rng.permutation(N).astype(np.uint64) * np.uint64(7) + np.uint64(3)          # distinct
    pick = rng.integers(0, N, size=(2, N))
    counts = np.bincount(pick.ravel(), minlength=N).astype(np.uint64)
    vals = np.stack([table[pick[0]], table[pick[1]], table])
    mult = np.stack([np.ones(N, dtype=np.uint64), np.ones(N, dtype=np.uint64), (np.uint64(p) - counts) % np.uint64(p)])
    alpha = challenge(rng, p)
    S, last, status = logup_dev(torch, p, w, vals, mult, alpha)
    assert status == 0 and (int(S[0]), int(S[N])) == (0, 0) and last == (0, 0)
    s = lambda i: (int(S[i]), int(S[N + i])) if i < N else last          # noqa: E731
    for i in rows_to_check(rng, N):
        step = E.zero
        for c in range(3):
            step = E.add(step, E.mul_base(E.inv(E.add(alpha, E.embed(vals[c][i]))), int(mult[c][i]) % p))
        assert s(i + 1) == E.add(s(i), step), (p, i)
    assert s(N // 2) != (0, 0)
    # the witness columns alone, all ones by d_mult == NULL, against the table alone
    Sw, last_w, _ = logup_dev(torch, p, w, vals[:2], None, alpha)
    St, last_t, _ = logup_dev(torch, p, w, vals[2:], counts.reshape(1, N), alpha)
    assert last_w == last_t != (0, 0)
    vals[0, 424242] = np.uint64(5)                                       # 5 = 7 k + 3 has no solution: a foreign value
    assert logup_dev(torch, p, w, vals, mult, alpha)[1] != (0, 0)


@pytest.mark.parametrize("p,w", [(GL, 7), (MONT, 10)])
def test_perm_product_under_stream_capture(torch, p, w):
    """no library workspace and no host round trip: the call is legal under capture, and two replays give the same words"""
    E = AR.Ext2(p, w)
    W, N = 3, 4097
    rng = np.random.default_rng(31)
    wires, ids, sigma = AR.cycle_instance(rng, N, W, 500)
    beta, gamma = challenge(rng, p), challenge(rng, p)
    want, want_last, _ = AR.perm_product_fast(E, wires.tolist(), ids.tolist(), sigma.tolist(), beta, gamma)
    assert want_last == (1, 0)
    bufs = (dev(torch, wires.ravel()), dev(torch, ids.ravel()), dev(torch, sigma.ravel()), dev(torch, np.array(beta, dtype=np.uint64)),
            dev(torch, np.array(gamma, dtype=np.uint64)), garbage(torch, 2 * N), garbage(torch, 2), work_for(torch, N),
            torch.full((1,), 7, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):     # warm-up outside the capture
        perm_dev(torch, p, w, wires, ids, sigma, beta, gamma, stream=s.cuda_stream, bufs=bufs)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        L.check(L.lib.ronk_perm_product_dev(p, w, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), W, N, bufs[3].data_ptr(),
                                            bufs[4].data_ptr(), bufs[5].data_ptr(), bufs[6].data_ptr(), bufs[7].data_ptr(),
                                            bufs[8].data_ptr(), st))
    for _ in range(2):
        bufs[5].fill_(-1); bufs[6].fill_(-1); bufs[7].fill_(-1); bufs[8].fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert host(torch, bufs[5]).tolist() == AR.planar(want) and tuple(host(torch, bufs[6]).tolist()) == (1, 0)
        assert int(bufs[8].item()) == 0


def test_python_wrappers(torch, f17):
    """callers.prefix_prod / prefix_sum / perm_product / logup_sum: the host-pointer forms"""
    from ronkathon_amd import callers

    class F:
        ORDER = GL
    E = AR.Ext2(GL, 7)
    n = 5000
    a = scan_input(77, n, GL, 2, "prod")
    for name, op in (("prefix_prod", "prod"), ("prefix_sum", "sum")):
        for exclusive in (False, True):
            out, total = getattr(callers, name)(F, a[:n], exclusive=exclusive)
            want, want_total = AR.base_scan(GL, a[:n].tolist(), op, int(exclusive))
            assert out.tolist() == want and total == want_total
            out, total = getattr(callers, name)(F, a, exclusive=exclusive, w=7)
            want, want_total = AR.ext_scan(E, AR.pairs(a.tolist()), op, int(exclusive))
            assert out.tolist() == AR.planar(want) and total == want_total

    class F17:
        ORDER = 17
    ch = f17["closing_challenges"][1]
    Z, last, status = callers.perm_product(F17, 3, f17["wires"], f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])
    want, _, _ = AR.perm_product(AR.Ext2(17, 3), f17["wires"], f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])
    assert Z.tolist() == AR.planar(want) and last == (1, 0) and status == 0
    S, last, status = callers.logup_sum(F17, 3, [[1, 4], [2, 2]], None, (13, 0))
    want, want_last, _ = AR.logup_sum(AR.Ext2(17, 3), [[1, 4], [2, 2]], None, (13, 0))
    assert S.tolist() == AR.planar(want) and last == want_last and status == 1
    with pytest.raises(L.RonkPanic) as e:
        callers.perm_product(F17, 2, f17["wires"], f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])     # 2 = 6^2 is a residue
    assert e.value.code == L.ERR_INVALID
