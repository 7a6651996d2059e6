"""The restatement tests/lookup_ref.py against what it must be: multiplicities that close the logUp running sum of
tests/accum_ref.py, and a quotient that is a polynomial of degree below C N - C exactly when the lookup holds.  Pure Python."""
import numpy as np
import pytest

import accum_ref as AR
import lookup_ref as LR
import plonk_ref as PR
import prime_classes as PC

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
FIELDS = [(GL, 7, 7), (MONT, 10, 10)]      # p, g, w


def instance(rng, p, N, C):
    """a table column with repeats and C - 1 lookup columns drawn from it: -> (lookups [C - 1][N], table [N])"""
    table = [int(v) % p for v in rng.integers(0, 2**62, size=N)]
    for j in range(N // 4):                      # repeats: only the first of each value counts
        table[int(rng.integers(0, N))] = table[int(rng.integers(0, N))]
    lookups = [[table[int(k)] for k in rng.integers(0, N, size=N)] for _ in range(C - 1)]
    return lookups, table


def argument(E, lookups, table, alpha):
    """the columns, the multiplicities and the running sum of one lookup argument: -> (vals, mult, S, S[N], missing)"""
    p = E.p
    m, missing, _ = LR.multiplicities(p, table, lookups, negate=True)
    vals, mult = lookups + [table], [[1] * len(table) for _ in lookups] + [m]
    S, last, status = AR.logup_sum(E, vals, mult, alpha)
    assert status == 0
    return vals, mult, S, last, missing


@pytest.mark.parametrize("N", [8, 16, 32])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_multiplicities_close_the_running_sum(p, g, w, N):
    rng = np.random.default_rng(N)
    E = LR.Ext2(p, w)
    for C in (2, 3):
        lookups, table = instance(rng, p, N, C)
        alpha = [int(v) for v in rng.integers(1, 2**62, size=2)]
        _, mult, _, last, missing = argument(E, lookups, table, alpha)
        assert last == E.zero and missing == 0
        # the counts themselves: every cell is counted once, at a first occurrence
        plain, _, _ = LR.multiplicities(p, table, lookups)
        assert sum(plain) == (C - 1) * N
        assert all(k == 0 for j, k in enumerate(plain) if table.index(table[j]) != j)
        assert mult[-1] == [(p - k) % p for k in plain]


def test_multiplicities_compare_reduced_words_and_report_what_is_missing():
    p = 17
    table = [3, 20, 5, 16, 5 + 17 * 4]                    # 20 = 3 and 73 = 5 (mod 17)
    vals = [[3, 3 + 17, 5, 1], [16, 33, 2, 5]]            # 1 and 2 are not in the table
    assert LR.multiplicities(p, table, vals) == ([2, 0, 2, 2, 0], 2, 3)
    assert LR.multiplicities(p, table, vals, negate=True) == ([15, 0, 15, 15, 0], 2, 3)
    assert LR.multiplicities(p, [1, 2], [[1] * 40]) == ([40 % 17, 0], 0, LR.NONE_MISSING)
    assert LR.multiplicities(p, [1, 2], [[1] * 34], negate=True) == ([0, 0], 0, LR.NONE_MISSING)


def high(E, dom, T, C):
    """the coefficients of both planes from C N - C upward"""
    return [PR.coset_coefficients(dom, [t[plane] for t in T])[C * dom.N - C:] for plane in (0, 1)]


def on_coset(dom, vals, mult, S):
    ext = lambda cols: [PR.extend(dom, col) for col in cols]      # noqa: E731
    return ext(vals), ext(mult), ext([[s[0] for s in S], [s[1] for s in S]])


@pytest.mark.parametrize("log2_b", [2, 3])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_the_quotient_is_a_polynomial_exactly_when_the_lookup_holds(p, g, w, log2_b):
    log2_n = 3
    N = 1 << log2_n
    E = LR.Ext2(p, w)
    dom = PR.Domain(p, g, log2_n, log2_b, g)
    rng = np.random.default_rng(10 * log2_b)
    alpha = [int(v) for v in rng.integers(1, 2**62, size=2)]
    lam = [[int(v) for v in rng.integers(1, 2**62, size=2)] for _ in range(2)]

    def coefficients(vals, mult, S, C):
        v, m, s = on_coset(dom, vals, mult, S)
        return high(E, dom, LR.quotient(E, dom, v, m, s, alpha, lam), C)

    for C in (2, 3, 4):
        lookups, table = instance(rng, p, N, C)
        vals, mult, S, last, _ = argument(E, lookups, table, alpha)
        assert last == E.zero
        hi = coefficients(vals, mult, S, C)
        assert len(hi[0]) == dom.M - (C * N - C) and not any(hi[0]) and not any(hi[1]), C
        if C != 3:
            continue
        # a lookup word the table does not hold: the sum no longer closes, the transition fails on the last row
        bad = [list(col) for col in lookups]
        bad[0][N - 1] = (max(table) + 1) % p if (max(table) + 1) % p not in table else (min(table) - 1) % p
        bvals, bmult, bS, blast, missing = argument(E, bad, table, alpha)
        assert missing == 1 and blast != E.zero
        hi = coefficients(bvals, bmult, bS, C)
        assert any(hi[0]) or any(hi[1])
        # one multiplicity changed, S as the prover would recompute it
        wrong = [list(col) for col in mult]
        j = next(k for k, v in enumerate(wrong[-1]) if v)
        wrong[-1][j] = (wrong[-1][j] + 1) % p
        wS, wlast, _ = AR.logup_sum(E, vals, wrong, alpha)
        assert wlast != E.zero
        hi = coefficients(vals, wrong, wS, C)
        assert any(hi[0]) or any(hi[1])
        # ... and with the honest S: the transition fails at row j
        hi = coefficients(vals, wrong, S, C)
        assert any(hi[0]) or any(hi[1])
        # S shifted by a constant: every transition holds, S = 0 at the first row does not
        shifted = [E.add(s, E.one) for s in S]
        hi = coefficients(vals, mult, shifted, C)
        assert any(hi[0]) or any(hi[1])


@pytest.mark.parametrize("p,g,w", FIELDS)
def test_adding_onto_t_in_is_the_sum(p, g, w):
    E = LR.Ext2(p, w)
    dom = PR.Domain(p, g, 2, 1, g)
    rng = np.random.default_rng(5)
    big = lambda k: [int(v) for v in rng.integers(0, 2**63, size=k)]      # noqa: E731
    vals, mult, S, T_in = [big(dom.M) for _ in range(3)], [big(dom.M) for _ in range(3)], [big(dom.M), big(dom.M)], [big(dom.M), big(dom.M)]
    alpha, lam = big(2), [big(2), big(2)]
    alone = LR.quotient(E, dom, vals, mult, S, alpha, lam)
    onto = LR.quotient(E, dom, vals, mult, S, alpha, lam, T_in)
    assert onto == [E.add(t, E.el((T_in[0][i], T_in[1][i]))) for i, t in enumerate(alone)]
    ones = [[1] * dom.M for _ in range(3)]
    assert LR.quotient(E, dom, vals, None, S, alpha, lam) == LR.quotient(E, dom, vals, ones, S, alpha, lam)


@pytest.mark.parametrize("p,g,w", FIELDS + [(GL, 7, 11), (PC.P_62, PC.GEN[PC.P_62], PC.GEN[PC.P_62])])
def test_the_fast_form_is_the_definition(p, g, w):
    E = LR.Ext2(p, w)
    rng = np.random.default_rng(9)
    big = lambda k: [int(v) * 2 + 1 for v in rng.integers(0, 2**63, size=k)]      # noqa: E731  (words >= p among them)
    for log2_n, log2_b, C in ((1, 0, 1), (2, 1, 2), (3, 2, 5), (2, 3, 16)):
        dom = PR.Domain(p, g, log2_n, log2_b, g)
        vals, mult = [big(dom.M) for _ in range(C)], [big(dom.M) for _ in range(C)]
        S, T_in, alpha, lam = [big(dom.M), big(dom.M)], [big(dom.M), big(dom.M)], big(2), [big(2), big(2)]
        for m, t in ((mult, T_in), (None, None), (mult, None), (None, T_in)):
            assert LR.quotient_fast(E, dom, vals, m, S, alpha, lam, t) == LR.quotient(E, dom, vals, m, S, alpha, lam, t)
