"""tests/air_ref.py (the constraint programs on Python integers) against what it must be, over Goldilocks with W = 7 and MONT_P:
the PLONK gate with both permutation constraints and the logUp pair, written as programs, give the words of tests/plonk_ref.py and
tests/lookup_ref.py; a Fibonacci AIR with all four kinds has a quotient of degree N - 2 exactly when its trace and boundary values
are right; and the evaluation at one point from opened values is T's polynomial at that point."""
import numpy as np
import pytest

import air_programs as AP
import air_ref as AR
import lookup_ref as LR
import plonk_ref as PR
import prime_classes as PC

GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
FIELDS = [(GL, 7, 7), (MONT, 10, 10)]


def words(rng, n, p):
    v = [int(a) * 2 + int(b) for a, b in zip(rng.integers(0, 2**63, size=n), rng.integers(0, 2, size=n))]
    for k in range(0, n, 7):
        v[k] = (p - 1, 0, p + 3 if p + 3 < 2**64 else p)[k % 3]
    return v


@pytest.mark.parametrize("p,g,w", FIELDS)
def test_the_plonk_quotient_as_a_program(p, g, w):
    rng = np.random.default_rng(1)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, 3, 2, g)
    M = dom.M
    wires, sel, sigma = ([words(rng, M, p) for _ in range(k)] for k in (3, 5, 3))
    pi, Z = words(rng, M, p), [words(rng, M, p) for _ in range(2)]
    alpha, beta, gamma = (words(rng, 2, p) for _ in range(3))
    want = PR.quotient(E, dom, PR.Columns(wires, sel, sigma, pi, Z), alpha, beta, gamma)
    a = E.el(alpha)
    got = AR.quotient(E, dom, AP.plonk(), wires + sel + sigma + [pi], [Z], [beta, gamma], [E.one, a, E.mul(a, a)])
    assert got == want


@pytest.mark.parametrize("C,with_mult", [(1, False), (2, True), (5, True), (5, False)])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_the_logup_pair_as_a_program(p, g, w, C, with_mult):
    rng = np.random.default_rng(2 + C)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, 3, 2, g)
    M = dom.M
    vals, mult = [words(rng, M, p) for _ in range(C)], [words(rng, M, p) for _ in range(C)]
    S, T_in = [words(rng, M, p) for _ in range(2)], [words(rng, M, p) for _ in range(2)]
    alpha, lam = words(rng, 2, p), [words(rng, 2, p) for _ in range(2)]
    want = LR.quotient(E, dom, vals, mult if with_mult else None, S, alpha, lam, T_in)
    got = AR.quotient(E, dom, AP.logup(C, with_mult), vals + (mult if with_mult else []), [S], [alpha], lam, T_in)
    assert got == want


def fibonacci_T(E, dom, trace, first, last, lam):
    base = [PR.extend(dom, col) for col in trace]
    return AR.quotient(E, dom, AP.fibonacci(), base, [], [first, last], lam)


def high(dom, T, lo):
    return [PR.coset_coefficients(dom, [t[plane] for t in T])[lo:] for plane in (0, 1)]


@pytest.mark.parametrize("log2_n", [3, 4, 5])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_fibonacci_quotient_is_a_polynomial_of_degree_n_minus_two(p, g, w, log2_n):
    rng = np.random.default_rng(log2_n)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, log2_n, 2, g)
    N = dom.N
    trace = AP.fibonacci_trace(p, N)
    lam = [words(rng, 2, p) for _ in range(5)]
    first, last = (trace[0][0], 0), (trace[1][-1], 0)
    T = fibonacci_T(E, dom, trace, first, last, lam)
    for plane in high(dom, T, N - 1):
        assert not any(plane)
    low = [PR.coset_coefficients(dom, [t[plane] for t in T])[:N - 1] for plane in (0, 1)]
    assert all(low[0]) or all(low[1])
    # one changed trace word, a wrong first value, a wrong last value: T is no such polynomial
    bad = [list(col) for col in trace]
    bad[1][N // 2] = (bad[1][N // 2] + 1) % p
    for tr, f, l in ((bad, first, last), (trace, (2, 0), last), (trace, first, ((last[0] + 1) % p, 0))):
        hi = high(dom, fibonacci_T(E, dom, tr, f, l, lam), N - 1)
        assert any(hi[0]) or any(hi[1])


@pytest.mark.parametrize("p,g,w", FIELDS)
def test_eval_point_is_the_quotient_polynomial_at_that_point(p, g, w):
    rng = np.random.default_rng(9)
    E, dom = PR.Ext2(p, w), PR.Domain(p, g, 4, 2, g)
    trace = AP.fibonacci_trace(p, dom.N, 3, 5)
    lam = [words(rng, 2, p) for _ in range(5)]
    chal = [(trace[0][0], 0), (trace[1][-1], 0)]
    prog = AP.fibonacci()
    T = fibonacci_T(E, dom, trace, chal[0], chal[1], lam)
    coef = [PR.coset_coefficients(dom, [t[plane] for t in T]) for plane in (0, 1)]
    z = E.el(words(rng, 2, p))
    Tz = E.add(PR.evaluate_ext(E, coef[0], z), E.mul(PR.evaluate_ext(E, coef[1], z), (0, 1)))
    cols = [PR.interpolate(p, dom.wN, col) for col in trace]
    cells = AR.cells(prog.ops)
    assert sorted(AR.decode(o) for o in cells) == [(AR.BASE, 0, 0), (AR.BASE, 0, 1), (AR.BASE, 1, 0), (AR.BASE, 1, 1), (AR.BASE, 2, 0)]
    opened = [PR.evaluate_ext(E, cols[AR.decode(o)[1]], E.mul_base(z, pow(dom.wN, AR.decode(o)[2], p))) for o in cells]
    assert AR.eval_point(E, dom, prog, z, opened, chal, lam) == Tz
    # a point of H has no quotient
    assert AR.eval_point(E, dom, prog, (dom.wN, 0), opened, chal, lam) is None
