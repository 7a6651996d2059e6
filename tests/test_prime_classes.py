"""The table of test primes (tests/prime_classes.py) re-derived on Python integers: primality, the generators, the 2-adicity, the
class of each prime from the exact shares of the three outcomes of a modular addition, and that the directed operand lists reach
every outcome and every edge they name.  Nothing here is sampled."""
from fractions import Fraction

import pytest

import prime_classes as PC

T = 1 << 64


@pytest.mark.parametrize("e", PC.TABLE, ids=lambda e: e.name)
def test_prime_generator_and_two_adicity(e):
    p, g = e.p, e.g
    assert p % 2 == 1 and p < T and PC.is_prime(p)
    assert (p - 1) % (1 << e.two_adicity) == 0 and (p - 1) % (2 << e.two_adicity) != 0
    assert PC.is_primitive(p, g)
    assert pow(g, (p - 1) // 2, p) == p - 1                     # a non-residue: x^2 - g is irreducible
    for k in (1, 12, 22, e.two_adicity):                        # omega_(2^k) has its exact order
        w = pow(g, (p - 1) >> k, p)
        assert pow(w, 1 << k, p) == 1 and pow(w, 1 << (k - 1), p) == p - 1
    assert not PC.is_primitive(p, g * g % p)                    # the check itself tells a square from a generator


def test_is_prime_and_factors_on_known_values():
    assert [n for n in range(60) if PC.is_prime(n)] == [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59]
    assert PC.is_prime(0xFFFFFFFF00000001) and not PC.is_prime(0xFFFFFFFF00000001 - 2) and not PC.is_prime(3215031751)
    assert PC.prime_factors(PC.MONT_P - 1) == [2, 3, 7, 11, 31, 151, 331]
    assert PC.prime_factors(PC.P_62 - 1) == [2, 29]
    assert PC.P_MID - 1 == (1 << 34) * 0x30000009


def test_p_mid_serves_every_family():
    p = PC.P_MID
    assert (p - 1) % 7 != 0                                     # x -> x^7 is a permutation
    assert PC.GEN[p] == 7 and 3 * T // 4 < p < 3 * T // 4 + (1 << 40)
    assert PC.BY_P[PC.P_62].g == 3


def test_classes_from_exact_shares():
    PC.assert_classes()
    keep, mid, wrap = PC.add_shares(PC.P_MID)
    assert mid > Fraction(1, 10) and wrap > Fraction(1, 10)
    assert abs(float(keep) - 0.500) < 1e-3 and abs(float(mid) - 0.278) < 1e-3 and abs(float(wrap) - 0.222) < 1e-3
    assert PC.add_shares(PC.P_62)[2] == 0 and PC.add_shares(PC.P_32)[2] == 0
    # why MONT_P is not enough alone
    _, mid, wrap = PC.add_shares(PC.MONT_P)
    assert 0 < mid < Fraction(1, 10**6) and wrap > Fraction(49, 100)
    for e in PC.TABLE:                                          # the closed forms: an upper bound and a first-order value
        p = e.p
        _, mid, wrap = PC.add_shares(p)
        if p > T // 2:
            assert mid <= Fraction(T - p, p)
            assert abs(wrap - Fraction((2 * p - T) ** 2, 2 * p * p)) < Fraction(1, p)
        else:
            assert wrap == 0 and abs(mid - Fraction(1, 2)) < Fraction(1, p)


def test_shares_by_enumeration_on_a_small_modulus():
    """add_shares' counting against every pair, with 2^64 scaled down to 2^6 (the formulas only see p and T)"""
    old = PC.T
    try:
        PC.T = 64
        for p in (29, 37, 47, 49, 61, 63):
            n = [0, 0, 0]
            for a in range(p):
                for b in range(p):
                    n[0 if a + b < p else 1 if a + b < 64 else 2] += 1
            assert PC.add_shares(p) == tuple(Fraction(v, p * p) for v in n), p
    finally:
        PC.T = old


@pytest.mark.parametrize("e", PC.TABLE, ids=lambda e: e.name)
def test_directed_operands_reach_what_they_name(e):
    p = e.p
    adds = PC.add_pairs(p)
    assert all(0 <= a < p and 0 <= b < p for a, b in adds)
    sums = {a + b for a, b in adds}
    want = {p - 1, p, p + 1, 2 * p - 2} | ({T - 1, T, T + 1} if p > T // 2 else set())
    assert sums == want == set(PC.add_targets(p))
    outcomes = {0 if s < p else 1 if s < T else 2 for s in sums}
    assert outcomes == ({0, 1, 2} if p > T // 2 else {0, 1})
    subs = PC.sub_pairs(p)
    assert all(0 <= a < p and 0 <= b < p for a, b in subs)
    assert {a - b for a, b in subs} == {-1, 0, 1, -(p - 1)}
    ops = PC.mul_operands(p)
    assert all(0 <= v < p for v in ops) and len(PC.mul_pairs(p)) == len(ops) ** 2 == 144
    assert {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, T % p, T * T % p} <= set(ops)
