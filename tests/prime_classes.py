"""The generic test primes of the GPU and emulator suites, classed by which outcome of a modular addition they can reach.

mont64::add (csrc/mont64.h) and PosMont::acc_mad (csrc/poseidon_kernels.h) form s = a + b on 64 bits with carry c2, d = s - p with
borrow b2, and select d when `c2 | !b2`.  For canonical a, b < p the select has three outcomes:

    s < p                 keep s            (c2 = 0, b2 = 1)
    p <= s < 2^64         take d by !b2     (c2 = 0, b2 = 0)   "nowrap_ge_p"
    s >= 2^64             take d by c2      (c2 = 1)           "wrap"

A prime just below 2^64 all but never reaches the second, a prime below 2^63 never reaches the third.  Only a prime around
3/4 * 2^64 reaches all three often, so that a mask with one term wrong gives wrong words in every tile.

The shares below are exact: the number of ordered pairs (a, b) of residues with each outcome, over p^2 (fractions.Fraction, no
sampling).  To first order in (2^64 - p) / p they are the closed forms  nowrap_ge_p ~ (2^64 - p) / p  and
wrap ~ (2 p - 2^64)^2 / (2 p^2)  for p > 2^63; the first is an upper bound, which tests/test_prime_classes.py asserts too.

A test helper, not product code."""
from collections import namedtuple
from fractions import Fraction

T = 1 << 64

P_MID = 0xC000002400000001      # 2^34 * 0x30000009 + 1, about 3/4 * 2^64: every outcome is common
P_62 = 29 * 2**57 + 1           # below 2^62: no sum carries out of bit 63
MONT_P = 0xFFFFFFFC00000001     # 2^34 * (2^30 - 1) + 1, just below 2^64: p <= s < 2^64 has probability about 10^-9
P_32 = 3 * 2**30 + 1            # a 32-bit prime: high limbs mostly zero

# g: a primitive element (so a quadratic non-residue: it serves as W of the quadratic extension)
# two_adicity: the largest k with 2^k | p - 1
# both / nowrap_only / wrap_only: the class asserted by assert_classes()
Prime = namedtuple("Prime", "name p g two_adicity cls")
TABLE = [Prime("P_MID", P_MID, 7, 34, "both"),
         Prime("P_62", P_62, 3, 57, "nowrap_only"),
         Prime("MONT_P", MONT_P, 10, 34, "wrap_only"),
         Prime("P_32", P_32, 5, 30, "nowrap_only")]
BY_P = {e.p: e for e in TABLE}
GEN = {e.p: e.g for e in TABLE}

# what the families that used to see MONT_P alone now run over as well
CLASS_FIELDS = [P_MID, P_62]
CLASS_PRIMES = [(P_MID, GEN[P_MID]), (P_62, GEN[P_62])]
GENERIC_PRIMES = [(e.p, e.g) for e in TABLE]


def add_shares(p):
    """(keep, nowrap_ge_p, wrap): the exact share of ordered pairs (a, b) in [0, p)^2 whose sum s = a + b has s < p,
    p <= s < 2^64, s >= 2^64.  The sum k < p has k + 1 pairs, the sum k >= p has 2 p - 1 - k."""
    keep = p * (p + 1) // 2
    m = max(0, 2 * p - 1 - T)               # sums T .. 2p - 2 have m, m - 1, .. 1 pairs
    wrap = m * (m + 1) // 2
    mid = p * p - keep - wrap
    return Fraction(keep, p * p), Fraction(mid, p * p), Fraction(wrap, p * p)


def assert_classes():
    """the classes of TABLE from the exact shares"""
    for e in TABLE:
        keep, mid, wrap = add_shares(e.p)
        assert keep + mid + wrap == 1
        if e.cls == "both":
            assert mid > Fraction(1, 10) and wrap > Fraction(1, 10), e.name
        elif e.cls == "nowrap_only":
            assert wrap == 0 and mid > Fraction(4, 10), e.name
        else:
            assert e.cls == "wrap_only" and mid < Fraction(1, 10**6) and wrap > Fraction(4, 10), e.name


assert_classes()


# ------------------------------------------------------------------------------------------------ number theory on Python integers
def is_prime(n):
    """deterministic Miller-Rabin for n < 2^64 (the first twelve primes as bases)"""
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in bases:
        if n % b == 0:
            return n == b
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for b in bases:
        x = pow(b, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_factors(n):
    """the prime factors of n by trial division up to 2^16; what is left must be 1 or a prime"""
    out = set()
    f = 2
    while f < (1 << 16) and f * f <= n:
        while n % f == 0:
            out.add(f)
            n //= f
        f += 1
    if n > 1:
        assert is_prime(n), "cofactor %d is neither 1 nor a prime" % n
        out.add(n)
    return sorted(out)


def is_primitive(p, g):
    return all(pow(g, (p - 1) // q, p) != 1 for q in prime_factors(p - 1))


# ------------------------------------------------------------------------------------------------ boundary operands
def add_targets(p):
    """the sums around each edge of the select that canonical operands can reach: p (the first sum reduced), 2^64 (the first
    sum that carries) and 2 p - 2 (the largest)"""
    return [t for t in (p - 1, p, p + 1, T - 1, T, T + 1, 2 * p - 2) if 0 <= t <= 2 * p - 2]


def add_pairs(p):
    """[(a, b)] of canonical residues: every target of add_targets(p) split at its smallest and largest first operand, in the
    middle, and at operands with a zero / an all-ones low or high limb"""
    out = []
    for t in add_targets(p):
        lo, hi = max(0, t - (p - 1)), min(p - 1, t)
        cand = [lo, hi, t // 2, (t + 1) // 2, lo + 1, hi - 1, 0xFFFFFFFF, 1 << 32, (p >> 32) << 32, t & 0xFFFFFFFF00000000]
        for a in cand:
            if lo <= a <= hi:
                out.append((a, t - a))
                out.append((t - a, a))
    return out


def sub_pairs(p):
    """[(a, b)] with a - b in {-1, 0, 1, -(p - 1)}, and the borrow crossing the limb boundary"""
    xs = [0, 1, p - 2, (p - 1) // 2, 0xFFFFFFFF, 1 << 32, (1 << 63) % p, (p >> 32) << 32]
    out = [(0, p - 1)]
    for x in xs:
        x %= p - 1                             # x + 1 stays canonical
        out += [(x, x + 1), (x, x), (x + 1, x + 1), (x + 1, x)]
    return out


def mul_operands(p):
    R = T % p
    return [v % p for v in (0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 63) % p, R, R * R % p)]


def mul_pairs(p):
    ops = mul_operands(p)
    return [(a, b) for a in ops for b in ops]
