"""The STARK instances the stark tests share: a program of tests/air_programs.py with its round shapes, and a valid trace with its
public inputs.  `rounds` is what stark_ref.prove takes: a matrix per round, or a function of the challenge pairs drawn so far.
A test helper, not product code."""
from collections import namedtuple

import accum_ref as AC
import air_programs as AP
import lookup_ref as LR

# columns[r] rows in round r, the last 2 n_ext[r] of them the planes of extension columns; n_chal = n_pub + sum(n_draw)
Shape = namedtuple("Shape", "prog columns n_ext n_pub n_draw n_chal")
Instance = namedtuple("Instance", "shape pub rounds")


def fibonacci_trace(p, N, a0, b0):
    """air_programs.fibonacci_trace in linear time, for the traces of 2^20 rows that tools/stark_time.py proves"""
    a, b = [a0 % p], [b0 % p]
    for _ in range(N - 1):
        a.append(b[-1])
        b.append((a[-2] + b[-1]) % p)
    return [a, b, [u * v % p for u, v in zip(a, b)]]


def fibonacci(p, N):
    """one round of three base columns; the public inputs are the first a and the last b.  T has degree N - 2: every piece but
    q_0 is zero, so the quotient round commits zero columns"""
    trace = fibonacci_trace(p, N, 2, 3)
    return Instance(Shape(AP.fibonacci(), (3,), (0,), 2, (0,), 2), [(trace[0][0], 0), (trace[1][-1], 0)], [trace])


def sbox_trace(p, N, state=(1, 2, 3), round_constants=(5, 6, 7)):
    rows = [[int(v) % p for v in state]]
    for _ in range(N - 1):
        s7 = [pow((v + rc) % p, 7, p) for v, rc in zip(rows[-1], round_constants)]
        rows.append([sum(m * s for m, s in zip(AP.MDS3[r], s7)) % p for r in range(3)])
    return [[row[c] for row in rows] for c in range(3)]


def sbox_row(p, N):
    """one round of three base columns with degree-7 transitions: T has degree about 6 N, so B = 8 holds it in six non-zero pieces
    and B = 4 does not"""
    trace = sbox_trace(p, N)
    return Instance(Shape(AP.sbox_row(), (3,), (0,), 2, (0,), 2), [(trace[0][0], 0), (trace[0][-1], 0)], [trace])


def lookup_columns(p, N, seed=5):
    """lookup values f (N words of the table, with repeats) and a table t of N distinct words"""
    table = [(seed + 3 * j * j + j) % p for j in range(N)]
    assert len(set(table)) == N
    return [table[(7 * i * i + seed) % (N // 2)] for i in range(N)], table


def logup(p, N, E):
    """two rounds: round 0 = f, t, the ones, the negated multiplicities of t (what ronk_lookup_mult_dev writes with negate = 1);
    alpha is drawn after it; round 1 = the two planes of S from the running sum.  The program is air_programs.logup(2, True)"""
    f, table = lookup_columns(p, N)
    mult, missing, _ = LR.multiplicities(p, table, [f], negate=True)
    assert missing == 0
    round0 = [f, table, [1] * N, mult]

    def round1(chal):
        S, last, status = AC.logup_sum(E, round0[:2], round0[2:], chal[0])
        assert status == 0 and last == (0, 0)
        return [[s[0] for s in S], [s[1] for s in S]]

    return Instance(Shape(AP.logup(2, True), (4, 2), (0, 1), 0, (1, 0), 1), [], [round0, round1])
