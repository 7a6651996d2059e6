"""Self-checks of the restatement tests/accum_ref.py, and the F_17 permutation fixture tests/golden/plonk_f17_permutation.json (the
reference's own S_sigma vectors and witness, src/compiler/program.rs:359-378 and :448).  No library, no device."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR

HERE = os.path.dirname(os.path.abspath(__file__))
GL = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def f17():
    with open(os.path.join(HERE, "golden", "plonk_f17_permutation.json")) as f:
        return json.load(f)


def test_scans_by_definition():
    p = 101
    a = [3, 0, 100, 205, 7, 1, 99]
    for op, fold in (("prod", lambda x, y: x * y % p), ("sum", lambda x, y: (x + y) % p)):
        incl, total = AR.base_scan(p, a, op, 0)
        excl, total2 = AR.base_scan(p, a, op, 1)
        e = 1 if op == "prod" else 0
        for i in range(len(a)):
            want = e
            for v in a[:i + 1]:
                want = fold(want, v % p)
            assert incl[i] == want
            assert excl[i] == (e if i == 0 else incl[i - 1])
        assert total == total2 == incl[-1]
    E = AR.Ext2(p, 99)
    els = [(3, 4), (0, 1), (100, 100), (7, 0)]
    incl, total = AR.ext_scan(E, els, "prod", 0)
    assert incl[1] == E.mul(els[0], els[1]) and total == E.mul(E.mul(incl[1], els[2]), els[3])
    excl, _ = AR.ext_scan(E, els, "sum", 1)
    assert excl == [(0, 0), (3, 4), (3, 5), (2, 4)]


def test_fixture_is_the_reference_program(f17):
    p, n, omega = f17["p"], f17["n"], f17["omega"]
    assert (p, n, f17["w"]) == (17, 4, 3) and omega == pow(3, (p - 1) // n, p) and pow(omega, n, p) == 1 and pow(omega, n // 2, p) != 1
    ids = [[(c + 1) * pow(omega, i, p) % p for i in range(n)] for c in range(3)]
    assert ids == f17["ids"]
    flat_ids = [v for col in ids for v in col]
    flat_sigma = [v for col in f17["sigma"] for v in col]
    assert len(set(flat_ids)) == 12 and sorted(flat_sigma) == sorted(flat_ids), "sigma permutes the labels"
    # the witness a = 2, d = 9, b = 9, c = -36 over the gates  a public | d === 9 | b <== a * a + 5 | c <== -2 * b - a * b
    a, d, b, c = 2, 9, 9, -36 % p
    assert f17["wires"] == [[a, 0, a, a], [0, 0, a, b], [0, d, b, c]]
    assert b == (a * a + 5) % p and c == (-2 * b - a * b) % p
    # a copy constraint joins equal values: the wire value is constant along sigma
    flat_w = [v for col in f17["wires"] for v in col]
    cell = {lab: k for k, lab in enumerate(flat_ids)}
    for k, lab in enumerate(flat_sigma):
        assert flat_w[k] == flat_w[cell[lab]]


def test_fixture_product_closes(f17):
    E = AR.Ext2(f17["p"], f17["w"])
    for ch in f17["closing_challenges"]:
        Z, last, status = AR.perm_product(E, f17["wires"], f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])
        assert status == 0 and Z[0] == E.one and last == E.one, ch
        assert len(set(Z)) > 1, "a product that never moves checks nothing"
    # one altered wire value no longer closes
    wires = [list(col) for col in f17["wires"]]
    wires[1][3] = (wires[1][3] + 1) % f17["p"]        # b as the right input of the last gate
    ch = f17["closing_challenges"][0]
    _, last, status = AR.perm_product(E, wires, f17["ids"], f17["sigma"], ch["beta"], ch["gamma"])
    assert status == 0 and last != E.one


def test_fixture_closure_count(f17):
    """every challenge pair with beta1, gamma1 in a quarter of the range: the product closes unless a factor is zero"""
    E = AR.Ext2(f17["p"], f17["w"])
    closed = degenerate = 0
    for b0 in range(17):
        for b1 in range(0, 17, 4):
            for g0 in range(17):
                for g1 in range(0, 17, 4):
                    Z, last, status = AR.perm_product(E, f17["wires"], f17["ids"], f17["sigma"], (b0, b1), (g0, g1))
                    num0 = any(AR.perm_factors(E, f17["wires"], f17["ids"], (b0, b1), (g0, g1), i) == E.zero for i in range(4))
                    if status or num0:
                        degenerate += 1
                    else:
                        assert last == E.one, (b0, b1, g0, g1)
                        closed += 1
    assert closed > 0 and degenerate > 0 and closed + degenerate == 17 * 5 * 17 * 5


def test_zero_denominator_convention():
    E = AR.Ext2(17, 3)
    # a + beta * sigma + gamma = 0: a = 5, beta = (2, 0), sigma = 3, gamma = (6, 0)
    Z, last, status = AR.perm_product(E, [[1, 5, 2]], [[1, 2, 3]], [[2, 3, 1]], (2, 0), (6, 0))
    assert status == 1 and Z[0] == E.one and Z[1] != E.zero and Z[2] == E.zero and last == E.zero
    S, last, status = AR.logup_sum(E, [[1, 4], [2, 2]], None, (13, 0))          # alpha + 4 = 0: that term alone is dropped
    assert status == 1 and S[1] == E.add(E.inv((14, 0)), E.inv((15, 0))) and last == E.add(S[1], E.inv((15, 0)))


def test_logup_multiset_identity():
    p = GL
    E = AR.Ext2(p, 7)
    rng = np.random.default_rng(5)
    table = [int(v) for v in rng.integers(0, 2**63, size=16, dtype=np.uint64)]
    witness = [table[int(k)] for k in rng.integers(0, 16, size=40)]
    counts = [witness.count(t) for t in table]
    alpha = (int(rng.integers(0, 2**63)), int(rng.integers(0, 2**63)))
    _, s_w, st_w = AR.logup_sum(E, [witness], None, alpha)
    _, s_t, st_t = AR.logup_sum(E, [table], [counts], alpha)
    assert st_w == st_t == 0 and E.sub(s_w, s_t) == E.zero
    # "-k" is the word p - k: witness and table in one call
    _, s, _ = AR.logup_sum(E, [witness[:16], table], [[1] * 16, [p - witness[:16].count(t) for t in table]], alpha)
    assert s == E.zero
    witness[7] = table[0] + 1                                                    # one foreign value breaks it
    _, s_w, _ = AR.logup_sum(E, [witness], None, alpha)
    assert E.sub(s_w, s_t) != E.zero


def test_cycle_instance_closes():
    rng = np.random.default_rng(11)
    wires, ids, sigma = AR.cycle_instance(rng, 64, 3, 40)
    assert sorted(sigma.ravel().tolist()) == ids.ravel().tolist()
    flat_w, flat_s = wires.ravel(), sigma.ravel()
    assert all(flat_w[k] == flat_w[int(flat_s[k]) - 1] for k in range(flat_w.size)), "the value is constant along sigma"
    assert (flat_s != ids.ravel()).any()
    E = AR.Ext2(GL, 7)
    Z, last, status = AR.perm_product(E, wires.tolist(), ids.tolist(), sigma.tolist(), (12345, 678), (9, 10))
    assert status == 0 and last == E.one and Z[1] != E.one


@pytest.mark.parametrize("p,w", [(17, 3), (101, 99), (GL, 7)])
def test_fast_forms_equal_the_definition(p, w):
    """small fields meet zero denominators by chance; over Goldilocks one is forced"""
    E = AR.Ext2(p, w)
    rng = np.random.default_rng(p % 1000)
    for trial in range(12):
        W, n = int(rng.integers(1, 5)), int(rng.integers(1, 40))
        cols = lambda: [[int(v) for v in rng.integers(0, 2**63, size=n)] for _ in range(W)]   # noqa: E731
        wires, ids, sigma, mult = cols(), cols(), cols(), cols()
        r = lambda: int(rng.integers(0, 2**63)) % p                                            # noqa: E731
        beta, gamma, alpha = (r(), r()), (r(), r()), (r(), r() if trial % 2 else 0)
        if trial % 3 == 0:
            wires[0][n // 2] = -alpha[0] % p                                    # alpha + v = 0 when alpha1 = 0
            beta, gamma = (beta[0], 0), (gamma[0], 0)
            sigma[0][n // 2] = 1
            wires[0][n // 2] = -(beta[0] + gamma[0]) % p if trial % 2 else wires[0][n // 2]
        assert AR.perm_product_fast(E, wires, ids, sigma, beta, gamma) == AR.perm_product(E, wires, ids, sigma, beta, gamma)
        for m in (None, mult):
            assert AR.logup_sum_fast(E, wires, m, alpha) == AR.logup_sum(E, wires, m, alpha)
    statuses = {AR.perm_product(E, [[-(3 + 5) % p]], [[2]], [[1]], (3, 0), (5, 0))[2], AR.logup_sum(E, [[p - 4]], None, (4, 0))[2]}
    assert statuses == {1}
