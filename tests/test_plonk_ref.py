"""The restatement tests/plonk_ref.py against what a quotient must be: for a valid circuit T is a polynomial (its coefficients
vanish from 3N - 3 upward: after the division by x^N - 1 the degree bounds are 3N - 4 for the first permutation constraint, N - 2
for the second and 2N - 3 for the gate), for a tampered one it is not, and the verifier's identity holds at a random extension
point.  Goldilocks with w = 7 and MONT_P, N = 4, 8, 16."""
import numpy as np
import pytest

import plonk_ref as PR
import prime_classes as PC

GL = 0xFFFFFFFF00000001
FIELDS = [(GL, 7, 7), (PC.MONT_P, PC.GEN[PC.MONT_P], PC.GEN[PC.MONT_P])]      # p, g, w
SHIFT = 7


def challenge(rng, p):
    return (int(rng.integers(0, 2**62)) % p, int(rng.integers(0, 2**62)) % p)


def instance(p, g, w, log2_n, log2_b, seed=0):
    rng = np.random.default_rng(1000 * log2_n + log2_b + seed)
    E = PR.Ext2(p, w)
    dom = PR.Domain(p, g, log2_n, log2_b, SHIFT)
    c = PR.circuit(rng, p, log2_n)
    wires = PR.witness(c)
    sigma = PR.sigma_of(c, PR.labels(dom))
    ch = [challenge(rng, p) for _ in range(3)]
    return E, dom, c, wires, sigma, ch


def high(E, dom, c, wires, sigma, ch, Z_edit=None):
    alpha, beta, gamma = ch
    t, last = PR.trace_columns(E, dom, c, wires, sigma, beta, gamma)
    if Z_edit:
        Z_edit(t.Z)
    T = PR.quotient(E, dom, PR.on_coset(dom, t), alpha, beta, gamma)
    return PR.high_coefficients(E, dom, T), last


@pytest.mark.parametrize("log2_b", [2, 3])
@pytest.mark.parametrize("log2_n", [2, 3, 4])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_valid_circuit_gives_a_polynomial(p, g, w, log2_n, log2_b):
    E, dom, c, wires, sigma, ch = instance(p, g, w, log2_n, log2_b)
    # the witness satisfies every gate and the product closes
    for i in range(c.N):
        a, b, o = (col[i] for col in wires)
        ql, qr, qm, qo, qc = (col[i] for col in c.sel)
        assert (a * ql + b * qr + a * b * qm + o * qo + qc + c.pi[i]) % p == 0
    hi, last = high(E, dom, c, wires, sigma, ch)
    assert last == (1, 0)
    assert len(hi[0]) == dom.M - (3 * dom.N - 3) > 0
    assert not any(hi[0]) and not any(hi[1])


@pytest.mark.parametrize("log2_n", [2, 3, 4])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_tampered_circuit_does_not(p, g, w, log2_n):
    E, dom, c, wires, sigma, ch = instance(p, g, w, log2_n, 2, seed=5)
    N = c.N
    # one tampered cell: the output of the last add / mul gate
    gate_rows = [i for i in range(N) if c.sel[3][i]]
    assert gate_rows
    bad = [col[:] for col in wires]
    bad[2][gate_rows[-1]] = (bad[2][gate_rows[-1]] + 1) % p
    hi, _ = high(E, dom, c, bad, sigma, ch)
    assert any(hi[0]) or any(hi[1])
    # one broken copy constraint: sigma joins two cells that hold different values (the gates still hold)
    cells = [(col, i) for col in range(3) for i in range(N)]
    x, y = next((u, v) for u in cells for v in cells if wires[u[0]][u[1]] != wires[v[0]][v[1]])
    sg = [col[:] for col in sigma]
    sg[x[0]][x[1]], sg[y[0]][y[1]] = sg[y[0]][y[1]], sg[x[0]][x[1]]
    hi, last = high(E, dom, c, wires, sg, ch)
    assert last != (1, 0) and (any(hi[0]) or any(hi[1]))
    # Z[N] != 1 with every gate satisfied: a padding cell (zero selectors) leaves the value of its variable
    pad = N - 1
    assert not any(col[pad] for col in c.sel) and c.pi[pad] == 0
    bad = [col[:] for col in wires]
    bad[1][pad] = (bad[1][pad] + 1) % p
    hi, last = high(E, dom, c, bad, sigma, ch)
    assert last != (1, 0) and (any(hi[0]) or any(hi[1]))
    # and Z itself off by a factor: only Z[0] = 1 fails
    def scale(Z):
        Z[0][:] = [3 * v % p for v in Z[0]]
        Z[1][:] = [3 * v % p for v in Z[1]]
    hi, last = high(E, dom, c, wires, sigma, ch, Z_edit=scale)
    assert last == (1, 0) and (any(hi[0]) or any(hi[1]))


@pytest.mark.parametrize("log2_n", [2, 3, 4])
@pytest.mark.parametrize("p,g,w", FIELDS)
def test_verifier_identity_at_a_random_point(p, g, w, log2_n):
    """G(z) + alpha P1(z) + alpha^2 P2(z) = T(z) (z^N - 1) with every polynomial evaluated from its coefficients"""
    E, dom, c, wires, sigma, ch = instance(p, g, w, log2_n, 2, seed=9)
    alpha, beta, gamma = ch
    N = dom.N
    t, _ = PR.trace_columns(E, dom, c, wires, sigma, beta, gamma)
    T = PR.quotient(E, dom, PR.on_coset(dom, t), alpha, beta, gamma)
    Tc = [PR.coset_coefficients(dom, [v[plane] for v in T]) for plane in (0, 1)]
    rng = np.random.default_rng(77 + log2_n)
    z = challenge(rng, p)
    at = lambda col: PR.evaluate_ext(E, PR.interpolate(p, dom.wN, col), z)                     # noqa: E731
    pair_at = lambda planes, pt: E.add(PR.evaluate_ext(E, planes[0], pt),                      # noqa: E731
                                       E.mul(PR.evaluate_ext(E, planes[1], pt), (0, 1)))
    a, b, o = (at(col) for col in t.wires)
    ql, qr, qm, qo, qc = (at(col) for col in t.sel)
    Zc = [PR.interpolate(p, dom.wN, plane) for plane in t.Z]
    Zz, Zwz = pair_at(Zc, z), pair_at(Zc, E.mul_base(z, dom.wN))
    G = E.add(E.add(E.add(E.mul(a, ql), E.mul(b, qr)), E.add(E.mul(E.mul(a, b), qm), E.mul(o, qo))), E.add(qc, at(t.pi)))
    num, den = Zz, Zwz
    for k, wv, sg in zip(PR.LABELS, (a, b, o), t.sigma):
        num = E.mul(num, E.add(E.add(wv, E.mul(beta, E.mul_base(z, k))), gamma))
        den = E.mul(den, E.add(E.add(wv, E.mul(beta, at(sg))), gamma))
    P1 = E.sub(num, den)
    vanish = E.sub(E.pow(z, N), E.one)
    L1 = E.mul(vanish, E.inv(E.mul_base(E.sub(z, E.one), N)))
    P2 = E.mul(E.sub(Zz, E.one), L1)
    lhs = E.add(E.add(G, E.mul(alpha, P1)), E.mul(E.mul(alpha, alpha), P2))
    assert lhs == E.mul(pair_at(Tc, z), vanish)
