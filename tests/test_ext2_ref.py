"""Pins tests/ext2_ref.py: the reference's own vectors over F_101[t] / (t^2 + 2) (tests/golden/gf101_2_vectors.json, the cases of
gf_101_2.rs recorded as data) and its algebraic identities (add_sub_neg_mul, pow, inv_div, add_sub_mul_subfield, generator_order)
with seeded values, over F_101 and the two 64-bit primes."""
import json
import os
import random

import pytest

import ext2_ref as ER

HERE = os.path.dirname(os.path.abspath(__file__))
GL, MONT = 0xFFFFFFFF00000001, 0xFFFFFFFC00000001
FIELDS = [(101, 99), (GL, 7), (MONT, 10)]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "gf101_2_vectors.json")) as f:
        return json.load(f)


def test_golden_vectors(golden):
    E = ER.Ext2(golden["p"], golden["w"])
    for op in ("add", "sub", "mul"):
        for c in golden[op]:
            assert getattr(E, op)(tuple(c["a"]), tuple(c["b"])) == tuple(c["out"]), (op, c)
    for c in golden["neg"]:
        assert E.neg(tuple(c["a"])) == tuple(c["out"])


def test_generator_order(golden):
    E = ER.Ext2(golden["p"], golden["w"])
    g = tuple(golden["primitive_element"])
    assert golden["primitive_element_order"] == 101 ** 2 - 1 == E.order(g)
    # the reference's loop: multiplying 101^2 - 1 times comes back to the generator, and not before
    val, seen = g, 0
    for k in range(1, 101 ** 2):
        val = E.mul(val, g)
        if val == g:
            seen = k
            break
    assert seen == 101 ** 2 - 1


def test_refuses_a_residue():
    for p, w in ((101, 4), (101, 0), (101, 101), (GL, 4)):
        with pytest.raises(AssertionError):
            ER.Ext2(p, w)


def rand_el(rng, p):
    return (rng.randrange(p), rng.randrange(p))


@pytest.mark.parametrize("p,w", FIELDS)
def test_add_sub_neg_mul(p, w):
    E, rng = ER.Ext2(p, w), random.Random(p % 1000)
    for _ in range(20):
        x, y, z = rand_el(rng, p), rand_el(rng, p), rand_el(rng, p)
        assert E.add(x, E.neg(x)) == E.zero and E.neg(x) == E.sub(E.zero, x)
        assert E.mul(x, E.neg(x)) == E.neg(E.mul(x, x))
        assert E.add(x, y) == E.add(y, x) and E.mul(x, y) == E.mul(y, x)
        assert E.mul(x, E.mul(y, z)) == E.mul(E.mul(x, y), z)
        assert E.sub(x, E.add(y, z)) == E.sub(E.sub(x, y), z)
        assert E.sub(E.add(x, y), z) == E.add(x, E.sub(y, z))
        assert E.mul(x, E.add(y, z)) == E.add(E.mul(x, y), E.mul(x, z))


@pytest.mark.parametrize("p,w", FIELDS)
def test_pow(p, w):
    E, rng = ER.Ext2(p, w), random.Random(p % 1000 + 1)
    x = rand_el(rng, p)
    assert E.pow(x, 0) == E.one and E.pow(x, 1) == x
    assert E.pow(x, 4) == E.mul(E.mul(x, x), E.mul(x, x))
    assert E.pow(x, p) == (x[0], -x[1] % p)            # Frobenius
    assert E.pow(x, p * p - 1) == E.one


@pytest.mark.parametrize("p,w", FIELDS)
def test_inv_div(p, w):
    E, rng = ER.Ext2(p, w), random.Random(p % 1000 + 2)
    assert E.inv(E.zero) is None
    for _ in range(10):
        x, y, z = (rand_el(rng, p) for _ in range(3))
        if E.zero in (x, y, z):
            continue
        assert E.mul(x, E.inv(x)) == E.one
        assert E.mul(E.inv(x), E.inv(y)) == E.inv(E.mul(x, y))
        assert E.mul(E.div(x, y), y) == x
        assert E.div(x, E.mul(y, z)) == E.div(E.div(x, y), z)
        assert E.div(E.mul(x, y), z) == E.mul(x, E.div(y, z))


@pytest.mark.parametrize("p,w", FIELDS)
def test_add_sub_mul_subfield(p, w):
    E, rng = ER.Ext2(p, w), random.Random(p % 1000 + 3)
    x, y = rand_el(rng, p), rand_el(rng, p)
    assert E.add(E.add(x, y), E.sub(x, y)) == E.mul_base(x, 2)
    assert E.mul(E.mul(x, y), E.mul(x, E.inv(y))) == E.mul(x, x)
    s = rng.randrange(p)
    assert E.mul_base(x, s) == E.mul(x, E.embed(s))
    assert E.norm(x) == E.mul(x, (x[0], -x[1] % p))[0]
