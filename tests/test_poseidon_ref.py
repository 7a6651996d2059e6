"""The Python restatement of Poseidon, its sponge and the Merkle tree (tests/poseidon_ref.py) against the reference's pinned value
and its own structural identities.  No library code runs here: this pins the yardstick the device tests compare with."""
import json
import os

import pytest

import poseidon_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_f101_w16.json")


@pytest.fixture(scope="module")
def f101():
    with open(GOLDEN) as f:
        return json.load(f)


def _params(v, rate):
    return PR.Params(v["p"], v["width"], v["alpha"], v["num_p"], v["num_f"], rate, v["rc"], v["mds"])


def test_reference_known_answer(f101):
    """src/hashes/poseidon/tests/mod.rs:85-91: hash([0; 16]) == 20 over F_101"""
    P = _params(f101, 15)
    assert len(f101["rc"]) == (f101["num_f"] + f101["num_p"]) * f101["width"]
    assert PR.hash_(P, [0] * 16) == f101["hash_zero_state"] == 20
    assert PR.hash_(P, []) == 20                    # padding with ZERO
    with pytest.raises(IndexError):
        PR.hash_(P, [0] * 17)


@pytest.mark.parametrize("rate", [1, 3, 6, 15])
def test_sponge_chunking(f101, rate):
    P = _params(f101, rate)
    data = [(7 * i + 3) % 101 for i in range(3 * rate + 2)]
    for n in (0, 1, rate - 1, rate, rate + 1, 3 * rate + 2):
        x = data[:n]
        one = PR.Sponge(P).absorb(x)
        assert one.permutations == n // rate
        out = one.squeeze(rate + 3)
        # ceil(len / rate) absorbing, one more each time rate outputs were taken and more are wanted
        assert one.permutations == -(-n // rate) + (-(-(rate + 3) // rate) - 1)
        for cut in (0, 1, n // 2, n):
            pieces = PR.Sponge(P).absorb(x[:cut]).absorb(x[cut:])
            assert pieces.squeeze(rate + 3) == out
        assert PR.sponge(P, x, rate) == out[:rate]
        s = PR.Sponge(P).absorb(x)
        assert s.squeeze(2) + s.squeeze(rate + 1) == out      # squeezing in pieces
    z = PR.Sponge(P)
    assert z.squeeze(rate) == [0] * rate and z.permutations == 0   # zero-length input: no permutation, zeros


@pytest.mark.parametrize("p", [PR.GOLDILOCKS, PR.MONT_P, 101])
def test_derived_parameters_are_a_permutation_input(p):
    P = PR.derive_params(p, 5, 7, 3, 5, 2)      # an odd num_f: 2 full rounds, 3 partial, 3 full
    assert all(0 <= c < p for c in P.rc) and all(0 < c < p for row in P.mds for c in row)
    a = PR.permute(P, [1, 2, 3, 4, 5])
    assert a != PR.permute(P, [1, 2, 3, 4, 6]) and all(0 <= v < p for v in a)
    assert PR.permute(P, [p + 1, 2, 3, 4, 5]) == a


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13])
def test_merkle_round_trip(f101, n):
    P = _params(f101, 8)
    leaves = [[(i * 5 + j) % 101 for j in range(3)] for i in range(n)]
    t = PR.MerkleTree(P, leaves, 2)
    sizes = [len(l) for l in t.levels]
    assert sizes[0] == n and sizes[-1] == 1 and all(b == (a + 1) // 2 for a, b in zip(sizes, sizes[1:]))
    proved = 0
    for i in range(n):
        try:
            proof = t.get_proof(i)
        except IndexError:
            continue
        proved += 1
        assert len(proof) == len(t.levels) - 1
        assert t.prove(leaves[i], proof)
        assert not t.prove([leaves[i][0] + 1] + leaves[i][1:], proof)
        if proof:
            bad = [([(proof[0][0][0] + 1) % 101] + proof[0][0][1:], proof[0][1])] + proof[1:]
            assert not t.prove(leaves[i], bad)
    assert proved >= 1
    if n == 1:
        assert t.get_proof(0) == [] and t.root_hash() == PR.sponge(P, leaves[0], 2)


def test_merkle_unpaired_node_raises(f101):
    P = _params(f101, 8)
    for n, bad in ((3, [2]), (5, [4]), (13, [12]), (6, [4, 5])):
        t = PR.MerkleTree(P, [[i] for i in range(n)], 1)
        for i in range(n):
            if i in bad:
                with pytest.raises(IndexError):
                    t.get_proof(i)
            else:
                t.get_proof(i)
    with pytest.raises(IndexError):
        PR.MerkleTree(P, [[1], [2]], 1).get_proof(2)
    # the unpaired node is hashed with itself
    t = PR.MerkleTree(P, [[1], [2], [3]], 1)
    assert t.levels[1][1] == PR.sponge(P, t.levels[0][2] + t.levels[0][2], 1)
