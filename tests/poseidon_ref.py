"""Pure-Python restatement of the reference's Poseidon permutation, sponge and Merkle tree (over the sponge) on Python integers:
src/hashes/poseidon/mod.rs:56-149, sponge.rs:69-275, src/tree/merkle.rs:31-99.  A test helper, not product code; it shares
nothing with the library or the oracle.

It also derives the TEST parameters the 64-bit primes are exercised with (the reference holds constants for F_101 only):
SplitMix64-seeded round constants and a Cauchy matrix 1 / (x_i + y_j).  They are test parameters, not a standard instance, and
nothing is claimed about their security."""

GOLDILOCKS = 0xFFFFFFFF00000001
MONT_P = 0xFFFFFFFC00000001


class Params:
    def __init__(self, p, width, alpha, num_p, num_f, rate, rc, mds):
        assert len(rc) == (num_p + num_f) * width and len(mds) == width and all(len(r) == width for r in mds)
        self.p, self.width, self.alpha, self.num_p, self.num_f, self.rate = p, width, alpha, num_p, num_f, rate
        self.rc = [c % p for c in rc]
        self.mds = [[c % p for c in row] for row in mds]

    def create_args(self):
        """the arguments of ronkathon_amd._lib.PoseidonHandle"""
        return (self.p, self.width, self.alpha, self.num_p, self.num_f, self.rate, self.rc, self.mds)


def splitmix64(seed):
    x = seed & (2**64 - 1)
    while True:
        x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        yield z ^ (z >> 31)


def derive_params(p, width, alpha, num_p, num_f, rate, seed=1):
    """deterministic TEST parameters: rc from SplitMix64, mds[i][j] = 1 / (x_i + y_j) with x_i = i, y_j = width + j"""
    g = splitmix64(seed * 1000003 + width * 131 + alpha)
    rc = [next(g) % p for _ in range((num_p + num_f) * width)]
    mds = [[pow((i + width + j) % p, p - 2, p) for j in range(width)] for i in range(width)]
    return Params(p, width, alpha, num_p, num_f, rate, rc, mds)


def permute(P, state):
    """mod.rs:131-149 on a full-width state"""
    p, w = P.p, P.width
    st = [s % p for s in state]
    assert len(st) == w
    for r in range(P.num_f + P.num_p):
        st = [(s + P.rc[r * w + i]) % p for i, s in enumerate(st)]
        if r < P.num_f // 2 or r >= P.num_p + P.num_f // 2:
            st = [pow(s, P.alpha, p) for s in st]
        else:
            st[0] = pow(st[0], P.alpha, p)
        st = [sum(st[j] * P.mds[i][j] for j in range(w)) % p for i in range(w)]
    return st


def hash_(P, values):
    """Poseidon::hash: pad with ZERO to width, permute, state[1]"""
    if len(values) > P.width:
        raise IndexError("input longer than the width")
    return permute(P, list(values) + [0] * (P.width - len(values)))[1]


class Sponge:
    """sponge.rs: absorb any number of times, then squeeze; `permutations` counts calls of the permutation"""

    def __init__(self, P):
        self.P = P
        self.state = [0] * P.width
        self.cap = P.width - P.rate
        self.absorb_index = 0
        self.squeeze_index = 0
        self.permutations = 0
        self.squeezing = False

    def _permute(self):
        self.state = permute(self.P, self.state)
        self.permutations += 1
        self.absorb_index = 0

    def absorb(self, elements):
        assert not self.squeezing
        p = self.P.p
        for e in elements:
            self.state[self.cap + self.absorb_index] = (self.state[self.cap + self.absorb_index] + e) % p
            self.absorb_index += 1
            if self.absorb_index == self.P.rate:
                self._permute()
        return self

    def squeeze(self, n):
        if not self.squeezing:
            if self.absorb_index != 0:
                self._permute()
            self.squeezing = True
        out = []
        while len(out) < n:
            if self.squeeze_index == self.P.rate:
                self._permute()
                self.squeeze_index = 0
            out.append(self.state[self.cap + self.squeeze_index])
            self.squeeze_index += 1
        return out


def sponge(P, elements, n_out):
    return Sponge(P).absorb(elements).squeeze(n_out)


class MerkleTree:
    """merkle.rs:31-99 with the sponge as the hash; levels[0] = leaf digests, levels[-1] = [root]"""

    def __init__(self, P, leaves, digest_len):
        assert len(leaves) >= 1 and 1 <= digest_len <= P.rate
        self.P, self.d = P, digest_len
        level = [sponge(P, leaf, digest_len) for leaf in leaves]
        self.levels = [level]
        while len(level) > 1:
            nxt = []
            for i in range(0, len(level) - 1, 2):
                nxt.append(sponge(P, level[i] + level[i + 1], digest_len))
            if len(level) % 2 == 1:
                nxt.append(sponge(P, level[-1] + level[-1], digest_len))
            self.levels.append(nxt)
            level = nxt

    def root_hash(self):
        return self.levels[-1][0]

    def flat(self):
        """the library's layout: every level, leaves first, the root last"""
        return [w for level in self.levels for node in level for w in node]

    def get_proof(self, leaf_index):
        """-> [(sibling digest, 'L' | 'R')] from the bottom up; IndexError where the reference's level[sibling_index] panics"""
        proof = []
        index = leaf_index
        if index >= len(self.levels[0]):
            raise IndexError("leaf index out of range")
        for level in self.levels[:-1]:
            side, sib = ("R", index + 1) if index % 2 == 0 else ("L", index - 1)
            if sib >= len(level):
                raise IndexError("unpaired last node: level[index + 1] is out of bounds")
            proof.append((level[sib], side))
            index //= 2
        return proof

    def prove(self, leaf, proof):
        h = sponge(self.P, leaf, self.d)
        for sib, side in proof:
            h = sponge(self.P, (sib + h) if side == "L" else (h + sib), self.d)
        return h == self.root_hash()
