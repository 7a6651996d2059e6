"""Pure-Python restatement of the quadratic extension F_p[t] / (t^2 - w) (include/ronk_ntt.h "quadratic extension"; the
reference's GaloisField<2, P>) on Python integers: elements are pairs (c0, c1) = c0 + c1 t.  A test helper, not product code; it
shares nothing with the library."""


class Ext2:
    def __init__(self, p, w):
        assert p > 2 and w % p != 0 and pow(w, (p - 1) // 2, p) == p - 1, "w must be a quadratic non-residue of the odd prime p"
        self.p, self.w = p, w % p
        self.zero, self.one = (0, 0), (1, 0)

    def el(self, a):
        return (int(a[0]) % self.p, int(a[1]) % self.p)

    def embed(self, x):
        return (int(x) % self.p, 0)

    def add(self, a, b):
        return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)

    def sub(self, a, b):
        return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)

    def neg(self, a):
        return (-a[0] % self.p, -a[1] % self.p)

    def mul(self, a, b):
        """the product of the two degree-1 polynomials reduced modulo t^2 - w, schoolbook"""
        return ((a[0] * b[0] + self.w * a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)

    def mul_base(self, a, s):
        return (a[0] * s % self.p, a[1] * s % self.p)

    def norm(self, a):
        return (a[0] * a[0] - self.w * a[1] * a[1]) % self.p

    def inv(self, a):
        """None for the zero element, like the reference's inverse()"""
        n = self.norm(a)
        if n == 0:
            return None
        return self.mul_base((a[0], -a[1] % self.p), pow(n, self.p - 2, self.p))

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def pow(self, a, e):
        r = self.one
        while e:
            if e & 1:
                r = self.mul(r, a)
            a = self.mul(a, a)
            e >>= 1
        return r

    def order(self, a):
        """the multiplicative order, by the prime factors of p^2 - 1 (small p only)"""
        n = self.p * self.p - 1
        assert a != self.zero and self.pow(a, n) == self.one
        m, q, order = n, 2, n
        while q * q <= m:
            if m % q == 0:
                while m % q == 0:
                    m //= q
                while order % q == 0 and self.pow(a, order // q) == self.one:
                    order //= q
            q += 1
        if m > 1 and self.pow(a, order // m) == self.one:
            order //= m
        return order


def planar(elements):
    """[(c0, c1)] -> the [2][n] words of the library's arrays"""
    return [e[0] for e in elements] + [e[1] for e in elements]


def pairs(words):
    n = len(words) // 2
    return [(int(words[i]), int(words[n + i])) for i in range(n)]
