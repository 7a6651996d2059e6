"""Host mirror of the reference's quadratic extension (src/algebra/field/extension: GaloisField<2, P>, arithmetic.rs,
gf_101_2.rs): Ext2(field, w) makes the class of F_p[t] / (t^2 - w).  An element is coeffs = (c0, c1) = c0 + c1 t in increasing
degree.  Scalar operators are host values, like the other mirrors; the array forms (vec_*) run on the GPU through the C ABI
(ronk_ext2_vec_*) on PLANAR arrays: n elements are [2][n] words, the c0 plane first."""
import numpy as np

from . import _lib as L
from .field import PlutoBaseField

_classes = {}


def Ext2(field, w):
    """the class of GaloisField<2, P> with irreducible t^2 - w over `field` (a PrimeField class); w a quadratic non-residue"""
    key = (field.ORDER, int(w) % field.ORDER)
    if key not in _classes:
        L.check(L.lib.ronk_ext2_check(field.ORDER, int(w)), "ronk_ext2_check")
        _classes[key] = type("GaloisField2_%d_%d" % key, (_Ext2Element,), {"BASE": field, "W": key[1], "P": field.ORDER,
                                                                          "ORDER": field.ORDER ** 2})
    return _classes[key]


class _Ext2Element:
    __slots__ = ("coeffs",)
    BASE, W, P, ORDER = None, 0, 0, 0

    def __init__(self, coeffs=(0, 0)):                # GaloisField::new
        c0, c1 = coeffs
        self.coeffs = (int(c0) % self.P, int(c1) % self.P)

    @classmethod
    def from_base(cls, x):                            # From<PrimeField<P>>: (x, 0)
        return cls((int(x), 0))

    @classmethod
    def zero(cls): return cls((0, 0))
    @classmethod
    def one(cls): return cls((1, 0))

    def _coerce(self, o):
        if isinstance(o, _Ext2Element):
            if (o.P, o.W) != (self.P, self.W):
                raise TypeError("elements of different extensions")
            return o
        return type(self).from_base(o)                # the mixed operations with PrimeField<P> / integers

    def __add__(self, o):
        o = self._coerce(o)
        return type(self)((self.coeffs[0] + o.coeffs[0], self.coeffs[1] + o.coeffs[1]))
    __radd__ = __add__

    def __sub__(self, o):
        o = self._coerce(o)
        return type(self)((self.coeffs[0] - o.coeffs[0], self.coeffs[1] - o.coeffs[1]))

    def __rsub__(self, o): return self._coerce(o) - self
    def __neg__(self): return type(self)((-self.coeffs[0], -self.coeffs[1]))

    def __mul__(self, o):                             # the product reduced modulo t^2 - w
        o = self._coerce(o)
        (a0, a1), (b0, b1) = self.coeffs, o.coeffs
        return type(self)((a0 * b0 + self.W * a1 * b1, a0 * b1 + a1 * b0))
    __rmul__ = __mul__

    def norm(self):                                   # a0^2 - w a1^2, a base element
        a0, a1 = self.coeffs
        return self.BASE(a0 * a0 - self.W * a1 * a1)

    def inverse(self):                                # None for zero; (a0, -a1) / norm
        n = int(self.norm())
        if n == 0:
            return None
        s = pow(n, self.P - 2, self.P)
        return type(self)((self.coeffs[0] * s, -self.coeffs[1] * s))

    def __truediv__(self, o):                         # self * rhs.inverse().expect("invalid inverse")
        inv = self._coerce(o).inverse()
        if inv is None:
            raise L.RonkPanic(L.ERR_ZERO_INVERSE)
        return self * inv

    def __mod__(self, o):                             # Rem: self - (self / rhs) * rhs
        o = self._coerce(o)
        return self - (self / o) * o

    def pow(self, power):
        r, a, e = type(self).one(), self, int(power)
        while e:
            if e & 1:
                r = r * a
            a = a * a
            e >>= 1
        return r

    def __eq__(self, o): return isinstance(o, _Ext2Element) and (o.P, o.W, o.coeffs) == (self.P, self.W, self.coeffs)
    def __hash__(self): return hash((self.P, self.W, self.coeffs))
    def __repr__(self): return "%d + %d t" % self.coeffs

    # --- array forms on planar [2][n] words: these run on the GPU through the C ABI
    @staticmethod
    def planar(elements):
        """[elements] -> [2][n] words"""
        return L.arr([e.coeffs[0] for e in elements] + [e.coeffs[1] for e in elements])

    @classmethod
    def _planar_arg(cls, a):
        a = L.arr(a)
        if a.size % 2:
            raise L.RonkPanic(L.ERR_INVALID, "a planar array holds [2][n] words")
        return a

    @classmethod
    def _v(cls, fn, a, b):
        a, b = cls._planar_arg(a), cls._planar_arg(b)
        if a.size != b.size:
            raise L.RonkPanic(L.ERR_INVALID, "operands of different lengths")
        out = np.empty_like(a)
        L.check(fn(cls.P, cls.W, L.ptr(a), L.ptr(b), L.ptr(out), a.size // 2))
        return out

    @classmethod
    def vec_add(cls, a, b): return cls._v(L.lib.ronk_ext2_vec_add, a, b)
    @classmethod
    def vec_sub(cls, a, b): return cls._v(L.lib.ronk_ext2_vec_sub, a, b)
    @classmethod
    def vec_mul(cls, a, b): return cls._v(L.lib.ronk_ext2_vec_mul, a, b)

    @classmethod
    def vec_neg(cls, a):
        a = cls._planar_arg(a); out = np.empty_like(a)
        L.check(L.lib.ronk_ext2_vec_neg(cls.P, cls.W, L.ptr(a), L.ptr(out), a.size // 2))
        return out

    @classmethod
    def vec_mul_base(cls, a, s):
        a, s = cls._planar_arg(a), L.arr(s)
        if 2 * s.size != a.size:
            raise L.RonkPanic(L.ERR_INVALID, "one base word per element")
        out = np.empty_like(a)
        L.check(L.lib.ronk_ext2_vec_mul_base(cls.P, cls.W, L.ptr(a), L.ptr(s), L.ptr(out), s.size))
        return out

    @classmethod
    def vec_pow(cls, a, e):
        a = cls._planar_arg(a); out = np.empty_like(a)
        L.check(L.lib.ronk_ext2_vec_pow(cls.P, cls.W, L.ptr(a), int(e), L.ptr(out), a.size // 2))
        return out

    @classmethod
    def vec_inv(cls, a):                              # a zero element: RonkPanic(ERR_ZERO_INVERSE), the reference's unwrap
        a = cls._planar_arg(a); out = np.empty_like(a)
        L.check(L.lib.ronk_ext2_vec_inv(cls.P, cls.W, L.ptr(a), L.ptr(out), a.size // 2))
        return out


PlutoBaseFieldExtension = Ext2(PlutoBaseField, 99)    # t^2 + 2 over F_101 (gf_101_2.rs)
