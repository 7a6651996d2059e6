// ext2.h -- the quadratic extension F_p[t] / (t^2 - W) of a 64-bit prime field: the reference's GaloisField<2, P>
// (src/algebra/field/extension/mod.rs, arithmetic.rs, gf_101_2.rs) over the device field policies.
//
// An element is the pair (c0, c1) = c0 + c1 t, the reference's `coeffs: [F; 2]` in increasing degree.  Ext2<F> is written on a
// base policy F that supplies add, sub, neg, mul, mul_w (the product with W) on words in REGISTER form (canonical for
// Goldilocks, x R mod p for a Montgomery prime) and one() / order(); both components of a pair are in that form, and so is W
// (a kernel argument: SGPRs).  The product
// is the reference's reduction modulo X^2 - K in Karatsuba form: three base products plus the product with W, which a policy
// may specialise (fri_kernels.h FriGlW7: Goldilocks with W = 7, 7 x = 8 x - x by a shift).
//
// Plain C++ on uint64, so tests/emu/emu_ext2.cpp compiles the same bodies for the host.
#pragma once
#include "gl64.h"
#include "mont64.h"

namespace ronk {

typedef uint64_t u64;
typedef uint32_t u32;

struct E2 {
  u64 c0, c1;
};

template <class F>
struct Ext2 {
  F f;
  u64 w;   // W in register form
  RONK_HD Ext2(const F& base, u64 w_reg) : f(base), w(w_reg) {}

  RONK_HD E2 zero() const { return E2{0, 0}; }
  RONK_HD E2 one() const { return E2{f.one(), 0}; }
  RONK_HD E2 add(E2 a, E2 b) const { return E2{f.add(a.c0, b.c0), f.add(a.c1, b.c1)}; }
  RONK_HD E2 sub(E2 a, E2 b) const { return E2{f.sub(a.c0, b.c0), f.sub(a.c1, b.c1)}; }
  RONK_HD E2 neg(E2 a) const { return E2{f.neg(a.c0), f.neg(a.c1)}; }
  // (a0 b0 + W a1 b1, (a0 + a1)(b0 + b1) - a0 b0 - a1 b1)
  RONK_HD E2 mul(E2 a, E2 b) const {
    const u64 p00 = f.mul(a.c0, b.c0), p11 = f.mul(a.c1, b.c1);
    const u64 mid = f.mul(f.add(a.c0, a.c1), f.add(b.c0, b.c1));
    return E2{f.add(p00, f.mul_w(p11, w)), f.sub(f.sub(mid, p00), p11)};
  }
  // (a0^2 + W a1^2, 2 a0 a1)
  RONK_HD E2 sqr(E2 a) const {
    const u64 p00 = f.mul(a.c0, a.c0), p11 = f.mul(a.c1, a.c1), p01 = f.mul(a.c0, a.c1);
    return E2{f.add(p00, f.mul_w(p11, w)), f.add(p01, p01)};
  }
  // the reference's Mul<PrimeField<P>>: both components times a base element
  RONK_HD E2 mul_base(E2 a, u64 s) const { return E2{f.mul(a.c0, s), f.mul(a.c1, s)}; }
  // a0^2 - W a1^2, a base element; zero only for the zero element when W is a non-residue
  RONK_HD u64 norm(E2 a) const { return f.sub(f.mul(a.c0, a.c0), f.mul_w(f.mul(a.c1, a.c1), w)); }
  RONK_HD u64 base_pow(u64 a, u64 e) const {
    u64 r = f.one();
    while (e) {
      if (e & 1) r = f.mul(r, a);
      a = f.mul(a, a);
      e >>= 1;
    }
    return r;
  }
  // the reference's inverse(): (a0, -a1) / norm; the zero element gives (0, 0) and the caller reports it
  RONK_HD E2 inv(E2 a) const { return mul_base(E2{a.c0, f.neg(a.c1)}, base_pow(norm(a), f.order() - 2)); }
  // square-and-multiply; the value of the reference's recursion, pow(_, 0) == ONE
  RONK_HD E2 pow(E2 a, u64 e) const {
    E2 r = one();
    while (e) {
      if (e & 1) r = mul(r, a);
      a = sqr(a);
      e >>= 1;
    }
    return r;
  }
};

// ---- host integer logic: is (p, w) an extension?  (the codes of ronk_ext2_check, without the primality test)
inline u64 ext2_mulmod(u64 a, u64 b, u64 p) { return (u64)(((unsigned __int128)a * b) % p); }
inline u64 ext2_powmod(u64 a, u64 e, u64 p) {
  u64 r = 1 % p;
  a %= p;
  while (e) { if (e & 1) r = ext2_mulmod(r, a, p); a = ext2_mulmod(a, a, p); e >>= 1; }
  return r;
}
// W must be a quadratic non-residue of the odd prime p (Euler's criterion), hence non-zero
inline bool ext2_non_residue(u64 p, u64 w) { return w % p != 0 && ext2_powmod(w, (p - 1) / 2, p) == p - 1; }
inline u64 ext2_reg_form(bool mont, u64 p, u64 c) { return mont ? (u64)((((unsigned __int128)(c % p)) << 64) % p) : c % p; }

}  // namespace ronk
