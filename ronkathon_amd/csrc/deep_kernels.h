// deep_kernels.h -- the pieces of a DEEP combination that do not depend on how many matrices are combined, shared by the
// polynomial commitment (csrc/mpcs_kernels.h, which holds the lane and the table of a call; csrc/ronk_mpcs.hip; DESIGN.md sections
// 15 and 21), csrc/plonk_kernels.h and csrc/accum_kernels.h: the two-level table of the domain points, the raw-word form of the
// alpha^c, the S accumulation, the norm and the Fermat inversion, the unrolling helper, and the evaluation of base-field
// polynomials at points of the quadratic extension.
//
// x_i = s w^i is a base element, so 1 / (x_i - z_k) = (d, z1) / (d^2 - W z1^2) with d = x_i - z0: a base inversion of the norm
// (deep_norm, deep_inverse).  A zero norm (z_k is the domain point x_i) is replaced by one and reported, so that the caller can
// make its term zero, as ronk_ext2_vec_inv_dev writes zero for a zero element.
//
// Field policies and forms are those of fri_kernels.h.  Plain C++ on uint64, so tests/emu/emu_deep.cpp compiles the same bodies
// for the host.
#pragma once
#include <type_traits>

#include "fri_kernels.h"

namespace ronk {

constexpr u32 DEEP_MAX_K = 8;       // points per opening
constexpr u32 DEEP_MAX_C = 1024;    // columns per matrix
constexpr int DEEP_PTS = 4;         // points per lane of the combine kernel, at stride N / 4
constexpr u32 DEEP_EVAL_LANES = 256;

// the points x_i = s w^i of the domain as a two-level table, x_i = hi[i >> kbits] * lo[i & (2^kbits - 1)], register form
struct DeepDomain {
  const u64* hi;   // s w^(j 2^kbits), 2^(log2n - kbits) entries
  const u64* lo;   // w^j, 2^kbits entries
  u32 kbits, log2n;
  u64 iota;        // w^(N / 4), the fourth root of unity: x_(i + t N/4) = x_i iota^t
  u64 sinv;        // 1 / s
};
template <class F>
RONK_HD u64 deep_point(const F& f, const DeepDomain& dm, u64 i) {
  const FriTable hi = (FriTable)dm.hi, lo = (FriTable)dm.lo;
  return f.mul(hi[i >> dm.kbits], lo[i & (((u64)1 << dm.kbits) - 1)]);
}

// A table word that multiplies a RAW matrix word: f.mul(raw, apx(a)) is a * raw in register form for any 64-bit raw (the
// Goldilocks product takes any representative; the Montgomery product of a raw word by a R^2 is a raw R).
template <class F>
RONK_HD u64 deep_apx(const F& f, u64 a_reg) { return f.in(a_reg); }

// ---------------------------------------------------------------------------------------------------- the table
// alpha^c for one column
template <class F>
RONK_HD void deep_prep_column(const Ext2<F>& x, E2 alpha, u32 c, u64* ap) {
  const E2 a = x.pow(alpha, c);
  ap[2 * (u64)c] = deep_apx(x.f, a.c0);
  ap[2 * (u64)c + 1] = deep_apx(x.f, a.c1);
}

// ---------------------------------------------------------------------------------------------------- combine
// S += alpha^c * m for a raw matrix word m
template <class F>
RONK_HD E2 deep_accumulate(const F& f, E2 S, u64 m, u64 ap0, u64 ap1) {
  return E2{f.add(S.c0, f.mul(m, ap0)), f.add(S.c1, f.mul(m, ap1))};
}

template <class F>
RONK_HD u64 deep_norm(const F& f, u64 d, u64 wz1sq, bool& zero) {
  const u64 n = f.sub(f.mul(d, d), wz1sq);
  zero = n == 0;
  return zero ? f.one() : n;
}

// a^(p - 2) for a base element in register form.  Goldilocks: p - 2 = 2^64 - 2^32 - 1 is 31 ones, a zero and 32 ones, so the
// chain through e_k = a^(2^k - 1) takes 64 squarings and 10 products where square-and-multiply takes 64 and 63.
template <class F>
RONK_HD u64 deep_sqn(const F& f, u64 a, int n) {
  for (int i = 0; i < n; i++) a = f.mul(a, a);
  return a;
}
template <class F>
RONK_HD u64 deep_inverse(const Ext2<F>& x, u64 a) {
  const F& f = x.f;
  if (f.order() != gl64::P) return x.base_pow(a, f.order() - 2);
  const u64 e2 = f.mul(f.mul(a, a), a);
  const u64 e3 = f.mul(f.mul(e2, e2), a);
  const u64 e6 = f.mul(deep_sqn(f, e3, 3), e3);
  const u64 e7 = f.mul(f.mul(e6, e6), a);
  const u64 e14 = f.mul(deep_sqn(f, e7, 7), e7);
  const u64 e15 = f.mul(f.mul(e14, e14), a);
  const u64 e30 = f.mul(deep_sqn(f, e15, 15), e15);
  const u64 e31 = f.mul(f.mul(e30, e30), a);
  const u64 e32 = f.mul(f.mul(e31, e31), a);
  return f.mul(deep_sqn(f, e31, 33), e32);
}

// fn(integral_constant<int, I>) for I = 0 .. N - 1 in order, unrolled by construction: the arrays below are indexed by
// compile-time constants only and stay in registers
template <int I, int N, class Fn>
RONK_HD void deep_for(Fn&& fn) {
  if constexpr (I < N) {
    fn(std::integral_constant<int, I>{});
    deep_for<I + 1, N>(fn);
  }
}

// ---------------------------------------------------------------------------------------------------- evaluation
// One column's share of one lane: the coefficients j = lane + r lanes, r >= 0, as sum_r coef[j] Z^r by Horner's rule in
// Z = z^lanes, times z^lane.  The sum of the lanes' shares is f(z_k).  K <= DEEP_MAX_K; zr: the points in register form.
template <class F, class Load>
RONK_HD void deep_eval_lane(const Ext2<F>& x, u64 d, u32 lane, u32 lanes, const E2 (&zr)[DEEP_MAX_K], u32 K, Load&& coef,
                            E2 (&share)[DEEP_MAX_K]) {
  const F& f = x.f;
  E2 Z[DEEP_MAX_K], acc[DEEP_MAX_K];
  deep_for<0, (int)DEEP_MAX_K>([&](auto J) {
    constexpr int k = decltype(J)::value;
    acc[k] = x.zero();
    Z[k] = (u32)k < K ? x.pow(zr[k], lanes) : x.zero();
  });
  const u64 rounds = (d + lanes - 1) / lanes;
  for (u64 r = rounds; r-- > 0;) {
    const u64 j = r * lanes + lane;
    const u64 cj = j < d ? f.in(coef(j)) : 0;
    deep_for<0, (int)DEEP_MAX_K>([&](auto J) {
      constexpr int k = decltype(J)::value;
      if ((u32)k < K) {
        const E2 m = x.mul(acc[k], Z[k]);
        acc[k] = E2{f.add(m.c0, cj), m.c1};
      }
    });
  }
  deep_for<0, (int)DEEP_MAX_K>([&](auto J) {
    constexpr int k = decltype(J)::value;
    share[k] = (u32)k < K ? x.mul(acc[k], x.pow(zr[k], lane)) : x.zero();
  });
}

// ---------------------------------------------------------------------------------------------------- host: tables
// lo (2^kbits words) then hi (2^(log2n - kbits) words) of the domain s <w_N>, register form
inline u32 deep_kbits(u32 log2n) { return (log2n + 1) / 2; }
inline void deep_host_domain(bool mont, u64 p, u64 g, u64 shift, u32 log2n, u64* lo, u64* hi, u64* iota, u64* sinv) {
  const u32 kb = deep_kbits(log2n);
  const u64 w = fri_powmod(g, (p - 1) >> log2n, p);
  u64 xv = 1 % p;
  for (u64 j = 0; j < ((u64)1 << kb); j++) { lo[j] = fri_reg_form(mont, p, xv); xv = fri_mulmod(xv, w, p); }
  const u64 step = xv;   // w^(2^kb)
  xv = shift % p;
  for (u64 j = 0; j < ((u64)1 << (log2n - kb)); j++) { hi[j] = fri_reg_form(mont, p, xv); xv = fri_mulmod(xv, step, p); }
  *iota = fri_reg_form(mont, p, log2n >= 2 ? fri_powmod(w, (u64)1 << (log2n - 2), p) : 1);
  *sinv = fri_reg_form(mont, p, fri_powmod(shift % p, p - 2, p));
}

}  // namespace ronk
