// deep_kernels.h -- the bodies of the batched FRI polynomial commitment (csrc/ronk_pcs.hip; include/ronk_ntt.h "batched FRI
// polynomial commitment"): the evaluation of C base-field polynomials at K points of the quadratic
// extension, the DEEP combination of a [C][N] matrix into one extension codeword, and the table both share.
//
//   G[i] = sum_(k < K) sum_(c < C) alpha^(k C + c) (M[c][i] - y[k][c]) / (x_i - z_k)
//        = sum_k B_k (S_i - Y_k) (x_i - z_k)^-1,     S_i = sum_c alpha^c M[c][i],  Y_k = sum_c alpha^c y[k][c],  B_k = alpha^(k C)
//
// x_i = s w^i is a base element, so 1 / (x_i - z_k) = (d, z1) / (d^2 - W z1^2) with d = x_i - z0: a base inversion.  What does
// not depend on i is computed once per call by deep_prep_* into a small table (DeepTab): the alpha^c, and per point z_k the words
// z0, W z1^2, B_k, B_k (0, z1), Y_k, so that B_k (d, z1) = B_k d + B_k (0, z1) is a product by a base element.  A lane then
//   1. accumulates S_i for its PTS points over the C rows (two base products per (point, column): alpha^c times a base word),
//   2. forms the PTS K norms, inverts their product ONCE (Fermat) and unwinds it with Montgomery's trick; the prefix products
//      stay in registers because K and PTS are compile-time, the norms are recomputed on the way back (one product each),
//   3. adds the K quotients.
// A zero norm (z_k is the domain point x_i) takes no part in the product and its term is zero, as ronk_ext2_vec_inv_dev writes
// zero for a zero element; deep_prep_point reports it by testing z_k itself.
//
// Field policies and forms are those of fri_kernels.h.  Plain C++ on uint64, so tests/emu/emu_deep.cpp compiles the same bodies
// for the host.
#pragma once
#include <type_traits>

#include "fri_kernels.h"

namespace ronk {

constexpr u32 DEEP_MAX_K = 8;       // points per opening
constexpr u32 DEEP_MAX_C = 1024;    // columns per matrix
constexpr u32 DEEP_KW = 8;          // table words per point
constexpr int DEEP_PTS = 4;         // points per lane of the combine kernel, at stride N / 4
constexpr u32 DEEP_EVAL_LANES = 256;

// the table of one call, register form: K records of DEEP_KW words, then the C pairs alpha^c in the form `apx` below
struct DeepTab {
  const u64* k;    // [K][8]: z0, W z1^2, B.c0, B.c1, (B (0, z1)).c0, .c1, Y.c0, Y.c1
  const u64* ap;   // [C][2]
};
RONK_HD u64 deep_tab_words(u32 K, u32 C) { return (u64)DEEP_KW * K + 2 * (u64)C; }

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
// The record of point k; z: planar [2][K], y: planar [2][K C], any 64-bit words.  Returns 32 when z_k lies on the domain
// (z1 = 0 and (z0 / s)^N = 1), else 0.
template <class F>
RONK_HD int deep_prep_point(const Ext2<F>& x, const DeepDomain& dm, E2 alpha, const u64* z, const u64* y, u32 K, u32 C, u32 k, u64* rec) {
  const F& f = x.f;
  const u64 z0 = f.in(z[k]), z1 = f.in(z[K + k]);
  const E2 B = x.pow(alpha, (u64)k * C);
  const E2 Bz = x.mul(B, E2{0, z1});
  E2 Y = x.zero();
  const u64 n = (u64)K * C;
  for (u32 c = C; c-- > 0;) Y = x.add(x.mul(Y, alpha), E2{f.in(y[(u64)k * C + c]), f.in(y[n + (u64)k * C + c])});
  rec[0] = z0;
  rec[1] = f.mul_w(f.mul(z1, z1), x.w);
  rec[2] = B.c0; rec[3] = B.c1; rec[4] = Bz.c0; rec[5] = Bz.c1; rec[6] = Y.c0; rec[7] = Y.c1;
  u64 t = f.mul(z0, dm.sinv);
  for (u32 b = 0; b < dm.log2n; b++) t = f.mul(t, t);
  return (z1 == 0 && t == f.one()) ? 32 : 0;
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

// G[t] = sum_k B_k (S[t] - Y_k) / (xs[t] - z_k) for the PTS points of a lane; S and G in register form
template <class F, int K, int PTS>
RONK_HD void deep_quotients(const Ext2<F>& x, const u64 (&krec)[K * DEEP_KW], const u64 (&xs)[PTS], const E2 (&S)[PTS], E2 (&G)[PTS]) {
  const F& f = x.f;
  u64 pre[PTS * K];
  u64 run = f.one();
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int t = decltype(I)::value / K, k = decltype(I)::value % K;
    bool zero;
    const u64 n = deep_norm(f, f.sub(xs[t], krec[k * DEEP_KW]), krec[k * DEEP_KW + 1], zero);
    pre[t * K + k] = run;
    run = f.mul(run, n);
  });
  u64 inv = deep_inverse(x, run);
  deep_for<0, PTS>([&](auto T) { G[decltype(T)::value] = x.zero(); });
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int J = PTS * K - 1 - decltype(I)::value, t = J / K, k = J % K, r = k * (int)DEEP_KW;
    bool zero;
    const u64 d = f.sub(xs[t], krec[r]);
    const u64 n = deep_norm(f, d, krec[r + 1], zero);
    u64 ninv = f.mul(inv, pre[J]);
    inv = f.mul(inv, n);
    if (zero) ninv = 0;
    const E2 B{f.add(f.mul(krec[r + 2], d), krec[r + 4]), f.add(f.mul(krec[r + 3], d), krec[r + 5])};   // B_k (d, z1)
    G[t] = x.add(G[t], x.mul_base(x.mul(x.sub(S[t], E2{krec[r + 6], krec[r + 7]}), B), ninv));
  });
}

// The lane that owns the points i + t q, t < PTS (q = N / PTS; PTS = 4, or 1 with q unused): load(c, t) = the raw word of
// column c at point t.  Returns the canonical pairs.
template <class F, int K, int PTS, class Load>
RONK_HD void deep_combine_lane(const Ext2<F>& x, const DeepDomain& dm, const DeepTab& tab, u32 C, u64 i, Load&& load, E2 (&out)[PTS]) {
  static_assert(PTS == 1 || PTS == 4, "a lane owns one point or the four points x, x iota, -x, -x iota");
  const F& f = x.f;
  E2 S[PTS];
  deep_for<0, PTS>([&](auto T) { S[decltype(T)::value] = x.zero(); });
  const FriTable ap = (FriTable)tab.ap;
  for (u32 c = 0; c < C; c++) {
    const u64 a0 = ap[2 * (u64)c], a1 = ap[2 * (u64)c + 1];
    deep_for<0, PTS>([&](auto T) { constexpr int t = decltype(T)::value; S[t] = deep_accumulate(f, S[t], load(c, t), a0, a1); });
  }
  u64 xs[PTS];
  xs[0] = deep_point(f, dm, i);
  if constexpr (PTS == 4) {
    xs[1] = f.mul(xs[0], dm.iota);
    xs[2] = f.neg(xs[0]);
    xs[3] = f.neg(xs[1]);
  }
  // the records are few and wave-uniform: a local copy keeps them in scalar registers
  u64 krec[K * DEEP_KW];
  const FriTable kr = (FriTable)tab.k;
  deep_for<0, K * (int)DEEP_KW>([&](auto J) { krec[decltype(J)::value] = kr[decltype(J)::value]; });
  E2 G[PTS];
  deep_quotients<F, K, PTS>(x, krec, xs, S, G);
  deep_for<0, PTS>([&](auto T) { constexpr int t = decltype(T)::value; out[t] = E2{f.out(G[t].c0), f.out(G[t].c1)}; });
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
