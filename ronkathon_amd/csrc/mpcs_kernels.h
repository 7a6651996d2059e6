// mpcs_kernels.h -- the bodies of the multi-matrix FRI polynomial commitment (csrc/ronk_mpcs.hip; include/ronk_ntt.h "multi-matrix
// polynomial commitment"): R committed matrices M_r of C_r columns each, round r opened at the points z_k
// with bit k of mask_r set, combined into ONE extension codeword.  With o_r = sum_(r' < r) C_r' and C_tot = sum_r C_r,
//
//   G[i] = sum_r sum_(k in mask_r) sum_(c < C_r) alpha^(k C_tot + o_r + c) (M_r[c][i] - y[r][k][c]) / (x_i - z_k)
//        = sum_r sum_(k in mask_r) B_k (S_r,i - Y_r,k) (x_i - z_k)^-1,
//   S_r,i = sum_c alpha^(o_r + c) M_r[c][i],   Y_r,k = sum_c alpha^(o_r + c) y[r][k][c],   B_k = alpha^(k C_tot).
//
// The pieces are those of deep_kernels.h (the domain table, the norm, the Fermat inversion, the raw-word form of the alpha^j).
// What does not depend on i is computed once per call into a small table (MpcsTab).  A lane
//   1. forms the PTS K norms of its points, inverts their product ONCE and unwinds it with Montgomery's trick INTO the array of
//      prefix products: the PTS K inverse norms do not depend on the matrices and are held across the rounds (a zero norm is
//      replaced by one and its inverse by zero, so its terms vanish);
//   2. per round walks the C_r rows into S_r (one accumulator set alive at a time), and
//   3. adds B_k (d, z1) ninv (S_r - Y_r,k) for the points of the round's mask; B_k (d, z1) = B_k d + B_k (0, z1) is recomputed per
//      round (two base products), which keeps K registers per point and not 3 K.
// The masks and column counts are wave-uniform; K and PTS are compile-time, so every (t, k) array is indexed by constants.
// R = 1 with the full mask (mpcs_full_mask) is the batched commitment of one matrix, ronk_pcs_* (csrc/ronk_pcs.hip; DESIGN.md
// section 15): G[i] = sum_k B_k (S_i - Y_k) (x_i - z_k)^-1 with B_k = alpha^(k C).  The prover's lane of a one-round handle takes
// the steps in another order, rows first (mpcs_one_round_lane); table, prep and check are the same.
//
// Plain C++ on uint64, so tests/emu/emu_mpcs.cpp compiles the same bodies for the host, and tests/emu/emu_deep.cpp the one-round
// case.
#pragma once
#include "deep_kernels.h"

namespace ronk {

constexpr u32 MPCS_MAX_R = 8;     // committed matrices per opening
constexpr u32 MPCS_KW = 6;        // table words per point

// the shape of a handle, passed to the kernels by value
struct MpcsShape {
  u32 R, K, Ctot, Y;              // Y: claims, sum_r popcount(mask_r) C_r
  u32 C[MPCS_MAX_R];              // columns of round r
  u32 mask[MPCS_MAX_R];           // bit k: round r is opened at z_k
  u32 off[MPCS_MAX_R];            // o_r
  u32 yoff[MPCS_MAX_R];           // the first claim of round r in a plane of y
};
// R device pointers by value: the matrices (combine), the opened leaves (check), the trees' roots (transcript)
struct MpcsPtrs {
  const u64* p[MPCS_MAX_R];
};

RONK_HD u32 mpcs_popcount(u32 v) {
  u32 n = 0;
  for (; v; v &= v - 1) n++;
  return n;
}
// every one of K <= DEEP_MAX_K points: the mask of the one round of ronk_pcs_* and of ronk_ext2_poly_eval_batch*
RONK_HD u32 mpcs_full_mask(u32 K) { return (1u << K) - 1; }
// the claim y[r][k][c] is element yoff_r + rank_r(k) C_r + c of a plane; rank_r(k): the set bits of mask_r below k
RONK_HD u32 mpcs_claim_index(const MpcsShape& sh, u32 r, u32 k, u32 c) {
  return sh.yoff[r] + mpcs_popcount(sh.mask[r] & ((1u << k) - 1)) * sh.C[r] + c;
}

// the table of one call, register form
struct MpcsTab {
  const u64* k;    // [K][6]: z0, W z1^2, B.c0, B.c1, (B (0, z1)).c0, .c1
  const u64* y;    // [R][K][2]: Y_r,k (zero where mask_r lacks k)
  const u64* ap;   // [C_tot][2]: alpha^j in the form deep_apx
};
RONK_HD u64 mpcs_tab_words(u32 R, u32 K, u32 Ctot) { return (u64)MPCS_KW * K + 2 * (u64)R * K + 2 * (u64)Ctot; }

// ---------------------------------------------------------------------------------------------------- the table
// The record of point k; z: planar [2][K], any 64-bit words.  Returns 32 when z_k lies on the domain, else 0.
template <class F>
RONK_HD int mpcs_prep_point(const Ext2<F>& x, const DeepDomain& dm, E2 alpha, const u64* z, const MpcsShape& sh, u32 k, u64* rec) {
  const F& f = x.f;
  const u64 z0 = f.in(z[k]), z1 = f.in(z[sh.K + k]);
  const E2 B = x.pow(alpha, (u64)k * sh.Ctot);
  const E2 Bz = x.mul(B, E2{0, z1});
  rec[0] = z0;
  rec[1] = f.mul_w(f.mul(z1, z1), x.w);
  rec[2] = B.c0; rec[3] = B.c1; rec[4] = Bz.c0; rec[5] = Bz.c1;
  u64 t = f.mul(z0, dm.sinv);
  for (u32 b = 0; b < dm.log2n; b++) t = f.mul(t, t);
  return (z1 == 0 && t == f.one()) ? 32 : 0;
}
// Y_r,k by Horner's rule over the round's claims, times alpha^(o_r); y: planar [2][Y], any 64-bit words
template <class F>
RONK_HD void mpcs_prep_claims(const Ext2<F>& x, E2 alpha, const u64* y, const MpcsShape& sh, u32 r, u32 k, u64* out) {
  const F& f = x.f;
  E2 acc = x.zero();
  if ((sh.mask[r] >> k) & 1) {
    const u64 base = mpcs_claim_index(sh, r, k, 0);
    for (u32 c = sh.C[r]; c-- > 0;) acc = x.add(x.mul(acc, alpha), E2{f.in(y[base + c]), f.in(y[(u64)sh.Y + base + c])});
    acc = x.mul(acc, x.pow(alpha, sh.off[r]));
  }
  out[0] = acc.c0; out[1] = acc.c1;
}

// ---------------------------------------------------------------------------------------------------- combine
// B_k (d, z1) does not depend on the round, so the compiler would hoist it out of the round loop and hold 3 K words per point
// where the lane means to hold K.  An empty asm on the point makes the two products belong to their round (device build; a
// no-op for the host emulator).
RONK_HD void mpcs_keep(u64& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#else
  (void)v;
#endif
}

// The lane that owns the points i + t q, t < PTS (q = N / PTS; PTS = 4, or 1 with q unused): load(r, c, t) = the raw word of
// column c of round r at point t.  Returns the canonical pairs.
template <class F, int K, int PTS, class Load>
RONK_HD void mpcs_combine_lane(const Ext2<F>& x, const DeepDomain& dm, const MpcsTab& tab, const MpcsShape& sh, u64 i, Load&& load,
                               E2 (&out)[PTS]) {
  static_assert(PTS == 1 || PTS == 4, "a lane owns one point or the four points x, x iota, -x, -x iota");
  const F& f = x.f;
  u64 xs[PTS];
  xs[0] = deep_point(f, dm, i);
  if constexpr (PTS == 4) {
    xs[1] = f.mul(xs[0], dm.iota);
    xs[2] = f.neg(xs[0]);
    xs[3] = f.neg(xs[1]);
  }
  // the records are few and wave-uniform: a local copy keeps them in scalar registers
  u64 krec[K * MPCS_KW];
  const FriTable kr = (FriTable)tab.k;
  deep_for<0, K * (int)MPCS_KW>([&](auto J) { krec[decltype(J)::value] = kr[decltype(J)::value]; });
  // the PTS K inverse norms: prefix products on the way up, the inverses in their place on the way back
  u64 ninv[PTS * K];
  u64 run = f.one();
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int t = decltype(I)::value / K, k = decltype(I)::value % K;
    bool zero;
    const u64 n = deep_norm(f, f.sub(xs[t], krec[k * MPCS_KW]), krec[k * MPCS_KW + 1], zero);
    ninv[t * K + k] = run;
    run = f.mul(run, n);
  });
  u64 inv = deep_inverse(x, run);
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int J = PTS * K - 1 - decltype(I)::value, t = J / K, k = J % K;
    bool zero;
    const u64 n = deep_norm(f, f.sub(xs[t], krec[k * MPCS_KW]), krec[k * MPCS_KW + 1], zero);
    const u64 v = f.mul(inv, ninv[J]);
    inv = f.mul(inv, n);
    ninv[J] = zero ? 0 : v;
  });
  E2 G[PTS];
  deep_for<0, PTS>([&](auto T) { G[decltype(T)::value] = x.zero(); });
  const FriTable ap = (FriTable)tab.ap, yt = (FriTable)tab.y;
  for (u32 r = 0; r < sh.R; r++) {
    E2 S[PTS];
    deep_for<0, PTS>([&](auto T) { S[decltype(T)::value] = x.zero(); });
    const u32 C = sh.C[r], mask = sh.mask[r];
    const u64 o = sh.off[r];
    for (u32 c = 0; c < C; c++) {
      const u64 a0 = ap[2 * (o + c)], a1 = ap[2 * (o + c) + 1];
      deep_for<0, PTS>([&](auto T) { constexpr int t = decltype(T)::value; S[t] = deep_accumulate(f, S[t], load(r, c, t), a0, a1); });
    }
    deep_for<0, K>([&](auto Kk) {
      constexpr int k = decltype(Kk)::value, rec = k * (int)MPCS_KW;
      if (!((mask >> k) & 1)) return;   // wave-uniform
      const E2 Yrk{yt[2 * ((u64)r * K + k)], yt[2 * ((u64)r * K + k) + 1]};
      deep_for<0, PTS>([&](auto T) {
        constexpr int t = decltype(T)::value;
        u64 xt = xs[t];
        mpcs_keep(xt);
        const u64 d = f.sub(xt, krec[rec]);
        const E2 B{f.add(f.mul(krec[rec + 2], d), krec[rec + 4]), f.add(f.mul(krec[rec + 3], d), krec[rec + 5])};   // B_k (d, z1)
        G[t] = x.add(G[t], x.mul_base(x.mul(x.sub(S[t], Yrk), B), ninv[t * K + k]));
      });
    });
  }
  deep_for<0, PTS>([&](auto T) { constexpr int t = decltype(T)::value; out[t] = E2{f.out(G[t].c0), f.out(G[t].c1)}; });
}

// The prover's lane of a ONE-round handle (R = 1, hence the full mask; every ronk_pcs handle): the same words from the same table
// in the order of the first combine kernel, S over the C rows FIRST, then the norms, the one inversion, and the quotients added
// while Montgomery's trick unwinds (the prefix products are kept, a norm is recomputed on the way back).  With one round nothing is
// held across rounds, and the loads of a lane are issued before its inversion chain: at K = 1 over Goldilocks the order above is
// 6 to 9 % slower.  The check kernel has one body, mpcs_combine_lane<F, K, 1>, whatever R.
template <class F, int K, class Load>
RONK_HD void mpcs_one_round_lane(const Ext2<F>& x, const DeepDomain& dm, const MpcsTab& tab, u32 C, u64 i, Load&& load,
                                 E2 (&out)[DEEP_PTS]) {
  constexpr int PTS = DEEP_PTS;
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
  xs[1] = f.mul(xs[0], dm.iota);
  xs[2] = f.neg(xs[0]);
  xs[3] = f.neg(xs[1]);
  // the records and the Y_k are few and wave-uniform: a local copy keeps them in scalar registers
  u64 krec[K * MPCS_KW], yrec[2 * K];
  const FriTable kr = (FriTable)tab.k, yt = (FriTable)tab.y;
  deep_for<0, K * (int)MPCS_KW>([&](auto J) { krec[decltype(J)::value] = kr[decltype(J)::value]; });
  deep_for<0, 2 * K>([&](auto J) { yrec[decltype(J)::value] = yt[decltype(J)::value]; });
  u64 pre[PTS * K];
  u64 run = f.one();
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int t = decltype(I)::value / K, k = decltype(I)::value % K;
    bool zero;
    const u64 n = deep_norm(f, f.sub(xs[t], krec[k * MPCS_KW]), krec[k * MPCS_KW + 1], zero);
    pre[t * K + k] = run;
    run = f.mul(run, n);
  });
  u64 inv = deep_inverse(x, run);
  E2 G[PTS];
  deep_for<0, PTS>([&](auto T) { G[decltype(T)::value] = x.zero(); });
  deep_for<0, PTS * K>([&](auto I) {
    constexpr int J = PTS * K - 1 - decltype(I)::value, t = J / K, k = J % K, r = k * (int)MPCS_KW;
    bool zero;
    const u64 d = f.sub(xs[t], krec[r]);
    const u64 n = deep_norm(f, d, krec[r + 1], zero);
    u64 ninv = f.mul(inv, pre[J]);
    inv = f.mul(inv, n);
    if (zero) ninv = 0;
    const E2 B{f.add(f.mul(krec[r + 2], d), krec[r + 4]), f.add(f.mul(krec[r + 3], d), krec[r + 5])};   // B_k (d, z1)
    G[t] = x.add(G[t], x.mul_base(x.mul(x.sub(S[t], E2{yrec[2 * k], yrec[2 * k + 1]}), B), ninv));
  });
  deep_for<0, PTS>([&](auto T) { constexpr int t = decltype(T)::value; out[t] = E2{f.out(G[t].c0), f.out(G[t].c1)}; });
}

// ---------------------------------------------------------------------------------------------------- host: the shape
// Fills sh from the arrays of a handle; false for what ronk_mpcs_check refuses (the FRI part aside).
inline bool mpcs_host_shape(u32 K, u32 R, const u32* C, const u32* masks, MpcsShape* sh) {
  if (!C || !masks || !K || !R || K > DEEP_MAX_K || R > MPCS_MAX_R) return false;
  *sh = MpcsShape{};
  sh->R = R; sh->K = K;
  u32 seen = 0;
  u64 ctot = 0, y = 0;
  for (u32 r = 0; r < R; r++) {
    if (!C[r] || !masks[r] || masks[r] >= (1u << K)) return false;
    sh->C[r] = C[r]; sh->mask[r] = masks[r]; sh->off[r] = (u32)ctot; sh->yoff[r] = (u32)y;
    ctot += C[r];
    if (ctot > DEEP_MAX_C) return false;
    y += (u64)mpcs_popcount(masks[r]) * C[r];
    seen |= masks[r];
  }
  if (seen != (1u << K) - 1) return false;
  sh->Ctot = (u32)ctot; sh->Y = (u32)y;
  return true;
}

}  // namespace ronk
