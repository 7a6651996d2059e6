// plonk_kernels.h -- the bodies of the fused PLONK quotient on the evaluation coset (csrc/ronk_plonk.hip; include/ronk_ntt.h
// "PLONK quotient").  On the coset x_i = s w_M^i, i < M = N B, with every column already extended:
//
//   G_i  = a ql + b qr + a b qm + o qo + qc + pi                                                   (base field)
//   P1_i = Z_i prod_c (w_c + beta k_c x_i + gamma) - Z_((i + B) mod M) prod_c (w_c + beta sigma_c + gamma)
//   T_i  = (G_i + alpha P1_i) / (x_i^N - 1) + alpha^2 (Z_i - 1) / (N (x_i - 1))
//
// The last term is alpha^2 P2_i / (x_i^N - 1) with P2 = (Z - 1) L1 and L1(x) = (x^N - 1) / (N (x - 1)): L1 itself is never formed.
// x_i^N - 1 = s^N w_B^(i mod B) - 1 takes B values; their inverses are a table of the handle (register form).  What is left to
// invert per row is the BASE element x_i - 1: a lane owns PTS rows at stride M / PTS (deep_kernels.h: x of the other rows is a
// product by a fourth or an eighth root of unity, every load of a wavefront is contiguous), multiplies the PTS differences up,
// inverts ONCE with deep_inverse and unwinds with Montgomery's trick.  ronk_plonk_check refuses s^M = 1, so no difference and no
// vanishing value is zero and there is no status word.
//
// The identity labels k_c x_i are generated here, from the two-level point table (DeepDomain).  sigma words are raw and meet beta
// in deep_apx form; the wires, selectors, pi and Z go through f.in.  Field policies and forms are those of fri_kernels.h.  Plain
// C++ on uint64, so tests/emu/emu_plonk.cpp compiles the same bodies for the host.
#pragma once
#include "deep_kernels.h"

namespace ronk {

// Rows per lane, at stride M / rows: 4 over Goldilocks, 8 over a Montgomery prime, whose Fermat power is a plain square-and-multiply
// (about 125 products where the Goldilocks chain takes 74) and whose rows need fewer registers; both forms run at 4 wavefronts per
// SIMD.  Below that many rows a lane owns one.
template <class F>
struct PlonkRows { static constexpr u32 LOG2 = 2; };
template <>
struct PlonkRows<FriMont> { static constexpr u32 LOG2 = 3; };
constexpr u32 PLONK_LANES = 256;
constexpr u32 PLONK_MAX_LOG2M = 28;

// what the handle knows beside the domain, register form
struct PlonkTab {
  const u64* vinv;   // [B]: 1 / (s^N w_B^j - 1)
  u32 log2b;
  u64 ninv;          // 1 / N
  u64 rho;           // w_M^(M / 8), the eighth root of unity: x_(i + t M/8) = x_i rho^t (with rho^2 = the domain's iota)
  u64 k[3];          // the label multipliers
};

// the arrays of a call
struct PlonkCols {
  const u64* wires;   // [3][M]
  const u64* sel;     // [5][M]: ql, qr, qm, qo, qc
  const u64* sigma;   // [3][M]
  const u64* pi;      // [M] or NULL
  const u64* Z;       // planar [2][M]
  const u64* alpha;
  const u64* beta;
  const u64* gamma;
};

// the challenges as a row uses them: wave-uniform, computed once per lane
struct PlonkChal {
  E2 alpha, gamma;
  E2 a2n;      // alpha^2 / N
  E2 bx;       // beta in deep_apx form: times a RAW sigma word
  E2 bk[3];    // beta k_c: times x_i
};
template <class F>
RONK_HD PlonkChal plonk_challenges(const Ext2<F>& x, const PlonkTab& tab, const u64* alpha, const u64* beta, const u64* gamma) {
  const F& f = x.f;
  PlonkChal ch;
  ch.alpha = E2{f.in(alpha[0]), f.in(alpha[1])};
  ch.gamma = E2{f.in(gamma[0]), f.in(gamma[1])};
  const E2 b{f.in(beta[0]), f.in(beta[1])};
  ch.a2n = x.mul_base(x.sqr(ch.alpha), tab.ninv);
  ch.bx = E2{deep_apx(f, b.c0), deep_apx(f, b.c1)};
  deep_for<0, 3>([&](auto C) { constexpr int c = decltype(C)::value; ch.bk[c] = x.mul_base(b, tab.k[c]); });
  return ch;
}

// the words of one row as they lie in memory
struct PlonkRow {
  u64 w[3], q[5], s[3], pi;
  E2 Z, Zn;   // Z at the row and at row (i + B) mod M
};
template <class Cols>
RONK_HD PlonkRow plonk_load_row(const Cols& c, u64 M, u64 B, u64 i) {
  PlonkRow r;
  const u64 in = (i + B) & (M - 1);
  deep_for<0, 3>([&](auto J) { constexpr int j = decltype(J)::value; r.w[j] = c.wires[(u64)j * M + i]; r.s[j] = c.sigma[(u64)j * M + i]; });
  deep_for<0, 5>([&](auto J) { constexpr int j = decltype(J)::value; r.q[j] = c.sel[(u64)j * M + i]; });
  r.pi = c.pi ? c.pi[i] : 0;
  r.Z = E2{c.Z[i], c.Z[M + i]};
  r.Zn = E2{c.Z[in], c.Z[M + in]};
  return r;
}

// T at one row: xi the point, dinv = 1 / (xi - 1), vinv = 1 / (xi^N - 1), all in register form.  Returns register form.
template <class F>
RONK_HD E2 plonk_row(const Ext2<F>& x, const PlonkChal& ch, const PlonkRow& r, u64 xi, u64 dinv, u64 vinv) {
  const F& f = x.f;
  const u64 a = f.in(r.w[0]), b = f.in(r.w[1]), o = f.in(r.w[2]);
  u64 gate = f.add(f.mul(a, f.in(r.q[0])), f.mul(b, f.in(r.q[1])));
  gate = f.add(gate, f.mul(f.mul(a, b), f.in(r.q[2])));
  gate = f.add(gate, f.mul(o, f.in(r.q[3])));
  gate = f.add(gate, f.add(f.in(r.q[4]), f.in(r.pi)));
  const E2 Z{f.in(r.Z.c0), f.in(r.Z.c1)};
  E2 num = Z, den{f.in(r.Zn.c0), f.in(r.Zn.c1)};
  const u64 wv[3] = {a, b, o};
  deep_for<0, 3>([&](auto C) {
    constexpr int c = decltype(C)::value;
    const u64 wg = f.add(wv[c], ch.gamma.c0);
    num = x.mul(num, E2{f.add(wg, f.mul(xi, ch.bk[c].c0)), f.add(ch.gamma.c1, f.mul(xi, ch.bk[c].c1))});
    den = x.mul(den, E2{f.add(wg, f.mul(r.s[c], ch.bx.c0)), f.add(ch.gamma.c1, f.mul(r.s[c], ch.bx.c1))});
  });
  E2 t = x.mul(ch.alpha, x.sub(num, den));
  t = x.mul_base(E2{f.add(t.c0, gate), t.c1}, vinv);
  const E2 p2 = x.mul(ch.a2n, x.mul_base(E2{f.sub(Z.c0, f.one()), Z.c1}, dinv));
  return x.add(t, p2);
}

// The lane that owns the rows i + t q, t < PTS (q = M / PTS; PTS = 8 or 4, or 1 with q unused): load(row) = the PlonkRow of a
// row, store(row, T) takes the canonical pair.
template <class F, int PTS, class Load, class Store>
RONK_HD void plonk_lane(const Ext2<F>& x, const DeepDomain& dm, const PlonkTab& tab, const PlonkChal& ch, u64 i, Load&& load,
                        Store&& store) {
  static_assert(PTS == 1 || PTS == 4 || PTS == 8, "a lane owns one row, or the rows x rho^t of an eighth or a fourth root rho");
  const F& f = x.f;
  const u64 q = ((u64)1 << dm.log2n) / PTS, bmask = ((u64)1 << tab.log2b) - 1;
  const FriTable vinv = (FriTable)tab.vinv;
  u64 xs[PTS], pre[PTS];
  xs[0] = deep_point(f, dm, i);
  if constexpr (PTS == 4) {
    xs[1] = f.mul(xs[0], dm.iota);
    xs[2] = f.neg(xs[0]);
    xs[3] = f.neg(xs[1]);
  }
  if constexpr (PTS == 8) {
    xs[1] = f.mul(xs[0], tab.rho);
    xs[2] = f.mul(xs[0], dm.iota);
    xs[3] = f.mul(xs[1], dm.iota);
    deep_for<0, 4>([&](auto J) { constexpr int j = decltype(J)::value; xs[4 + j] = f.neg(xs[j]); });
  }
  u64 run = f.one();
  deep_for<0, PTS>([&](auto T) {
    constexpr int t = decltype(T)::value;
    pre[t] = run;
    run = f.mul(run, f.sub(xs[t], f.one()));
  });
  u64 inv = deep_inverse(x, run);
  deep_for<0, PTS>([&](auto T) {
    constexpr int t = PTS - 1 - decltype(T)::value;
    const u64 row = i + (u64)t * q;
    const u64 dinv = f.mul(inv, pre[t]);
    inv = f.mul(inv, f.sub(xs[t], f.one()));
    const E2 v = plonk_row(x, ch, load(row), xs[t], dinv, vinv[row & bmask]);
    store(row, E2{f.out(v.c0), f.out(v.c1)});
  });
}

// ---------------------------------------------------------------------------------------------------- host: the handle's tables
// vinv[j] = 1 / (s^N w_B^j - 1), j < B, register form: the B products up, one power, and back
inline void plonk_host_vanishing(bool mont, u64 p, u64 g, u64 shift, u32 log2n, u32 log2b, u64* vinv) {
  const u64 B = (u64)1 << log2b;
  const u64 wb = fri_powmod(g, (p - 1) >> log2b, p);
  u64 sn = shift % p;
  for (u32 j = 0; j < log2n; j++) sn = fri_mulmod(sn, sn, p);
  u64 run = 1 % p, v = sn;
  for (u64 j = 0; j < B; j++) {       // vinv[j] holds the prefix product on the way up
    vinv[j] = run;
    run = fri_mulmod(run, (v ? v - 1 : p - 1), p);
    v = fri_mulmod(v, wb, p);
  }
  u64 inv = fri_powmod(run, p - 2, p);
  const u64 wbinv = fri_powmod(wb, p - 2, p);
  for (u64 j = B; j-- > 0;) {
    v = fri_mulmod(v, wbinv, p);      // s^N w_B^j
    const u64 one = fri_mulmod(inv, vinv[j], p);
    inv = fri_mulmod(inv, (v ? v - 1 : p - 1), p);
    vinv[j] = fri_reg_form(mont, p, one);
  }
}

#if defined(__HIPCC__)
// one lane per PTS rows i + t M / PTS: adjacent lanes read adjacent words of every column and write adjacent words of both planes
template <class F, int PTS>
__global__ void __launch_bounds__(PLONK_LANES) plonk_quotient_kernel(FriConsts k, u64 w, DeepDomain dm, PlonkTab tab, PlonkCols cols,
                                                                     u64* __restrict__ T) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 M = (u64)1 << dm.log2n, q = M / PTS;
  const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= q) return;
  const PlonkChal ch = plonk_challenges(x, tab, cols.alpha, cols.beta, cols.gamma);
  plonk_lane<F, PTS>(x, dm, tab, ch, i, [&](u64 row) { return plonk_load_row(cols, M, (u64)1 << tab.log2b, row); },
                     [&](u64 row, E2 v) { T[row] = v.c0; T[M + row] = v.c1; });
}
#endif

}  // namespace ronk
