// fri_kernels.h -- the bodies of the FRI prover and verifier over the 64-bit fields (csrc/ronk_fri.hip; include/ronk_ntt.h
// "FRI"): the fused split-and-fold of one layer, the Fiat-Shamir transcript on the Poseidon sponge, the
// per-query consistency check and the degree check of the final layer.
//
// One layer of arity A = 2^eta is eta arity-2 folds  f'[i] = (a + b) / 2 + beta (a - b) / (2 x_i),  a = f[i], b = f[i + N/2],
// x_i = s w_N^i, with the challenges beta, beta^2, beta^4.  Output i < m = N / A reads only the coset f[i + t m], t < A, and
// the point of the pair (i + t m, i + t m + N/2) is x_i w_A^t; after a fold the points are squared.  With gamma = beta / x_i
// the steps are therefore
//   step 1   v[t] = (v[t] + v[t + A/2]) + gamma   (v[t] - v[t + A/2]) w_A^-t        t < A/2
//   step 2   v[t] = (v[t] + v[t + A/4]) + gamma^2 (v[t] - v[t + A/4]) w_(A/2)^-t    t < A/4
//   step 3   v[0] = (v[0] + v[1])       + gamma^4 (v[0] - v[1])
// and one multiplication by 2^-eta at the end: A - 1 butterflies, A - 1 + 2 + (eta - 1) products for A inputs.  The in-leaf
// roots are compile-time constants: shifts in Goldilocks (w_8 = -2^24, w_4 = 2^48 under the reference's root convention, as
// is 2^-eta = -2^(96 - eta)), table constants in SGPRs for a Montgomery prime.  1 / x_i = s^-1 w_N^-i comes from a two-level
// table of the layer, hi[i >> k] * lo[i & (2^k - 1)].
//
// Field policies: FriGl keeps canonical words (field_policy.h GlField); FriMont keeps x R mod p (MontField): a word is
// reduced AND converted by the one product with R^2 on the way in, and the final product with the PLAIN constant 2^-eta
// converts back.  Every body takes any 64-bit input word and writes canonical words.
//
// Plain C++ on uint32 / uint64, so tests/emu/emu_fri.cpp compiles the same bodies for the host.
#pragma once
#include "ext2.h"
#include "field_policy.h"
#include "poseidon_kernels.h"

namespace ronk {

// what a launch knows about the field (kernel argument: SGPRs).  fc.p == 0: Goldilocks with shift roots.
struct FriConsts {
  FieldConst fc;   // fc.w16[J * (16 / A)] = w_A^-J R mod p (Montgomery only)
  u64 fin;         // 2^-eta mod p, plain (Montgomery only)
};

// one committed layer: the inverse-point table and where its openings sit in the proof
struct FriLayer {
  const u64* hi;   // s_l^-1 w^-(j 2^kbits), register form, 2^(log2m - kbits) entries
  const u64* lo;   // w^-j, register form, 2^kbits entries
  u32 kbits, log2m;   // m = N_l / A leaves
  u64 leaf_off, path_off;   // word offsets in the proof: [Q][A] leaf values, [Q][log2m][D] paths
};

// a layer's tables are in global memory even where the pointer itself was loaded from memory (the verifier's layer array):
// saying so keeps those loads global ones instead of flat ones
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) u64* FriTable;
#else
typedef const u64* FriTable;
#endif

struct FriGl {
  GlField f;
  RONK_HD explicit FriGl(const FriConsts&) {}
  RONK_HD u64 in(u64 x) const { return gl64::canon(x); }
  RONK_HD u64 out(u64 x) const { return x; }
  RONK_HD u64 add(u64 a, u64 b) const { return gl64::add(a, b); }
  RONK_HD u64 sub(u64 a, u64 b) const { return gl64::sub(a, b); }
  RONK_HD u64 neg(u64 a) const { return gl64::neg(a); }
  RONK_HD u64 mul(u64 a, u64 b) const { return gl64::mul(a, b); }
  RONK_HD u64 mul_w(u64 a, u64 w) const { return gl64::mul(a, w); }   // the extension's product with W (ext2.h)
  RONK_HD u64 one() const { return 1; }
  RONK_HD u64 order() const { return gl64::P; }
  template <int N, int J>
  RONK_HD u64 sub_root(u64 a, u64 b) const { return f.template sub_mul_root<N, J, true>(a, b); }   // (a - b) w_N^-J
  template <int ETA>
  RONK_HD u64 fin(u64 x) const { return gl64::mul_2exp_neg<96 - ETA>(x); }   // 2^-eta = 2^(192 - eta) = -2^(96 - eta)
};

// FriGl for the extension with W = 7: the product with W is 8 x - x, a shift and a subtraction (fewer
// VALU instructions in the fold's listing than the ordinary product)
struct FriGlW7 : FriGl {
  RONK_HD explicit FriGlW7(const FriConsts& k) : FriGl(k) {}
  RONK_HD u64 mul_w(u64 a, u64) const { return gl64::sub(gl64::mul_2exp<3>(a), a); }
};

struct FriMont {
  MontField f;
  u64 finc;
  RONK_HD explicit FriMont(const FriConsts& k) : f(k.fc), finc(k.fin) {}
  RONK_HD u64 in(u64 x) const { return mont64::mmul(f.f, x, f.f.r2); }   // any 64-bit x -> x R mod p
  RONK_HD u64 out(u64 x) const { return mont64::from_mont(f.f, x); }
  RONK_HD u64 add(u64 a, u64 b) const { return f.add(a, b); }
  RONK_HD u64 sub(u64 a, u64 b) const { return f.sub(a, b); }
  RONK_HD u64 neg(u64 a) const { return mont64::neg(f.f, a); }
  RONK_HD u64 mul(u64 a, u64 b) const { return f.mul(a, b); }
  RONK_HD u64 mul_w(u64 a, u64 w) const { return f.mul(a, w); }
  RONK_HD u64 one() const { return f.f.one; }
  RONK_HD u64 order() const { return f.f.p; }
  template <int N, int J>
  RONK_HD u64 sub_root(u64 a, u64 b) const { return f.template sub_mul_root<N, J, true>(a, b); }
  template <int ETA>
  RONK_HD u64 fin(u64 x) const { return mont64::mmul(f.f, x, finc); }   // x R * 2^-eta * R^-1: plain and canonical
};

// ---------------------------------------------------------------------------------------------------- fold
// What a layer's values are.  FriWord: base words, multiplier a base word (the base form).  FriPair: pairs of the quadratic
// extension (ext2.h), multiplier a pair; the in-leaf roots and 2^-eta stay base-field values and act on each component.
template <class F>
struct FriWord {
  typedef u64 V;
  const F& f;
  RONK_HD explicit FriWord(const F& base) : f(base) {}
  RONK_HD u64 add(u64 a, u64 b) const { return f.add(a, b); }
  RONK_HD u64 mul(u64 a, u64 g) const { return f.mul(a, g); }
  RONK_HD u64 sqr(u64 g) const { return f.mul(g, g); }
  template <int N, int J>
  RONK_HD u64 sub_root(u64 a, u64 b) const { return f.template sub_root<N, J>(a, b); }
  template <int ETA>
  RONK_HD u64 fin(u64 a) const { return f.template fin<ETA>(a); }
};
template <class F>
struct FriPair {
  typedef E2 V;
  const Ext2<F>& x;
  RONK_HD explicit FriPair(const Ext2<F>& ext) : x(ext) {}
  RONK_HD E2 add(E2 a, E2 b) const { return x.add(a, b); }
  RONK_HD E2 mul(E2 a, E2 g) const { return x.mul(a, g); }
  RONK_HD E2 sqr(E2 g) const { return x.sqr(g); }
  template <int N, int J>
  RONK_HD E2 sub_root(E2 a, E2 b) const {
    return E2{x.f.template sub_root<N, J>(a.c0, b.c0), x.f.template sub_root<N, J>(a.c1, b.c1)};
  }
  template <int ETA>
  RONK_HD E2 fin(E2 a) const { return E2{x.f.template fin<ETA>(a.c0), x.f.template fin<ETA>(a.c1)}; }
};

// the butterflies (T - 1, T - 1 + H), ..., (0, H) of one step with multiplier gm
template <class O, int H, int T>
struct FriStep {
  typedef typename O::V V;
  static RONK_HD void run(const O& o, V* v, V gm) {
    FriStep<O, H, T - 1>::run(o, v, gm);
    const V a = v[T - 1], b = v[T - 1 + H];
    v[T - 1] = o.add(o.add(a, b), o.mul(o.template sub_root<2 * H, T - 1>(a, b), gm));
  }
};
template <class O, int H>
struct FriStep<O, H, 0> {
  static RONK_HD void run(const O&, typename O::V*, typename O::V) {}
};
// the first step of an extension fold over BASE values: (a + b) + gamma ((a - b) w^-t) with a base difference is a product of
// a pair by a base element, two base products instead of three and no product with W
template <class F, int H, int T>
struct FriMixStep {
  static RONK_HD void run(const F& f, const u64* b, E2* v, E2 gm) {
    FriMixStep<F, H, T - 1>::run(f, b, v, gm);
    const u64 d = f.template sub_root<2 * H, T - 1>(b[T - 1], b[T - 1 + H]);
    v[T - 1] = E2{f.add(f.add(b[T - 1], b[T - 1 + H]), f.mul(d, gm.c0)), f.mul(d, gm.c1)};
  }
};
template <class F, int H>
struct FriMixStep<F, H, 0> {
  static RONK_HD void run(const F&, const u64*, E2*, E2) {}
};

// the steps from butterfly distance H0 = 2^(ETA0 - 1) down to 1 on values already in register form; v[0] is the result before
// the product with 2^-eta
template <class O, int ETA0>
RONK_HD void fri_fold_steps(const O& o, typename O::V* v, typename O::V gm) {
  if constexpr (ETA0 >= 3) { FriStep<O, 4, 4>::run(o, v, gm); gm = o.sqr(gm); }
  if constexpr (ETA0 >= 2) { FriStep<O, 2, 2>::run(o, v, gm); gm = o.sqr(gm); }
  if constexpr (ETA0 >= 1) FriStep<O, 1, 1>::run(o, v, gm);
}

// one output of a layer from its coset: load(t) = word t of the leaf (any 64-bit value), gamma = beta / x_i in register form;
// returns the canonical word
template <class F, int ETA, class Load>
RONK_HD u64 fri_fold_leaf(const F& f, u64 gamma, Load&& load) {
  constexpr int A = 1 << ETA;
  u64 v[A];
#pragma unroll
  for (int t = 0; t < A; t++) v[t] = f.in(load(t));
  const FriWord<F> o(f);
  fri_fold_steps<FriWord<F>, ETA>(o, v, gamma);
  return o.template fin<ETA>(v[0]);
}

// the same with the challenge, and so every folded value, in the quadratic extension: gamma = beta / x_i is a pair in register
// form.  EXT_IN: the leaf is 2 A words, load(c * A + t) = component c of value t (a planar layer); else A base words embedded
// as (x, 0), and the first step is the mixed one.  Returns the canonical pair.
template <class F, int ETA, bool EXT_IN, class Load>
RONK_HD E2 fri_fold_leaf_ext(const Ext2<F>& x, E2 gamma, Load&& load) {
  constexpr int A = 1 << ETA;
  const FriPair<F> o(x);
  E2 v[A];
  if constexpr (EXT_IN) {
#pragma unroll
    for (int t = 0; t < A; t++) v[t] = E2{x.f.in(load(t)), x.f.in(load(A + t))};
    fri_fold_steps<FriPair<F>, ETA>(o, v, gamma);
  } else {
    u64 b[A];
#pragma unroll
    for (int t = 0; t < A; t++) b[t] = x.f.in(load(t));
    FriMixStep<F, A / 2, A / 2>::run(x.f, b, v, gamma);
    fri_fold_steps<FriPair<F>, ETA - 1>(o, v, x.sqr(gamma));
  }
  return o.template fin<ETA>(v[0]);
}

// beta / x_i for leaf i < 2^log2m of a layer, beta in register form
template <class F>
RONK_HD u64 fri_gamma(const F& f, const FriLayer& ly, u64 i, u64 beta) {
  const FriTable hi = (FriTable)ly.hi, lo = (FriTable)ly.lo;
  const u64 xinv = f.mul(hi[i >> ly.kbits], lo[i & (((u64)1 << ly.kbits) - 1)]);
  return f.mul(xinv, beta);
}
// the same for a challenge in the extension: 1 / x_i is a base element
template <class F>
RONK_HD E2 fri_gamma_ext(const Ext2<F>& x, const FriLayer& ly, u64 i, E2 beta) {
  const FriTable hi = (FriTable)ly.hi, lo = (FriTable)ly.lo;
  return x.mul_base(beta, x.f.mul(hi[i >> ly.kbits], lo[i & (((u64)1 << ly.kbits) - 1)]));
}

// ---------------------------------------------------------------------------------------------------- transcript
// t = sponge(c || root) squeezing d words: beta = t[0], the next chain value = t
template <class PF, int W>
RONK_HD void fri_chain_step(const PF& pf, const PoseidonConsts& k, u32 d, const u64* c, const u64* root, u64* t) {
  poseidon_sponge<PF, W>(pf, k, 2 * (u64)d, d, [&](u64 j) { return j < d ? c[j] : root[j - d]; }, [&](u64 q, u64 v) { t[q] = v; });
}
// u = sponge(c || final values) squeezing d words
template <class PF, int W>
RONK_HD void fri_chain_final(const PF& pf, const PoseidonConsts& k, u32 d, const u64* c, const u64* fin, u64 nl, u64* u) {
  poseidon_sponge<PF, W>(pf, k, d + nl, d, [&](u64 j) { return j < d ? c[j] : fin[j - d]; }, [&](u64 q, u64 v) { u[q] = v; });
}
// the first word of sponge(u || [q])
template <class PF, int W>
RONK_HD u64 fri_query_word(const PF& pf, const PoseidonConsts& k, u32 d, const u64* u, u64 q) {
  u64 r = 0;
  poseidon_sponge<PF, W>(pf, k, (u64)d + 1, 1, [&](u64 j) { return j < d ? u[j] : q; }, [&](u64, u64 v) { r = v; });
  return r;
}
// The whole chain for the layers [l0, l1): chain[0 .. d) = seed (l0 == 0), chain[(l + 1) d ..] = sponge(chain[l d ..] ||
// roots[l d ..]), betas[l] = its first word; with `fin` (after the last layer, l1 == n_layers) also u.  One lane.
// Extension challenges (bw == 2): betas[2 l], betas[2 l + 1] = its first two words, and `fin` is both planes, nl = 2 N_L words.
template <class PF, int W>
RONK_HD void fri_transcript(const PF& pf, const PoseidonConsts& k, u32 d, const u64* seed, u64* chain, const u64* roots, u32 l0, u32 l1,
                            u64* betas, const u64* fin, u64 nl, u64* u, u32 bw = 1) {
  if (l0 == 0)
    for (u32 j = 0; j < d; j++) chain[j] = seed[j];
  for (u32 l = l0; l < l1; l++) {
    fri_chain_step<PF, W>(pf, k, d, chain + (u64)l * d, roots + (u64)l * d, chain + (u64)(l + 1) * d);
    for (u32 b = 0; b < bw; b++) betas[(u64)l * bw + b] = chain[(u64)(l + 1) * d + b];
  }
  if (fin) fri_chain_final<PF, W>(pf, k, d, chain + (u64)l1 * d, fin, nl, u);
}
// query q: j_0 = word & (m_0 - 1), and the leaf index of every layer, idx[l * n_queries + q] = j_0 mod m_l
template <class PF, int W>
RONK_HD void fri_query_indices(const PF& pf, const PoseidonConsts& k, u32 d, const u64* u, const FriLayer* layers, u32 n_layers,
                               u64 n_queries, u64 q, u64* idx) {
  const u64 j0 = fri_query_word<PF, W>(pf, k, d, u, q) & (((u64)1 << layers[0].log2m) - 1);
  for (u32 l = 0; l < n_layers; l++) idx[(u64)l * n_queries + q] = j0 & (((u64)1 << layers[l].log2m) - 1);
}

// ---------------------------------------------------------------------------------------------------- verifier
// Query q: the fold of the opened leaf of layer l must be slot j_l div m_(l+1) of the opened leaf of layer l + 1, and the word
// final[j_(L-1)] after the last committed layer.  The compared words are taken as they stand in the proof: a word >= p never
// equals a folded value.  Returns 1 when every layer is consistent.
template <class F, int ETA>
RONK_HD int fri_check_query(const F& f, const FriLayer* layers, u32 n_layers, u64 n_queries, const u64* proof, u64 final_off,
                            const u64* betas, const u64* idx, u64 q) {
  constexpr int A = 1 << ETA;
  int ok = 1;
  for (u32 l = 0; l < n_layers; l++) {
    const FriLayer ly = layers[l];
    const u64 j = idx[(u64)l * n_queries + q];
    const u64* leaf = proof + ly.leaf_off + q * A;
    const u64 got = fri_fold_leaf<F, ETA>(f, fri_gamma(f, ly, j, f.in(betas[l])), [&](int t) { return leaf[t]; });
    u64 want;
    if (l + 1 < n_layers) {
      const FriLayer nx = layers[l + 1];
      want = proof[nx.leaf_off + q * A + (j >> nx.log2m)];
    } else {
      want = proof[final_off + j];
    }
    ok &= got == want;
  }
  return ok;
}

// The same with extension challenges (include/ronk_ntt.h, "FRI with extension challenges"): a planar leaf is 2 A words, c0 values
// then c1 values; layer 0 is A base words unless in_ext.  The fold must equal the words at slots s and A + s of the next leaf,
// s = j_l div m_(l+1), and (final[j], final[N_L + j]) at the end.
template <class F, int ETA>
RONK_HD int fri_check_query_ext(const Ext2<F>& x, const FriLayer* layers, u32 n_layers, u64 n_queries, const u64* proof, u64 final_off,
                                u64 nl, bool in_ext, const u64* betas, const u64* idx, u64 q) {
  constexpr int A = 1 << ETA;
  int ok = 1;
  for (u32 l = 0; l < n_layers; l++) {
    const FriLayer ly = layers[l];
    const u64 j = idx[(u64)l * n_queries + q];
    const E2 gamma = fri_gamma_ext(x, ly, j, E2{x.f.in(betas[2 * l]), x.f.in(betas[2 * l + 1])});
    E2 got;
    if (l == 0 && !in_ext) {
      const u64* leaf = proof + ly.leaf_off + q * A;
      got = fri_fold_leaf_ext<F, ETA, false>(x, gamma, [&](int t) { return leaf[t]; });
    } else {
      const u64* leaf = proof + ly.leaf_off + q * 2 * A;
      got = fri_fold_leaf_ext<F, ETA, true>(x, gamma, [&](int t) { return leaf[t]; });
    }
    E2 want;
    if (l + 1 < n_layers) {
      const FriLayer nx = layers[l + 1];
      const u64* nleaf = proof + nx.leaf_off + q * 2 * A;
      want = E2{nleaf[j >> nx.log2m], nleaf[A + (j >> nx.log2m)]};
    } else {
      want = E2{proof[final_off + j], proof[final_off + nl + j]};
    }
    ok &= (got.c0 == want.c0) & (got.c1 == want.c1);
  }
  return ok;
}

// Coefficient k of the interpolant of the final layer, up to the non-zero factor s^-k / n: sum_i final[i] w^-(i k).
// wtab[j] = w^-j in register form, n a power of two; the result is zero exactly when the coefficient is.
template <class F>
RONK_HD u64 fri_final_coeff(const F& f, const u64* wtab, const u64* fin, u32 n, u32 k) {
  u64 acc = 0;
  for (u32 i = 0; i < n; i++) acc = f.add(acc, f.mul(f.in(fin[i]), wtab[(i * k) & (n - 1)]));
  return acc;
}

// ---------------------------------------------------------------------------------------------------- host: sizes and tables
struct FriShape {
  u32 n, eta, log2_final, layers;   // layers = (n - log2_final) / eta committed layers
  u64 queries, d;
  u32 ext = 0, in_ext = 0;          // extension challenges (layers 1 .. L planar pairs); layer 0 planar pairs too
  u64 size(u32 l) const { return (u64)1 << (n - eta * l); }          // N_l
  u64 vw(u32 l) const { return ext && (l > 0 || in_ext) ? 2 : 1; }   // words per value of layer l
  u64 leaf_len(u32 l) const { return vw(l) << eta; }
  u32 log2m(u32 l) const { return n - eta * (l + 1); }               // leaves of layer l = 2^log2m
  u64 tree_words(u32 l) const { return (((u64)2 << log2m(l)) - 1) * d; }
  u64 leaf_off(u32 l) const {
    u64 off = layers * d + vw(layers) * size(layers);
    for (u32 t = 0; t < l; t++) off += queries * leaf_len(t) + queries * log2m(t) * d;
    return off;
  }
  u64 path_off(u32 l) const { return leaf_off(l) + queries * leaf_len(l); }
  u64 proof_words() const { return leaf_off(layers); }
  // the transcript's and the openings' small state: betas [L] ([L][2] in the extension), chain [(L + 1) d], u [d], leaf indices
  // [L][Q], open status [Q]
  u64 small_words() const { return (ext ? 2 : 1) * layers + (layers + 2) * d + layers * queries + queries; }
  u64 idx_off() const { return (ext ? 2 : 1) * layers + (layers + 2) * d; }   // the leaf indices inside that state; layer 0 first
  // folded layers 1 .. L, the trees of layers 0 .. L - 1, the small state
  u64 workspace_words() const {
    u64 w = small_words();
    for (u32 l = 0; l < layers; l++) w += vw(l + 1) * size(l + 1) + tree_words(l);
    return w;
  }
};

inline u64 fri_mulmod(u64 a, u64 b, u64 p) { return (u64)(((unsigned __int128)a * b) % p); }
inline u64 fri_powmod(u64 a, u64 e, u64 p) {
  u64 r = 1 % p;
  a %= p;
  while (e) { if (e & 1) r = fri_mulmod(r, a, p); a = fri_mulmod(a, a, p); e >>= 1; }
  return r;
}
inline u64 fri_reg_form(bool mont, u64 p, u64 c) { return mont ? (u64)((((unsigned __int128)c) << 64) % p) : c; }
// the shift roots hold when w_A is the power of two GlField assumes (the reference's root convention under g = 7)
inline bool fri_gl_shift_roots(u64 p, u64 g, u32 eta) {
  if (p != gl64::P) return false;
  const int a = 1 << eta;
  return fri_powmod(g, (p - 1) / a, p) == fri_powmod(2, root_exp(a, 1, false), p);
}
inline FriConsts fri_host_consts(bool mont, u64 p, u64 g, u32 eta) {
  FriConsts k{};
  if (!mont) return k;
  const mont64::Field mf = mont64::make_field(p);
  k.fc.p = p; k.fc.pinv = mf.pinv; k.fc.r2 = mf.r2;
  const u32 a = 1u << eta;
  const u64 wa_inv = fri_powmod(fri_powmod(g, (p - 1) / a, p), p - 2, p);
  for (u32 j = 0; j < 8; j++) k.fc.w16[j] = mf.one;
  for (u32 j = 0; j * (16 / a) < 8; j++) k.fc.w16[j * (16 / a)] = fri_reg_form(true, p, fri_powmod(wa_inv, j, p));
  k.fin = fri_powmod(fri_powmod(2, eta, p), p - 2, p);
  return k;
}
inline u32 fri_kbits(u32 log2m) { return (log2m + 1) / 2; }
// the inverse-point table of layer l: lo (2^kbits words) then hi (2^(log2m - kbits) words), register form
inline void fri_host_layer_table(bool mont, u64 p, u64 g, u64 shift, const FriShape& sh, u32 l, u64* lo, u64* hi) {
  const u32 lm = sh.log2m(l), kb = fri_kbits(lm);
  u64 s = shift % p;
  for (u32 t = 0; t < sh.eta * l; t++) s = fri_mulmod(s, s, p);   // s^(A^l)
  const u64 sinv = fri_powmod(s, p - 2, p);
  const u64 winv = fri_powmod(fri_powmod(g, (p - 1) / sh.size(l), p), p - 2, p);
  u64 x = 1 % p;
  for (u64 j = 0; j < ((u64)1 << kb); j++) { lo[j] = fri_reg_form(mont, p, x); x = fri_mulmod(x, winv, p); }
  const u64 step = x;   // winv^(2^kb)
  x = sinv;
  for (u64 j = 0; j < ((u64)1 << (lm - kb)); j++) { hi[j] = fri_reg_form(mont, p, x); x = fri_mulmod(x, step, p); }
}
// w^-j of the final layer's domain, j < 2^log2_final, register form
inline void fri_host_final_table(bool mont, u64 p, u64 g, const FriShape& sh, u64* wtab) {
  const u64 nl = sh.size(sh.layers);
  const u64 winv = fri_powmod(fri_powmod(g, (p - 1) / nl, p), p - 2, p);
  u64 x = 1 % p;
  for (u64 j = 0; j < nl; j++) { wtab[j] = fri_reg_form(mont, p, x); x = fri_mulmod(x, winv, p); }
}
}  // namespace ronk
