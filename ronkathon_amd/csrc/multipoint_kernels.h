// multipoint_kernels.h -- evaluation of one polynomial at many arbitrary points and interpolation through arbitrary nodes, on
// the product tree of roots_kernels.h (csrc/ronk_multipoint.hip; DESIGN.md "Multipoint evaluation and interpolation").
//
// The reference evaluates point by point (Polynomial::evaluate in Shamir's split, src/shamir/mod.rs:33-60) and interpolates by
// the Lagrange sum (Message::decode, src/codes/reed_solomon.rs:55-107).
//
// Evaluation is the transposed ("middle product") walk down the tree.  A node S of s points carries a window of s words.  With
// A_S(z) = prod_{i in S} (1 - x_i z) = rev(M_S), f padded to D >= M coefficients and W_S = coefficients [D - s, D) of
// rev_{D-1}(f) / A_S -- equivalently the first s coefficients of rev_{s-1}(f mod M_S) / A_S -- the window is stored REVERSED,
// V_S[t] = W_S[s - 1 - t], because then one step down uses the tree's own nodes, not their reversals:
//     V_L = coefficients [s/2, s) of V_S * M_R,      V_R = coefficients [s/2, s) of V_S * M_L.
// V_S * M_R has degree < 3s/2, so in the cyclic product of s points the wrap-around lands below s/2 and the kept half is exact.
// A stored node is its s/2 low coefficients, the leading ONE implicit (roots_kernels.h): V_S * M_R = V_S * low(M_R) + x^(s/2) V_S,
// and `mp_window_elem` adds that second term while it writes the kept halves straight into the children's rows.
// At a leaf (G points) rev(r) = W * A_leaf mod z^G gives r = f mod M_leaf, which every lane evaluates at its own point.
//
// Interpolation walks up once more: with w_i = y_i / Z'(x_i) (Z' evaluated by the walk above on the same tree),
//     N_leaf = sum_i w_i M_leaf / (x - x_i),      N_S = N_L M_R + N_R M_L,
// the pair step on the retained transforms of M_L and M_R; the root is x^pad times the interpolant (the padding roots are ZERO
// and carry the weight ZERO).
//
// Every body is plain C++ over a field policy, so the host emulator (tests/emu/emu_multipoint.cpp) runs the same code on fibers.
#pragma once
#include "roots_kernels.h"

namespace ronk {

// coefficients per LDS chunk of the direct form, and points per workgroup there
constexpr u32 MP_CH = 1024;
constexpr u32 MP_DIRECT_BLOCK = 256;

// The direct form: out[i] = sum_j c[j] x_i^j by Horner, one point per lane, the coefficients staged through LDS in chunks of
// MP_CH (top chunk first) that the workgroup's points share.  O(m d).  lds: MP_CH words.
template <class FLD, class Barrier>
RONK_HD void mp_horner_body(const FLD& f, u64 p, const u64* c, u64 d, const u64* xs, u64 m, u64* out, u64* lds, u32 tid, u64 bid,
                            u32 nthreads, Barrier&& barrier) {
  const u64 idx = bid * nthreads + tid;
  const u64 x = idx < m ? xs[idx] % p : 0;
  u64 acc = 0;
  const u64 chunks = (d + MP_CH - 1) / MP_CH;
  for (u64 ch = chunks; ch-- > 0;) {
    const u64 j0 = ch * MP_CH;
    const u32 len = (u32)(d - j0 < MP_CH ? d - j0 : MP_CH);
    for (u32 j = tid; j < len; j += nthreads) lds[j] = c[j0 + j] % p;
    barrier();
    for (u32 j = len; j-- > 0;) acc = f.add(f.mul_plain(acc, x), lds[j]);
    barrier();
  }
  if (idx < m) out[idx] = acc;
}

// a[k] = z[top - k] % p for k <= top, ZERO above, k < len: the reversal of a coefficient vector (rev(Z) = A_root, rev_{D-1}(f))
RONK_HD void mp_reverse_elem(u64 p, const u64* z, u64 top, u64 have, u64* a, u64 k) {
  a[k] = (k <= top && top - k < have) ? z[top - k] % p : 0;
}

// g = [1, 0, 0, ..]: the precision-1 start of the Newton ladder (A_root(0) = 1)
RONK_HD void mp_one_elem(u64* g, u64 k) { g[k] = k == 0; }

// out[i] = in[i] % p: the O(m^2) interpolation kernels take canonical residues
RONK_HD void mp_reduce_elem(u64 p, const u64* in, u64* out, u64 i) { out[i] = in[i] % p; }

// the status word of the direct interpolation from the flag of the O(m^2) kernels (non-zero: coincident nodes)
RONK_HD int mp_status_code(int flag, int zero_code) { return flag ? zero_code : 0; }

// One step down, element e of the M words of the children's windows (pairs parents of 2d points; child c at vn + c * d):
//   left child (j < d):   vn = pl[row][d + j] + v[row][j]      pl = cyclic V_S * low(M_R)   (the b half's transforms)
//   right child (j >= d): vn = pr[row][j]     + v[row][j - d]  pr = cyclic V_S * low(M_L)   (the a half's transforms)
template <class FLD>
RONK_HD void mp_window_elem(const FLD& f, const u64* v, const u64* pl, const u64* pr, u64 d, u64* vn, u64 e) {
  const u64 row = e / (2 * d) * (2 * d), j = e % (2 * d);
  vn[e] = j < d ? f.add(pl[row + d + j], v[row + j]) : f.add(pr[row + j], v[row + j - d]);
}

// the stored leaf `bid` in the level-0 spread layout (roots_put): half (bid & 1), row (bid >> 1) of 2G words
RONK_HD const u64* mp_leaf_node(const u64* leaves, u64 M, u32 G, u64 bid) { return leaves + (bid & 1) * M + (bid >> 1) * 2 * G; }

// One leaf of the evaluation: workgroup `bid` of G lanes.  Lane n computes r[n] = V[n] + sum_{j=1}^{G-1-n} V[n+j] c[G-j]
// (c: the leaf's low coefficients, read as LDS broadcasts; V at stride 1), the truncated product rev(r) = W * A_leaf mod z^G;
// then lane i runs Horner on r at x_i with r read as broadcasts.  G^2 field products per leaf.  Padding lanes store nothing.
// lds: 3G words.
template <class FLD, class Barrier>
RONK_HD void mp_eval_leaf_body(const FLD& f, u64 p, const u64* v, const u64* leaves, const u64* xs, u64 m, u64 M, u32 G, u64* out,
                               u64* lds, u32 tid, u64 bid, Barrier&& barrier) {
  u64* vv = lds;
  u64* cc = lds + G;
  u64* rr = lds + 2 * G;
  const u64 idx = bid * G + tid;
  vv[tid] = v[idx];
  cc[tid] = mp_leaf_node(leaves, M, G, bid)[tid];
  barrier();
  u64 r = vv[tid];
  for (u32 j = 1; j + tid < G; j++) r = f.add(r, f.mul_plain(vv[tid + j], cc[G - j]));
  rr[tid] = r;
  barrier();
  if (idx >= m) return;
  const u64 x = xs[idx] % p;
  u64 acc = 0;
  for (u32 n = G; n-- > 0;) acc = f.add(f.mul_plain(acc, x), rr[n]);
  out[idx] = acc;
}

// dz[j] = (j + 1) z[j + 1], j < m: the derivative of Z (m + 1 coefficients)
template <class FLD>
RONK_HD void mp_deriv_elem(const FLD& f, u64 p, const u64* z, u64* dz, u64 j) {
  dz[j] = f.mul_plain((j + 1) % p, z[j + 1]);
}

// w[i] = y_i / Z'(x_i) for a chunk of REC_CH points (i >= m: the padding, weight ZERO): prefix products, ONE inversion,
// back-substitution (rec_batch_inv_chunk's scheme).  A ZERO Z'(x_i) -- coincident nodes -- writes `zero_code` to *status.
template <class FLD>
RONK_HD void mp_weights_chunk(const FLD& f, u64 p, const u64* dzx, const u64* ys, u64 m, u64* w, int* status, int zero_code, u64 c) {
  u64 v[REC_CH], pre[REC_CH];
  u64 acc = 1;
  const u64 t0 = c * REC_CH;
  for (u32 t = 0; t < REC_CH; t++) {
    u64 a = t0 + t < m ? dzx[t0 + t] : 1;
    if (a == 0) { *status = zero_code; a = 1; }
    v[t] = a; pre[t] = acc; acc = f.mul_plain(acc, a);
  }
  u64 inv = fld_pow(f, acc, p - 2);
  for (int t = (int)REC_CH - 1; t >= 0; t--) {
    const u64 i = t0 + t;
    w[i] = i < m ? f.mul_plain(f.mul_plain(inv, pre[t]), ys[i] % p) : 0;
    inv = f.mul_plain(inv, v[t]);
  }
}

// where a node of the interpolation goes: the next level's spread layout (as roots_put), or -- at the root -- the caller's m
// coefficients, the x^shift of the padding dropped
struct InterpStore {
  u64* out;
  u64 half;
  int final_;
  u64 shift;
};
RONK_HD void mp_interp_put(const InterpStore& s, u64 i, u64 d, u64 j, u64 v) {
  if (s.final_) {
    if (j >= s.shift) s.out[j - s.shift] = v;
    return;
  }
  u64* o = s.out + (i & 1) * s.half + (i >> 1) * 2 * d;
  o[j] = v;
  o[j + d] = 0;
}

// One leaf of the interpolation: N = sum_i w_i M_leaf / (x - x_i).  Lane i divides M_leaf by (x - x_i) synthetically
// (q_{G-1} = 1, q_{j-1} = c_j + x_i q_j) and leaves w_i q_j in row i of a G x (G + 1) LDS matrix (the odd stride keeps the
// column writes off one bank); lane j then sums column j.  G^2 field products per leaf.  lds: G + G (G + 1) words.
template <class FLD, class Barrier>
RONK_HD void mp_interp_leaf_body(const FLD& f, u64 p, const u64* w, const u64* leaves, const u64* xs, u64 m, u64 M, u32 G,
                                 const InterpStore& st, u64* lds, u32 tid, u64 bid, Barrier&& barrier) {
  u64* cc = lds;
  u64* mat = lds + G;
  const u64 idx = bid * G + tid;
  cc[tid] = mp_leaf_node(leaves, M, G, bid)[tid];
  const u64 x = idx < m ? xs[idx] % p : 0;
  const u64 wi = w[idx];
  barrier();
  u64 q = 1;
  for (u32 j = G; j-- > 0;) {
    mat[(u64)tid * (G + 1) + j] = f.mul_plain(wi, q);
    q = f.add(cc[j], f.mul_plain(x, q));
  }
  barrier();
  u64 acc = 0;
  for (u32 i = 0; i < G; i++) acc = f.add(acc, mat[(u64)i * (G + 1) + tid]);
  mp_interp_put(st, bid, G, tid, acc);
}

// the pointwise step of one level up, element e of the M transform values: x = N_L^ * M_R^ + N_R^ * M_L^
// (fn: the transforms of the spread N halves, a rows then b rows; tk: the retained transforms of the tree's level)
template <class FLD>
RONK_HD void mp_interp_pointwise_elem(const FLD& f, const u64* fn, const u64* tk, u64 M, u64* x, u64 e) {
  x[e] = f.add(f.mul_plain(fn[e], tk[M + e]), f.mul_plain(fn[M + e], tk[e]));
}

// One level's combine, element e = i * 2d + j: the monic terms x^d (N_L + N_R) added to the inverse's output
template <class FLD>
RONK_HD void mp_interp_combine_elem(const FLD& f, const u64* prod, const u64* spread, u64 pairs, u64 d, const InterpStore& st, u64 e) {
  const u64 i = e / (2 * d), j = e % (2 * d);
  u64 v = prod[e];
  if (j >= d) {
    const u64 o = i * 2 * d + (j - d);
    v = f.add(v, f.add(spread[o], spread[pairs * 2 * d + o]));
  }
  mp_interp_put(st, i, 2 * d, j, v);
}

}  // namespace ronk
