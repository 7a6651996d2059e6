// roots_kernels.h -- the product of linear factors Z(x) = prod_i (x - r_i) as a product tree, and the element-wise steps of
// Reed-Solomon erasure recovery (csrc/ronk_recover.hip; DESIGN.md "Erasure recovery and the product tree").
//
// The reference computes Z in two places: Message::decode's x_combinations are the elementary symmetric polynomials of the nodes
// (src/codes/reed_solomon.rs:54-106), and Lagrange::evaluate folds by prod (x - x_i) (src/polynomial/mod.rs:382-415).
//
// Layout.  A node of degree d is stored as its d LOW coefficients; the leading ONE is implicit.  For a pair (a, b)
//     (x^d + a)(x^d + b) = a*b + x^d (a + b) + x^2d,
// and a*b has degree <= 2d - 2, so a cyclic product of 2d points does not wrap.  A level of the tree keeps its `count` nodes
// SPREAD for the next product: node i lives in half (i & 1) -- the a's first, then the b's -- at row (i >> 1), each row 2d
// words long, the node's d coefficients followed by d zeros.  One level is then: forward NTTs of both halves (batched plans of
// 2d points), the inverse of the first half with the second multiplied on load (the tile kernels' fused pointwise product,
// TileArgs::in2), and `roots_combine_elem`, which adds a + b at offset d and writes the product straight into the next
// level's spread layout.  The leaves (`roots_leaf_body`) build G = 2^L factors per workgroup by c <- c * (x - r).
//
// Every body is plain C++ over a field policy (field_policy.h), so the host emulator (tests/emu/emu_roots.cpp) runs the same
// code on fibers.  All values are canonical residues.
#pragma once
#include "field_policy.h"

namespace ronk {

// where a finished node goes: the next level's spread layout, or -- at the root -- the caller's m + 1 coefficients
// (the tree ran on m roots padded with `shift` zero roots, so it built x^shift * Z: Z is its coefficients moved down by shift)
struct RootsStore {
  u64* out;
  u64 half;    // spread: offset of the b half (count / 2 rows of 2d)
  int final_;  // 1: out[j - shift] for j >= shift, out[m] = ONE
  u64 shift, m;
};

RONK_HD void roots_put(const RootsStore& s, u64 i, u64 d, u64 j, u64 v) {
  if (s.final_) {
    if (j >= s.shift) s.out[j - s.shift] = v;
    if (j == 0) s.out[s.m] = 1;
    return;
  }
  u64* o = s.out + (i & 1) * s.half + (i >> 1) * 2 * d;
  o[j] = v;
  o[j + d] = 0;   // the zero half of a 2d-point row
}

// a tree that is ONE retained leaf (kept in the spread layout): element j of the leaf -> the caller's m + 1 coefficients
RONK_HD void roots_single_leaf_elem(const u64* leaf, u64 shift, u64 m, u64* out, u64 j) {
  if (j >= shift) out[j - shift] = leaf[j];
  if (j == 0) out[m] = 1;
}

template <class FLD>
RONK_HD u64 fld_pow(const FLD& f, u64 a, u64 e) {
  u64 r = 1;
  while (e) {
    if (e & 1) r = f.mul_plain(r, a);
    a = f.mul_plain(a, a);
    e >>= 1;
  }
  return r;
}

// One leaf: workgroup `bid` of G lanes multiplies the factors (x - r_t), t = bid*G .. bid*G + G - 1 (indices >= m read as the
// root ZERO: the padding).  Lane j holds coefficient j; step t computes c'_j = c_{j-1} - r_t c_j with the coefficient of the
// previous step in LDS -- two halves used alternately, so ONE barrier per step separates a step's reads from the writes two
// steps later.  The leading ONE of step t sits at index t + 1 <= G - 1 until the last step moves it to G, which no lane holds:
// it is the implicit leading coefficient.  G^2 field operations per leaf.  lds: 3G words.
template <class FLD, class Barrier>
RONK_HD void roots_leaf_body(const FLD& f, u64 p, const u64* roots, u64 m, u32 G, const RootsStore& st, u64* lds, u32 tid,
                             u64 bid, Barrier&& barrier) {
  u64* rr = lds;
  u64* cb = lds + G;
  const u64 idx = bid * G + tid;
  rr[tid] = idx < m ? roots[idx] % p : 0;
  u64 c = tid == 0 ? 1 : 0;
  barrier();
  for (u32 t = 0; t < G; t++) {
    u64* buf = cb + (t & 1) * G;
    buf[tid] = c;
    barrier();
    const u64 prev = tid ? buf[tid - 1] : 0;
    c = f.sub(prev, f.mul_plain(rr[t], c));
  }
  roots_put(st, bid, G, tid, c);
}

// One level's combine, element e = i * 2d + j of the pairs' products (i < pairs, j < 2d):
//     v = prod[e] + (j >= d ? a_i[j - d] + b_i[j - d] : 0)
// prod: the inverse's output (pairs rows of 2d); spread: this level's input layout (a rows, then b rows, 2d each).
template <class FLD>
RONK_HD void roots_combine_elem(const FLD& f, const u64* prod, const u64* spread, u64 pairs, u64 d, const RootsStore& st, u64 e) {
  const u64 i = e / (2 * d), j = e % (2 * d);
  u64 v = prod[e];
  if (j >= d) {
    const u64 o = i * 2 * d + (j - d);
    v = f.add(v, f.add(spread[o], spread[pairs * 2 * d + o]));
  }
  roots_put(st, i, 2 * d, j, v);
}

// ---- erasure recovery (ronk_rs_recover_batch_dev), one erasure set E shared by B rows of N values

enum { REC_BAD_INDEX = 1, REC_REPEAT = 2 };

// positions -> roots omega^pos; a bitmap of N bits finds repeats, positions >= N raise REC_BAD_INDEX.  Atom: or32(u32*, u32)
// and or_i(int*, int) returning the old value (device: vector atomics; the emulator: plain read-modify-write)
template <class FLD, class Atom>
RONK_HD void rec_roots_elem(const FLD& f, const Atom& atom, const u64* erased, u64 n, u64 omega, u64 i, u32* bitmap, int* err,
                            u64* roots) {
  const u64 pos = erased[i];
  if (pos >= n) {
    atom.or_i(err, REC_BAD_INDEX);
  } else {
    const u32 bit = 1u << (pos & 31);
    if (atom.or32(bitmap + (pos >> 5), bit) & bit) atom.or_i(err, REC_REPEAT);
  }
  roots[i] = fld_pow(f, omega, pos & (n - 1));
}

// the error word of the erasure list as the status every row reports
RONK_HD int rec_err_code(int err) {
  return (err & REC_BAD_INDEX) ? -6 /* RONK_ERR_INDEX */ : (err & REC_REPEAT) ? -2 /* RONK_ERR_ZERO_INVERSE */ : 0;
}

// Chunks of REC_CH consecutive coefficients of one row per lane: s^j is one power per chunk, then one product per element.
constexpr u32 REC_CH = 16;

// z row 0: Z (e + 1 coefficients written by the tree) zero-extended to N; row 1: the same times s^j (the coset s * <omega_N>)
template <class FLD>
RONK_HD void rec_zprep_chunk(const FLD& f, u64* zz, u64 n, u64 e, u64 s, u64 c) {
  const u64 j0 = c * REC_CH;
  u64 sj = fld_pow(f, s, j0);
  for (u32 t = 0; t < REC_CH; t++) {
    const u64 j = j0 + t;
    const u64 z = j <= e ? zz[j] : 0;
    zz[j] = z;
    zz[n + j] = f.mul_plain(z, sj);
    sj = f.mul_plain(sj, s);
  }
}

// w[b][i] = y[b][i] * zhat[i]: Z vanishes at the erased points, so their (ignored) values drop out here
template <class FLD>
RONK_HD void rec_mask_mul_elem(const FLD& f, const u64* y, const u64* zhat, u64* w, u64 n, u64 t) {
  w[t] = f.mul_plain(y[t], zhat[t & (n - 1)]);
}

// w[b][j] *= s^j, chunk c of the B x N array (N a multiple of REC_CH)
template <class FLD>
RONK_HD void rec_scale_chunk(const FLD& f, u64* w, u64 n, u64 s, u64 c) {
  const u64 t0 = c * REC_CH;
  u64 sj = fld_pow(f, s, t0 & (n - 1));
  for (u32 t = 0; t < REC_CH; t++) {
    w[t0 + t] = f.mul_plain(w[t0 + t], sj);
    sj = f.mul_plain(sj, s);
  }
}

// x[i] <- 1 / x[i] for a chunk of REC_CH non-zero values: prefix products, ONE inversion (Fermat), back-substitution
template <class FLD>
RONK_HD void rec_batch_inv_chunk(const FLD& f, u64 p, u64* x, u64 c) {
  u64 v[REC_CH], pre[REC_CH];
  u64 acc = 1;
  const u64 t0 = c * REC_CH;
  for (u32 t = 0; t < REC_CH; t++) { v[t] = x[t0 + t]; pre[t] = acc; acc = f.mul_plain(acc, v[t]); }
  u64 inv = fld_pow(f, acc, p - 2);
  for (int t = (int)REC_CH - 1; t >= 0; t--) { x[t0 + t] = f.mul_plain(inv, pre[t]); inv = f.mul_plain(inv, v[t]); }
}

// w[b][i] *= zinv[i]
template <class FLD>
RONK_HD void rec_div_elem(const FLD& f, u64* w, const u64* zinv, u64 n, u64 t) {
  w[t] = f.mul_plain(w[t], zinv[t & (n - 1)]);
}

// q_j = w[b][j] * s^-j: j < k goes to the message, any non-zero q_j above is a row whose survivors lie on no polynomial of
// degree < k (status NOT_CODEWORD, -14) -- unless the erasure list itself was malformed (the status already holds that)
template <class FLD>
RONK_HD void rec_finish_chunk(const FLD& f, const u64* w, u64 n, u64 k, u64 sinv, const int* err, u64* msgs, int* status, u64 c) {
  const u64 t0 = c * REC_CH, b = t0 / n, j0 = t0 & (n - 1);
  u64 sj = fld_pow(f, sinv, j0);
  bool bad = false;
  for (u32 t = 0; t < REC_CH; t++) {
    const u64 j = j0 + t;
    const u64 q = f.mul_plain(w[t0 + t], sj);
    sj = f.mul_plain(sj, sinv);
    if (j < k) msgs[b * k + j] = q;
    else if (q != 0) bad = true;
  }
  if (bad && *err == 0) status[b] = -14;   // RONK_ERR_NOT_CODEWORD
}

}  // namespace ronk
