// poseidon_kernels.h -- the Poseidon permutation, its sponge and a Merkle tree over the sponge, one lane per state
// (csrc/ronk_hash.hip; DESIGN.md "Poseidon and Merkle commitment").
//
// The reference: hashes::poseidon::Poseidon (src/hashes/poseidon/mod.rs:56-149), PoseidonSponge (sponge.rs:69-275) and
// tree::merkle::MerkleTree (src/tree/merkle.rs:31-99, with the sponge in the place of SHA-256).
//
// A round is  state += rc[r];  s-box (every element in a full round, element 0 in a partial one);  state = MDS * state  with
// the DENSE matrix, as the reference has it.  The state lives in registers: the width is a template parameter W, so every
// index is a compile-time constant, and a caller's width below W is padded with zero constants (exact: a zero element stays
// zero through add 0, x^alpha and zero matrix rows / columns).  rc and mds are read through wave-uniform addresses in the
// constant address space: scalar loads, and the products take their constant from an SGPR.
//
// The matrix row is where the instructions go.  new[i] = sum_j state[j] * mds[i][j] is accumulated WITHOUT reducing the
// products: W <= 16 products below 2^128 fit a three-word accumulator (< 2^132), reduced once per output element.
//   Goldilocks   lo + hi 2^64 + top 2^128 with 2^64 = 2^32 - 1, 2^96 = -1, 2^128 = -2^32 (mod p).
//   Montgomery   the state and the constants are kept as x R mod p (R = 2^64), so a product x R * m R needs one REDC to be
//                (x m) R again.  The accumulator keeps its upper word BELOW p (the 65th bit of hi + hi' + carry is folded
//                by one conditional subtraction of p, i.e. of p 2^64 from the sum): the third word never materialises and one
//                mont64::redc finishes the row, for any odd p < 2^64.
// RONK_POSEIDON_LAZY=0 builds the reduce-after-every-product form instead (the A/B of DESIGN.md section 10).
//
// The sponge keeps its state in a layout that makes the absorb and squeeze positions compile-time constants whatever the rate:
//   internal[0] = state[0] (the partial rounds' element), internal[1 .. rate] = state[capacity ..], then state[1 .. capacity-1].
// The host permutes rc and mds accordingly (a simultaneous row / column permutation of the matrix), so the results are
// those of the reference's layout.  ronk_poseidon_permute_dev uses the constants in their natural order.
//
// Plain C++ on uint32 / uint64, so tests/emu/emu_poseidon.cpp compiles the same bodies for the host.
#pragma once
#include <stddef.h>

#include "gl64.h"
#include "mont64.h"

#ifndef RONK_POSEIDON_LAZY
#define RONK_POSEIDON_LAZY 1
#endif

namespace ronk {

typedef uint64_t u64;
typedef uint32_t u32;

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) u64* PosTable;   // constant address space: uniform address -> s_load
#define RONK_POS_TABLE(p) ((PosTable)(p))
// The matrix is the same in every round, so the compiler would hoist all W * W scalar loads out of the round loop and then
// spill the SGPRs they need into VGPR lanes.  An empty asm on the row pointer makes each row's loads belong to its round.
#define RONK_POS_ROW(p) asm volatile("" : "+s"(p))
#else
typedef const u64* PosTable;
#define RONK_POS_TABLE(p) (p)
#define RONK_POS_ROW(p) (void)0
#endif

// what a launch knows about the hash (kernel argument: SGPRs).  p == 0: Goldilocks.
struct PoseidonConsts {
  const u64* rc;    // [rounds][W], table form (canonical / x R), zero padded
  const u64* mds;   // [W][W] row-major, table form, zero padded
  u64 alpha;
  u32 rounds;       // num_f + num_p
  u32 full_lo;      // num_f / 2: rounds below are full
  u32 full_from;    // num_p + num_f / 2: rounds from here on are full
  u32 rate;
  u64 p, pinv, r2;
};

// ---------------------------------------------------------------------------------------------------- field policies
struct PosGl {
  RONK_HD explicit PosGl(const PoseidonConsts&) {}
  RONK_HD u64 in(u64 x) const { return gl64::canon(x); }   // caller's word -> register form
  RONK_HD u64 out(u64 x) const { return x; }
  RONK_HD u64 add(u64 a, u64 b) const { return gl64::add(a, b); }
  RONK_HD u64 mul(u64 a, u64 b) const { return gl64::mul(a, b); }
  struct Acc { u32 w[5]; };   // 160 bits on 32-bit limbs
  RONK_HD void acc_zero(Acc& a) const { a.w[0] = a.w[1] = a.w[2] = a.w[3] = a.w[4] = 0; }
  // a += x * m, any 64-bit x and m; at most 16 products per accumulator
  RONK_HD void acc_mad(Acc& a, u64 x, u64 m) const {
    u64 lo, hi;
    mont64::mul64(x, m, lo, hi);
#if defined(__clang__)
    u32 c;
    a.w[0] = __builtin_addc(a.w[0], (u32)lo, 0u, &c);
    a.w[1] = __builtin_addc(a.w[1], (u32)(lo >> 32), c, &c);
    a.w[2] = __builtin_addc(a.w[2], (u32)hi, c, &c);
    a.w[3] = __builtin_addc(a.w[3], (u32)(hi >> 32), c, &c);
    a.w[4] += c;
#else
    const unsigned __int128 s = (((unsigned __int128)a.w[3] << 96) | ((unsigned __int128)a.w[2] << 64) | ((u64)a.w[1] << 32) | a.w[0]);
    const unsigned __int128 pr = ((unsigned __int128)hi << 64) | lo;
    const unsigned __int128 t = s + pr;
    a.w[0] = (u32)t; a.w[1] = (u32)(t >> 32); a.w[2] = (u32)(t >> 64); a.w[3] = (u32)(t >> 96);
    a.w[4] += t < pr;
#endif
  }
  // lo - w3 - w4 2^32 + w2 EPS: w4 <= 15, so w4 2^32 is far below p (gl64::sub takes any a and b <= p)
  RONK_HD u64 acc_reduce(const Acc& a) const {
    const u64 lo = ((u64)a.w[1] << 32) | a.w[0];
    const u64 t0 = gl64::sub32(lo, a.w[3]);
    const u64 t1 = gl64::sub(t0, (u64)a.w[4] << 32);
    return gl64::mad_eps_canon(a.w[2], t1);
  }
};

struct PosMont {
  mont64::Field f;
  RONK_HD explicit PosMont(const PoseidonConsts& k) { f.p = k.p; f.pinv = k.pinv; f.r2 = k.r2; f.one = 0; }
  RONK_HD u64 in(u64 x) const { return mont64::to_mont(f, x); }   // any 64-bit x: also the reduction mod p
  RONK_HD u64 out(u64 x) const { return mont64::from_mont(f, x); }
  RONK_HD u64 add(u64 a, u64 b) const { return mont64::add(f, a, b); }
  RONK_HD u64 mul(u64 a, u64 b) const { return mont64::mmul(f, a, b); }
  struct Acc { u32 w[4]; };   // hi:lo with hi < p
  RONK_HD void acc_zero(Acc& a) const { a.w[0] = a.w[1] = a.w[2] = a.w[3] = 0; }
  // a += x * m for x, m < p: the product's upper word is below p, so is the accumulator's, and their sum plus the carry of the
  // lower words is below 2p (possibly above 2^64 when p > 2^63): one conditional subtraction of p restores hi < p
  RONK_HD void acc_mad(Acc& a, u64 x, u64 m) const {
    u64 lo, hi;
    mont64::mul64(x, m, lo, hi);
#if defined(__clang__)
    u32 c, b1, b2;
    a.w[0] = __builtin_addc(a.w[0], (u32)lo, 0u, &c);
    a.w[1] = __builtin_addc(a.w[1], (u32)(lo >> 32), c, &c);
    const u32 sl = __builtin_addc(a.w[2], (u32)hi, c, &c);
    const u32 sh = __builtin_addc(a.w[3], (u32)(hi >> 32), c, &c);
    const u32 dl = __builtin_subc(sl, (u32)f.p, 0u, &b1);
    const u32 dh = __builtin_subc(sh, (u32)(f.p >> 32), b1, &b2);
    const bool take = c | !b2;
    a.w[2] = take ? dl : sl;
    a.w[3] = take ? dh : sh;
#else
    const u64 alo = ((u64)a.w[1] << 32) | a.w[0], ahi = ((u64)a.w[3] << 32) | a.w[2];
    const u64 nlo = alo + lo;
    const unsigned __int128 s = (unsigned __int128)ahi + hi + (nlo < lo);
    const u64 nhi = (s >= f.p) ? (u64)(s - f.p) : (u64)s;
    a.w[0] = (u32)nlo; a.w[1] = (u32)(nlo >> 32); a.w[2] = (u32)nhi; a.w[3] = (u32)(nhi >> 32);
#endif
  }
  RONK_HD u64 acc_reduce(const Acc& a) const {
    return mont64::redc(f, ((u64)a.w[1] << 32) | a.w[0], ((u64)a.w[3] << 32) | a.w[2]);
  }
};

// ---------------------------------------------------------------------------------------------------- permutation
// x^alpha, alpha >= 1 wave-uniform: fixed chains for 3, 5 and 7, square-and-multiply from the top bit otherwise
template <class F>
RONK_HD u64 poseidon_pow_any(const F& f, u64 x, u64 alpha) {
  int top = 63;
  while (top > 0 && !((alpha >> top) & 1)) top--;
  u64 r = x;
  for (int b = top - 1; b >= 0; b--) {
    r = f.mul(r, r);
    if ((alpha >> b) & 1) r = f.mul(r, x);
  }
  return r;
}
template <class F, int A>
RONK_HD u64 poseidon_pow_fixed(const F& f, u64 x) {
  const u64 x2 = f.mul(x, x);
  if (A == 3) return f.mul(x2, x);
  const u64 x4 = f.mul(x2, x2);
  if (A == 5) return f.mul(x4, x);
  return f.mul(f.mul(x4, x2), x);
}
// the s-box on s[0 .. N): the switch is outside the element loop (uniform branches only)
template <class F, int N>
RONK_HD void poseidon_sbox(const F& f, u64 alpha, u64* s) {
  if (alpha == 1) return;
  if (alpha == 3) {
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = poseidon_pow_fixed<F, 3>(f, s[i]);
  } else if (alpha == 5) {
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = poseidon_pow_fixed<F, 5>(f, s[i]);
  } else if (alpha == 7) {
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = poseidon_pow_fixed<F, 7>(f, s[i]);
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = poseidon_pow_any(f, s[i], alpha);
  }
}

// the permutation on a state in register form (src/hashes/poseidon/mod.rs:131-149)
template <class F, int W>
RONK_HD void poseidon_permute(const F& f, const PoseidonConsts& k, u64 (&s)[W]) {
  PosTable rc = RONK_POS_TABLE(k.rc);
  PosTable mds = RONK_POS_TABLE(k.mds);
  for (u32 r = 0; r < k.rounds; r++) {
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = f.add(s[i], rc[(u64)r * W + i]);
    if (r < k.full_lo || r >= k.full_from) poseidon_sbox<F, W>(f, k.alpha, s);
    else poseidon_sbox<F, 1>(f, k.alpha, s);
    u64 t[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
      PosTable row = mds + i * W;
      RONK_POS_ROW(row);
#if RONK_POSEIDON_LAZY
      typename F::Acc a;
      f.acc_zero(a);
#pragma unroll
      for (int j = 0; j < W; j++) f.acc_mad(a, s[j], row[j]);
      t[i] = f.acc_reduce(a);
#else
      u64 a = f.mul(s[0], row[0]);
#pragma unroll
      for (int j = 1; j < W; j++) a = f.add(a, f.mul(s[j], row[j]));
      t[i] = a;
#endif
    }
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = t[i];
  }
}

// one state of `width` caller words at st[0 .. width), natural order, in place (a lane of ronk_poseidon_permute_dev)
template <class F, int W>
RONK_HD void poseidon_permute_words(const F& f, const PoseidonConsts& k, u32 width, u64* st) {
  u64 s[W];
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = (u32)i < width ? f.in(st[i]) : 0;
  poseidon_permute<F, W>(f, k, s);
#pragma unroll
  for (int i = 0; i < W; i++)
    if ((u32)i < width) st[i] = f.out(s[i]);
}

// ---------------------------------------------------------------------------------------------------- sponge
// One-shot absorb of `len` elements, then squeeze `n_out` (sponge.rs:110-275): ceil(len / rate) permutations while absorbing
// (none for len == 0: the squeeze then returns zeros), one more each time `rate` elements were taken and more are wanted.
// load(j): caller word j of the item (any 64-bit value); store(k, v): output k.  k holds the SPONGE-ordered constants.  The
// steps -- absorb chunks, then squeeze blocks -- share one loop so that the permutation is inlined once.
template <class F, int W, class Load, class Store>
RONK_HD void poseidon_sponge(const F& f, const PoseidonConsts& k, u64 len, u64 n_out, Load&& load, Store&& store) {
  u64 s[W];
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = 0;
  const u32 rate = k.rate;
  const u64 nab = (len + rate - 1) / rate, nsq = (n_out + rate - 1) / rate;
  const u64 steps = nab + nsq, perm_until = nsq ? steps - 1 : nab;
  for (u64 t = 0; t < steps; t++) {
    if (t < nab) {
      const u64 base = t * rate;
#pragma unroll
      for (int i = 0; i < W - 1; i++)
        if ((u32)i < rate && base + i < len) s[1 + i] = f.add(s[1 + i], f.in(load(base + i)));
    } else {
      const u64 base = (t - nab) * rate;
#pragma unroll
      for (int i = 0; i < W - 1; i++)
        if ((u32)i < rate && base + i < n_out) store(base + i, f.out(s[1 + i]));
    }
    if (t < perm_until) poseidon_permute<F, W>(f, k, s);
  }
}

// ---------------------------------------------------------------------------------------------------- Merkle tree
// Levels from the leaves up: level 0 = n leaf digests, level l + 1 = ceil(count_l / 2) nodes, the root last; every node is
// `d` words.  An unpaired last node is hashed with itself (merkle.rs:48-52).
RONK_HD u64 merkle_levels(u64 n) {   // number of levels, n >= 1
  u64 l = 1;
  while (n > 1) { n = (n + 1) / 2; l++; }
  return l;
}
RONK_HD u64 merkle_level_count(u64 n, u64 level) {
  for (u64 l = 0; l < level; l++) n = (n + 1) / 2;
  return n;
}
RONK_HD u64 merkle_level_offset(u64 n, u64 d, u64 level) {   // in words
  u64 off = 0;
  for (u64 l = 0; l < level; l++) { off += n * d; n = (n + 1) / 2; }
  return off;
}

static constexpr u32 MERKLE_BLOCK = 256;       // nodes a workgroup reduces
static constexpr u32 MERKLE_BLOCK_LEVELS = 8;  // log2 of it: levels one launch climbs

// A workgroup holds `cnt` <= 256 consecutive nodes of level `lvl` (the nodes bid * 256 ..; only the LAST workgroup of a level
// can hold fewer, so the odd end of a level is the odd end of that workgroup) in bufa, d words each, and climbs `climb` <= 8
// levels: lane t of a step hashes nodes 2t and 2t + 1 (or 2t twice) into node t of the other buffer and into the tree.
// bufa: 256 d words, bufb: 128 d words.  off: word offset of level lvl + 1 in the tree.  lanes(fn) runs fn(tid) for every lane
// of the workgroup after everything before it is visible: a barrier and the lane's own call on the device, a loop over the
// lanes in the host emulator.
template <class F, int W, class Lanes>
RONK_HD void merkle_climb(const F& f, const PoseidonConsts& k, u64* bufa, u64* bufb, u64 bid, u32 cnt, u32 d, u32 climb, u64 n_lvl,
                          u64 off, u64* tree, Lanes&& lanes) {
  u64* src = bufa;
  u64* dst = bufb;
  for (u32 s = 1; s <= climb; s++) {
    const u32 cn = (cnt + 1) / 2;
    lanes([&](u32 tid) {
      if (tid >= cn) return;
      const u64* l = src + (u64)(2 * tid) * d;
      const u64* r = (2 * tid + 1 < cnt) ? l + d : l;
      u64* o = dst + (u64)tid * d;
      u64* g = tree + off + (bid * (MERKLE_BLOCK >> s) + tid) * d;
      poseidon_sponge<F, W>(f, k, 2 * (u64)d, d, [&](u64 j) { return j < d ? l[j] : r[j - d]; },
                            [&](u64 q, u64 v) { o[q] = v; g[q] = v; });
    });
    cnt = cn;
    n_lvl = (n_lvl + 1) / 2;
    off += n_lvl * d;
    u64* x = src; src = dst; dst = x;
  }
}

// One node of the level above, one lane per node (the levels too large for one workgroup): node t = sponge(node 2t || node
// 2t + 1), the last node of an odd level with itself.  lvl: the cnt nodes of the level, nxt: the level above.
template <class F, int W>
RONK_HD void merkle_level_node(const F& f, const PoseidonConsts& k, const u64* lvl, u64 cnt, u32 d, u64* nxt, u64 t) {
  const u64* l = lvl + 2 * t * d;
  const u64* r = (2 * t + 1 < cnt) ? l + d : l;
  u64* o = nxt + t * d;
  poseidon_sponge<F, W>(f, k, 2 * (u64)d, d, [&](u64 j) { return j < d ? l[j] : r[j - d]; }, [&](u64 q, u64 v) { o[q] = v; });
}

// MerkleTree::get_proof (merkle.rs:66-81) for one query: the sibling digests from the bottom up.  The reference indexes
// level[index + 1] out of bounds for the unpaired last node of an odd level: code 1 (the caller's RONK_ERR_INDEX), as for
// index >= n; the path is then zero-filled.
RONK_HD int merkle_open_one(const u64* tree, u64 n, u64 d, u64 index, u64* path) {
  const u64 depth = merkle_levels(n) - 1;
  int bad = index >= n;
  u64 cnt = n, off = 0;
  for (u64 l = 0; l < depth && !bad; l++) {
    const u64 sib = index ^ 1;
    if (sib >= cnt) { bad = 1; break; }
    for (u64 j = 0; j < d; j++) path[l * d + j] = tree[off + sib * d + j];
    index >>= 1;
    off += cnt * d;
    cnt = (cnt + 1) / 2;
  }
  if (bad)
    for (u64 j = 0; j < depth * d; j++) path[j] = 0;
  return bad;
}

// MerkleTree::prove (merkle.rs:84-98) for one query: the leaf's digest folded with its path, the sibling's side by the parity
// of the index, compared with the root.  h: 3 d words of lane-private memory (LDS on the device): the running digest, then the
// pair a node absorbs.  The sibling is COPIED next to the digest, on the side its parity gives, so that the sponge reads one
// array in one address space (a select between an LDS and a global pointer would make every load a flat one).
template <class F, int W, class Load>
RONK_HD int merkle_verify_one(const F& f, const PoseidonConsts& k, u64 leaf_len, Load&& load, u64 index, const u64* path, u64 n,
                              u32 d, const u64* root, u64* h) {
  u64* pair = h + d;
  poseidon_sponge<F, W>(f, k, leaf_len, d, load, [&](u64 q, u64 v) { h[q] = v; });
  const u64 depth = merkle_levels(n) - 1;
  int ok = index < n;
  for (u64 l = 0; l < depth; l++) {
    const u64* sib = path + l * d;
    const u32 so = (index & 1) ? 0 : d, ho = d - so;   // a sibling on the left comes first
    for (u32 j = 0; j < d; j++) { pair[so + j] = sib[j]; pair[ho + j] = h[j]; }
    poseidon_sponge<F, W>(f, k, 2 * (u64)d, d, [&](u64 j) { return pair[j]; }, [&](u64 q, u64 v) { h[q] = v; });
    index >>= 1;
  }
  for (u32 j = 0; j < d; j++) ok &= h[j] == root[j];
  return ok;
}

// ---------------------------------------------------------------------------------------------------- host: the tables
// the instantiated register widths: a caller's width runs on the next one up, zero padded
inline u32 poseidon_padded_width(u32 width) { return width <= 4 ? 4 : width <= 8 ? 8 : width <= 12 ? 12 : 16; }
inline u64 poseidon_table_form(u64 p, u64 c) {
  if (p == gl64::P) return c % p;
  return (u64)((((unsigned __int128)(c % p)) << 64) % p);   // c R mod p
}
// tab (zero-filled, 2 * (rounds * W + W * W) words) = rc natural, mds natural, rc in the sponge's layout, mds in the sponge's
// layout, every entry reduced and in table form
inline void poseidon_host_tables(u64 p, u32 width, u32 rate, u32 rounds, const u64* rc, const u64* mds, u64* tab) {
  const u32 W = poseidon_padded_width(width), cap = width - rate;
  u32 perm[16];   // internal position -> the reference's state index
  perm[0] = 0;
  for (u32 i = 0; i < rate; i++) perm[1 + i] = cap + i;
  for (u32 t = 0; t + 1 < cap; t++) perm[1 + rate + t] = 1 + t;
  const size_t nrc = (size_t)rounds * W, nm = (size_t)W * W;
  u64 *rc_n = tab, *m_n = rc_n + nrc, *rc_s = m_n + nm, *m_s = rc_s + nrc;
  for (u32 r = 0; r < rounds; r++)
    for (u32 i = 0; i < width; i++) {
      rc_n[(size_t)r * W + i] = poseidon_table_form(p, rc[(size_t)r * width + i]);
      rc_s[(size_t)r * W + i] = poseidon_table_form(p, rc[(size_t)r * width + perm[i]]);
    }
  for (u32 i = 0; i < width; i++)
    for (u32 j = 0; j < width; j++) {
      m_n[i * W + j] = poseidon_table_form(p, mds[i * width + j]);
      m_s[i * W + j] = poseidon_table_form(p, mds[perm[i] * width + perm[j]]);
    }
}
}  // namespace ronk
