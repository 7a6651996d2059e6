// fr_ntt_kernels.h -- the number-theoretic transform over BN254's scalar field Fr (bn254_fr.h): what the reference's
// Polynomial::{fft, ifft, Mul} (src/polynomial/mod.rs:240-323, :430-453, src/polynomial/arithmetic.rs:97-119) are over
// F = Fr, the field kzg::commit / kzg::open run over on a production curve (DESIGN.md "NTT over the BN254 scalar field").
//
// Elements in global memory: 4 x u64 little endian, STANDARD form, 32 B (the ABI of ronk_msm_bn254 / ronk_kzg_open_bn254);
// inputs are any 256-bit integers (canonicalised on the first load), outputs canonical.  Every multiplier (butterfly
// twiddles, inter-pass twiddles, the inverse's 1/n) is stored in MONTGOMERY form, so fr_mul(x, wR) = x w keeps the data
// in standard form throughout.  omega_n = 5^((r-1)/n) (field/mod.rs:70-75); r - 1 = 2^28 * odd.
//
// Structure: n = R_0 R_1 .. R_(P-1), one pass per factor, every pass the same kernel.  Pass t is the radix-R_t step of
// the self-sorting (Stockham) decimation in frequency: with s = R_0 .. R_(t-1), n_t = n / s, m = n_t / R_t and a column
// c = q + s p (q < s, p < m),
//     out[q + s (R_t p + k)] = omega_(n_t)^(p k) * sum_j in[c + (n / R_t) j] omega_(R_t)^(j k)          j, k < R_t
// natural order in, natural order out after the last pass (m = 1, no twiddle), no transposition pass.  A workgroup takes
// C = 2^logc adjacent columns: its R_t x C tile is R_t row segments of C * 32 contiguous bytes on the way in and the same
// (s >= C) or one contiguous R_t * C * 32 bytes (s = 1) on the way out.  The R_t-point transforms of the tile run in LDS as
// log2 R_t radix-2 Stockham stages (read b and b + N/2, write q + 2 s' p' and + s'), so they too come out in natural order;
// the last stage of every tile has the twiddle ONE and multiplies nothing.
//
// LDS image: LIMB-PAIR PLANAR -- four planes of N u64, element e's words at plane[w][e] -- so that a wave's 64 lanes on 64
// adjacent elements read 64 adjacent 8-byte words (DESIGN.md has the bank count against the 32-byte array of structures).
//
// Inter-pass twiddles omega_(n_t)^(p k): a table of n_t entries when that is at most n / 16 (every pass but the first),
// else two tables of about sqrt(n_t) entries, omega^(e mod 2^h) and omega^(e - e mod 2^h), and two products.  No table
// has n entries.  The inverse folds 1/n (and, for the multiply, the Montgomery factor 2^256 that the pointwise product
// fr_mul(a, b) = a b / 2^256 of two standard-form operands leaves behind) into the first pass's table.
//
// Every body is plain C++ with the thread index and the barrier passed in: the host emulator (tests/emu/emu_fr_ntt.cpp)
// runs the same code on fibers.  No inline assembly.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bn254_fr.h"

namespace ronk {

using bn254::Fr;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 FR_TWO_ADICITY = 28;    // r - 1 = 2^28 * odd
constexpr u32 FR_GENERATOR = 5;       // generates Fr* (2 and 3 do not)
constexpr u32 FR_LOGR_MAX = 10;       // rows of a tile: 2^10 x 4 columns x 32 B = 128 KiB of the CU's 160 KiB LDS
constexpr u32 FR_LOGC = 2;            // columns per workgroup: 4 x 32 B = 128 contiguous bytes per row segment
constexpr u32 FR_MAX_PASSES = 4;
constexpr u32 FR_BPT = 2;             // butterflies per lane and stage: a tile of N elements runs on max(64, N / 4) lanes
constexpr u32 FR_DIRECT_SHIFT = 4;    // a direct inter-pass table when n_t <= n >> 4

// ---------------------------------------------------------------------------------------------------------------- host field
// (also device-callable; used on the host only: table construction, roots)
RONK_HD Fr fr_from_u64(u64 v) { Fr r = bn254::fr_zero(); r.l[0] = (u32)v; r.l[1] = (u32)(v >> 32); return r; }
RONK_HD Fr fr_from_mont(const Fr& a) { return bn254::fr_mul(a, fr_from_u64(1)); }
RONK_HD bool fr_eq(const Fr& a, const Fr& b) { u32 d = 0; for (int i = 0; i < 8; i++) d |= a.l[i] ^ b.l[i]; return d == 0; }
// r - k for small k, as limbs (the exponents (r - 1) >> j and r - 2 come from it)
RONK_HD Fr fr_mod_minus(u32 k) {
  Fr e;
  u64 borrow = k;
  for (int i = 0; i < 8; i++) { const u64 t = (u64)bn254::fr_mod(i) - borrow; e.l[i] = (u32)t; borrow = (t >> 32) & 1; }
  return e;
}
RONK_HD Fr fr_shr(const Fr& a, u32 s) {   // s < 32
  Fr r;
  for (int i = 0; i < 8; i++) r.l[i] = s ? (a.l[i] >> s) | (i < 7 ? a.l[i + 1] << (32 - s) : 0) : a.l[i];
  return r;
}
// bm^e: bm and the result in Montgomery form, e any 256-bit integer
RONK_HD Fr fr_pow_mont(const Fr& bm, const Fr& e) {
  Fr acc = bn254::fr_const_one_mont();
  for (int bit = 255; bit >= 0; bit--) {
    acc = bn254::fr_mul(acc, acc);
    if ((e.l[bit >> 5] >> (bit & 31)) & 1) acc = bn254::fr_mul(acc, bm);
  }
  return acc;
}
// a^e and 1/a (Fermat; the inverse of ZERO is ZERO) on standard-form values, a taken mod r
RONK_HD Fr fr_pow(const Fr& a, const Fr& e) { return fr_from_mont(fr_pow_mont(bn254::fr_to_mont(a), e)); }
RONK_HD Fr fr_inv(const Fr& a) { return fr_pow(a, fr_mod_minus(2)); }
// omega_(2^log2n) = 5^((r-1) / 2^log2n) in Montgomery form; log2n <= 28
RONK_HD Fr fr_root_of_unity_mont(u32 log2n) {
  Fr w = fr_pow_mont(bn254::fr_to_mont(fr_from_u64(FR_GENERATOR)), fr_shr(fr_mod_minus(1), FR_TWO_ADICITY));
  for (u32 i = log2n; i < FR_TWO_ADICITY; i++) w = bn254::fr_mul(w, w);
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- the plan
enum FrTwMode { FR_TW_NONE = 0, FR_TW_DIRECT = 1, FR_TW_SPLIT = 2, FR_TW_SCALE = 3 };

// what a pass's kernel needs besides the buffers
struct FrPassGeom {
  u32 log2n;
  u32 logr;      // rows of the tile: R = 2^logr
  u32 logc;      // columns per workgroup
  u32 log_s;     // s = product of the earlier factors
  u32 tw_mode;   // FrTwMode
  u32 lo_bits;   // FR_TW_SPLIT: tw[e & (2^lo_bits - 1)] * tw[2^lo_bits + (e >> lo_bits)]
};
struct FrPassArgs {
  FrPassGeom g;
  const u64* in;
  u64* out;
  const Fr* wr;   // omega_R^t, t < R / 2 (at least one entry)
  const Fr* tw;   // inter-pass table(s); FR_TW_SCALE: one entry, the constant
};
struct FrPassDesc {
  FrPassGeom g;
  std::vector<Fr> wr, tw;
};
struct FrPlanDesc {
  u32 log2n = 0;
  std::vector<FrPassDesc> passes;
  size_t table_bytes() const {
    size_t b = 0;
    for (auto& p : passes) b += (p.wr.size() + p.tw.size()) * sizeof(Fr);
    return b;
  }
};

// lanes and LDS bytes of a pass's workgroup
inline u32 fr_pass_threads(const FrPassGeom& g) { const u32 N = 1u << (g.logr + g.logc); return N / 4 < 64 ? 64 : N / 4; }
inline size_t fr_pass_lds_bytes(const FrPassGeom& g) { return (size_t)32 << (g.logr + g.logc); }
inline u64 fr_pass_blocks(const FrPassGeom& g) { return (u64)1 << (g.log2n - g.logr - g.logc); }   // per transform

// the factors: as few passes as the cap allows, as even as possible, the larger ones first.  false: more than FR_MAX_PASSES.
inline bool fr_plan_factors(u32 log2n, u32 max_log2_tile, std::vector<u32>* logr) {
  u32 cap = max_log2_tile == 0 || max_log2_tile > FR_LOGR_MAX ? FR_LOGR_MAX : max_log2_tile;
  const u32 P = log2n == 0 ? 1 : (log2n + cap - 1) / cap;
  if (P > FR_MAX_PASSES) return false;
  logr->clear();
  for (u32 t = 0; t < P; t++) logr->push_back(log2n / P + (t < log2n % P ? 1 : 0));
  return true;
}

// tables of one direction.  `scale` (Montgomery form) multiplies every output: 1/n for the inverse, R/n for the inverse of
// the multiply, ONE (nullptr) for the forward transform.
inline bool fr_build_plan(u32 log2n, u32 max_log2_tile, bool inverse, const Fr* scale, FrPlanDesc* pd) {
  using namespace bn254;
  std::vector<u32> f;
  if (log2n > FR_TWO_ADICITY || !fr_plan_factors(log2n, max_log2_tile, &f)) return false;
  pd->log2n = log2n;
  pd->passes.clear();
  Fr wn = fr_root_of_unity_mont(log2n);
  if (inverse) wn = fr_pow_mont(wn, fr_mod_minus(2));   // omega^-1 (Montgomery form in, Montgomery form out)
  u32 log_s = 0;
  for (size_t t = 0; t < f.size(); t++) {
    FrPassDesc ps;
    ps.g.log2n = log2n; ps.g.logr = f[t]; ps.g.log_s = log_s;
    const u32 cols = log2n - f[t];
    ps.g.logc = cols < FR_LOGC ? cols : FR_LOGC;
    const u32 log_nt = log2n - log_s, log_m = log_nt - f[t];
    // omega_R = omega_n^(n / R)
    Fr wR = wn;
    for (u32 i = f[t]; i < log2n; i++) wR = fr_mul(wR, wR);
    const size_t half = f[t] ? (size_t)1 << (f[t] - 1) : 1;
    ps.wr.resize(half);
    Fr x = fr_const_one_mont();
    for (size_t i = 0; i < half; i++) { ps.wr[i] = x; x = fr_mul(x, wR); }
    // omega_(n_t) = omega_n^s
    Fr wt = wn;
    for (u32 i = 0; i < log_s; i++) wt = fr_mul(wt, wt);
    const bool scaled = scale && t == 0;
    if (log_m == 0) {
      ps.g.tw_mode = scaled ? FR_TW_SCALE : FR_TW_NONE;
      ps.g.lo_bits = 0;
      if (scaled) ps.tw.push_back(*scale);
    } else if (log_nt + FR_DIRECT_SHIFT <= log2n) {
      ps.g.tw_mode = FR_TW_DIRECT;
      ps.g.lo_bits = 0;
      ps.tw.resize((size_t)1 << log_nt);
      x = scaled ? *scale : fr_const_one_mont();
      for (size_t e = 0; e < ps.tw.size(); e++) { ps.tw[e] = x; x = fr_mul(x, wt); }
    } else {
      ps.g.tw_mode = FR_TW_SPLIT;
      ps.g.lo_bits = (log_nt + 1) / 2;
      const size_t lo = (size_t)1 << ps.g.lo_bits, hi = (size_t)1 << (log_nt - ps.g.lo_bits);
      ps.tw.resize(lo + hi);
      x = fr_const_one_mont();
      for (size_t e = 0; e < lo; e++) { ps.tw[e] = x; x = fr_mul(x, wt); }   // x ends as omega^(2^lo_bits)
      const Fr step = x;
      x = scaled ? *scale : fr_const_one_mont();
      for (size_t e = 0; e < hi; e++) { ps.tw[lo + e] = x; x = fr_mul(x, step); }
    }
    pd->passes.push_back(ps);
    log_s += f[t];
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- the pass
// the limb-pair planar LDS image: word w of element e at lds[w * N + e]
RONK_HD Fr fr_lds_get(const u64* lds, u32 N, u32 e) {
  Fr r;
#pragma unroll
  for (int w = 0; w < 4; w++) { const u64 v = lds[(u32)w * N + e]; r.l[2 * w] = (u32)v; r.l[2 * w + 1] = (u32)(v >> 32); }
  return r;
}
RONK_HD void fr_lds_put(u64* lds, u32 N, u32 e, const Fr& a) {
#pragma unroll
  for (int w = 0; w < 4; w++) lds[(u32)w * N + e] = ((u64)a.l[2 * w + 1] << 32) | a.l[2 * w];
}

// One workgroup of one pass: tile `tile` (C adjacent columns) of transform `row` of the batch.  lds: 4 N words, N = R C.
// nthreads >= N / (2 FR_BPT).
template <class Barrier>
RONK_HD void fr_ntt_pass_body(const FrPassArgs& a, u64* lds, u32 tid, u32 nthreads, u64 tile, u64 row, Barrier&& barrier) {
  using namespace bn254;
  const FrPassGeom& g = a.g;
  const u32 N = 1u << (g.logr + g.logc), C = 1u << g.logc, R = 1u << g.logr;
  const u64 n = (u64)1 << g.log2n, ncols = n >> g.logr;
  const u64* in = a.in + 4 * n * row;
  u64* out = a.out + 4 * n * row;
  const u64 c0 = tile << g.logc;
  // load: row segments of C adjacent elements; tile index cc + C j
  for (u32 e = tid; e < N; e += nthreads) {
    const u32 cc = e & (C - 1), j = e >> g.logc;
    fr_lds_put(lds, N, e, fr_canon(fr_load(in + 4 * (c0 + cc + ncols * j))));
  }
  barrier();
  // log2 R radix-2 Stockham stages over the rows; the columns ride along as the low bits of the stride
  for (u32 u = 0; u < g.logr; u++) {
    const u32 ls = g.logc + u;   // stride s' = C 2^u
    Fr y0[FR_BPT], y1[FR_BPT];
#pragma unroll
    for (u32 i = 0; i < FR_BPT; i++) {
      const u32 b = tid + i * nthreads;
      if (b < N / 2) {
        const Fr x0 = fr_lds_get(lds, N, b), x1 = fr_lds_get(lds, N, b + N / 2);
        y0[i] = fr_add(x0, x1);
        y1[i] = fr_sub(x0, x1);
        if (u + 1 < g.logr) y1[i] = fr_mul(y1[i], a.wr[(b >> ls) << u]);
      }
    }
    barrier();
#pragma unroll
    for (u32 i = 0; i < FR_BPT; i++) {
      const u32 b = tid + i * nthreads;
      if (b < N / 2) {
        const u32 q = b & ((1u << ls) - 1), p = b >> ls;
        const u32 o = q + (p << (ls + 1));
        fr_lds_put(lds, N, o, y0[i]);
        fr_lds_put(lds, N, o + (1u << ls), y1[i]);
      }
    }
    barrier();
  }
  // inter-pass twiddle and store: tile index cc + C k holds output k of column c0 + cc
  const u64 smask = ((u64)1 << g.log_s) - 1;
  for (u32 e = tid; e < N; e += nthreads) {
    u32 cc, k;
    if (g.log_s == 0) { k = e & (R - 1); cc = e >> g.logr; }   // first pass: a column's outputs are adjacent in memory
    else { cc = e & (C - 1); k = e >> g.logc; }
    Fr v = fr_lds_get(lds, N, cc + (k << g.logc));
    const u64 c = c0 + cc, q = c & smask, p = c >> g.log_s;
    if (g.tw_mode == FR_TW_DIRECT) {
      v = fr_mul(v, a.tw[p * k]);
    } else if (g.tw_mode == FR_TW_SPLIT) {
      const u64 ex = p * k;
      v = fr_mul(fr_mul(v, a.tw[ex & (((u64)1 << g.lo_bits) - 1)]), a.tw[((u64)1 << g.lo_bits) + (ex >> g.lo_bits)]);
    } else if (g.tw_mode == FR_TW_SCALE) {
      v = fr_mul(v, a.tw[0]);
    }
    fr_store(out + 4 * (q + (((p << g.logr) + k) << g.log_s)), v);
  }
}

// the pointwise middle of the multiply, element i: x[i] = a[i] b[i] / 2^256 (both operands canonical, standard form; the
// inverse plan's scale carries the 2^256 back)
RONK_HD void fr_pointwise_elem(const u64* a, const u64* b, u64* x, u64 i) {
  bn254::fr_store(x + 4 * i, bn254::fr_mul(bn254::fr_load(a + 4 * i), bn254::fr_load(b + 4 * i)));
}
// out[i] = in[i] for i < have, ZERO up to n: the zero-padded operand of the multiply
RONK_HD void fr_pad_elem(const u64* in, u64 have, u64* out, u64 i) {
#pragma unroll
  for (int w = 0; w < 4; w++) out[4 * i + w] = i < have ? in[4 * i + w] : 0;
}

}  // namespace ronk
