// accum_kernels.h -- running products and sums over the 64-bit fields and their quadratic extension, and the two accumulator
// columns a PLONK- or STARK-style prover builds on them: the permutation grand product and the logUp running sum
// (csrc/ronk_accum.hip; include/ronk_ntt.h "running products and sums").
//
// A scan is reduce-then-scan in three LAUNCHES.  No workgroup waits for another: there is no flag, no look-back and no grid
// barrier, only launch boundaries.
//   phase 1   workgroup b reduces its block of ACC_BLOCK = 2048 elements to one total, work[b]
//   phase 2   ONE workgroup turns the B totals into their exclusive scan in place (lane l owns ceil(B / 256) consecutive totals:
//             a serial pass, a scan over the 256 lane sums, a serial pass) and writes the grand total
//   phase 3   workgroup b redoes its block from the base work[b] and writes the prefixes
// Inside a block a lane owns ACC_EPL = 8 consecutive elements (a serial pass in registers); the 256 lane sums meet in LDS, by
// a halving tree in phase 1 and by a Hillis-Steele scan on two buffers in phases 2 and 3 (one barrier per step).  n <= 2^28 is
// B <= 2^17 totals, 512 per lane of phase 2: the only size-dependent quantity is that count, which leaves 1 at n = 2^19 + 1.
// Field arithmetic is exact and both operators commute, so every blocking gives the same words.
//
// The fused accumulators are phase-1 variants: a lane forms the terms of its 8 rows in registers (the columns are read once,
// 64 contiguous bytes per lane and column), inverts the 8 denominators through their norms with ONE Fermat power (Montgomery's
// trick; a zero norm is replaced by one and its term forced to ZERO), writes the terms into the output array and joins the
// block's reduction.  Phases 2 and 3 are the generic exclusive scan of that array in place.
//
// One family, templated on the operator, the element (a base word or a pair) and the field policy of fri_kernels.h (FriGl,
// FriGlW7, FriMont).  Totals in the workspace stay in REGISTER form; arrays the caller sees are canonical.  Plain C++ on
// uint64, so tests/emu/emu_accum.cpp compiles the same bodies for the host.
#pragma once
#include "deep_kernels.h"
#include "ext2_kernels.h"

namespace ronk {

constexpr int ACC_EPL = 8;                          // elements per lane
constexpr u32 ACC_LANES = 256;                      // lanes per workgroup
constexpr u32 ACC_BLOCK = ACC_LANES * ACC_EPL;      // elements per workgroup
constexpr u32 ACC_LOG2_LANES = 8;
constexpr u64 ACC_MAX_N = (u64)1 << 28;
constexpr u32 ACC_MAX_COLUMNS = 16;

RONK_HD u64 acc_blocks(u64 n) { return (n + ACC_BLOCK - 1) / ACC_BLOCK; }
// the workspace of one call: two planes of totals, one of flags
RONK_HD u64 acc_work_words(u64 n) { return (n == 0 || n > ACC_MAX_N) ? 0 : 3 * acc_blocks(n); }

// ---------------------------------------------------------------------------------------------------- elements
// what a scan runs over: load / store convert (any 64-bit word in, canonical words out), raw_* keep the register form
template <class F>
struct AccWord {
  typedef u64 V;
  typedef F Field;
  F f;
  RONK_HD AccWord(const FriConsts& k, u64) : f(k) {}
  RONK_HD u64 load(const u64* a, size_t, size_t i) const { return f.in(a[i]); }
  RONK_HD void store(u64* out, size_t, size_t i, u64 v) const { out[i] = f.out(v); }
  RONK_HD u64 raw_load(const u64* a, size_t, size_t i) const { return a[i]; }
  RONK_HD void raw_store(u64* out, size_t, size_t i, u64 v) const { out[i] = v; }
  RONK_HD u64 mul(u64 a, u64 b) const { return f.mul(a, b); }
  RONK_HD u64 add(u64 a, u64 b) const { return f.add(a, b); }
  RONK_HD u64 one() const { return f.one(); }
  RONK_HD u64 zero() const { return 0; }
};
// planar [2][n]
template <class F>
struct AccPair {
  typedef E2 V;
  typedef F Field;
  Ext2<F> x;
  RONK_HD AccPair(const FriConsts& k, u64 w) : x(F(k), w) {}
  RONK_HD E2 load(const u64* a, size_t n, size_t i) const { return ext2_load(x.f, a, n, i); }
  RONK_HD void store(u64* out, size_t n, size_t i, E2 v) const { ext2_store(x.f, out, n, i, v); }
  RONK_HD E2 raw_load(const u64* a, size_t n, size_t i) const { return E2{a[i], a[n + i]}; }
  RONK_HD void raw_store(u64* out, size_t n, size_t i, E2 v) const { out[i] = v.c0; out[n + i] = v.c1; }
  RONK_HD E2 mul(E2 a, E2 b) const { return x.mul(a, b); }
  RONK_HD E2 add(E2 a, E2 b) const { return x.add(a, b); }
  RONK_HD E2 one() const { return x.one(); }
  RONK_HD E2 zero() const { return x.zero(); }
};

enum AccOperator { ACC_PROD, ACC_SUM };
template <class E, int OP>
struct AccOp {
  typedef typename E::V V;
  E e;
  RONK_HD AccOp(const FriConsts& k, u64 w) : e(k, w) {}
  RONK_HD V comb(V a, V b) const { if constexpr (OP == ACC_PROD) return e.mul(a, b); else return e.add(a, b); }
  RONK_HD V identity() const { if constexpr (OP == ACC_PROD) return e.one(); else return e.zero(); }
};

// ---------------------------------------------------------------------------------------------------- a lane's chunk
// the ACC_EPL elements from i0 on; the identity past the end
template <class O>
RONK_HD void acc_load_chunk(const O& op, const u64* a, size_t n, size_t i0, typename O::V (&v)[ACC_EPL]) {
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = decltype(R)::value;
    v[r] = i0 + r < n ? op.e.load(a, n, i0 + r) : op.identity();
  });
}
template <class O>
RONK_HD typename O::V acc_chunk_total(const O& op, const typename O::V (&v)[ACC_EPL]) {
  typename O::V t = v[0];
  deep_for<1, ACC_EPL>([&](auto R) { t = op.comb(t, v[decltype(R)::value]); });
  return t;
}
// the prefixes of the chunk from `base` (everything before it), inclusive or exclusive
template <class O>
RONK_HD void acc_write_chunk(const O& op, typename O::V base, const typename O::V (&v)[ACC_EPL], int exclusive, u64* out, size_t n,
                             size_t i0) {
  typename O::V run = base;
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = decltype(R)::value;
    const typename O::V next = op.comb(run, v[r]);
    if (i0 + r < n) op.e.store(out, n, i0 + r, exclusive ? run : next);
    run = next;
  });
}

// ---------------------------------------------------------------------------------------------------- the 256 lane sums
// step of the halving tree, stride s = 128, 64, .. 1, a barrier before each: buf[0] ends as the sum of all
template <class O>
RONK_HD void acc_tree_step(const O& op, typename O::V* buf, u32 lane, u32 s) {
  if (lane < s) buf[lane] = op.comb(buf[lane], buf[lane + s]);
}
// step s = 0 .. 7 of the Hillis-Steele scan: what lane writes to the OTHER buffer; after step 7 that is the inclusive scan
template <class O>
RONK_HD typename O::V acc_hs_step(const O& op, const typename O::V* src, u32 lane, u32 s) {
  const u32 d = (u32)1 << s;
  return lane >= d ? op.comb(src[lane - d], src[lane]) : src[lane];
}

// ---------------------------------------------------------------------------------------------------- phase 2
// lane l owns the totals [l chunk, (l + 1) chunk) of the B; flags (may be NULL): one word per block, OR-ed into *flag
template <class O>
RONK_HD typename O::V acc_totals_reduce(const O& op, const u64* work, u64 B, u32 lane, u64 chunk, const u64* flags, u64* flag) {
  typename O::V t = op.identity();
  const u64 j0 = (u64)lane * chunk;
  for (u64 j = j0; j < j0 + chunk && j < B; j++) {
    t = op.comb(t, op.e.raw_load(work, B, j));
    if (flags) *flag |= flags[j];
  }
  return t;
}
// the same totals become their exclusive prefixes, from `excl` = everything before the lane's first
template <class O>
RONK_HD void acc_totals_rewrite(const O& op, u64* work, u64 B, u32 lane, u64 chunk, typename O::V excl) {
  const u64 j0 = (u64)lane * chunk;
  for (u64 j = j0; j < j0 + chunk && j < B; j++) {
    const typename O::V v = op.e.raw_load(work, B, j);
    op.e.raw_store(work, B, j, excl);
    excl = op.comb(excl, v);
  }
}

// ---------------------------------------------------------------------------------------------------- the fused terms
// nrm[r] <- 1 / nrm[r] for the chunk's ACC_EPL base elements with one Fermat power; a zero becomes zero.  Returns whether there
// was one.
template <class F>
RONK_HD bool acc_chunk_invert(const Ext2<F>& x, u64 (&nrm)[ACC_EPL]) {
  const F& f = x.f;
  u64 pre[ACC_EPL];
  u64 run = f.one();
  u32 zeros = 0;
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = decltype(R)::value;
    if (nrm[r] == 0) { zeros |= (u32)1 << r; nrm[r] = f.one(); }
    pre[r] = run;
    run = f.mul(run, nrm[r]);
  });
  u64 inv = deep_inverse(x, run);
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = ACC_EPL - 1 - decltype(R)::value;
    const u64 ninv = f.mul(inv, pre[r]);
    inv = f.mul(inv, nrm[r]);
    nrm[r] = (zeros >> r) & 1 ? 0 : ninv;
  });
  return zeros != 0;
}
// num / den for the chunk: term[r] = num[r] conj(den[r]) / norm(den[r]), ZERO where den[r] is
template <class F>
RONK_HD bool acc_chunk_quotients(const Ext2<F>& x, const E2 (&num)[ACC_EPL], const E2 (&den)[ACC_EPL], E2 (&term)[ACC_EPL]) {
  u64 nrm[ACC_EPL];
  deep_for<0, ACC_EPL>([&](auto R) { constexpr int r = decltype(R)::value; nrm[r] = x.norm(den[r]); });
  const bool zero = acc_chunk_invert(x, nrm);
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = decltype(R)::value;
    term[r] = x.mul_base(x.mul(num[r], E2{den[r].c0, x.f.neg(den[r].c1)}), nrm[r]);
  });
  return zero;
}

// The permutation terms num_i / den_i of the rows i0 .. i0 + 7: num_i = prod_c (a_c[i] + beta id_c[i] + gamma), den_i the same
// with sigma_c.  wires, ids, sigma: [W][N] row-major, any 64-bit words; beta, gamma in register form.  Rows past N give ONE.
// Returns whether a denominator was ZERO.
template <class F>
RONK_HD bool acc_perm_chunk(const Ext2<F>& x, E2 beta, E2 gamma, const u64* wires, const u64* ids, const u64* sigma, u32 W, size_t N,
                            size_t i0, E2 (&term)[ACC_EPL]) {
  const F& f = x.f;
  // f.mul(raw, bx) is beta * raw in register form for any 64-bit raw word (deep_kernels.h deep_apx)
  const E2 bx{deep_apx(f, beta.c0), deep_apx(f, beta.c1)};
  E2 num[ACC_EPL], den[ACC_EPL];
  deep_for<0, ACC_EPL>([&](auto R) { constexpr int r = decltype(R)::value; num[r] = den[r] = x.one(); });
  for (u32 c = 0; c < W; c++) {
    const u64* ac = wires + (size_t)c * N;
    const u64* ic = ids + (size_t)c * N;
    const u64* sc = sigma + (size_t)c * N;
    deep_for<0, ACC_EPL>([&](auto R) {
      constexpr int r = decltype(R)::value;
      if (i0 + r < N) {
        const u64 id = ic[i0 + r], sg = sc[i0 + r];
        const u64 ag = f.add(f.in(ac[i0 + r]), gamma.c0);
        num[r] = x.mul(num[r], E2{f.add(ag, f.mul(id, bx.c0)), f.add(gamma.c1, f.mul(id, bx.c1))});
        den[r] = x.mul(den[r], E2{f.add(ag, f.mul(sg, bx.c0)), f.add(gamma.c1, f.mul(sg, bx.c1))});
      }
    });
  }
  return acc_chunk_quotients(x, num, den, term);
}

// The logUp terms sum_c m_c[i] / (alpha + v_c[i]) of the rows i0 .. i0 + 7 over the row's common denominator.  vals, mult:
// [C][N] row-major (mult NULL: all ones).  A column whose denominator is ZERO takes no part in its row (its term is ZERO); the
// common denominator is then never zero.  Rows past N give ZERO.  Returns whether there was such a column.
template <class F>
RONK_HD bool acc_logup_chunk(const Ext2<F>& x, E2 alpha, const u64* vals, const u64* mult, u32 C, size_t N, size_t i0,
                             E2 (&term)[ACC_EPL]) {
  const F& f = x.f;
  E2 num[ACC_EPL], den[ACC_EPL];
  bool zero = false;
  deep_for<0, ACC_EPL>([&](auto R) { constexpr int r = decltype(R)::value; num[r] = x.zero(); den[r] = x.one(); });
  for (u32 c = 0; c < C; c++) {
    const u64* vc = vals + (size_t)c * N;
    const u64* mc = mult ? mult + (size_t)c * N : nullptr;
    deep_for<0, ACC_EPL>([&](auto R) {
      constexpr int r = decltype(R)::value;
      if (i0 + r < N) {
        const E2 d{f.add(alpha.c0, f.in(vc[i0 + r])), alpha.c1};
        if ((d.c0 | d.c1) == 0) {
          zero = true;
        } else {
          const E2 share = mc ? x.mul_base(den[r], f.in(mc[i0 + r])) : den[r];
          num[r] = x.add(x.mul(num[r], d), share);
          den[r] = x.mul(den[r], d);
        }
      }
    });
  }
  acc_chunk_quotients(x, num, den, term);
  return zero;
}

// the chunk's terms as the caller sees them (canonical, planar [2][N])
template <class F>
RONK_HD void acc_store_terms(const Ext2<F>& x, const E2 (&term)[ACC_EPL], u64* out, size_t N, size_t i0) {
  deep_for<0, ACC_EPL>([&](auto R) {
    constexpr int r = decltype(R)::value;
    if (i0 + r < N) ext2_store(x.f, out, N, i0 + r, term[r]);
  });
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------- kernels
// the block's total from the lanes' totals: buf[0] after the tree
template <class O>
__device__ __forceinline__ void acc_block_reduce(const O& op, typename O::V t, typename O::V* buf) {
  const u32 lane = threadIdx.x;
  buf[lane] = t;
  for (u32 s = ACC_LANES / 2; s > 0; s >>= 1) {
    __syncthreads();
    acc_tree_step(op, buf, lane, s);
  }
  __syncthreads();
}
// the inclusive scan of the lanes' totals: returns the buffer that holds it
template <class O>
__device__ __forceinline__ const typename O::V* acc_block_scan(const O& op, typename O::V t, typename O::V (*buf)[ACC_LANES]) {
  const u32 lane = threadIdx.x;
  buf[0][lane] = t;
  __syncthreads();
  for (u32 s = 0; s < ACC_LOG2_LANES; s++) {
    buf[(s + 1) & 1][lane] = acc_hs_step(op, buf[s & 1], lane, s);
    __syncthreads();
  }
  return buf[ACC_LOG2_LANES & 1];
}

// no __restrict__ on a / out: the plain scans may run in place
template <class O>
__global__ void __launch_bounds__(ACC_LANES) acc_phase1_kernel(FriConsts k, u64 w, const u64* a, size_t n, u64* work) {
  __shared__ typename O::V buf[ACC_LANES];
  const O op(k, w);
  const u64 B = gridDim.x;
  typename O::V v[ACC_EPL];
  acc_load_chunk(op, a, n, (size_t)blockIdx.x * ACC_BLOCK + (size_t)threadIdx.x * ACC_EPL, v);
  acc_block_reduce(op, acc_chunk_total(op, v), buf);
  if (threadIdx.x == 0) op.e.raw_store(work, B, blockIdx.x, buf[0]);
}

// one workgroup; d_total: one element as the caller sees it (may be NULL); d_status (may be NULL): 0 or 1 from the blocks' flags
template <class O>
__global__ void __launch_bounds__(ACC_LANES) acc_phase2_kernel(FriConsts k, u64 w, u64* work, u64 B, u64* d_total, int* d_status) {
  __shared__ typename O::V buf[2][ACC_LANES];
  __shared__ int raised;
  const O op(k, w);
  const u32 lane = threadIdx.x;
  const u64 chunk = (B + ACC_LANES - 1) / ACC_LANES;
  if (lane == 0) raised = 0;
  u64 flag = 0;
  const typename O::V t = acc_totals_reduce(op, work, B, lane, chunk, d_status ? work + 2 * B : nullptr, &flag);
  const typename O::V* incl = acc_block_scan(op, t, buf);
  if (flag) raised = 1;
  acc_totals_rewrite(op, work, B, lane, chunk, lane ? incl[lane - 1] : op.identity());
  __syncthreads();
  if (lane == 0) {
    if (d_total) op.e.store(d_total, 1, 0, incl[ACC_LANES - 1]);
    if (d_status) *d_status = raised;
  }
}

template <class O>
__global__ void __launch_bounds__(ACC_LANES) acc_phase3_kernel(FriConsts k, u64 w, const u64* a, u64* out, size_t n, int exclusive,
                                                               const u64* work) {
  __shared__ typename O::V buf[2][ACC_LANES];
  const O op(k, w);
  const u64 B = gridDim.x;
  const u32 lane = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * ACC_BLOCK + (size_t)lane * ACC_EPL;
  typename O::V v[ACC_EPL];
  acc_load_chunk(op, a, n, i0, v);
  const typename O::V* incl = acc_block_scan(op, acc_chunk_total(op, v), buf);
  typename O::V base = op.e.raw_load(work, B, blockIdx.x);
  if (lane) base = op.comb(base, incl[lane - 1]);
  acc_write_chunk(op, base, v, exclusive, out, n, i0);
}

// phase 1 of the permutation product: the terms into Z, the block's product and flag into the workspace
template <class F>
__global__ void __launch_bounds__(ACC_LANES) acc_perm_terms_kernel(FriConsts k, u64 w, const u64* __restrict__ wires,
                                                                   const u64* __restrict__ ids, const u64* __restrict__ sigma, u32 W,
                                                                   size_t N, const u64* __restrict__ d_beta,
                                                                   const u64* __restrict__ d_gamma, u64* __restrict__ Z,
                                                                   u64* __restrict__ work) {
  typedef AccOp<AccPair<F>, ACC_PROD> O;
  __shared__ E2 buf[ACC_LANES];
  __shared__ int raised;
  const O op(k, w);
  const Ext2<F>& x = op.e.x;
  const u64 B = gridDim.x;
  const u32 lane = threadIdx.x;
  if (lane == 0) raised = 0;
  const size_t i0 = (size_t)blockIdx.x * ACC_BLOCK + (size_t)lane * ACC_EPL;
  const E2 beta{x.f.in(d_beta[0]), x.f.in(d_beta[1])}, gamma{x.f.in(d_gamma[0]), x.f.in(d_gamma[1])};
  E2 term[ACC_EPL];
  const bool zero = acc_perm_chunk(x, beta, gamma, wires, ids, sigma, W, N, i0, term);
  acc_store_terms(x, term, Z, N, i0);
  __syncthreads();
  if (zero) raised = 1;
  acc_block_reduce(op, acc_chunk_total(op, term), buf);
  if (lane == 0) {
    op.e.raw_store(work, B, blockIdx.x, buf[0]);
    work[2 * B + blockIdx.x] = (u64)raised;
  }
}

// phase 1 of the logUp sum
template <class F>
__global__ void __launch_bounds__(ACC_LANES) acc_logup_terms_kernel(FriConsts k, u64 w, const u64* __restrict__ vals,
                                                                    const u64* __restrict__ mult, u32 C, size_t N,
                                                                    const u64* __restrict__ d_alpha, u64* __restrict__ S,
                                                                    u64* __restrict__ work) {
  typedef AccOp<AccPair<F>, ACC_SUM> O;
  __shared__ E2 buf[ACC_LANES];
  __shared__ int raised;
  const O op(k, w);
  const Ext2<F>& x = op.e.x;
  const u64 B = gridDim.x;
  const u32 lane = threadIdx.x;
  if (lane == 0) raised = 0;
  const size_t i0 = (size_t)blockIdx.x * ACC_BLOCK + (size_t)lane * ACC_EPL;
  const E2 alpha{x.f.in(d_alpha[0]), x.f.in(d_alpha[1])};
  E2 term[ACC_EPL];
  const bool zero = acc_logup_chunk(x, alpha, vals, mult, C, N, i0, term);
  acc_store_terms(x, term, S, N, i0);
  __syncthreads();
  if (zero) raised = 1;
  acc_block_reduce(op, acc_chunk_total(op, term), buf);
  if (lane == 0) {
    op.e.raw_store(work, B, blockIdx.x, buf[0]);
    work[2 * B + blockIdx.x] = (u64)raised;
  }
}
#endif

}  // namespace ronk
