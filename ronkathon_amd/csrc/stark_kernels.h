// stark_kernels.h -- the bodies the STARK layer adds to the merged stages (csrc/ronk_stark.hip; include/ronk_ntt.h "STARK";
// DESIGN.md section 23): the quotient split, the coset scaling of a trace round's coefficients, and the one-lane transcript steps
// on the sponge body of poseidon_kernels.h.
//
// The split reads the planar [2][M] output of the two inverse transforms of T, c'_j = c_j s^j, and writes
//   coef [2B][N]   row 2 i + pl, word k = c'_(i N + k) s^-(i N + k)    the monomial coefficients of piece i: what the opening evaluates
//   msg  [2B][N]   row 2 i + pl, word k = c'_(i N + k) s^-(i N)        piece i in the coset basis: what the encode transforms
// A lane owns the residue k of the index: it walks the B pieces i N + k of both planes, so adjacent lanes read adjacent words of
// every piece and write adjacent words of every row, 8 bytes per lane per access.  Its two multipliers start at s^-k (ONE power
// per lane) and 1 and advance by the constant s^-N from piece to piece; a lane that owns several residues (grid-stride)
// advances its start by the constant s^-stride.  No power per element and no table.
//
// Field policies are those of fri_kernels.h; any 64-bit input word is reduced, outputs are canonical.  Plain C++ on uint64, so
// tests/emu/emu_stark.cpp compiles the same bodies for the host.
#pragma once
#include "ext2.h"
#include "fri_kernels.h"

namespace ronk {

static constexpr u32 STARK_MAX_R = 4;    // trace rounds
static constexpr u32 STARK_MAX_K = 8;    // opening points: zeta and its rotations
static constexpr u32 STARK_MAX_CHAL = 32, STARK_MAX_J = 64;   // the limits of ronk_air_check

// a^e on words in register form
template <class F>
RONK_HD u64 stark_pow(const F& f, u64 a, u64 e) {
  u64 r = f.one();
  while (e) {
    if (e & 1) r = f.mul(r, a);
    a = f.mul(a, a);
    e >>= 1;
  }
  return r;
}

// the canonical word of x e for ANY 64-bit word x and a multiplier in register form
template <class F>
RONK_HD u64 stark_scale(const F& f, u64 x, u64 e) { return f.out(f.mul(f.in(x), e)); }
// Montgomery: x (e R) R^-1 is that word already -- one product, no conversion on either side (field_policy.h)
RONK_HD u64 stark_scale(const FriMont& f, u64 x, u64 e) { return f.mul(x, e); }

// what a split launch knows about the shift (register form): s^-1, s^-N and s^-stride, stride the lanes of the grid
struct StarkShift {
  u64 sinv, sinv_n, sinv_stride;
};

// the residues k0, k0 + stride, .. < N of one lane.  cin: [2][M]; coef, msg: [2B][N].
template <class F>
RONK_HD void stark_split_lane(const F& f, const StarkShift& sh, u32 log2n, u32 log2b, u64 k0, u64 stride, const u64* cin, u64* coef,
                              u64* msg) {
  const u64 N = (u64)1 << log2n, B = (u64)1 << log2b, M = N << log2b;
  if (k0 >= N) return;
  u64 e0 = stark_pow(f, sh.sinv, k0);
  for (u64 k = k0; k < N; k += stride) {
    u64 ea = e0, eb = f.one();
    for (u64 i = 0; i < B; i++) {
      const u64 j = (i << log2n) + k, row = ((2 * i) << log2n) + k;
      const u64 c0 = cin[j], c1 = cin[M + j];
      coef[row] = stark_scale(f, c0, ea);
      coef[row + N] = stark_scale(f, c1, ea);
      msg[row] = stark_scale(f, c0, eb);
      msg[row + N] = stark_scale(f, c1, eb);
      ea = f.mul(ea, sh.sinv_n);
      eb = f.mul(eb, sh.sinv_n);
    }
    e0 = f.mul(e0, sh.sinv_stride);
  }
}

// a trace round's coefficients into the coset basis: msg[c][k] = coef[c][k] s^k for the C rows of N words; the lane's multiplier
// is one power and serves every row.  sh: s, unused, s^stride.
template <class F>
RONK_HD void stark_shift_lane(const F& f, const StarkShift& sh, u32 log2n, u32 C, u64 k0, u64 stride, const u64* coef, u64* msg) {
  const u64 N = (u64)1 << log2n;
  if (k0 >= N) return;
  u64 e = stark_pow(f, sh.sinv, k0);
  for (u64 k = k0; k < N; k += stride) {
    for (u32 c = 0; c < C; c++) msg[((u64)c << log2n) + k] = stark_scale(f, coef[((u64)c << log2n) + k], e);
    e = f.mul(e, sh.sinv_stride);
  }
}

// ---------------------------------------------------------------------------------------------------- transcript, one lane
// t = sponge(seed[d] || pub[2 n_pub]) squeezing d words; the public pairs are the first entries of the challenge table
template <class PF, int W>
RONK_HD void stark_begin(const PF& pf, const PoseidonConsts& k, u32 d, const u64* seed, const u64* pub, u32 n_pub, u64* t, u64* chal) {
  poseidon_sponge<PF, W>(pf, k, (u64)d + 2 * (u64)n_pub, d, [&](u64 j) { return j < d ? seed[j] : pub[j - d]; },
                         [&](u64 q, u64 v) { t[q] = v; });
  for (u32 j = 0; j < 2 * n_pub; j++) chal[j] = pf.out(pf.in(pub[j]));
}

// out = sponge(t || root) squeezing d + n_draw words: t <- out[:d], draw <- the rest (canonical).  The sponge absorbs all of
// its input before it squeezes, so t is rewritten in place.
template <class PF, int W>
RONK_HD void stark_draw(const PF& pf, const PoseidonConsts& k, u32 d, u64* t, const u64* root, u32 n_draw, u64* draw) {
  poseidon_sponge<PF, W>(pf, k, 2 * (u64)d, (u64)d + n_draw, [&](u64 j) { return j < d ? t[j] : root[j - d]; },
                         [&](u64 q, u64 v) {
                           if (q < d) t[q] = v;
                           else draw[q - d] = v;
                         });
}

// lambda_j = lambda^j, j < J, as [J][2] canonical words, by repeated products
template <class F>
RONK_HD void stark_weights(const Ext2<F>& x, const u64* lambda, u32 J, u64* out) {
  const E2 l{x.f.in(lambda[0]), x.f.in(lambda[1])};
  E2 a = x.one();
  for (u32 j = 0; j < J; j++) {
    out[2 * j] = x.f.out(a.c0);
    out[2 * j + 1] = x.f.out(a.c1);
    a = x.mul(a, l);
  }
}

// the multipliers w_N^rot of the K points, register form
struct StarkRots {
  u64 m[STARK_MAX_K];
  u32 K;
};
// z_k = zeta w_N^rot_k as planar [2][K] canonical words
template <class F>
RONK_HD void stark_points(const F& f, const u64* zeta, const StarkRots& r, u64* z) {
  const u64 c0 = f.in(zeta[0]), c1 = f.in(zeta[1]);
  for (u32 k = 0; k < r.K; k++) {
    z[k] = f.out(f.mul(c0, r.m[k]));
    z[r.K + k] = f.out(f.mul(c1, r.m[k]));
  }
}

#if defined(__HIPCC__)
template <class F>
__global__ void __launch_bounds__(256) stark_split_kernel(FriConsts k, StarkShift sh, u32 log2n, u32 log2b, const u64* __restrict__ cin,
                                                          u64* __restrict__ coef, u64* __restrict__ msg) {
  const F f(k);
  stark_split_lane(f, sh, log2n, log2b, blockIdx.x * (u64)blockDim.x + threadIdx.x, (u64)gridDim.x * blockDim.x, cin, coef, msg);
}

template <class F>
__global__ void __launch_bounds__(256) stark_shift_kernel(FriConsts k, StarkShift sh, u32 log2n, u32 C, const u64* __restrict__ coef,
                                                          u64* __restrict__ msg) {
  const F f(k);
  stark_shift_lane(f, sh, log2n, C, blockIdx.x * (u64)blockDim.x + threadIdx.x, (u64)gridDim.x * blockDim.x, coef, msg);
}

template <class PF, int W>
__global__ void __launch_bounds__(64) stark_begin_kernel(PoseidonConsts k, u32 d, const u64* seed, const u64* pub, u32 n_pub, u64* t,
                                                         u64* chal) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  stark_begin<PF, W>(pf, k, d, seed, pub, n_pub, t, chal);
}

template <class PF, int W>
__global__ void __launch_bounds__(64) stark_draw_kernel(PoseidonConsts k, u32 d, u64* t, const u64* root, u32 n_draw, u64* draw) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  stark_draw<PF, W>(pf, k, d, t, root, n_draw, draw);
}

template <class F>
__global__ void __launch_bounds__(64) stark_weights_kernel(FriConsts k, u64 w, const u64* lambda, u32 J, u64* out) {
  if (blockIdx.x || threadIdx.x) return;
  const F f(k);
  const Ext2<F> x(f, w);
  stark_weights(x, lambda, J, out);
}

template <class F>
__global__ void __launch_bounds__(64) stark_points_kernel(FriConsts k, const u64* zeta, StarkRots r, u64* z) {
  if (blockIdx.x || threadIdx.x) return;
  const F f(k);
  stark_points(f, zeta, r, z);
}

// bit 128: zeta (canonical, as squeezed) has a zero second word
__global__ void __launch_bounds__(64) stark_flag_kernel(const u64* zeta, int* status) {
  if (blockIdx.x || threadIdx.x) return;
  if (zeta[1] == 0) atomicOr(status, 128);
}
#endif

}  // namespace ronk
