// ext2_kernels.h -- element-wise kernels over the quadratic extension F_p[t] / (t^2 - W) (ext2.h; csrc/ronk_ext2.hip;
// include/ronk_ntt.h "quadratic extension").  Arrays are PLANAR: n elements are [2][n] words, the c0 plane first, the c1 plane at
// offset n -- the layout of the extension FRI layers (fri_kernels.h), so the two families feed each other, and the many-array
// NTT over the two planes is the transform of an extension-valued polynomial.
//
// Grid-stride, one element per lane per step, 8 bytes per lane per plane (field_kernels.h).  The base policies are those of the
// FRI bodies: FriGl keeps canonical words, FriMont keeps x R mod p; any 64-bit input word is reduced by `in`, outputs are
// canonical.  An element is read whole before it is written, so `out` may alias an input elementwise.
#pragma once
#include "ext2.h"
#include "fri_kernels.h"

namespace ronk {

enum Ext2Op { EXT2_ADD, EXT2_SUB, EXT2_MUL };

template <class F>
RONK_HD E2 ext2_load(const F& f, const u64* a, size_t n, size_t i) { return E2{f.in(a[i]), f.in(a[n + i])}; }
template <class F>
RONK_HD void ext2_store(const F& f, u64* out, size_t n, size_t i, E2 v) { out[i] = f.out(v.c0); out[n + i] = f.out(v.c1); }

// the constants of a launch for a field without transform roots: only the Montgomery numbers are read
inline FriConsts ext2_host_consts(bool mont, u64 p) {
  FriConsts k{};
  if (!mont) return k;
  const mont64::Field mf = mont64::make_field(p);
  k.fc.p = p; k.fc.pinv = mf.pinv; k.fc.r2 = mf.r2;
  for (u32 j = 0; j < 8; j++) k.fc.w16[j] = mf.one;
  return k;
}

#if defined(__HIPCC__)
// no __restrict__: in and out may be the same array
template <class F, int OP>
__global__ void __launch_bounds__(256) ext2_binary_kernel(FriConsts k, u64 w, const u64* a, const u64* b, u64* out, size_t n) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const E2 u = ext2_load(f, a, n, i), v = ext2_load(f, b, n, i);
    ext2_store(f, out, n, i, OP == EXT2_ADD ? x.add(u, v) : OP == EXT2_SUB ? x.sub(u, v) : x.mul(u, v));
  }
}

template <class F>
__global__ void __launch_bounds__(256) ext2_neg_kernel(FriConsts k, u64 w, const u64* a, u64* out, size_t n) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    ext2_store(f, out, n, i, x.neg(ext2_load(f, a, n, i)));
}

// s: n base words
template <class F>
__global__ void __launch_bounds__(256) ext2_mul_base_kernel(FriConsts k, u64 w, const u64* a, const u64* s, u64* out, size_t n) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    ext2_store(f, out, n, i, x.mul_base(ext2_load(f, a, n, i), f.in(s[i])));
}

template <class F>
__global__ void __launch_bounds__(256) ext2_pow_kernel(FriConsts k, u64 w, const u64* a, u64 e, u64* out, size_t n) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    ext2_store(f, out, n, i, x.pow(ext2_load(f, a, n, i), e));
}

// the reference's inverse(); the zero element raises *flag and is written as (0, 0), as vec_pow_kernel does for a zero word
template <class F>
__global__ void __launch_bounds__(256) ext2_inv_kernel(FriConsts k, u64 w, const u64* a, u64* out, size_t n, int* flag) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const E2 u = ext2_load(f, a, n, i);
    if (flag && (u.c0 | u.c1) == 0) *flag = 1;
    ext2_store(f, out, n, i, x.inv(u));
  }
}
#endif

}  // namespace ronk
