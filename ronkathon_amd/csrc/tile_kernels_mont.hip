// tile_kernels_mont.hip -- the tile kernels over ANY odd prime p < 2^64 with enough 2-adicity (Montgomery form, R = 2^64).
//
// ronkathon's PrimeField<P> and Polynomial::fft / ifft are generic over the modulus (reference
// src/algebra/field/prime/mod.rs:39-52, src/polynomial/mod.rs:273-323, :430-484).  The bodies are ntt_tile.h / ntt_small.h
// instantiated with field_policy.h's MontField: the prime, -p^-1 mod 2^64, 2^128 mod p and the eight roots of a 16-point
// register round arrive in TileArgs::fc (kernel arguments -> SGPRs); every table the plan uploads holds w * 2^64 mod p, so a
// twiddle costs one Montgomery product and coefficients stay canonical everywhere (plan.h HostField::tab).
//   generic instantiation (KIND 0)  every pass size 2^4 .. 2^12, every feature (zero padding, second operand, truncation):
//                                   the polynomial multiply, the staged single-pass plans, three-pass plans
//   specialised shapes              RONK_CFG_TABLE (tile_cfg_table.h): the column / row passes of the two-pass plans
//   (the latency form, ntt_small.h: small_kernels.hip)
#include "tile_cfg_table.h"
#include "tile_kernel_def.h"

namespace ronk {

template <int LOGR, bool INV, int LOGC, int KIND>
__global__ void __launch_bounds__(1024) ntt_tile_kernel_mont(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_kernel_main<LOGR, INV, LOGC, KIND, false, 0, MontField>(a, lds);
}

hipError_t launch_mont_generic(int logr, bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
  switch (logr) {
#define RONK_MONT_GENERIC_CASE(LR)                                                                           \
    case LR: return inverse ? launch_dyn<ntt_tile_kernel_mont<LR, true, -1, 0>>(grid, block, lds, s, a)      \
                            : launch_dyn<ntt_tile_kernel_mont<LR, false, -1, 0>>(grid, block, lds, s, a);
    RONK_MONT_GENERIC_CASE(4) RONK_MONT_GENERIC_CASE(5) RONK_MONT_GENERIC_CASE(6) RONK_MONT_GENERIC_CASE(7) RONK_MONT_GENERIC_CASE(8)
    RONK_MONT_GENERIC_CASE(9) RONK_MONT_GENERIC_CASE(10) RONK_MONT_GENERIC_CASE(11) RONK_MONT_GENERIC_CASE(12)
#undef RONK_MONT_GENERIC_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_mont_cfg(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
#define RONK_MONT_CASE(LR, LC, KD)                                                                   \
  if (logr == LR && (int)a.logc == LC && kind == KD)                                                 \
    return inverse ? launch_dyn<ntt_tile_kernel_mont<LR, true, LC, KD>>(grid, block, lds, s, a)      \
                   : launch_dyn<ntt_tile_kernel_mont<LR, false, LC, KD>>(grid, block, lds, s, a);
  RONK_CFG_TABLE(RONK_MONT_CASE)
#undef RONK_MONT_CASE
  return hipErrorInvalidValue;
}

}  // namespace ronk
