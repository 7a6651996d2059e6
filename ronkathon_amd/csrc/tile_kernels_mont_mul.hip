// tile_kernels_mont_mul.hip -- the fused middle of a polynomial multiply (ntt_mul.h) over a Montgomery prime: forward row pass of
// both operands, pointwise product in registers (mul_plain: two Montgomery products, operands and result canonical), inverse
// column pass -- one launch instead of two, NTT(a) / NTT(b) never in HBM (reference src/polynomial/arithmetic.rs:97-119 for any
// PrimeField<P>).  Same shapes as the Goldilocks instantiations of tile_kernels_mul.hip that conv_dev uses: 2^11-row passes
// (NTT sizes 2^22, 2^23) and 2^10-row passes (2^21), 4-column tiles, both inverse twiddle forms.
#include <hip/hip_runtime.h>

#include "hip_launch.h"
#include "ntt_mul.h"
#include "tile_launch.h"

namespace ronk {

template <int LOGR, int LOGC, int KINDI>
__global__ void __launch_bounds__(1024) ntt_mul_mid_kernel_mont(const TileArgs fa, const TileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  mul_mid_body<LOGR, LOGC, KINDI, MontField>(fa, ia, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); });
}

hipError_t launch_mont_mul_mid(int logr, int kindi, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds,
                               hipStream_t s) {
#define RONK_MID_CASE(LR, LC, KD) \
  if (logr == LR && (int)fa.logc == LC && kindi == KD) return launch_dyn<ntt_mul_mid_kernel_mont<LR, LC, KD>>(grid, block, lds, s, fa, ia);
  RONK_MUL_MID_TABLE_MONT(RONK_MID_CASE)
#undef RONK_MID_CASE
  return hipErrorInvalidValue;
}

}  // namespace ronk
