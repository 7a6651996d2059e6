// tile_kernels_mul.hip -- gfx950 instantiations of the fused middle of a polynomial multiply (ntt_mul.h): forward row pass of
// both operands, pointwise product in registers, inverse column pass -- one launch instead of two, NTT(a) / NTT(b) never in HBM.
#include <hip/hip_runtime.h>

#include "hip_launch.h"
#include "ntt_mul.h"
#include "tile_launch.h"

namespace ronk {

template <int LOGR, int LOGC, int KINDI>
__global__ void __launch_bounds__(1024) ntt_mul_mid_kernel(const TileArgs fa, const TileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  mul_mid_body<LOGR, LOGC, KINDI>(fa, ia, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); });
}

bool mul_mid_available(int logr, int logc, int kindi, bool mont) {
#define RONK_MID_HAS(LR, LC, KD) if (logr == LR && logc == LC && kindi == KD) return true;
  if (mont) { RONK_MUL_MID_TABLE_MONT(RONK_MID_HAS) }
  else { RONK_MUL_MID_TABLE(RONK_MID_HAS) }
#undef RONK_MID_HAS
  return false;
}

hipError_t launch_mul_mid(int logr, int kindi, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds, hipStream_t s) {
  if (fa.fc.p) return launch_mont_mul_mid(logr, kindi, fa, ia, grid, block, lds, s);   // tile_kernels_mont_mul.hip
#define RONK_MID_CASE(LR, LC, KD) \
  if (logr == LR && (int)fa.logc == LC && kindi == KD) return launch_dyn<ntt_mul_mid_kernel<LR, LC, KD>>(grid, block, lds, s, fa, ia);
  RONK_MUL_MID_TABLE(RONK_MID_CASE)
#undef RONK_MID_CASE
  return hipErrorInvalidValue;
}

}  // namespace ronk
