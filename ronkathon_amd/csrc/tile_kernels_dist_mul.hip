// tile_kernels_dist_mul.hip -- gfx950 instantiations of the fused middle of a SHARDED polynomial multiply (ntt_mul.h
// mul_mid_body, ronk_dist.hip ronk_poly_mul_sharded_dev): per rank, forward phase 2 of both operands read from the exchange's
// receive buffer, the pointwise product in registers, phase 1 of the swapped-split inverse with its global twiddle, stored into the
// inverse's send buffer -- one launch per inverse column chunk, the two spectra never in HBM.  Goldilocks and Montgomery primes.
// Shapes: the single-pass phases of NTT sizes 2^18 .. 2^25 (C = 2^9 .. 2^12 rows per pass) at the tile widths plan.h picks for
// them (pick_logc: 2^9 / 2^10 rows -> 16 columns, 2^11 -> 8, 2^12 -> 4).
#include <hip/hip_runtime.h>

#include "hip_launch.h"
#include "ntt_mul.h"
#include "tile_launch.h"

namespace ronk {

template <int LOGR, int LOGC, class FLD>
__global__ void __launch_bounds__(1024) ntt_mul_mid_dist_kernel(const TileArgs fa, const TileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  mul_mid_body<LOGR, LOGC, 4, FLD>(fa, ia, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); });
}

#define RONK_MUL_MID_DIST_TABLE(X) X(9, 4) X(10, 4) X(11, 3) X(12, 2)

bool mul_mid_dist_available(int logr, int logc) {
#define RONK_MID_HAS(LR, LC) if (logr == LR && logc == LC) return true;
  RONK_MUL_MID_DIST_TABLE(RONK_MID_HAS)
#undef RONK_MID_HAS
  return false;
}

hipError_t launch_mul_mid_dist(int logr, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds, hipStream_t s,
                               bool* found) {
#define RONK_MID_CASE(LR, LC)                                                                                  \
  if (logr == LR && (int)fa.logc == LC && mul_mid_matches_dist(fa, ia, LR, LC)) {                              \
    *found = true;                                                                                             \
    return fa.fc.p ? launch_dyn<ntt_mul_mid_dist_kernel<LR, LC, MontField>>(grid, block, lds, s, fa, ia)       \
                   : launch_dyn<ntt_mul_mid_dist_kernel<LR, LC, GlField>>(grid, block, lds, s, fa, ia);        \
  }
  RONK_MUL_MID_DIST_TABLE(RONK_MID_CASE)
#undef RONK_MID_CASE
  *found = false;
  return hipSuccess;
}

}  // namespace ronk
