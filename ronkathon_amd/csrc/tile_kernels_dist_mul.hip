// tile_kernels_dist_mul.hip -- gfx950 instantiations of the fused middle of a SHARDED polynomial multiply (ntt_mul.h
// mul_mid_body, ronk_dist.hip ronk_poly_mul_sharded_dev): per rank, forward phase 2 of both operands read from the exchange's
// receive buffer, the pointwise product in registers, phase 1 of the swapped-split inverse with its global twiddle, stored into the
// inverse's send buffer -- one launch per inverse column chunk, the two spectra never in HBM.  Goldilocks and Montgomery primes.
// Shapes: the single-pass phases of NTT sizes 2^18 .. 2^25 (C = 2^9 .. 2^12 rows per pass) at the tile widths plan.h picks for
// them (pick_logc: 2^9 / 2^10 rows -> 16 columns, 2^11 -> 8, 2^12 -> 4).
#include <hip/hip_runtime.h>

#include "ntt_mul.h"
#include "tile_launch.h"

namespace ronk {

template <int LOGR, int LOGC, class FLD>
__global__ void __launch_bounds__(1024) ntt_mul_mid_dist_kernel(const TileArgs fa, const TileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  // XCD-aware renumbering (tile_kernel_def.h): each XCD works on a contiguous run of tiles
  const u32 nb = gridDim.x, b = blockIdx.x;
  const u32 q = nb >> 3, r = nb & 7, xcd = b & 7, idx = b >> 3;
  const u32 bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  mul_mid_body<LOGR, LOGC, 4, FLD>(fa, ia, lds, threadIdx.x, bid, [] { __syncthreads(); });
}

template <int LOGR, int LOGC, class FLD>
static hipError_t launch_mid_dist(const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds, hipStream_t s) {
  static bool attr_done[64] = {};   // per (kernel, device), see launch_one
  if (lds > 48 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !attr_done[dev]) {
      e = hipFuncSetAttribute((const void*)ntt_mul_mid_dist_kernel<LOGR, LOGC, FLD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_done[dev] = true;
    }
  }
  hipLaunchKernelGGL((ntt_mul_mid_dist_kernel<LOGR, LOGC, FLD>), dim3(grid), dim3(block), lds, s, fa, ia);
  return hipGetLastError();
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
    return fa.fc.p ? launch_mid_dist<LR, LC, MontField>(fa, ia, grid, block, lds, s)                           \
                   : launch_mid_dist<LR, LC, GlField>(fa, ia, grid, block, lds, s);                            \
  }
  RONK_MUL_MID_DIST_TABLE(RONK_MID_CASE)
#undef RONK_MID_CASE
  *found = false;
  return hipSuccess;
}

}  // namespace ronk
