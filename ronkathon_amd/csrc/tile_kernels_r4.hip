// tile_kernels_r4.hip -- the column / row passes of 2^9 and 2^10 rows with the R4 round structure (TileCfg::R4, ntt_tile.h):
// rounds of radix 16, 4 and R/64, the twiddle after the first round a wave-uniform SHIFT (omega_64^(a k1) = +-2^K with the
// reference's root convention omega = 7^((p-1)/n), src/algebra/field/mod.rs:70-75), ONE table twiddle per pass.  Same results
// as the (16, 16, 2 | 4) kernels of tile_kernels_cfg.hip.  OPT-IN (RONK_R4MID=1, tile_select.h): measured in round 5 it
// executes 5.5 % fewer VALU instructions per pass and is not faster (profiles/r05_r4_ab.txt), so the default stays with the
// (16, 16, 2 | 4) kernels; kept instantiated so that the measurement can be repeated and the parity tests keep covering it.
#include "tile_cfg_table.h"
#include "tile_kernel_def.h"

namespace ronk {

template <int LOGR, bool INV, int LOGC, int KIND>
__global__ void __launch_bounds__(1024) ntt_tile_kernel_r4(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_body<LOGR, INV, 0, TileCfg<LOGC, KIND, false, false, 0, true>>(a, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); });
}

template <int LR, int LC, int KD>
static hipError_t launch_r4(bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
  if constexpr (cfg_r4(LR, LC, KD))
    return inverse ? launch_dyn<ntt_tile_kernel_r4<LR, true, LC, KD>>(grid, block, lds, s, a)
                   : launch_dyn<ntt_tile_kernel_r4<LR, false, LC, KD>>(grid, block, lds, s, a);
  else return hipErrorInvalidValue;
}

hipError_t launch_tile_r4(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
#define RONK_R4_CASE(LR, LC, KD) \
  if (logr == LR && (int)a.logc == LC && kind == KD) return launch_r4<LR, LC, KD>(inverse, a, grid, block, lds, s);
  RONK_CFG_TABLE(RONK_R4_CASE)
#undef RONK_R4_CASE
  return hipErrorInvalidValue;
}

}  // namespace ronk
