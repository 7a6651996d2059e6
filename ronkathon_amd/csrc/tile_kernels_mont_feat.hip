// tile_kernels_mont_feat.hip -- Montgomery-prime instantiations of the specialised passes that carry FEATURES (TileCfg::FEAT,
// ntt_tile.h; list RONK_CFG_TABLE_FEAT in tile_cfg_table.h): the pieces of a polynomial multiply over a generic odd 64-bit prime
// (reference src/polynomial/arithmetic.rs:97-119 for any PrimeField<P>) -- zero-padded forward transforms (FEAT 1, forward
// direction only), the second operand multiplied in on load (FEAT 2) and the truncated store (FEAT 4) of the inverse -- and the
// zero-padded batched Reed-Solomon encode (src/codes/reed_solomon.rs:42-52).  Without an instantiation a pass with features runs
// the generic Montgomery kernel (tile_kernels_mont.hip).
#include "tile_cfg_table.h"
#include "tile_kernel_def.h"

namespace ronk {

template <int LOGR, bool INV, int LOGC, int KIND, int FEAT>
__global__ void __launch_bounds__(1024) ntt_tile_kernel_mont_feat(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_kernel_main<LOGR, INV, LOGC, KIND, false, FEAT, MontField>(a, lds);
}

// instantiated in the direction a feature occurs in (tile_select.h): padding limits belong to forward transforms (multiply
// operands, encode), the second operand and the truncation to the multiply's inverse
hipError_t launch_mont_feat(int logr, bool inverse, int kind, int feat, const TileArgs& a, u32 grid, u32 block, size_t lds,
                            hipStream_t s) {
#define RONK_MONT_FEAT_CASE(LR, LC, KD, FT)                                                              \
  if (logr == LR && (int)a.logc == LC && kind == KD && feat == FT && inverse == (FT != 1))               \
    return launch_dyn<ntt_tile_kernel_mont_feat<LR, (FT != 1), LC, KD, FT>>(grid, block, lds, s, a);
  RONK_CFG_TABLE_FEAT(RONK_MONT_FEAT_CASE)
#undef RONK_MONT_FEAT_CASE
  return hipErrorInvalidValue;
}

}  // namespace ronk
