// tile_kernels.hip -- gfx950 instantiations of the generic NTT tile kernel (ntt_tile.h) and the launcher of a tile pass.
//
// One __global__ per (LOGR, direction) that reads every stride and flag from TileArgs; passes whose shape has a specialised
// instantiation run that one instead.  tile_select.h decides which, for both fields.
#include "tile_kernel_def.h"
#include "tile_launch.h"
#include "tile_select.h"

namespace ronk {

template <bool INV>
static hipError_t launch_dir(int logr, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
  switch (logr) {
#define RONK_GENERIC_CASE(LR) case LR: return launch_one<LR, INV, -1, 0>(a, grid, block, lds, s);
    RONK_GENERIC_CASE(4) RONK_GENERIC_CASE(5) RONK_GENERIC_CASE(6) RONK_GENERIC_CASE(7) RONK_GENERIC_CASE(8)
    RONK_GENERIC_CASE(9) RONK_GENERIC_CASE(10) RONK_GENERIC_CASE(11) RONK_GENERIC_CASE(12)
#undef RONK_GENERIC_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_tile(int logr, bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
  const TileChoice c = select_tile(a, logr, inverse, grid, block, tile_env());
  const bool mont = a.fc.p != 0;   // a Montgomery prime (field_policy.h)
  switch (c.form) {
    case TileForm::CFG:
      return mont ? launch_mont_cfg(logr, inverse, c.kind, a, grid, block, lds, s) : launch_tile_cfg(logr, inverse, c.kind, a, grid, block, lds, s);
    case TileForm::HALF: return launch_tile_cfg_half(logr, inverse, c.kind, a, grid, block, lds, s);
    case TileForm::FEAT:
      return mont ? launch_mont_feat(logr, inverse, c.kind, c.feat, a, grid, block, lds, s)
                  : launch_tile_cfg_feat(logr, inverse, c.kind, c.feat, a, grid, block, lds, s);
    case TileForm::WL_FULL:
    case TileForm::WL_HALF: return launch_tile_wl(logr, inverse, c.kind, c.form == TileForm::WL_HALF, a, grid, s);
    case TileForm::R4: return launch_tile_r4(logr, inverse, c.kind, a, grid, block, lds, s);
    case TileForm::GENERIC: break;
  }
  if (mont) return launch_mont_generic(logr, inverse, a, grid, block, lds, s);
  return inverse ? launch_dir<true>(logr, a, grid, block, lds, s) : launch_dir<false>(logr, a, grid, block, lds, s);
}

}  // namespace ronk
