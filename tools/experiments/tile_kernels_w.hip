// tile_kernels_w.hip -- EXPERIMENT (not built into the library; see ntt_tile_w.h): gfx950 instantiations of the tile body with a wave-local first exchange (ntt_tile_w.h): 2^11-row,
// 4-column tiles of the two-pass plans (the two-lane plan of ronk_ntt_forward_many_dev, 2^21 / 2^22 / 2^23 shapes).
#include <hip/hip_runtime.h>

#include "ntt_tile_w.h"
#include "../../ronkathon_amd/csrc/hip_launch.h"
#include "../../ronkathon_amd/csrc/tile_launch.h"

namespace ronk {

template <bool INV, int KIND>
__global__ void __launch_bounds__(512, 2) ntt_tile_w_kernel(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_body_w<INV, KIND>(a, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); }, [] { __builtin_amdgcn_wave_barrier(); });
}

template <bool INV, int KIND>
static hipError_t launch_w(const TileArgs& a, u32 grid, hipStream_t s) {
  return launch_dyn<ntt_tile_w_kernel<INV, KIND>>(grid, 512, TW_LDS_BYTES, s, a);
}

hipError_t launch_tile_w(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, hipStream_t s, bool* found) {
  *found = tile_w_matches(a, logr, kind);
  if (!*found) return hipSuccess;
  switch (kind) {
    case 1: return inverse ? launch_w<true, 1>(a, grid, s) : launch_w<false, 1>(a, grid, s);
    case 2: return inverse ? launch_w<true, 2>(a, grid, s) : launch_w<false, 2>(a, grid, s);
    default: return inverse ? launch_w<true, 3>(a, grid, s) : launch_w<false, 3>(a, grid, s);
  }
}

}  // namespace ronk
