// tile_kernel_def.h -- the __global__ wrappers of ntt_tile.h's tile body, shared by the translation units that instantiate
// them, and the per-form walkers that map a pass's (logr, logc, kind[, feat]) to an instantiation.  Which form runs a pass is
// decided in one place, tile_select.h (called by launch_tile, tile_kernels.hip); a walker only finds the instantiation and
// returns hipErrorInvalidValue when there is none.
#pragma once
#include "hip_launch.h"
#include "ntt_tile.h"

namespace ronk {

// Workgroup = 2^LOGR * C / 16 work-items (<= 1024), dynamic LDS = (2^LOGR + 2^LOGR/16) * C * 8 bytes (<= 136 KiB of the
// CU's 160 KiB).
template <int LOGR, bool INV, int LOGC, int KIND, bool HALF, int FEAT = 0, class FLD = GlField>
__device__ __forceinline__ void tile_kernel_main(const TileArgs& a, u64* lds) {
  tile_body<LOGR, INV, 0, TileCfg<LOGC, KIND, !HALF && !FEAT && !FLD::MONT && cfg_ldstw(LOGR, LOGC, KIND), HALF, FEAT>, FLD>(
      a, lds, threadIdx.x, xcd_tile_id(), [] { __syncthreads(); });
}

// the shapes with features (tile_cfg_table.h RONK_CFG_TABLE_FEAT; tile_kernels_feat.hip)
template <int LOGR, bool INV, int LOGC, int KIND, int FEAT>
__global__ void __launch_bounds__(1024) ntt_tile_kernel_feat(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_kernel_main<LOGR, INV, LOGC, KIND, false, FEAT>(a, lds);
}

template <int LOGR, bool INV, int LOGC, int KIND>
__global__ void __launch_bounds__(1024) ntt_tile_kernel(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_kernel_main<LOGR, INV, LOGC, KIND, false>(a, lds);
}

// TileCfg::HALF (two-phase 32-bit LDS exchanges, half the image): built for 8 resident waves per SIMD (<= 64 VGPRs), which
// is the point of halving the image
// waves per SIMD a HALF kernel is built for: 8 (64 VGPRs), except the two-round column pass with the full twiddle matrix
// (16 table entries + 16 coefficients live at the end), which spills 70-80 bytes per lane at 64 and gets 6 (80 VGPRs)
constexpr int half_wpe(int logr, int kind) { return (logr == 8 && kind == 3) ? 6 : 8; }

template <int LOGR, bool INV, int LOGC, int KIND>
__global__ void __launch_bounds__(1024, half_wpe(LOGR, KIND)) ntt_tile_kernel_half(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  tile_kernel_main<LOGR, INV, LOGC, KIND, true>(a, lds);
}

// `lds` is the full-size image: a HALF image holds 4-byte cells; an LDSTW shape stages its round twiddles behind the image
template <int LOGR, bool INV, int LOGC, int KIND, bool HALF = false>
static hipError_t launch_one(const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s) {
  if constexpr (HALF) return launch_dyn<ntt_tile_kernel_half<LOGR, INV, LOGC, KIND>>(grid, block, lds / 2, s, a);
  else return launch_dyn<ntt_tile_kernel<LOGR, INV, LOGC, KIND>>(grid, block, lds + (cfg_ldstw(LOGR, LOGC, KIND) ? (size_t)8 << LOGR : 0), s, a);
}

// the walkers, one per form (tile_select.h TileForm) and field
// tile_kernels_cfg.hip: RONK_CFG_TABLE and RONK_CFG_TABLE_DIST
hipError_t launch_tile_cfg(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s);
// tile_kernels_half.hip: RONK_CFG_TABLE with TileCfg::HALF (`lds` is the full-size image, the launcher halves it)
hipError_t launch_tile_cfg_half(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s);
// tile_kernels_feat.hip: RONK_CFG_TABLE_FEAT (zero-padded input, fused second operand, truncated output)
hipError_t launch_tile_cfg_feat(int logr, bool inverse, int kind, int feat, const TileArgs& a, u32 grid, u32 block, size_t lds,
                                hipStream_t s);
// tile_kernels_r4.hip: the 2^9 / 2^10-row shapes of RONK_CFG_TABLE with the [16 . 4] . [8 | 16] round structure (TileCfg::R4:
// one table-twiddle layer and one wave-uniform shift layer per pass instead of two table layers)
hipError_t launch_tile_r4(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s);
// tile_kernels_wl.hip (ntt_tile_wl.h): 2^10 .. 2^12-row x 4-column passes with one wave-local and one cross-wave exchange, both
// fields (a.fc); half = the half-image form (Goldilocks, 2^11 rows)
hipError_t launch_tile_wl(int logr, bool inverse, int kind, bool half, const TileArgs& a, u32 grid, hipStream_t s);
// tile_kernels_mont.hip: over a Montgomery prime (field_policy.h MontField; TileArgs::fc.p != 0) -- the generic kernel for every
// pass size and the shapes of RONK_CFG_TABLE; tile_kernels_mont_feat.hip: the shapes with features
hipError_t launch_mont_generic(int logr, bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s);
hipError_t launch_mont_cfg(int logr, bool inverse, int kind, const TileArgs& a, u32 grid, u32 block, size_t lds, hipStream_t s);
hipError_t launch_mont_feat(int logr, bool inverse, int kind, int feat, const TileArgs& a, u32 grid, u32 block, size_t lds,
                            hipStream_t s);

}  // namespace ronk
