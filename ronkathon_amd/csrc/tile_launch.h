// tile_launch.h -- the launchers of the instantiated tile kernels, Goldilocks or Montgomery prime by TileArgs::fc.p
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_tile.h"

namespace ronk {
// one pass of a plan (tile_kernels.hip): tile_select.h picks the body, the per-form walkers (tile_kernel_def.h) launch it
hipError_t launch_tile(int logr, bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds_bytes, hipStream_t stream);
// the latency form of a pass (ntt_small.h: 4 coefficients per work-item), 2^4 .. 2^10 rows (small_kernels.hip)
hipError_t launch_small(int logr, bool inverse, const TileArgs& a, u32 grid, u32 block, size_t lds_bytes, hipStream_t stream);
// the fused middle of a polynomial multiply (ntt_mul.h, tile_kernels_mul.hip / tile_kernels_mont_mul.hip): fa = the forward
// plan's row pass over the batch of two operands, ia = the inverse plan's column pass; grid = tiles of ONE operand.
// mul_mid_available: is there an instantiation for (rows, log2 tile columns, inverse twiddle form) over this field?  Asked
// BEFORE the forward column pass is enqueued; launch_mul_mid returns hipErrorInvalidValue without one
bool mul_mid_available(int logr, int logc, int kindi, bool mont);
hipError_t launch_mul_mid(int logr, int kindi, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds_bytes,
                          hipStream_t stream);
hipError_t launch_mont_mul_mid(int logr, int kindi, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds_bytes,
                               hipStream_t stream);   // (the Montgomery walker behind launch_mul_mid)
// the sharded multiply's middle (tile_kernels_dist_mul.hip): fa = forward phase 2 over the operand pair, ia = phase 1 of the
// swapped-split inverse, both restricted to one inverse column chunk; grid = tiles of ONE operand; Goldilocks or Montgomery (fa.fc)
bool mul_mid_dist_available(int logr, int logc);
hipError_t launch_mul_mid_dist(int logr, const TileArgs& fa, const TileArgs& ia, u32 grid, u32 block, size_t lds_bytes,
                               hipStream_t stream, bool* found);
}
