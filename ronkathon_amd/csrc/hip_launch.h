// hip_launch.h -- what every kernel launch of the library shares: the dynamic-LDS launch helper and the XCD-aware numbering of
// a grid's tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ronk {

// Launches kernel K with `lds` bytes of dynamic LDS.  Above the default 48 KiB the kernel must be allowed the CU's 160 KiB
// first; HIP keeps that attribute per (kernel, DEVICE), so it is set once per device ordinal (benign race: the call is
// idempotent).
template <auto K, class... A>
hipError_t launch_dyn(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  static bool attr_done[64] = {};
  if (lds > 48 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !attr_done[dev]) {
      e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_done[dev] = true;
    }
  }
  hipLaunchKernelGGL(K, grid, block, lds, s, args...);
  return hipGetLastError();
}

// The dispatcher hands workgroup b to XCD b % 8 (observed, for speed only): renumber so that each XCD works on a contiguous
// run of tiles -- neighbouring tiles share 128-byte lines and twiddle rows, which then hit in that XCD's private L2.
// Bijective for any grid size.
__device__ __forceinline__ uint32_t xcd_tile_id() {
  const uint32_t nb = gridDim.x, b = blockIdx.x;
  const uint32_t q = nb >> 3, r = nb & 7, xcd = b & 7, idx = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace ronk
