// ronk_pow.hip -- C ABI of libronk_ntt.so, part 14: proof-of-work grinding on the Poseidon sponge (csrc/pow_kernels.h;
// include/ronk_ntt.h "proof of work").  ronk_fri.hip uses pow_grind_launch / pow_reseed_launch (runtime.h)
// for the step between FRI's commit phase and its query phase.
#include "runtime.h"
#include "hip_launch.h"
#include "poseidon_handle.h"
#include "pow_kernels.h"

// ------------------------------------------------------------------------------------- kernels
template <class PF, int W>
__global__ void __launch_bounds__(64) pow_prefix_kernel(PoseidonConsts k, u32 seed_len, const u64* seed, u64* state0, u64* nonce) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  pow_prefix<PF, W>(pf, k, seed_len, seed, state0, nonce);
}

// The found word before a candidate: a relaxed atomic load at agent scope, a real load in every iteration (it bypasses the CU's
// L1).  RONK_POW_POLL_RMW=1 builds the other form of the A/B in DESIGN.md section 18: once per wavefront, the first active lane
// reads the word by an agent-scope atomic minimum with 2^64 - 1, which changes nothing and is performed where the hits' minima
// are, and the other lanes take its value.
#ifndef RONK_POW_POLL_RMW
#define RONK_POW_POLL_RMW 0
#endif
__device__ __forceinline__ u64 pow_found_word(u64* nonce) {
#if RONK_POW_POLL_RMW
  u64 v = 0;
  if (__lane_id() == (unsigned)__builtin_ctzll(__ballot(1)))
    v = __hip_atomic_fetch_min(nonce, POW_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
#else
  return __hip_atomic_load(nonce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// Lane g tries g, g + T, ...; the found word is read from memory before every candidate and lowered by a hit.  The result is the
// smallest solution whatever the order in which the lanes run (pow_kernels.h): no lane waits for another.  state0 was written
// by the launch before this one and is read through wave-uniform addresses (scalar loads).
template <class PF, int W>
__global__ void __launch_bounds__(256) pow_search_kernel(PoseidonConsts k, const u64* state0, u32 slot, u32 bits, u32 log2_limit, u64 T,
                                                         u64* nonce) {
  u64 n = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (n >= T) return;
  const PF pf(k);
  PosTable st = RONK_POS_TABLE(state0);
  u64 s0[W];
#pragma unroll
  for (int i = 0; i < W; i++) s0[i] = st[i];
  const u64 mask = ((u64)1 << bits) - 1, limit = (u64)1 << log2_limit;
  while (pow_search_step<PF, W>(
      pf, k, s0, slot, mask, limit, T, n, [&]() { return pow_found_word(nonce); },
      [&](u64 hit) { atomicMin((unsigned long long*)nonce, (unsigned long long)hit); })) {
  }
}

template <class PF, int W>
__global__ void __launch_bounds__(64) pow_verify_kernel(PoseidonConsts k, u32 seed_len, const u64* seed, u32 bits, u32 log2_limit,
                                                        const u64* nonce, int* ok) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  u64 word;
  *ok = pow_squeeze<PF, W>(pf, k, seed_len, seed, *nonce, bits, log2_limit, 1, &word);
}

// u <- sponge(u || [*nonce]) squeezing d words, in place; with `status`, bit 64 when the nonce is out of range or fails
template <class PF, int W>
__global__ void __launch_bounds__(64) pow_reseed_kernel(PoseidonConsts k, u32 d, u64* u, u32 bits, u32 log2_limit, const u64* nonce,
                                                        int* status) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  const int ok = pow_squeeze<PF, W>(pf, k, d, u, *nonce, bits, log2_limit, d, u);
  if (status && !ok) atomicOr(status, 64);
}

// ------------------------------------------------------------------------------------- launches
// The default number of lanes: a quarter of those the device keeps resident for the search kernel of this field and width (per
// device ordinal, asked once).  With every resident slot taken the wavefronts of a SIMD advance unevenly, some run far past the
// nonce while the one that holds it lags, and the time per call scatters; at a quarter the rate is the highest and even
// (DESIGN.md section 18).
template <class PF, int W>
static int pow_default_lanes(u64* lanes) {
  static u64 cache[64] = {};
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && cache[dev]) { *lanes = cache[dev]; return RONK_OK; }
  int blocks = 0, cus = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, pow_search_kernel<PF, W>, 256, 0));
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const u64 resident = (u64)(blocks > 0 ? blocks : 1) * (u64)(cus > 0 ? cus : 1) * 256;
  const u64 v = resident / 4 > 256 ? resident / 4 : 256;
  if (dev >= 0 && dev < 64) cache[dev] = v;
  *lanes = v;
  return RONK_OK;
}

int pow_grind_launch(const ronk_poseidon* h, const u64* d_seed, u32 seed_len, u32 bits, u32 log2_limit, u64 max_lanes, u64* d_work,
                     u64* d_nonce, hipStream_t s) {
  u64 T = max_lanes;
  if (!T) POS_DISPATCH(h, RCHK((pow_default_lanes<FLD, W>(&T))));
  const u64 limit = (u64)1 << log2_limit, cap = (u64)1 << 30;   // the grid stays far below 2^31 workgroups
  if (T > limit) T = limit;
  if (T > cap) T = cap;
  POS_DISPATCH(h, hipLaunchKernelGGL((pow_prefix_kernel<FLD, W>), dim3(1), dim3(64), 0, s, h->sp, seed_len, d_seed, d_work, d_nonce));
  HIPCHK(hipGetLastError());
  POS_DISPATCH(h, hipLaunchKernelGGL((pow_search_kernel<FLD, W>), dim3((u32)((T + 255) / 256)), dim3(256), 0, s, h->sp, d_work,
                                     pow_slot(seed_len, h->rate), bits, log2_limit, T, d_nonce));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

int pow_reseed_launch(const ronk_poseidon* h, u32 d, u64* d_u, u32 bits, u32 log2_limit, const u64* d_nonce, int* d_status, hipStream_t s) {
  POS_DISPATCH(h, hipLaunchKernelGGL((pow_reseed_kernel<FLD, W>), dim3(1), dim3(64), 0, s, h->sp, d, d_u, bits, log2_limit, d_nonce,
                                     d_status));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- arguments
extern "C" int ronk_pow_check(uint64_t p, uint32_t rate, size_t seed_len, uint32_t bits, uint32_t log2_limit) {
  if (p < 2) return RONK_ERR_INVALID;
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  if (!(p & 1)) return RONK_ERR_NOT_PRIME;
  RCHK(ronk_check_prime(p));
  if (!rate) return RONK_ERR_INVALID;
  const int c = pow_host_check(p, seed_len, bits, log2_limit);
  return c == 1 ? RONK_ERR_INVALID : c == 2 ? RONK_ERR_UNSUPPORTED : RONK_OK;
}

extern "C" size_t ronk_pow_workspace_words(void) { return POW_WORK_WORDS; }

// ------------------------------------------------------------------------------------- device entry points
extern "C" int ronk_pow_grind_dev(const ronk_poseidon* h, const uint64_t* d_seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                                  size_t max_lanes, uint64_t* d_work, uint64_t* d_nonce, void* stream) {
  if (!h || (!d_seed && seed_len) || !d_work || !d_nonce) return RONK_ERR_INVALID;
  RCHK(ronk_pow_check(h->p, h->rate, seed_len, bits, log2_limit));
  return pow_grind_launch(h, d_seed, (u32)seed_len, bits, log2_limit, max_lanes, d_work, d_nonce, (hipStream_t)stream);
}

extern "C" int ronk_pow_verify_dev(const ronk_poseidon* h, const uint64_t* d_seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                                   const uint64_t* d_nonce, int* d_ok, void* stream) {
  if (!h || (!d_seed && seed_len) || !d_nonce || !d_ok) return RONK_ERR_INVALID;
  RCHK(ronk_pow_check(h->p, h->rate, seed_len, bits, log2_limit));
  POS_DISPATCH(h, hipLaunchKernelGGL((pow_verify_kernel<FLD, W>), dim3(1), dim3(64), 0, (hipStream_t)stream, h->sp, (u32)seed_len, d_seed,
                                     bits, log2_limit, d_nonce, d_ok));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
extern "C" int ronk_pow_grind(const ronk_poseidon* h, const uint64_t* seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                              size_t max_lanes, uint64_t* nonce) {
  if (!h || (!seed && seed_len) || !nonce) return RONK_ERR_INVALID;
  RCHK(ronk_pow_check(h->p, h->rate, seed_len, bits, log2_limit));
  RCHK(need_device());
  HostCall hc;
  const u64* ds = hc.in(seed_len ? seed : nullptr, seed_len);
  u64 *dw = hc.out(POW_WORK_WORDS), *dn = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_pow_grind_dev(h, ds, seed_len, bits, log2_limit, max_lanes, dw, dn, nullptr));
  RCHK(hc.get(nonce, dn, 8));
  return *nonce == POW_NONE ? RONK_ERR_INDEX : RONK_OK;
}

extern "C" int ronk_pow_verify(const ronk_poseidon* h, const uint64_t* seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                               uint64_t nonce, int* ok) {
  if (!h || (!seed && seed_len) || !ok) return RONK_ERR_INVALID;
  RCHK(ronk_pow_check(h->p, h->rate, seed_len, bits, log2_limit));
  RCHK(need_device());
  HostCall hc;
  const u64 *ds = hc.in(seed_len ? seed : nullptr, seed_len), *dn = hc.in(&nonce, 1);
  u64* dk = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_pow_verify_dev(h, ds, seed_len, bits, log2_limit, dn, (int*)dk, nullptr));
  return hc.get(ok, dk, sizeof(int));
}
