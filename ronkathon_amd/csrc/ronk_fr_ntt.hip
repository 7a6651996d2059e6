// ronk_fr_ntt.hip -- plans, transforms and the polynomial product over BN254's scalar field (csrc/fr_ntt_kernels.h;
// include/ronk_ntt.h "NTT over the BN254 scalar field").
#include <map>
#include <memory>

#include "workspace.h"
#include "hip_launch.h"
#include "fr_ntt_kernels.h"

namespace {

// two instantiations: the register budget follows the workgroup's lanes (tiles of up to 2^10 elements run on 256 lanes)
template <int MAXT>
__global__ void __launch_bounds__(MAXT) fr_ntt_pass_kernel(const FrPassArgs a, u32 log_tiles) {
  extern __shared__ __attribute__((aligned(16))) u64 fr_lds[];
  const u32 b = xcd_tile_id();
  fr_ntt_pass_body(a, fr_lds, threadIdx.x, blockDim.x, (u64)(b & ((1u << log_tiles) - 1)), (u64)(b >> log_tiles),
                   [] { __syncthreads(); });
}

__global__ void __launch_bounds__(256) fr_pointwise_kernel(const u64* __restrict__ a, const u64* __restrict__ b, u64* x, u64 n) {   // x may be a
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) fr_pointwise_elem(a, b, x, i);
}
__global__ void __launch_bounds__(256) fr_pad_kernel(const u64* __restrict__ in, u64 have, u64* __restrict__ out, u64 n) {
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) fr_pad_elem(in, have, out, i);
}

// one direction's tables on the device
struct FrCompiled {
  std::vector<FrPassGeom> geom;
  std::vector<Fr*> d_wr, d_tw;
  size_t table_bytes = 0;
  int compile(const FrPlanDesc& pd) {
    table_bytes = pd.table_bytes();
    for (auto& ps : pd.passes) {
      Fr *wr = nullptr, *tw = nullptr;
      HIPCHK(hipMalloc((void**)&wr, ps.wr.size() * sizeof(Fr)));
      d_wr.push_back(wr);
      HIPCHK(hipMemcpy(wr, ps.wr.data(), ps.wr.size() * sizeof(Fr), hipMemcpyHostToDevice));
      HIPCHK(hipMalloc((void**)&tw, (ps.tw.size() + 1) * sizeof(Fr)));
      d_tw.push_back(tw);
      if (!ps.tw.empty()) HIPCHK(hipMemcpy(tw, ps.tw.data(), ps.tw.size() * sizeof(Fr), hipMemcpyHostToDevice));
      geom.push_back(ps.g);
    }
    return RONK_OK;
  }
  void release() {
    for (auto* q : d_wr) (void)hipFree(q);
    for (auto* q : d_tw) (void)hipFree(q);
    d_wr.clear(); d_tw.clear(); geom.clear();
  }
  // in -> out through the scratch buffers t1, t2 (each batch * n elements; t1 is needed from two passes on, t2 from three;
  // neither may alias in or out).  A single pass reads its whole tile before it writes it, so in == out is safe there.
  int run(const u64* in, u64* out, u64* t1, u64* t2, size_t batch, hipStream_t s) const {
    const size_t P = geom.size();
    const u64* src = in;
    for (size_t t = 0; t < P; t++) {
      u64* dst = t + 1 == P ? out : ((t & 1) ? t2 : t1);
      FrPassArgs a;
      a.g = geom[t]; a.in = src; a.out = dst; a.wr = d_wr[t]; a.tw = d_tw[t];
      const u32 log_tiles = a.g.log2n - a.g.logr - a.g.logc;
      const u64 blocks = ((u64)batch) << log_tiles;
      if (blocks >= ((u64)1 << 31)) return RONK_ERR_UNSUPPORTED;
      const u32 T = fr_pass_threads(a.g);
      const size_t lds = fr_pass_lds_bytes(a.g);
      hipError_t e = T <= 256 ? launch_dyn<fr_ntt_pass_kernel<256>>(dim3((u32)blocks), dim3(T), lds, s, a, log_tiles)
                              : launch_dyn<fr_ntt_pass_kernel<1024>>(dim3((u32)blocks), dim3(T), lds, s, a, log_tiles);
      if (e != hipSuccess) return hip_fail(e, "fr_ntt_pass_kernel");
      src = dst;
    }
    return RONK_OK;
  }
};

Fr fr_scale_mont(u32 log2n, bool times_r) {   // 1/n (or 2^256 / n) in Montgomery form
  Fr v = bn254::fr_to_mont(fr_inv(fr_from_u64((u64)1 << log2n)));
  return times_r ? bn254::fr_to_mont(v) : v;
}

}  // namespace

struct ronk_fr_plan {
  u32 log2n = 0;
  int device = 0;
  FrCompiled fwd, inv, inv_mul;   // inv_mul: the inverse that also undoes the pointwise product's 1 / 2^256
  // scratch of the multi-pass plans: two buffers of scratch_batch * n elements, sized at creation (one row) or by
  // ronk_plan_reserve_bn254; a transform never touches their size: a larger batch runs in slices of scratch_batch rows
  std::mutex mu;
  u64 *t1 = nullptr, *t2 = nullptr;
  size_t scratch_batch = 0;
  ~ronk_fr_plan() {
    fwd.release(); inv.release(); inv_mul.release();
    if (t1) (void)hipFree(t1);
    if (t2) (void)hipFree(t2);
  }
  int reserve(size_t batch) {
    const size_t P = fwd.geom.size();
    if (P < 2 || batch <= scratch_batch) return RONK_OK;
    // growing replaces buffers that queued work may still use: wait for it (hipFree alone would, this says so)
    HIPCHK(hipDeviceSynchronize());
    if (t1) { (void)hipFree(t1); t1 = nullptr; }
    if (t2) { (void)hipFree(t2); t2 = nullptr; }
    scratch_batch = 0;
    const size_t bytes = (batch << log2n) * 32;
    HIPCHK(hipMalloc((void**)&t1, bytes));
    if (P >= 3) HIPCHK(hipMalloc((void**)&t2, bytes));
    scratch_batch = batch;
    return RONK_OK;
  }
};

static int fr_plan_new(ronk_fr_plan** out, u32 log2n, u32 max_log2_tile, bool with_mul) {
  std::unique_ptr<ronk_fr_plan> pl(new ronk_fr_plan());
  pl->log2n = log2n;
  HIPCHK(hipGetDevice(&pl->device));
  FrPlanDesc pd;
  if (!fr_build_plan(log2n, max_log2_tile, false, nullptr, &pd)) return RONK_ERR_UNSUPPORTED;
  RCHK(pl->fwd.compile(pd));
  const Fr sc = fr_scale_mont(log2n, false);
  if (!fr_build_plan(log2n, max_log2_tile, true, &sc, &pd)) return RONK_ERR_UNSUPPORTED;
  RCHK(pl->inv.compile(pd));
  if (with_mul) {
    const Fr scm = fr_scale_mont(log2n, true);
    if (!fr_build_plan(log2n, max_log2_tile, true, &scm, &pd)) return RONK_ERR_UNSUPPORTED;
    RCHK(pl->inv_mul.compile(pd));
  }
  *out = pl.release();
  return RONK_OK;
}

extern "C" int ronk_root_of_unity_bn254(uint32_t log2n, uint64_t out[4]) {
  if (!out) return RONK_ERR_INVALID;
  if (log2n > FR_TWO_ADICITY) return RONK_ERR_NO_ROOT;
  bn254::fr_store(out, fr_from_mont(fr_root_of_unity_mont(log2n)));
  return RONK_OK;
}

extern "C" int ronk_plan_create_bn254(ronk_fr_plan** out, uint32_t log2n, uint32_t max_log2_tile) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (log2n > FR_TWO_ADICITY) return RONK_ERR_NO_ROOT;
  std::vector<u32> f;
  if (!fr_plan_factors(log2n, max_log2_tile, &f)) return RONK_ERR_UNSUPPORTED;   // more than four passes under this cap
  RCHK(need_device());
  RCHK(fr_plan_new(out, log2n, max_log2_tile, false));
  const int rc = (*out)->reserve(1);
  if (rc != RONK_OK) { delete *out; *out = nullptr; }
  return rc;
}

extern "C" int ronk_plan_info_bn254(const ronk_fr_plan* pl, uint32_t* num_passes, uint32_t log2_rows[4]) {
  if (!pl || !num_passes) return RONK_ERR_INVALID;
  *num_passes = (uint32_t)pl->fwd.geom.size();
  if (log2_rows)
    for (size_t t = 0; t < FR_MAX_PASSES; t++) log2_rows[t] = t < pl->fwd.geom.size() ? pl->fwd.geom[t].logr : 0;
  return RONK_OK;
}

extern "C" int ronk_plan_destroy_bn254(ronk_fr_plan* pl) {
  if (!pl) return RONK_ERR_INVALID;
  (void)hipDeviceSynchronize();   // queued transforms may still read the tables and the scratch
  delete pl;
  return RONK_OK;
}

static int fr_transform_dev(ronk_fr_plan* pl, bool inverse, const uint64_t* d_in, uint64_t* d_out, size_t batch, void* stream) {
  if (!pl || !d_in || !d_out || batch == 0) return RONK_ERR_INVALID;
  std::lock_guard<std::mutex> lk(pl->mu);
  const FrCompiled& c = inverse ? pl->inv : pl->fwd;
  // enqueue only: rows beyond the reserved scratch go in further slices, ordered behind the earlier ones by the stream
  const size_t per = c.geom.size() < 2 ? batch : pl->scratch_batch;
  const size_t row = (size_t)4 << pl->log2n;
  for (size_t b0 = 0; b0 < batch; b0 += per) {
    const size_t cnt = batch - b0 < per ? batch - b0 : per;
    RCHK(c.run(d_in + b0 * row, d_out + b0 * row, pl->t1, pl->t2, cnt, (hipStream_t)stream));
  }
  return RONK_OK;
}
extern "C" int ronk_plan_reserve_bn254(ronk_fr_plan* pl, size_t batch) {
  if (!pl || batch == 0) return RONK_ERR_INVALID;
  std::lock_guard<std::mutex> lk(pl->mu);
  return pl->reserve(batch);
}
extern "C" int ronk_ntt_forward_bn254_dev(ronk_fr_plan* pl, const uint64_t* d_in, uint64_t* d_out, size_t batch, void* stream) {
  return fr_transform_dev(pl, false, d_in, d_out, batch, stream);
}
extern "C" int ronk_ntt_inverse_bn254_dev(ronk_fr_plan* pl, const uint64_t* d_in, uint64_t* d_out, size_t batch, void* stream) {
  return fr_transform_dev(pl, true, d_in, d_out, batch, stream);
}

static int fr_transform_host(u32 log2n, bool inverse, const uint64_t* in, uint64_t* out) {
  if (!in || !out) return RONK_ERR_INVALID;
  if (log2n > FR_TWO_ADICITY) return RONK_ERR_NO_ROOT;
  RCHK(need_device());
  ronk_fr_plan* raw = nullptr;
  RCHK(ronk_plan_create_bn254(&raw, log2n, 0));
  std::unique_ptr<ronk_fr_plan> pl(raw);
  HostCall hc;
  u64* d = hc.in(in, (size_t)4 << log2n);
  RCHK(hc.rc);
  RCHK(fr_transform_dev(pl.get(), inverse, d, d, 1, nullptr));
  RCHK(hc.get(out, d, (size_t)32 << log2n));   // orders behind the null stream's work
  HIPCHK(hipDeviceSynchronize());
  return RONK_OK;
}
extern "C" int ronk_ntt_forward_bn254(uint32_t log2n, const uint64_t* in, uint64_t* out) { return fr_transform_host(log2n, false, in, out); }
extern "C" int ronk_ntt_inverse_bn254(uint32_t log2n, const uint64_t* in, uint64_t* out) { return fr_transform_host(log2n, true, in, out); }

// the product's plans: tables only (immutable, shared by every stream), one per (device, size); the scratch is leased per call
static int fr_mul_plan(u32 log2n, ronk_fr_plan** out) {
  static std::mutex mu;
  static std::map<std::pair<int, u32>, ronk_fr_plan*> cache;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({dev, log2n});
  if (it == cache.end()) {
    ronk_fr_plan* pl = nullptr;
    RCHK(fr_plan_new(&pl, log2n, 0, true));
    it = cache.emplace(std::make_pair(dev, log2n), pl).first;
  }
  *out = it->second;
  return RONK_OK;
}

extern "C" int ronk_poly_mul_bn254_dev(const uint64_t* d_a, size_t d, const uint64_t* d_b, size_t d2, uint64_t* d_out, void* stream) {
  if (!d_a || !d_b || !d_out || d == 0 || d2 == 0) return RONK_ERR_INVALID;
  const size_t len = d + d2 - 1;
  if (len < d || len > ((size_t)1 << FR_TWO_ADICITY)) return RONK_ERR_UNSUPPORTED;
  RCHK(need_device());
  const u32 k = (u32)ilog2(len);
  const size_t n = (size_t)1 << k;
  hipStream_t s = (hipStream_t)stream;
  ronk_fr_plan* pl = nullptr;
  RCHK(fr_mul_plan(k, &pl));
  // workspace: the two padded operands (one batch of two rows), then two scratch buffers of two rows each
  WsLease ws;
  RCHK(ws.acquire(6 * n * 32, s));
  Carve c{ws.u()};
  u64 *ab = c.take(8 * n), *t1 = c.take(8 * n), *t2 = c.take(8 * n);
  hipLaunchKernelGGL(fr_pad_kernel, dim3(grid_for(n)), dim3(256), 0, s, d_a, (u64)d, ab, (u64)n);
  hipLaunchKernelGGL(fr_pad_kernel, dim3(grid_for(n)), dim3(256), 0, s, d_b, (u64)d2, ab + 4 * n, (u64)n);
  HIPCHK(hipGetLastError());
  RCHK(pl->fwd.run(ab, ab, t1, t2, 2, s));
  hipLaunchKernelGGL(fr_pointwise_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const u64*)ab, (const u64*)(ab + 4 * n), ab, (u64)n);
  HIPCHK(hipGetLastError());
  RCHK(pl->inv_mul.run(ab, ab + 4 * n, t1, t2, 1, s));
  HIPCHK(hipMemcpyAsync(d_out, ab + 4 * n, len * 32, hipMemcpyDeviceToDevice, s));
  return RONK_OK;
}

extern "C" int ronk_poly_mul_bn254(const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out) {
  if (!a || !b || !out || d == 0 || d2 == 0) return RONK_ERR_INVALID;
  const size_t len = d + d2 - 1;
  if (len < d || len > ((size_t)1 << FR_TWO_ADICITY)) return RONK_ERR_UNSUPPORTED;
  RCHK(need_device());
  HostCall hc;
  const u64 *da = hc.in(a, 4 * d), *db = hc.in(b, 4 * d2);
  u64* dc = hc.out(4 * len);
  RCHK(hc.rc);
  RCHK(ronk_poly_mul_bn254_dev(da, d, db, d2, dc, nullptr));
  RCHK(hc.get(out, dc, len * 32));
  HIPCHK(hipDeviceSynchronize());
  return RONK_OK;
}
