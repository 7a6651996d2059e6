// ronk_accum.hip -- C ABI of libronk_ntt.so, part 12: running products and sums over the 64-bit fields and their quadratic
// extension, the permutation grand product and the logUp running sum (csrc/accum_kernels.h; include/ronk_ntt.h "running
// products and sums").  Three launches per call, no host round trip and no library workspace: every _dev
// call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "accum_kernels.h"

extern "C" size_t ronk_scan_workspace_words(size_t n) { return (size_t)acc_work_words(n); }

extern "C" int ronk_accum_check(uint64_t p, uint64_t w, uint32_t n_columns, size_t n) {
  RCHK(ronk_ext2_check(p, w));
  if (n_columns == 0 || n == 0) return RONK_ERR_INVALID;
  if (n_columns > ACC_MAX_COLUMNS || n > ACC_MAX_N) return RONK_ERR_UNSUPPORTED;
  return RONK_OK;
}

namespace {
// the codes of a base-field scan: those of ronk_ext2_check without the extension's
int base_check(u64 p) {
  if (p < 2) return RONK_ERR_INVALID;
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  return ronk_check_prime(p);
}
int scan_args(const void* a, const void* out, const void* work, size_t n, int exclusive) {
  if (!a || !out || !work || n == 0 || (exclusive != 0 && exclusive != 1)) return RONK_ERR_INVALID;
  if (n > ACC_MAX_N) return RONK_ERR_UNSUPPORTED;
  return RONK_OK;
}

// what a launch knows: the policy, its constants and W in register form (w = 0: a base-field call)
struct AccCtx {
  bool mont, w7;
  FriConsts k;
  u64 w;
};
AccCtx acc_ctx(u64 p, u64 w) {
  AccCtx c;
  c.mont = p != RONK_GOLDILOCKS_P;
  c.w7 = !c.mont && w % p == 7;
  c.k = ext2_host_consts(c.mont, p);
  c.w = ext2_reg_form(c.mont, p, w);
  return c;
}
}  // namespace

// run the launch with FF bound to the policy of the context
#define ACC_DISPATCH(c, ...)                                \
  do {                                                      \
    if ((c).mont) { typedef FriMont FF; __VA_ARGS__; }      \
    else if ((c).w7) { typedef FriGlW7 FF; __VA_ARGS__; }   \
    else { typedef FriGl FF; __VA_ARGS__; }                 \
  } while (0)

// phases 2 and 3 over `a` (phase 1 has left the blocks' totals in d_work); d_status NULL: no flags
template <class O>
static int scan_tail(const AccCtx& c, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, int* d_status,
                     hipStream_t s) {
  const u64 B = acc_blocks(n);
  hipLaunchKernelGGL((acc_phase2_kernel<O>), dim3(1), dim3(ACC_LANES), 0, s, c.k, c.w, d_work, B, d_total, d_status);
  hipLaunchKernelGGL((acc_phase3_kernel<O>), dim3((u32)B), dim3(ACC_LANES), 0, s, c.k, c.w, a, out, n, exclusive, (const u64*)d_work);
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
template <class O>
static int scan_launch(const AccCtx& c, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, hipStream_t s) {
  hipLaunchKernelGGL((acc_phase1_kernel<O>), dim3((u32)acc_blocks(n)), dim3(ACC_LANES), 0, s, c.k, c.w, a, n, d_work);
  return scan_tail<O>(c, a, out, n, exclusive, d_total, d_work, nullptr, s);
}

template <int OP>
static int base_scan_dev(u64 p, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, void* st) {
  RCHK(scan_args(a, out, d_work, n, exclusive));
  RCHK(base_check(p));
  RCHK(need_device());
  const AccCtx c = acc_ctx(p, 0);
  int rc = RONK_OK;
  if (c.mont) rc = scan_launch<AccOp<AccWord<FriMont>, OP>>(c, a, out, n, exclusive, d_total, d_work, (hipStream_t)st);
  else rc = scan_launch<AccOp<AccWord<FriGl>, OP>>(c, a, out, n, exclusive, d_total, d_work, (hipStream_t)st);
  return rc;
}
template <int OP>
static int ext2_scan_dev(u64 p, u64 w, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, void* st) {
  RCHK(scan_args(a, out, d_work, n, exclusive));
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  const AccCtx c = acc_ctx(p, w);
  int rc = RONK_OK;
  ACC_DISPATCH(c, rc = (scan_launch<AccOp<AccPair<FF>, OP>>(c, a, out, n, exclusive, d_total, d_work, (hipStream_t)st)));
  return rc;
}

extern "C" int ronk_vec_prefix_prod_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive, uint64_t* d_total,
                                        uint64_t* d_work, void* stream) {
  return base_scan_dev<ACC_PROD>(p, d_a, d_out, n, exclusive, d_total, d_work, stream);
}
extern "C" int ronk_vec_prefix_sum_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive, uint64_t* d_total,
                                       uint64_t* d_work, void* stream) {
  return base_scan_dev<ACC_SUM>(p, d_a, d_out, n, exclusive, d_total, d_work, stream);
}
extern "C" int ronk_ext2_vec_prefix_prod_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive,
                                             uint64_t* d_total, uint64_t* d_work, void* stream) {
  return ext2_scan_dev<ACC_PROD>(p, w, d_a, d_out, n, exclusive, d_total, d_work, stream);
}
extern "C" int ronk_ext2_vec_prefix_sum_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive,
                                            uint64_t* d_total, uint64_t* d_work, void* stream) {
  return ext2_scan_dev<ACC_SUM>(p, w, d_a, d_out, n, exclusive, d_total, d_work, stream);
}

// ------------------------------------------------------------------------------------- the fused accumulators
extern "C" int ronk_perm_product_dev(uint64_t p, uint64_t w, const uint64_t* d_wires, const uint64_t* d_ids, const uint64_t* d_sigma,
                                     uint32_t n_columns, size_t n, const uint64_t* d_beta, const uint64_t* d_gamma, uint64_t* d_Z,
                                     uint64_t* d_last, uint64_t* d_work, int* d_status, void* stream) {
  if (!d_wires || !d_ids || !d_sigma || !d_beta || !d_gamma || !d_Z || !d_last || !d_work || !d_status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const AccCtx c = acc_ctx(p, w);
  hipStream_t s = (hipStream_t)stream;
  int rc = RONK_OK;
  ACC_DISPATCH(c, {
    hipLaunchKernelGGL((acc_perm_terms_kernel<FF>), dim3((u32)acc_blocks(n)), dim3(ACC_LANES), 0, s, c.k, c.w, d_wires, d_ids, d_sigma,
                       n_columns, n, d_beta, d_gamma, d_Z, d_work);
    rc = (scan_tail<AccOp<AccPair<FF>, ACC_PROD>>(c, d_Z, d_Z, n, 1, d_last, d_work, d_status, s));
  });
  return rc;
}

extern "C" int ronk_logup_sum_dev(uint64_t p, uint64_t w, const uint64_t* d_vals, const uint64_t* d_mult, uint32_t n_columns, size_t n,
                                  const uint64_t* d_alpha, uint64_t* d_S, uint64_t* d_last, uint64_t* d_work, int* d_status,
                                  void* stream) {
  if (!d_vals || !d_alpha || !d_S || !d_last || !d_work || !d_status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const AccCtx c = acc_ctx(p, w);
  hipStream_t s = (hipStream_t)stream;
  int rc = RONK_OK;
  ACC_DISPATCH(c, {
    hipLaunchKernelGGL((acc_logup_terms_kernel<FF>), dim3((u32)acc_blocks(n)), dim3(ACC_LANES), 0, s, c.k, c.w, d_vals, d_mult,
                       n_columns, n, d_alpha, d_S, d_work);
    rc = (scan_tail<AccOp<AccPair<FF>, ACC_SUM>>(c, d_S, d_S, n, 1, d_last, d_work, d_status, s));
  });
  return rc;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
namespace {
struct HostIn {
  const u64* h;
  size_t words;
  DevBuf d;
  int up() {
    RCHK(d.alloc(words * 8));
    if (h && words) HIPCHK(hipMemcpy(d.p, h, words * 8, hipMemcpyHostToDevice));
    return RONK_OK;
  }
};
// `ew` words per element; the scan runs in place on the device copy
template <class Call>
int scan_host(int check, int ew, const u64* a, u64* out, size_t n, int exclusive, u64* total, Call&& call) {
  if (!a || !out || n == 0 || (exclusive != 0 && exclusive != 1)) return RONK_ERR_INVALID;
  if (n > ACC_MAX_N) return RONK_ERR_UNSUPPORTED;
  RCHK(check);
  RCHK(need_device());
  HostIn in{a, (size_t)ew * n};
  DevBuf work, tot;
  RCHK(in.up()); RCHK(work.alloc(acc_work_words(n) * 8)); RCHK(tot.alloc(16));
  RCHK(call(in.d.u(), tot.u(), work.u()));
  HIPCHK(hipMemcpy(out, in.d.p, (size_t)ew * n * 8, hipMemcpyDeviceToHost));
  if (total) HIPCHK(hipMemcpy(total, tot.p, (size_t)ew * 8, hipMemcpyDeviceToHost));
  return RONK_OK;
}
}  // namespace

extern "C" int ronk_vec_prefix_prod(uint64_t p, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total) {
  return scan_host(base_check(p), 1, a, out, n, exclusive, total,
                   [&](u64* x, u64* t, u64* wk) { return ronk_vec_prefix_prod_dev(p, x, x, n, exclusive, t, wk, nullptr); });
}
extern "C" int ronk_vec_prefix_sum(uint64_t p, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total) {
  return scan_host(base_check(p), 1, a, out, n, exclusive, total,
                   [&](u64* x, u64* t, u64* wk) { return ronk_vec_prefix_sum_dev(p, x, x, n, exclusive, t, wk, nullptr); });
}
extern "C" int ronk_ext2_vec_prefix_prod(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int exclusive,
                                         uint64_t* total) {
  return scan_host(ronk_ext2_check(p, w), 2, a, out, n, exclusive, total,
                   [&](u64* x, u64* t, u64* wk) { return ronk_ext2_vec_prefix_prod_dev(p, w, x, x, n, exclusive, t, wk, nullptr); });
}
extern "C" int ronk_ext2_vec_prefix_sum(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int exclusive,
                                        uint64_t* total) {
  return scan_host(ronk_ext2_check(p, w), 2, a, out, n, exclusive, total,
                   [&](u64* x, u64* t, u64* wk) { return ronk_ext2_vec_prefix_sum_dev(p, w, x, x, n, exclusive, t, wk, nullptr); });
}

// the outputs of an accumulator call back to the host: the column [2][n], the last value, the status
static int accum_host_out(const DevBuf& col, const DevBuf& tail, u64* out, size_t n, u64* last, int* status) {
  HIPCHK(hipMemcpy(out, col.p, 2 * n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(last, tail.p, 16, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(status, (const char*)tail.p + 16, sizeof(int), hipMemcpyDeviceToHost));
  return RONK_OK;
}

extern "C" int ronk_perm_product(uint64_t p, uint64_t w, const uint64_t* wires, const uint64_t* ids, const uint64_t* sigma,
                                 uint32_t n_columns, size_t n, const uint64_t* beta, const uint64_t* gamma, uint64_t* Z, uint64_t* last,
                                 int* status) {
  if (!wires || !ids || !sigma || !beta || !gamma || !Z || !last || !status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const size_t m = (size_t)n_columns * n;
  HostIn a{wires, m}, i{ids, m}, s{sigma, m}, b{beta, 2}, g{gamma, 2};
  DevBuf col, tail, work;   // tail: the last value, then the status
  RCHK(a.up()); RCHK(i.up()); RCHK(s.up()); RCHK(b.up()); RCHK(g.up());
  RCHK(col.alloc(2 * n * 8)); RCHK(tail.alloc(24)); RCHK(work.alloc(acc_work_words(n) * 8));
  RCHK(ronk_perm_product_dev(p, w, a.d.u(), i.d.u(), s.d.u(), n_columns, n, b.d.u(), g.d.u(), col.u(), tail.u(), work.u(),
                             (int*)((char*)tail.p + 16), nullptr));
  return accum_host_out(col, tail, Z, n, last, status);
}

extern "C" int ronk_logup_sum(uint64_t p, uint64_t w, const uint64_t* vals, const uint64_t* mult, uint32_t n_columns, size_t n,
                              const uint64_t* alpha, uint64_t* S, uint64_t* last, int* status) {
  if (!vals || !alpha || !S || !last || !status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const size_t m = (size_t)n_columns * n;
  HostIn v{vals, m}, mu{mult, mult ? m : 0}, al{alpha, 2};
  DevBuf col, tail, work;
  RCHK(v.up()); RCHK(mu.up()); RCHK(al.up());
  RCHK(col.alloc(2 * n * 8)); RCHK(tail.alloc(24)); RCHK(work.alloc(acc_work_words(n) * 8));
  RCHK(ronk_logup_sum_dev(p, w, v.d.u(), mult ? mu.d.u() : nullptr, n_columns, n, al.d.u(), col.u(), tail.u(), work.u(),
                          (int*)((char*)tail.p + 16), nullptr));
  return accum_host_out(col, tail, S, n, last, status);
}
