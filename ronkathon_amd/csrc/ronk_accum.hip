// ronk_accum.hip -- C ABI of libronk_ntt.so, part 12: running products and sums over the 64-bit fields and their quadratic
// extension, the permutation grand product and the logUp running sum (csrc/accum_kernels.h, csrc/ext2_launch.h;
// include/ronk_ntt.h "running products and sums").  Three launches per call, no host round trip and no
// library workspace: every _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "accum_kernels.h"
#include "ext2_launch.h"

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
}  // namespace

// phases 2 and 3 over `a` (phase 1 has left the blocks' totals in d_work); d_status NULL: no flags
template <class O>
static int scan_tail(const Ext2Launch& c, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, int* d_status,
                     hipStream_t s) {
  const u64 B = acc_blocks(n);
  hipLaunchKernelGGL((acc_phase2_kernel<O>), dim3(1), dim3(ACC_LANES), 0, s, c.k, c.w, d_work, B, d_total, d_status);
  hipLaunchKernelGGL((acc_phase3_kernel<O>), dim3((u32)B), dim3(ACC_LANES), 0, s, c.k, c.w, a, out, n, exclusive, (const u64*)d_work);
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
template <class O>
static int scan_launch(const Ext2Launch& c, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, hipStream_t s) {
  hipLaunchKernelGGL((acc_phase1_kernel<O>), dim3((u32)acc_blocks(n)), dim3(ACC_LANES), 0, s, c.k, c.w, a, n, d_work);
  return scan_tail<O>(c, a, out, n, exclusive, d_total, d_work, nullptr, s);
}

template <int OP>
static int base_scan_dev(u64 p, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, void* st) {
  RCHK(scan_args(a, out, d_work, n, exclusive));
  RCHK(base_check(p));
  RCHK(need_device());
  const Ext2Launch c = ext2_launch(p, 0);
  int rc = RONK_OK;
  EXT2_DISPATCH2(c, rc = (scan_launch<AccOp<AccWord<FF>, OP>>(c, a, out, n, exclusive, d_total, d_work, (hipStream_t)st)));
  return rc;
}
template <int OP>
static int ext2_scan_dev(u64 p, u64 w, const u64* a, u64* out, size_t n, int exclusive, u64* d_total, u64* d_work, void* st) {
  RCHK(scan_args(a, out, d_work, n, exclusive));
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  const Ext2Launch c = ext2_launch(p, w);
  int rc = RONK_OK;
  EXT2_DISPATCH3(c, rc = (scan_launch<AccOp<AccPair<FF>, OP>>(c, a, out, n, exclusive, d_total, d_work, (hipStream_t)st)));
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
  const Ext2Launch c = ext2_launch(p, w);
  hipStream_t s = (hipStream_t)stream;
  int rc = RONK_OK;
  EXT2_DISPATCH3(c, {
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
  const Ext2Launch c = ext2_launch(p, w);
  hipStream_t s = (hipStream_t)stream;
  int rc = RONK_OK;
  EXT2_DISPATCH3(c, {
    hipLaunchKernelGGL((acc_logup_terms_kernel<FF>), dim3((u32)acc_blocks(n)), dim3(ACC_LANES), 0, s, c.k, c.w, d_vals, d_mult,
                       n_columns, n, d_alpha, d_S, d_work);
    rc = (scan_tail<AccOp<AccPair<FF>, ACC_SUM>>(c, d_S, d_S, n, 1, d_last, d_work, d_status, s));
  });
  return rc;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
// `ew` words per element; the scan runs in place on the device copy.  `check` is the field's code, reported after the arguments'.
template <class Call>
static int scan_host(int check, int ew, const u64* a, u64* out, size_t n, int exclusive, u64* total, Call&& call) {
  if (!a || !out || n == 0 || (exclusive != 0 && exclusive != 1)) return RONK_ERR_INVALID;
  if (n > ACC_MAX_N) return RONK_ERR_UNSUPPORTED;
  RCHK(check);
  RCHK(need_device());
  HostCall hc;
  u64 *da = hc.in(a, (size_t)ew * n), *work = hc.out(acc_work_words(n)), *tot = hc.out(2);
  RCHK(hc.rc);
  RCHK(call(da, tot, work));
  RCHK(hc.get(out, da, (size_t)ew * n * 8));
  return total ? hc.get(total, tot, (size_t)ew * 8) : RONK_OK;
}

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

// The host form of an accumulator: the column [2][n], the last value and the status come back.  tail: the last value, then the
// status.  call(column, last, work, status) queues the _dev form.
template <class Call>
static int accum_host(HostCall& hc, u64* out, size_t n, u64* last, int* status, Call&& call) {
  u64 *col = hc.out(2 * n), *tail = hc.out(3), *work = hc.out(acc_work_words(n));
  RCHK(hc.rc);
  RCHK(call(col, tail, work, (int*)(tail + 2)));
  RCHK(hc.get(out, col, 2 * n * 8));
  RCHK(hc.get(last, tail, 16));
  return hc.get(status, tail + 2, sizeof(int));
}

extern "C" int ronk_perm_product(uint64_t p, uint64_t w, const uint64_t* wires, const uint64_t* ids, const uint64_t* sigma,
                                 uint32_t n_columns, size_t n, const uint64_t* beta, const uint64_t* gamma, uint64_t* Z, uint64_t* last,
                                 int* status) {
  if (!wires || !ids || !sigma || !beta || !gamma || !Z || !last || !status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const size_t m = (size_t)n_columns * n;
  HostCall hc;
  const u64 *a = hc.in(wires, m), *i = hc.in(ids, m), *s = hc.in(sigma, m), *b = hc.in(beta, 2), *g = hc.in(gamma, 2);
  return accum_host(hc, Z, n, last, status, [&](u64* col, u64* tail, u64* work, int* st) {
    return ronk_perm_product_dev(p, w, a, i, s, n_columns, n, b, g, col, tail, work, st, nullptr);
  });
}

extern "C" int ronk_logup_sum(uint64_t p, uint64_t w, const uint64_t* vals, const uint64_t* mult, uint32_t n_columns, size_t n,
                              const uint64_t* alpha, uint64_t* S, uint64_t* last, int* status) {
  if (!vals || !alpha || !S || !last || !status) return RONK_ERR_INVALID;
  RCHK(ronk_accum_check(p, w, n_columns, n));
  RCHK(need_device());
  const size_t m = (size_t)n_columns * n;
  HostCall hc;
  const u64 *v = hc.in(vals, m), *mu = hc.in(mult, m), *al = hc.in(alpha, 2);   // mult is optional
  return accum_host(hc, S, n, last, status, [&](u64* col, u64* tail, u64* work, int* st) {
    return ronk_logup_sum_dev(p, w, v, mu, n_columns, n, al, col, tail, work, st, nullptr);
  });
}
