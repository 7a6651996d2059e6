// ronk_ext2.hip -- C ABI of libronk_ntt.so, part 10: element-wise arithmetic over the quadratic extension F_p[t] / (t^2 - W) of
// a 64-bit prime field on planar arrays (csrc/ext2.h, csrc/ext2_kernels.h; the launch context and dispatch of csrc/ext2_launch.h;
// DESIGN.md section 14).  No library workspace: every _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_launch.h"

extern "C" int ronk_ext2_check(uint64_t p, uint64_t w) {
  if (p < 2) return RONK_ERR_INVALID;
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  RCHK(ronk_check_prime(p));
  return ext2_non_residue(p, w) ? RONK_OK : RONK_ERR_INVALID;
}

// the context of a call after the field check and the device check
static int ext2_ctx(u64 p, u64 w, Ext2Launch* c) {
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  *c = ext2_launch(p, w);
  return RONK_OK;
}

template <int OP>
static int ext2_binary_dev(u64 p, u64 w, const u64* a, const u64* b, u64* out, size_t n, void* st) {
  if (!a || !b || !out) return RONK_ERR_INVALID;
  Ext2Launch c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH2(c, hipLaunchKernelGGL((ext2_binary_kernel<FF, OP>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, b,
                                             out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_add_dev(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* st) {
  return ext2_binary_dev<EXT2_ADD>(p, w, a, b, out, n, st);
}
extern "C" int ronk_ext2_vec_sub_dev(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* st) {
  return ext2_binary_dev<EXT2_SUB>(p, w, a, b, out, n, st);
}
extern "C" int ronk_ext2_vec_mul_dev(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* st) {
  return ext2_binary_dev<EXT2_MUL>(p, w, a, b, out, n, st);
}
extern "C" int ronk_ext2_vec_neg_dev(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, void* st) {
  if (!a || !out) return RONK_ERR_INVALID;
  Ext2Launch c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH2(c, hipLaunchKernelGGL((ext2_neg_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_mul_base_dev(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* d_s, uint64_t* out, size_t n,
                                          void* st) {
  if (!a || !d_s || !out) return RONK_ERR_INVALID;
  Ext2Launch c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH2(c, hipLaunchKernelGGL((ext2_mul_base_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, d_s,
                                             out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_pow_dev(uint64_t p, uint64_t w, const uint64_t* a, uint64_t e, uint64_t* out, size_t n, void* st) {
  if (!a || !out) return RONK_ERR_INVALID;
  Ext2Launch c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH2(c, hipLaunchKernelGGL((ext2_pow_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, e, out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
// *d_status (may be NULL) is set non-zero when an element is ZERO, as ronk_vec_inv_dev does for a zero word; (0, 0) is written
extern "C" int ronk_ext2_vec_inv_dev(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int* d_status, void* st) {
  if (!a || !out) return RONK_ERR_INVALID;
  Ext2Launch c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH2(c, hipLaunchKernelGGL((ext2_inv_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, out, n,
                                             d_status));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
// `words_b` words of the second operand (2 n for an element array, n for base words, 0 for none); the call runs in place on the
// device copy of `a`.  d_flag: the call may raise it, and a raised flag is RONK_ERR_ZERO_INVERSE with `out` not written.
template <class Call>
static int ext2_host(u64 p, u64 w, const u64* a, const u64* b, size_t words_b, u64* out, size_t n, Call&& call, bool flag = false) {
  if (!a || !out || (words_b && !b)) return RONK_ERR_INVALID;
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  HostCall hc;
  u64* da = hc.in(a, 2 * n);
  u64* db = hc.in(words_b ? b : nullptr, words_b);
  int* d_flag = flag ? (int*)hc.out(1) : nullptr;
  RCHK(hc.rc);
  if (flag) HIPCHK(hipMemset(d_flag, 0, 4));
  RCHK(call(da, db, d_flag));
  int raised = 0;
  if (flag) RCHK(hc.get(&raised, d_flag, 4));
  if (raised) return RONK_ERR_ZERO_INVERSE;
  return hc.get(out, da, 2 * n * 8);
}
extern "C" int ronk_ext2_vec_add(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y, int*) { return ronk_ext2_vec_add_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_sub(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y, int*) { return ronk_ext2_vec_sub_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_mul(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y, int*) { return ronk_ext2_vec_mul_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_neg(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, nullptr, 0, out, n, [&](u64* x, u64*, int*) { return ronk_ext2_vec_neg_dev(p, w, x, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_mul_base(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* s, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, s, n, out, n, [&](u64* x, u64* y, int*) { return ronk_ext2_vec_mul_base_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_pow(uint64_t p, uint64_t w, const uint64_t* a, uint64_t e, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, nullptr, 0, out, n, [&](u64* x, u64*, int*) { return ronk_ext2_vec_pow_dev(p, w, x, e, x, n, nullptr); });
}
// a ZERO element: RONK_ERR_ZERO_INVERSE and `out` is not written, as ronk_vec_inv
extern "C" int ronk_ext2_vec_inv(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, nullptr, 0, out, n, [&](u64* x, u64*, int* fl) { return ronk_ext2_vec_inv_dev(p, w, x, x, n, fl, nullptr); }, true);
}
