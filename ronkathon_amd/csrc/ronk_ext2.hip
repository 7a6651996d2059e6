// ronk_ext2.hip -- C ABI of libronk_ntt.so, part 10: element-wise arithmetic over the quadratic extension F_p[t] / (t^2 - W) of
// a 64-bit prime field on planar arrays (csrc/ext2.h, csrc/ext2_kernels.h).  No library workspace: every
// _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_kernels.h"

extern "C" int ronk_ext2_check(uint64_t p, uint64_t w) {
  if (p < 2) return RONK_ERR_INVALID;
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  RCHK(ronk_check_prime(p));
  return ext2_non_residue(p, w) ? RONK_OK : RONK_ERR_INVALID;
}

namespace {
// what a launch knows: the policy (Goldilocks arithmetic or Montgomery), its constants and W in register form
struct Ext2Ctx {
  bool mont;
  FriConsts k;
  u64 w;
};
int ext2_ctx(u64 p, u64 w, Ext2Ctx* c) {
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  c->mont = p != RONK_GOLDILOCKS_P;
  c->k = ext2_host_consts(c->mont, p);
  c->w = ext2_reg_form(c->mont, p, w);
  return RONK_OK;
}
}  // namespace

// run the launch with FF bound to the policy of the context
#define EXT2_DISPATCH(c, ...)                               \
  do {                                                      \
    if ((c).mont) { typedef FriMont FF; __VA_ARGS__; }      \
    else { typedef FriGl FF; __VA_ARGS__; }                 \
  } while (0)

template <int OP>
static int ext2_binary_dev(u64 p, u64 w, const u64* a, const u64* b, u64* out, size_t n, void* st) {
  if (!a || !b || !out) return RONK_ERR_INVALID;
  Ext2Ctx c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH(c, hipLaunchKernelGGL((ext2_binary_kernel<FF, OP>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, b,
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
  Ext2Ctx c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH(c, hipLaunchKernelGGL((ext2_neg_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_mul_base_dev(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* d_s, uint64_t* out, size_t n,
                                          void* st) {
  if (!a || !d_s || !out) return RONK_ERR_INVALID;
  Ext2Ctx c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH(c, hipLaunchKernelGGL((ext2_mul_base_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, d_s,
                                             out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_pow_dev(uint64_t p, uint64_t w, const uint64_t* a, uint64_t e, uint64_t* out, size_t n, void* st) {
  if (!a || !out) return RONK_ERR_INVALID;
  Ext2Ctx c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH(c, hipLaunchKernelGGL((ext2_pow_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, e, out, n));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
// *d_status (may be NULL) is set non-zero when an element is ZERO, as ronk_vec_inv_dev does for a zero word; (0, 0) is written
extern "C" int ronk_ext2_vec_inv_dev(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int* d_status, void* st) {
  if (!a || !out) return RONK_ERR_INVALID;
  Ext2Ctx c;
  RCHK(ext2_ctx(p, w, &c));
  if (n) EXT2_DISPATCH(c, hipLaunchKernelGGL((ext2_inv_kernel<FF>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, c.k, c.w, a, out, n,
                                             d_status));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
// `words_b` words of the second operand (2 n for an element array, n for base words, 0 for none)
template <class Call>
static int ext2_host(u64 p, u64 w, const u64* a, const u64* b, size_t words_b, u64* out, size_t n, Call&& call) {
  if (!a || !out || (words_b && !b)) return RONK_ERR_INVALID;
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  DevBuf da, db;
  RCHK(da.alloc(2 * n * 8)); RCHK(db.alloc(words_b * 8));
  HIPCHK(hipMemcpy(da.p, a, 2 * n * 8, hipMemcpyHostToDevice));
  if (words_b) HIPCHK(hipMemcpy(db.p, b, words_b * 8, hipMemcpyHostToDevice));
  RCHK(call(da.u(), db.u()));
  HIPCHK(hipMemcpy(out, da.p, 2 * n * 8, hipMemcpyDeviceToHost));
  return RONK_OK;
}
extern "C" int ronk_ext2_vec_add(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y) { return ronk_ext2_vec_add_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_sub(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y) { return ronk_ext2_vec_sub_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_mul(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, b, 2 * n, out, n, [&](u64* x, u64* y) { return ronk_ext2_vec_mul_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_neg(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, nullptr, 0, out, n, [&](u64* x, u64*) { return ronk_ext2_vec_neg_dev(p, w, x, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_mul_base(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* s, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, s, n, out, n, [&](u64* x, u64* y) { return ronk_ext2_vec_mul_base_dev(p, w, x, y, x, n, nullptr); });
}
extern "C" int ronk_ext2_vec_pow(uint64_t p, uint64_t w, const uint64_t* a, uint64_t e, uint64_t* out, size_t n) {
  return ext2_host(p, w, a, nullptr, 0, out, n, [&](u64* x, u64*) { return ronk_ext2_vec_pow_dev(p, w, x, e, x, n, nullptr); });
}
// a ZERO element: RONK_ERR_ZERO_INVERSE and `out` is not written, as ronk_vec_inv
extern "C" int ronk_ext2_vec_inv(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n) {
  if (!a || !out) return RONK_ERR_INVALID;
  RCHK(ronk_ext2_check(p, w));
  RCHK(need_device());
  DevBuf da, dflag;
  RCHK(da.alloc(2 * n * 8)); RCHK(dflag.alloc(4));
  HIPCHK(hipMemcpy(da.p, a, 2 * n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dflag.p, 0, 4));
  RCHK(ronk_ext2_vec_inv_dev(p, w, da.u(), da.u(), n, (int*)dflag.p, nullptr));
  int hflag = 0;
  HIPCHK(hipMemcpy(&hflag, dflag.p, 4, hipMemcpyDeviceToHost));
  if (hflag) return RONK_ERR_ZERO_INVERSE;
  HIPCHK(hipMemcpy(out, da.p, 2 * n * 8, hipMemcpyDeviceToHost));
  return RONK_OK;
}
