// ronk_plonk.hip -- C ABI of libronk_ntt.so, part 13: the fused PLONK quotient on the evaluation coset (csrc/plonk_kernels.h;
// include/ronk_ntt.h "PLONK quotient").  One launch per call, no host round trip and no library workspace:
// the _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_kernels.h"
#include "plonk_kernels.h"

struct ronk_plonk {
  u64 p = 0;
  u32 log2m = 0;
  bool mont = false, w7 = false;
  FriConsts k;
  u64 w_reg = 0;
  DeepDomain dm{};
  PlonkTab tab{};
  u64* d_dom = nullptr;    // lo, hi of the domain
  u64* d_vinv = nullptr;   // the B inverses of the vanishing polynomial
};

extern "C" int ronk_plonk_check(uint64_t p, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup, uint64_t coset_shift,
                                const uint64_t k[3]) {
  (void)g;   // as ronk_root_of_unity: whether g has the full power-of-two order is the caller's concern
  RCHK(ronk_ext2_check(p, w));
  if (!k || coset_shift % p == 0 || k[0] % p == 0 || k[1] % p == 0 || k[2] % p == 0) return RONK_ERR_INVALID;
  const u64 lm = (u64)log2_n + log2_blowup;
  if (lm > 63 || ((p - 1) & (((u64)1 << lm) - 1))) return RONK_ERR_NO_ROOT;
  if (log2_n < 1 || lm > PLONK_MAX_LOG2M) return RONK_ERR_UNSUPPORTED;
  if (h_powmod(coset_shift, (u64)1 << lm, p) == 1) return RONK_ERR_UNSUPPORTED;   // some x_i^N - 1 or x_i - 1 would vanish
  return RONK_OK;
}

extern "C" int ronk_plonk_destroy(ronk_plonk* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->d_dom) (void)hipFree(h->d_dom);
  if (h->d_vinv) (void)hipFree(h->d_vinv);
  delete h;
  return RONK_OK;
}

extern "C" int ronk_plonk_create(ronk_plonk** out, uint64_t p, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                                 uint64_t coset_shift, const uint64_t k[3]) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  RCHK(ronk_plonk_check(p, g, w, log2_n, log2_blowup, coset_shift, k));
  RCHK(need_device());
  ronk_plonk* h = new ronk_plonk;
  h->p = p; h->log2m = log2_n + log2_blowup;
  h->mont = p != RONK_GOLDILOCKS_P;
  h->w7 = !h->mont && w % p == 7;
  h->k = ext2_host_consts(h->mont, p);
  h->w_reg = ext2_reg_form(h->mont, p, w);
  const u32 kb = deep_kbits(h->log2m);
  std::vector<u64> dom(((size_t)1 << kb) + ((size_t)1 << (h->log2m - kb))), vinv((size_t)1 << log2_blowup);
  deep_host_domain(h->mont, p, g % p, coset_shift, h->log2m, dom.data(), dom.data() + ((size_t)1 << kb), &h->dm.iota, &h->dm.sinv);
  plonk_host_vanishing(h->mont, p, g % p, coset_shift, log2_n, log2_blowup, vinv.data());
  int rc = upload(dom, &h->d_dom);
  if (rc == RONK_OK) rc = upload(vinv, &h->d_vinv);
  if (rc != RONK_OK) { ronk_plonk_destroy(h); return rc; }
  h->dm.lo = h->d_dom; h->dm.hi = h->d_dom + ((size_t)1 << kb); h->dm.kbits = kb; h->dm.log2n = h->log2m;
  h->tab.vinv = h->d_vinv; h->tab.log2b = log2_blowup;
  h->tab.ninv = ext2_reg_form(h->mont, p, h_powmod(((u64)1 << log2_n) % p, p - 2, p));
  h->tab.rho = ext2_reg_form(h->mont, p, h->log2m >= 3 ? h_powmod(g, (p - 1) >> 3, p) : 1);
  for (int c = 0; c < 3; c++) h->tab.k[c] = ext2_reg_form(h->mont, p, k[c]);
  *out = h;
  return RONK_OK;
}

// one launch with the rows per lane of the field policy, or one row per lane below that many rows
template <class FF>
static void plonk_launch(const ronk_plonk* h, const PlonkCols& cols, u64* d_T, hipStream_t s) {
  constexpr u32 LP = PlonkRows<FF>::LOG2;
  const u64 M = (u64)1 << h->log2m;
  if (h->log2m < LP)
    hipLaunchKernelGGL((plonk_quotient_kernel<FF, 1>), dim3((u32)((M + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES), 0, s, h->k,
                       h->w_reg, h->dm, h->tab, cols, d_T);
  else
    hipLaunchKernelGGL((plonk_quotient_kernel<FF, 1 << LP>), dim3((u32)(((M >> LP) + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES),
                       0, s, h->k, h->w_reg, h->dm, h->tab, cols, d_T);
}

extern "C" int ronk_plonk_quotient_dev(const ronk_plonk* h, const uint64_t* d_wires, const uint64_t* d_sel, const uint64_t* d_sigma,
                                       const uint64_t* d_pi, const uint64_t* d_Z, const uint64_t* d_alpha, const uint64_t* d_beta,
                                       const uint64_t* d_gamma, uint64_t* d_T, void* stream) {
  if (!h || !d_wires || !d_sel || !d_sigma || !d_Z || !d_alpha || !d_beta || !d_gamma || !d_T) return RONK_ERR_INVALID;
  const PlonkCols cols{d_wires, d_sel, d_sigma, d_pi, d_Z, d_alpha, d_beta, d_gamma};
  if (h->mont) plonk_launch<FriMont>(h, cols, d_T, (hipStream_t)stream);
  else if (h->w7) plonk_launch<FriGlW7>(h, cols, d_T, (hipStream_t)stream);
  else plonk_launch<FriGl>(h, cols, d_T, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_plonk_quotient(const ronk_plonk* h, const uint64_t* wires, const uint64_t* sel, const uint64_t* sigma,
                                   const uint64_t* pi, const uint64_t* Z, const uint64_t* alpha, const uint64_t* beta,
                                   const uint64_t* gamma, uint64_t* T) {
  if (!h || !wires || !sel || !sigma || !Z || !alpha || !beta || !gamma || !T) return RONK_ERR_INVALID;
  const size_t M = (size_t)1 << h->log2m;
  const struct { const u64* src; size_t words; } in[8] = {{wires, 3 * M}, {sel, 5 * M}, {sigma, 3 * M}, {pi, M},
                                                          {Z, 2 * M},     {alpha, 2},   {beta, 2},      {gamma, 2}};
  DevBuf d[8], out;
  for (int j = 0; j < 8; j++) {
    if (!in[j].src) continue;
    RCHK(d[j].alloc(in[j].words * 8));
    HIPCHK(hipMemcpy(d[j].p, in[j].src, in[j].words * 8, hipMemcpyHostToDevice));
  }
  RCHK(out.alloc(2 * M * 8));
  RCHK(ronk_plonk_quotient_dev(h, d[0].u(), d[1].u(), d[2].u(), pi ? d[3].u() : nullptr, d[4].u(), d[5].u(), d[6].u(), d[7].u(), out.u(),
                               nullptr));
  HIPCHK(hipMemcpy(T, out.p, 2 * M * 8, hipMemcpyDeviceToHost));
  return RONK_OK;
}
