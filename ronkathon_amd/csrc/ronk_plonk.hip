// ronk_plonk.hip -- C ABI of libronk_ntt.so, part 13: the fused PLONK quotient on the evaluation coset (csrc/plonk_kernels.h;
// csrc/ext2_launch.h; include/ronk_ntt.h "PLONK quotient").  One launch per call, no host round trip and no
// library workspace: the _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_launch.h"
#include "plonk_kernels.h"
#include "plonk_handle.h"

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
  h->p = p; h->g = g % p; h->w = w % p; h->s = coset_shift % p; h->log2m = log2_n + log2_blowup;
  h->c = ext2_launch(p, w);
  const bool mont = h->c.mont;
  const u32 kb = deep_kbits(h->log2m);
  std::vector<u64> dom(((size_t)1 << kb) + ((size_t)1 << (h->log2m - kb))), vinv((size_t)1 << log2_blowup);
  deep_host_domain(mont, p, g % p, coset_shift, h->log2m, dom.data(), dom.data() + ((size_t)1 << kb), &h->dm.iota, &h->dm.sinv);
  plonk_host_vanishing(mont, p, g % p, coset_shift, log2_n, log2_blowup, vinv.data());
  int rc = upload(dom, &h->d_dom);
  if (rc == RONK_OK) rc = upload(vinv, &h->d_vinv);
  if (rc != RONK_OK) { ronk_plonk_destroy(h); return rc; }
  h->dm.lo = h->d_dom; h->dm.hi = h->d_dom + ((size_t)1 << kb); h->dm.kbits = kb; h->dm.log2n = h->log2m;
  h->tab.vinv = h->d_vinv; h->tab.log2b = log2_blowup;
  h->tab.ninv = ext2_reg_form(mont, p, h_powmod(((u64)1 << log2_n) % p, p - 2, p));
  h->tab.rho = ext2_reg_form(mont, p, h->log2m >= 3 ? h_powmod(g, (p - 1) >> 3, p) : 1);
  for (int c = 0; c < 3; c++) h->tab.k[c] = ext2_reg_form(mont, p, k[c]);
  *out = h;
  return RONK_OK;
}

// one launch with the rows per lane of the field policy, or one row per lane below that many rows
template <class FF>
static void plonk_launch(const ronk_plonk* h, const PlonkCols& cols, u64* d_T, hipStream_t s) {
  constexpr u32 LP = PlonkRows<FF>::LOG2;
  const u64 M = (u64)1 << h->log2m;
  if (h->log2m < LP)
    hipLaunchKernelGGL((plonk_quotient_kernel<FF, 1>), dim3((u32)((M + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES), 0, s, h->c.k,
                       h->c.w, h->dm, h->tab, cols, d_T);
  else
    hipLaunchKernelGGL((plonk_quotient_kernel<FF, 1 << LP>), dim3((u32)(((M >> LP) + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES),
                       0, s, h->c.k, h->c.w, h->dm, h->tab, cols, d_T);
}

extern "C" int ronk_plonk_quotient_dev(const ronk_plonk* h, const uint64_t* d_wires, const uint64_t* d_sel, const uint64_t* d_sigma,
                                       const uint64_t* d_pi, const uint64_t* d_Z, const uint64_t* d_alpha, const uint64_t* d_beta,
                                       const uint64_t* d_gamma, uint64_t* d_T, void* stream) {
  if (!h || !d_wires || !d_sel || !d_sigma || !d_Z || !d_alpha || !d_beta || !d_gamma || !d_T) return RONK_ERR_INVALID;
  const PlonkCols cols{d_wires, d_sel, d_sigma, d_pi, d_Z, d_alpha, d_beta, d_gamma};
  EXT2_DISPATCH3(h->c, plonk_launch<FF>(h, cols, d_T, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_plonk_quotient(const ronk_plonk* h, const uint64_t* wires, const uint64_t* sel, const uint64_t* sigma,
                                   const uint64_t* pi, const uint64_t* Z, const uint64_t* alpha, const uint64_t* beta,
                                   const uint64_t* gamma, uint64_t* T) {
  if (!h || !wires || !sel || !sigma || !Z || !alpha || !beta || !gamma || !T) return RONK_ERR_INVALID;
  const size_t M = (size_t)1 << h->log2m;
  HostCall hc;
  const u64 *dw = hc.in(wires, 3 * M), *dsel = hc.in(sel, 5 * M), *dsg = hc.in(sigma, 3 * M), *dpi = hc.in(pi, M);   // pi is optional
  const u64 *dZ = hc.in(Z, 2 * M), *da = hc.in(alpha, 2), *db = hc.in(beta, 2), *dg = hc.in(gamma, 2);
  u64* dT = hc.out(2 * M);
  RCHK(hc.rc);
  RCHK(ronk_plonk_quotient_dev(h, dw, dsel, dsg, dpi, dZ, da, db, dg, dT, nullptr));
  return hc.get(T, dT, 2 * M * 8);
}
