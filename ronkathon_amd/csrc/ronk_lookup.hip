// ronk_lookup.hip -- C ABI of libronk_ntt.so, part 15: the multiplicities of lookup columns in a table and the logUp quotient on
// the evaluation coset (csrc/lookup_kernels.h; include/ronk_ntt.h "lookup multiplicities and the logUp quotient"; DESIGN.md
// section 19).  Four launches per multiplicity call and one per quotient call, no host round trip and no library workspace: every
// _dev call is legal under stream capture.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_launch.h"
#include "plonk_handle.h"
#include "lookup_kernels.h"

extern "C" size_t ronk_lookup_workspace_words(size_t n_table) { return (size_t)lookup_work_words(n_table); }

extern "C" int ronk_lookup_check(uint64_t p, size_t n_table, uint32_t n_columns, size_t n) {
  if (n_table == 0 || n == 0 || n_columns == 0) return RONK_ERR_INVALID;
  if (n_table > LOOKUP_MAX_N || n > LOOKUP_MAX_N || n_columns > LOOKUP_MAX_COLUMNS) return RONK_ERR_UNSUPPORTED;
  if (p < 2) return RONK_ERR_INVALID;          // the codes of a base-field scan
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  return ronk_check_prime(p);
}

static u32 lookup_grid(u64 elements) {
  const u64 b = (elements + LOOKUP_LANES - 1) / LOOKUP_LANES;
  return (u32)(b < LOOKUP_GRID_MAX ? b : LOOKUP_GRID_MAX);
}

template <class FF>
static void lookup_launch(const Ext2Launch& c, const LookupTab& t, const u64* d_table, u64 T, const u64* d_vals, u64 total, int negate,
                          u64* d_mult, u64* d_missing, hipStream_t s) {
  const u64 cap = lookup_cap(t);
  hipLaunchKernelGGL(lookup_clear_kernel, dim3(lookup_grid(cap)), dim3(LOOKUP_LANES), 0, s, t, T, d_mult, d_missing, cap);
  hipLaunchKernelGGL((lookup_build_kernel<FF>), dim3(lookup_grid(T)), dim3(LOOKUP_LANES), 0, s, c.k, t, d_table, T);
  const u32 grid = (u32)std::min<u64>(lookup_grid(total), LOOKUP_COUNT_GRID);
  const u64 lanes = (u64)grid * LOOKUP_LANES;
  hipLaunchKernelGGL((lookup_count_kernel<FF>), dim3(grid), dim3(LOOKUP_LANES), 0, s, c.k, t, d_vals, total, (total + lanes - 1) / lanes,
                     d_missing);
  hipLaunchKernelGGL((lookup_finalise_kernel<FF>), dim3(lookup_grid(cap)), dim3(LOOKUP_LANES), 0, s, c.k, t, negate, d_mult);
}

extern "C" int ronk_lookup_mult_dev(uint64_t p, const uint64_t* d_table, size_t n_table, const uint64_t* d_vals, uint32_t n_columns,
                                    size_t n, int negate, uint64_t* d_mult, uint64_t* d_missing, uint64_t* d_work, void* stream) {
  if (!d_table || !d_vals || !d_mult || !d_missing || !d_work) return RONK_ERR_INVALID;
  RCHK(ronk_lookup_check(p, n_table, n_columns, n));
  if (negate != 0 && negate != 1) return RONK_ERR_INVALID;
  RCHK(need_device());
  const Ext2Launch c = ext2_launch(p, 0);
  LookupTab t;
  t.log2cap = lookup_log2_cap(n_table);
  t.keys = d_work;
  t.info = d_work + lookup_cap(t);
  EXT2_DISPATCH2(c, lookup_launch<FF>(c, t, d_table, n_table, d_vals, (u64)n_columns * n, negate, d_mult, d_missing, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_lookup_mult(uint64_t p, const uint64_t* table, size_t n_table, const uint64_t* vals, uint32_t n_columns, size_t n,
                                int negate, uint64_t* mult, uint64_t* missing) {
  if (!table || !vals || !mult || !missing) return RONK_ERR_INVALID;
  RCHK(ronk_lookup_check(p, n_table, n_columns, n));
  if (negate != 0 && negate != 1) return RONK_ERR_INVALID;
  RCHK(need_device());
  HostCall hc;
  const u64 *dt = hc.in(table, n_table), *dv = hc.in(vals, (size_t)n_columns * n);
  u64 *dm = hc.out(n_table), *dmiss = hc.out(2), *work = hc.out(lookup_work_words(n_table));
  RCHK(hc.rc);
  RCHK(ronk_lookup_mult_dev(p, dt, n_table, dv, n_columns, n, negate, dm, dmiss, work, nullptr));
  RCHK(hc.get(mult, dm, n_table * 8));
  return hc.get(missing, dmiss, 16);
}

// ------------------------------------------------------------------------------------- the logUp quotient
// one launch with the rows per lane of the field policy, or one row per lane below that many rows (as plonk_launch)
template <class FF>
static void logup_launch(const ronk_plonk* h, const LogupCols& cols, u64* d_T, hipStream_t s) {
  constexpr u32 LP = PlonkRows<FF>::LOG2;
  const u64 M = (u64)1 << h->log2m;
  if (h->log2m < LP)
    hipLaunchKernelGGL((logup_quotient_kernel<FF, 1>), dim3((u32)((M + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES), 0, s, h->c.k,
                       h->c.w, h->dm, h->tab, cols, d_T);
  else
    hipLaunchKernelGGL((logup_quotient_kernel<FF, 1 << LP>), dim3((u32)(((M >> LP) + PLONK_LANES - 1) / PLONK_LANES)), dim3(PLONK_LANES),
                       0, s, h->c.k, h->c.w, h->dm, h->tab, cols, d_T);
}

extern "C" int ronk_logup_quotient_dev(const ronk_plonk* h, const uint64_t* d_vals, const uint64_t* d_mult, uint32_t n_columns,
                                       const uint64_t* d_S, const uint64_t* d_alpha, const uint64_t* d_lambda, const uint64_t* d_T_in,
                                       uint64_t* d_T_out, void* stream) {
  if (!h || !d_vals || !d_S || !d_alpha || !d_lambda || !d_T_out || n_columns == 0) return RONK_ERR_INVALID;
  if (n_columns > LOOKUP_MAX_COLUMNS) return RONK_ERR_UNSUPPORTED;
  const LogupCols cols{d_vals, d_mult, n_columns, d_S, d_alpha, d_lambda, d_T_in};
  EXT2_DISPATCH3(h->c, logup_launch<FF>(h, cols, d_T_out, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_logup_quotient(const ronk_plonk* h, const uint64_t* vals, const uint64_t* mult, uint32_t n_columns, const uint64_t* S,
                                   const uint64_t* alpha, const uint64_t* lambda, const uint64_t* T_in, uint64_t* T_out) {
  if (!h || !vals || !S || !alpha || !lambda || !T_out || n_columns == 0) return RONK_ERR_INVALID;
  if (n_columns > LOOKUP_MAX_COLUMNS) return RONK_ERR_UNSUPPORTED;
  const size_t M = (size_t)1 << h->log2m;
  HostCall hc;
  const u64 *dv = hc.in(vals, n_columns * M), *dm = hc.in(mult, n_columns * M), *dS = hc.in(S, 2 * M);   // mult, T_in: optional
  const u64 *da = hc.in(alpha, 2), *dl = hc.in(lambda, 4), *dTin = hc.in(T_in, 2 * M);
  u64* dT = hc.out(2 * M);
  RCHK(hc.rc);
  RCHK(ronk_logup_quotient_dev(h, dv, dm, n_columns, dS, da, dl, dTin, dT, nullptr));
  return hc.get(T_out, dT, 2 * M * 8);
}
