// fr_ntt_host.cpp -- the host-side pieces of csrc/fr_ntt_kernels.h behind a C surface for tests/test_fr_ntt_host.py (TEST
// INFRASTRUCTURE ONLY): fr_pow / fr_inv, the root of unity, the planner's factors and the table bytes of a plan.
#include "../../ronkathon_amd/csrc/fr_ntt_kernels.h"

using namespace ronk;

extern "C" {
void h_fr_pow(const u64* a, const u64* e, u64* out) { bn254::fr_store(out, fr_pow(bn254::fr_load(a), bn254::fr_load(e))); }
void h_fr_inv(const u64* a, u64* out) { bn254::fr_store(out, fr_inv(bn254::fr_load(a))); }
void h_fr_root(u32 log2n, u64* out) { bn254::fr_store(out, fr_from_mont(fr_root_of_unity_mont(log2n))); }
// number of passes (0: none under this cap) and their log2 rows
u32 h_fr_factors(u32 log2n, u32 cap, u32* rows) {
  std::vector<u32> f;
  if (!fr_plan_factors(log2n, cap, &f)) return 0;
  for (size_t i = 0; i < f.size(); i++) rows[i] = f[i];
  return (u32)f.size();
}
// bytes of every table of the forward plan; the largest single table's entries in *max_entries
u64 h_fr_table_bytes(u32 log2n, u32 cap, u64* max_entries) {
  FrPlanDesc pd;
  if (!fr_build_plan(log2n, cap, false, nullptr, &pd)) return 0;
  u64 m = 0;
  for (auto& p : pd.passes) { if (p.wr.size() > m) m = p.wr.size(); if (p.tw.size() > m) m = p.tw.size(); }
  *max_entries = m;
  return pd.table_bytes();
}
}
