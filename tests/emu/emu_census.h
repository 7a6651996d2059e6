// emu_census.h -- the branch-census counters of the host emulators (tests/test_emu_gl_directed.py).  gl64.h's counting hooks
// (-DRONK_GL64_CENSUS, host compilers only) report to the block gl64::census::cur points at; an emulator names the body it is
// about to drive with census_stage("name"), and at exit every stage's counts are printed as
//   census pass=0 phase=<name> fn=<function> outcome=<outcome> count=<n>
// (the format of emu_tile's census: the stage takes the place of the phase).  Without RONK_GL64_CENSUS all of it is empty.
// Include after the product headers.  Test infrastructure only; never part of the product library.
#pragma once
#ifdef RONK_GL64_CENSUS
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace emu_census {
enum { MAX_STAGES = 128 };
struct Stage {
  char name[48];
  unsigned long long n[gl64::census::NFN][gl64::census::NOUT];
};
static Stage g_stage[MAX_STAGES];
static int g_stages = 0;
static void print() {
  static const char* const fn[gl64::census::NFN] = {"add", "add_lazy", "mad_eps_canon", "sub", "sub32", "mul"};
  static const char* const oc[gl64::census::NFN][gl64::census::NOUT] = {
      {"none", "wrap", "ge_p"}, {"none", "wrap", "ge_p"}, {"none", "wrap", "ge_p"}, {"none", "wrap", "-"}, {"none", "wrap", "-"}, {"none", "-", "ge_p"}};
  for (int s = 0; s < g_stages; s++)
    for (int f = 0; f < gl64::census::NFN; f++) {
      unsigned long long tot = 0;
      for (int o = 0; o < gl64::census::NOUT; o++) tot += g_stage[s].n[f][o];
      if (!tot) continue;
      for (int o = 0; o < gl64::census::NOUT; o++)
        if (oc[f][o][0] != '-') printf("census pass=0 phase=%s fn=%s outcome=%s count=%llu\n", g_stage[s].name, fn[f], oc[f][o], g_stage[s].n[f][o]);
    }
}
}  // namespace emu_census

// the calls that follow belong to the body `name` (no blanks, no '=') under the field policy last given to census_policy;
// nullptr stops the counting
static const char* g_census_policy = "";
static inline void census_policy(const char* policy) { g_census_policy = policy; }
static inline void census_stage(const char* body) {
  using namespace emu_census;
  if (!body) { gl64::census::cur = nullptr; return; }
  char name[sizeof g_stage[0].name];
  if (snprintf(name, sizeof name, "%s%s", g_census_policy, body) >= (int)sizeof name) { fprintf(stderr, "census stage name too long\n"); abort(); }
  int s = 0;
  while (s < g_stages && strcmp(g_stage[s].name, name)) s++;
  if (s == g_stages) {
    if (g_stages == MAX_STAGES) { fprintf(stderr, "census stage table too small\n"); abort(); }
    if (!g_stages) atexit(print);
    strcpy(g_stage[g_stages++].name, name);
  }
  gl64::census::cur = g_stage[s].n;
}
#else
static inline void census_policy(const char*) {}
static inline void census_stage(const char*) {}
#endif
