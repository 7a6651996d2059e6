// emu_plonk.cpp -- the bodies of csrc/plonk_kernels.h (the challenges, the row, the lane with its one inversion, the handle's
// table of vanishing inverses) compiled for the host and run lane by lane over the whole grid of the kernel.  Test infrastructure
// only; never part of the product library.
//
//   emu_plonk <p> <g> <w> <log2_n> <log2_blowup> <shift> <with_pi>
//       random inputs with the edges mixed in, checked against a plain `unsigned __int128 % p` restatement in this file;
//   emu_plonk <p> <g> <w> <log2_n> <log2_blowup> <shift> <with_pi> <in> <out>
//       the words of <in> (wires 3M, sel 5M, sigma 3M, pi M when with_pi, Z 2M, alpha, beta, gamma: 2 each; little-endian u64),
//       T (2M words) of every policy that serves the field written to <out> one after the other, for tests/test_emu_plonk.py.
//   The last line is "OK ..." on success.  Goldilocks runs the Goldilocks policy, its W = 7 form when w = 7, AND the Montgomery
//   policy.  The label multipliers are 1, 2, 3.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/plonk_kernels.h"
using namespace ronk;
#include "emu_ref.h"
#include "emu_census.h"

// ---------------------------------------------------------------------------------------------------- the restatement
struct Shape {
  u64 p, g, w, shift;
  u32 log2n, log2b;
  u64 N() const { return (u64)1 << log2n; }
  u64 B() const { return (u64)1 << log2b; }
  u64 M() const { return (u64)1 << (log2n + log2b); }
};
struct Inputs {
  std::vector<u64> wires, sel, sigma, pi, Z;
  u64 alpha[2], beta[2], gamma[2];
  bool with_pi;
};

static R2 restated_row(const Shape& s, const Inputs& in, u64 i) {
  const u64 p = s.p, M = s.M(), w = s.w % p;
  const u64 wM = r_pow(s.g, (p - 1) / M, p), x = r_mul(s.shift % p, r_pow(wM, i, p), p);
  const u64 a = in.wires[i] % p, b = in.wires[M + i] % p, o = in.wires[2 * M + i] % p;
  u64 G = r_add(r_mul(a, in.sel[i] % p, p), r_mul(b, in.sel[M + i] % p, p), p);
  G = r_add(G, r_mul(r_mul(a, b, p), in.sel[2 * M + i] % p, p), p);
  G = r_add(G, r_mul(o, in.sel[3 * M + i] % p, p), p);
  G = r_add(G, r_add(in.sel[4 * M + i] % p, in.with_pi ? in.pi[i] % p : 0, p), p);
  const R2 al{in.alpha[0] % p, in.alpha[1] % p}, be{in.beta[0] % p, in.beta[1] % p}, ga{in.gamma[0] % p, in.gamma[1] % p};
  const u64 j = (i + s.B()) % M;
  const R2 Z{in.Z[i] % p, in.Z[M + i] % p};
  R2 num = Z, den{in.Z[j] % p, in.Z[M + j] % p};
  const u64 wv[3] = {a, b, o};
  for (u64 c = 0; c < 3; c++) {
    num = x_mul(num, x_add(x_add(R2{wv[c], 0}, x_scale(be, r_mul(c + 1, x, p), p), p), ga, p), w, p);
    den = x_mul(den, x_add(x_add(R2{wv[c], 0}, x_scale(be, in.sigma[c * M + i] % p, p), p), ga, p), w, p);
  }
  const R2 P1 = x_sub(num, den, p);
  const u64 vanish = r_sub(r_pow(x, s.N(), p), 1, p);
  const u64 L1 = r_mul(vanish, r_pow(r_mul(s.N() % p, r_sub(x, 1, p), p), p - 2, p), p);
  const R2 P2 = x_scale(x_sub(Z, R2{1, 0}, p), L1, p);
  const R2 total = x_add(x_add(R2{G, 0}, x_mul(al, P1, w, p), p), x_mul(x_mul(al, al, w, p), P2, w, p), p);
  return x_scale(total, r_pow(vanish, p - 2, p), p);
}

// ---------------------------------------------------------------------------------------------------- the kernel, lane by lane
template <class F>
static std::vector<u64> emu_quotient(bool mont, const Shape& s, const Inputs& in) {
  const u64 p = s.p, M = s.M();
  const u32 log2m = s.log2n + s.log2b;
  const F f(ext2_host_consts(mont, p));
  const Ext2<F> x(f, ext2_reg_form(mont, p, s.w));
  // the handle
  const u32 kb = deep_kbits(log2m);
  std::vector<u64> dom(((size_t)1 << kb) + ((size_t)1 << (log2m - kb))), vinv((size_t)s.B());
  DeepDomain dm{};
  deep_host_domain(mont, p, s.g % p, s.shift, log2m, dom.data(), dom.data() + ((size_t)1 << kb), &dm.iota, &dm.sinv);
  dm.lo = dom.data(); dm.hi = dom.data() + ((size_t)1 << kb); dm.kbits = kb; dm.log2n = log2m;
  plonk_host_vanishing(mont, p, s.g % p, s.shift, s.log2n, s.log2b, vinv.data());
  PlonkTab tab{};
  tab.vinv = vinv.data(); tab.log2b = s.log2b;
  tab.ninv = ext2_reg_form(mont, p, r_pow(s.N() % p, p - 2, p));
  tab.rho = ext2_reg_form(mont, p, log2m >= 3 ? r_pow(s.g % p, (p - 1) >> 3, p) : 1);
  for (u64 c = 0; c < 3; c++) tab.k[c] = ext2_reg_form(mont, p, c + 1);
  const PlonkCols cols{in.wires.data(), in.sel.data(), in.sigma.data(), in.with_pi ? in.pi.data() : nullptr, in.Z.data(),
                       in.alpha, in.beta, in.gamma};
  std::vector<u64> T(2 * M, ~(u64)0);
  census_stage("plonk");
  auto run = [&](auto PP) {
    constexpr int PTS = decltype(PP)::value;
    const u64 q = M / PTS, grid = (q + PLONK_LANES - 1) / PLONK_LANES;
    for (u64 blk = 0; blk < grid; blk++)
      for (u64 lane = 0; lane < PLONK_LANES; lane++) {
        const u64 i = blk * PLONK_LANES + lane;
        if (i >= q) continue;
        const PlonkChal ch = plonk_challenges(x, tab, cols.alpha, cols.beta, cols.gamma);
        plonk_lane<F, PTS>(x, dm, tab, ch, i, [&](u64 row) { return plonk_load_row(cols, M, s.B(), row); }, [&](u64 row, E2 v) {
          CHECK(row < M && T[row] == ~(u64)0, "row %llu out of range or written twice", (unsigned long long)row);
          if (row < M) { T[row] = v.c0; T[M + row] = v.c1; }
        });
      }
  };
  if (log2m < PlonkRows<F>::LOG2) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 1 << PlonkRows<F>::LOG2>{});
  census_stage(nullptr);
  return T;
}

static bool read_words(FILE* fp, std::vector<u64>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), 8, n, fp) == n;
}

int main(int argc, char** argv) {
  if (argc != 8 && argc != 10) { fprintf(stderr, "usage: emu_plonk p g w log2_n log2_blowup shift with_pi [in out]\n"); return 2; }
  Shape s;
  s.p = strtoull(argv[1], nullptr, 0); s.g = strtoull(argv[2], nullptr, 0); s.w = strtoull(argv[3], nullptr, 0);
  s.log2n = (u32)atoi(argv[4]); s.log2b = (u32)atoi(argv[5]); s.shift = strtoull(argv[6], nullptr, 0);
  const u64 p = s.p;
  if (p < 3 || !(p & 1) || !ext2_non_residue(p, s.w)) { fprintf(stderr, "p must be an odd prime, w a quadratic non-residue\n"); return 2; }
  if (s.log2n < 1 || s.log2n + s.log2b > 24 || (p - 1) % s.M() || s.shift % p == 0 || r_pow(s.shift % p, s.M(), p) == 1) {
    fprintf(stderr, "a shape that ronk_plonk_check refuses (or more than 2^24 rows)\n");
    return 2;
  }
  const u64 M = s.M();
  Inputs in;
  in.with_pi = atoi(argv[7]) != 0;
  g_rng = p ^ s.w ^ (M << 8) ^ s.log2b ^ 17;
  if (argc == 10) {
    FILE* fp = fopen(argv[8], "rb");
    std::vector<u64> ch;
    if (!fp || !read_words(fp, in.wires, 3 * M) || !read_words(fp, in.sel, 5 * M) || !read_words(fp, in.sigma, 3 * M) ||
        (in.with_pi && !read_words(fp, in.pi, M)) || !read_words(fp, in.Z, 2 * M) || !read_words(fp, ch, 6)) {
      fprintf(stderr, "cannot read the inputs from %s\n", argv[8]);
      return 2;
    }
    fclose(fp);
    for (int j = 0; j < 2; j++) { in.alpha[j] = ch[j]; in.beta[j] = ch[2 + j]; in.gamma[j] = ch[4 + j]; }
  } else {
    in.wires.resize(3 * M); in.sel.resize(5 * M); in.sigma.resize(3 * M); in.pi.resize(M); in.Z.resize(2 * M);
    for (auto* v : {&in.wires, &in.sel, &in.sigma, &in.pi, &in.Z})
      for (auto& t : *v) t = edge_word(p);
    for (int j = 0; j < 2; j++) { in.alpha[j] = edge_word(p); in.beta[j] = emu_small() ? edge_word(p) : rnd(); in.gamma[j] = emu_small() ? edge_word(p) : rnd(); }   // (the directed mode of emu_ref.h: small challenges too)
  }
  const Inputs before = in;
  std::vector<std::vector<u64>> results;
  int policies = 0;
  if (p == gl64::P) {
    census_policy("gl.");
    results.push_back(emu_quotient<FriGl>(false, s, in)); policies |= 1;
    census_policy("w7.");
    if (s.w % p == 7) { results.push_back(emu_quotient<FriGlW7>(false, s, in)); policies |= 2; }
  }
  census_policy("mont.");
  results.push_back(emu_quotient<FriMont>(true, s, in)); policies |= 4;
  CHECK(before.wires == in.wires && before.sel == in.sel && before.sigma == in.sigma && before.Z == in.Z, "an input changed");
  // every row at the small sizes, else the ends, the stride boundaries and a sample
  std::vector<u64> rows;
  if (M <= 4096) {
    for (u64 i = 0; i < M; i++) rows.push_back(i);
  } else {
    for (u64 q = 0; q < 8; q++)
      for (u64 d = 0; d < 2 * s.B(); d++) { rows.push_back(q * (M / 8) + d); rows.push_back((q + 1) * (M / 8) - 1 - d); }
    for (int j = 0; j < 1024; j++) rows.push_back(rnd() % M);
  }
  for (u64 i : rows) {
    const R2 want = restated_row(s, in, i);
    for (size_t r = 0; r < results.size(); r++)
      CHECK(results[r][i] == want.c0 && results[r][M + i] == want.c1, "policy %zu row %llu", r, (unsigned long long)i);
  }
  for (size_t r = 1; r < results.size(); r++) CHECK(results[r] == results[0], "policy %zu differs from the first", r);
  if (argc == 10) {
    FILE* fp = fopen(argv[9], "wb");
    bool ok = fp != nullptr;
    for (size_t r = 0; ok && r < results.size(); r++) ok = fwrite(results[r].data(), 8, 2 * M, fp) == 2 * M;
    if (fp) ok = fclose(fp) == 0 && ok;
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu w=%llu M=%llu B=%llu pi=%d policies=%d results=%zu\n", (unsigned long long)p, (unsigned long long)s.w,
         (unsigned long long)M, (unsigned long long)s.B(), (int)in.with_pi, policies, results.size());
  return 0;
}
