// emu_lookup.cpp -- the bodies of csrc/lookup_kernels.h (the four multiplicity launches: clear, build, count, finalise; the logUp
// quotient's challenges, row and lane) compiled for the host and run lane by lane over the grids of the kernels, the atomic
// operations being plain reads and writes in program order.  Test infrastructure only; never part of the product library.
//
//   emu_lookup <p> <g> <w>
//       a battery of random cases of both families against a plain restatement in this file (`std::map`, `unsigned __int128 % p`);
//       the multiplicity launches run with their lanes forward, reversed and shuffled, and all three must agree word for word.
//   emu_lookup mult <p> <T> <n> <C> <negate> <order> <in> <out>
//       the words of <in> (table T, vals C n; little-endian u64); mult (T) and missing (2) written to <out>.  order: 0 forward,
//       1 reverse, else the seed of a shuffle.
//   emu_lookup quot <p> <g> <w> <log2_n> <log2_blowup> <shift> <C> <with_mult> <with_tin> <in> <out>
//       the words of <in> (vals C M, mult C M when with_mult, S 2M, alpha 2, lambda 4, T_in 2M when with_tin); T_out (2M words) of
//       every policy that serves the field written to <out> one after the other.
//   The last line is "OK ..." on success.  Goldilocks runs the Goldilocks policy, its W = 7 form when w = 7, AND Montgomery.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/lookup_kernels.h"
using namespace ronk;
#include "emu_ref.h"

// ---------------------------------------------------------------------------------------------------- multiplicities
// The atomics of a host that runs one lane at a time.  add_combined models the carry of the device policy (LookupDeviceAtomics:
// what the first round of a wavefront retires is owed to its slot and added only when the slot changes, or in flush at the end)
// with the lane as the "wavefront": the adds of consecutive lanes to one slot are owed, not made, until another slot comes or the
// launch ends.  The ballots and shuffles of the device form have no host form; tests/test_gpu_lookup.py covers them.
struct HostAtomics {
  u32 carried_slot = 0;
  u64 carried = 0;
  u64 flushes = 0;   // how often an owed count was added: the tests see that the carry was exercised
  u64 cas(u64* p, u64 expected, u64 desired) const { const u64 old = *p; if (old == expected) *p = desired; return old; }
  void min(u64* p, u64 v) const { if (v < *p) *p = v; }
  void flush(u64* base) {
    if (carried) { base[carried_slot] += carried; flushes++; }
    carried = 0;
  }
  void add_combined(u64* base, u32 slot, bool active) {
    if (!active) return;             // a dead lane keeps what is owed
    if (carried && carried_slot != slot) flush(base);
    carried_slot = slot;
    carried += 1;
  }
  void missing(u64* out, bool is_missing, u64 e) const {
    if (is_missing) { out[0] += 1; if (e < out[1]) out[1] = e; }
  }
};

// the lanes 0 .. count - 1 of one launch in the order asked for
static std::vector<u64> lane_order(u64 count, u64 order) {
  std::vector<u64> v(count);
  for (u64 i = 0; i < count; i++) v[i] = i;
  if (order == 1) std::reverse(v.begin(), v.end());
  if (order > 1) {
    u64 s = order;
    for (u64 i = count; i > 1; i--) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(v[i - 1], v[(s >> 33) % i]);
    }
  }
  return v;
}

struct MultOut {
  std::vector<u64> mult;
  u64 missing[2];
  bool operator==(const MultOut& o) const { return mult == o.mult && missing[0] == o.missing[0] && missing[1] == o.missing[1]; }
};

template <class F>
static MultOut emu_mult(bool mont, u64 p, const std::vector<u64>& table, const std::vector<u64>& vals, int negate, u64 order) {
  const F f(ext2_host_consts(mont, p));
  HostAtomics at;
  const u64 T = table.size(), total = vals.size();
  std::vector<u64> work(lookup_work_words(T), 0x5555555555555555ull);
  LookupTab t;
  t.log2cap = lookup_log2_cap(T);
  t.keys = work.data();
  t.info = work.data() + lookup_cap(t);
  const u64 cap = lookup_cap(t);
  CHECK(2 * cap == work.size() && cap >= 2 * T, "capacity %llu for T = %llu", (unsigned long long)cap, (unsigned long long)T);
  MultOut out;
  out.mult.assign(T, ~(u64)0);
  out.missing[0] = out.missing[1] = 0x1234;
  for (u64 e : lane_order(cap, order)) lookup_clear(t, T, out.mult.data(), out.missing, e);
  for (u64 j : lane_order(T, order)) lookup_build(f, at, t, table.data(), j);
  // the count kernel's grid: whole workgroups, lanes past the end take part
  const u64 padded = (total + LOOKUP_LANES - 1) / LOOKUP_LANES * LOOKUP_LANES;
  for (u64 e : lane_order(padded, order)) lookup_count(f, at, t, vals.data(), total, out.missing, e);
  at.flush(t.info);
  CHECK(at.carried == 0 && at.flushes <= total - out.missing[0] && (at.flushes > 0 || total == out.missing[0]), "the carry: %llu flushes",
        (unsigned long long)at.flushes);
  for (u64 s : lane_order(cap, order)) lookup_finalise(f, t, negate, out.mult.data(), s);
  return out;
}

static MultOut restated_mult(u64 p, const std::vector<u64>& table, const std::vector<u64>& vals, int negate) {
  std::map<u64, u64> first;
  for (u64 j = 0; j < table.size(); j++) first.emplace(table[j] % p, j);
  std::vector<u64> count(table.size(), 0);
  MultOut out;
  out.missing[0] = 0; out.missing[1] = ~(u64)0;
  for (u64 e = 0; e < vals.size(); e++) {
    auto it = first.find(vals[e] % p);
    if (it == first.end()) { out.missing[0]++; out.missing[1] = std::min(out.missing[1], e); }
    else count[it->second]++;
  }
  for (u64 c : count) { const u64 v = c % p; out.mult.push_back(negate && v ? p - v : v); }
  return out;
}

// every policy that serves p, every order asked for: all equal; returns the common result
static MultOut run_mult(u64 p, const std::vector<u64>& table, const std::vector<u64>& vals, int negate, const std::vector<u64>& orders) {
  std::vector<MultOut> r;
  for (u64 o : orders) {
    if (p == gl64::P) r.push_back(emu_mult<FriGl>(false, p, table, vals, negate, o));
    r.push_back(emu_mult<FriMont>(true, p, table, vals, negate, o));
  }
  for (size_t k = 1; k < r.size(); k++) CHECK(r[k] == r[0], "run %zu differs from the first", k);
  return r[0];
}

// ---------------------------------------------------------------------------------------------------- the quotient
struct Shape {
  u64 p, g, w, shift;
  u32 log2n, log2b;
  u64 N() const { return (u64)1 << log2n; }
  u64 B() const { return (u64)1 << log2b; }
  u64 M() const { return (u64)1 << (log2n + log2b); }
};
struct Inputs {
  std::vector<u64> vals, mult, S, Tin;
  u64 alpha[2], lambda[4];
  u32 C;
  bool with_mult, with_tin;
};

static R2 restated_row(const Shape& s, const Inputs& in, u64 i) {
  const u64 p = s.p, M = s.M(), w = s.w % p;
  const u64 wM = r_pow(s.g, (p - 1) / M, p), x = r_mul(s.shift % p, r_pow(wM, i, p), p);
  const R2 al{in.alpha[0] % p, in.alpha[1] % p}, l0{in.lambda[0] % p, in.lambda[1] % p}, l1{in.lambda[2] % p, in.lambda[3] % p};
  R2 P{1 % p, 0}, Q{0, 0};
  for (u64 c = 0; c < in.C; c++) {       // Q by its definition: the products that leave one column out
    R2 term{in.with_mult ? in.mult[c * M + i] % p : 1 % p, 0};
    for (u64 k = 0; k < in.C; k++)
      if (k != c) term = x_mul(term, x_add(al, R2{in.vals[k * M + i] % p, 0}, p), w, p);
    Q = x_add(Q, term, p);
    P = x_mul(P, x_add(al, R2{in.vals[c * M + i] % p, 0}, p), w, p);
  }
  const u64 j = (i + s.B()) % M;
  const R2 S{in.S[i] % p, in.S[M + i] % p}, Sn{in.S[j] % p, in.S[M + j] % p};
  const R2 R = x_sub(x_mul(x_sub(Sn, S, p), P, w, p), Q, p);
  const u64 vanish = r_sub(r_pow(x, s.N(), p), 1, p);
  const u64 L1 = r_mul(vanish, r_pow(r_mul(s.N() % p, r_sub(x, 1, p), p), p - 2, p), p);
  R2 t = x_scale(x_add(x_mul(l0, R, w, p), x_mul(l1, x_scale(S, L1, p), w, p), p), r_pow(vanish, p - 2, p), p);
  if (in.with_tin) t = x_add(t, R2{in.Tin[i] % p, in.Tin[M + i] % p}, p);
  return t;
}

template <class F>
static std::vector<u64> emu_quotient(bool mont, const Shape& s, const Inputs& in) {
  const u64 p = s.p, M = s.M();
  const u32 log2m = s.log2n + s.log2b;
  const F f(ext2_host_consts(mont, p));
  const Ext2<F> x(f, ext2_reg_form(mont, p, s.w));
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
  // in place when there is a T_in: row i reads T_in at row i only
  std::vector<u64> T = in.with_tin ? in.Tin : std::vector<u64>(2 * M, ~(u64)0);
  std::vector<char> written(M, 0);
  const LogupCols cols{in.vals.data(), in.with_mult ? in.mult.data() : nullptr, in.C, in.S.data(), in.alpha, in.lambda,
                       in.with_tin ? T.data() : nullptr};
  auto run = [&](auto PP) {
    constexpr int PTS = decltype(PP)::value;
    const u64 q = M / PTS, grid = (q + PLONK_LANES - 1) / PLONK_LANES;
    for (u64 blk = 0; blk < grid; blk++)
      for (u64 lane = 0; lane < PLONK_LANES; lane++) {
        const u64 i = blk * PLONK_LANES + lane;
        if (i >= q) continue;
        const LogupChal ch = logup_challenges(x, tab, cols.alpha, cols.lambda);
        logup_lane<F, PTS>(x, dm, tab, ch, cols, i, [&](u64 row, E2 v) {
          CHECK(row < M && !written[row], "row %llu out of range or written twice", (unsigned long long)row);
          if (row < M) { T[row] = v.c0; T[M + row] = v.c1; written[row] = 1; }
        });
      }
  };
  if (log2m < PlonkRows<F>::LOG2) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 1 << PlonkRows<F>::LOG2>{});
  for (u64 i = 0; i < M; i++) CHECK(written[i], "row %llu not written", (unsigned long long)i);
  return T;
}

static std::vector<std::vector<u64>> run_quotient(const Shape& s, const Inputs& in) {
  std::vector<std::vector<u64>> results;
  if (s.p == gl64::P) {
    results.push_back(emu_quotient<FriGl>(false, s, in));
    if (s.w % s.p == 7) results.push_back(emu_quotient<FriGlW7>(false, s, in));
  }
  results.push_back(emu_quotient<FriMont>(true, s, in));
  const u64 M = s.M();
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
  return results;
}

static bool shape_ok(const Shape& s) {
  return s.log2n >= 1 && s.log2n + s.log2b <= 24 && (s.p - 1) % s.M() == 0 && s.shift % s.p != 0 && r_pow(s.shift % s.p, s.M(), s.p) != 1;
}

static bool read_words(FILE* fp, std::vector<u64>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), 8, n, fp) == n;
}
static bool write_words(FILE* fp, const u64* v, size_t n) { return fwrite(v, 8, n, fp) == n; }

// ---------------------------------------------------------------------------------------------------- the battery
static void battery_mult(u64 p) {
  const std::vector<u64> orders{0, 1, 77};
  const u64 shapes[][3] = {{1, 1, 1}, {2, 65, 1}, {40, 700, 2}, {255, 300, 2}, {256, 1000, 3}, {257, 513, 1}, {1025, 3000, 2}};
  for (auto& sh : shapes) {
    const u64 T = sh[0], n = sh[1], C = sh[2];
    for (int negate = 0; negate < 2; negate++) {
      std::vector<u64> table(T), vals(C * n);
      for (auto& t : table) t = rnd() % 3 ? edge_word(p) : rnd() % 64;          // duplicates for sure once T > 64 or p is small
      for (auto& v : vals) {
        const u64 k = rnd() % 16;
        v = k == 0 ? rnd() : table[rnd() % T];                                  // a few words the table may lack
        if (k == 1 && v % p <= ~(u64)0 - p) v = v % p + p;                       // the same value as another word
      }
      vals[vals.size() - 1] = T > 1 ? table[0] ^ 0x55 : vals[vals.size() - 1];  // the last lane of the last column
      const MultOut got = run_mult(p, table, vals, negate, orders), want = restated_mult(p, table, vals, negate);
      CHECK(got == want, "multiplicities T=%llu n=%llu C=%llu negate=%d: missing %llu/%llu want %llu/%llu", (unsigned long long)T,
            (unsigned long long)n, (unsigned long long)C, negate, (unsigned long long)got.missing[0],
            (unsigned long long)got.missing[1], (unsigned long long)want.missing[0], (unsigned long long)want.missing[1]);
    }
  }
}

static void battery_quotient(u64 p, u64 g, u64 w) {
  const u32 shapes[][3] = {{1, 0, 1}, {1, 1, 2}, {2, 1, 1}, {3, 1, 3}, {4, 2, 16}, {9, 3, 3}};   // log2 n, log2 b, C
  int k = 0;
  for (auto& sh : shapes) {
    Shape s{p, g, w, g, sh[0], sh[1]};
    if (!shape_ok(s)) continue;
    const u64 M = s.M();
    Inputs in;
    in.C = sh[2];
    in.with_mult = k & 1; in.with_tin = (k >> 1) & 1; k++;
    in.vals.resize(in.C * M); in.mult.resize(in.C * M); in.S.resize(2 * M); in.Tin.resize(2 * M);
    for (auto* v : {&in.vals, &in.mult, &in.S, &in.Tin})
      for (auto& t : *v) t = edge_word(p);
    for (auto& a : in.alpha) a = edge_word(p);
    for (auto& l : in.lambda) l = rnd();
    run_quotient(s, in);
  }
}

int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "mult")) {
    const u64 p = strtoull(argv[2], nullptr, 0), T = strtoull(argv[3], nullptr, 0), n = strtoull(argv[4], nullptr, 0);
    const u64 C = strtoull(argv[5], nullptr, 0), order = strtoull(argv[7], nullptr, 0);
    const int negate = atoi(argv[6]);
    if (p < 3 || !(p & 1) || !T || !n || !C || T > (1 << 22) || C * n > (1 << 24)) { fprintf(stderr, "bad shape\n"); return 2; }
    std::vector<u64> table, vals;
    FILE* fp = fopen(argv[8], "rb");
    if (!fp || !read_words(fp, table, T) || !read_words(fp, vals, C * n)) { fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
    fclose(fp);
    const std::vector<u64> t0 = table, v0 = vals;
    const MultOut got = run_mult(p, table, vals, negate, {order});
    CHECK(t0 == table && v0 == vals, "an input changed");
    CHECK(got == restated_mult(p, table, vals, negate), "differs from the restatement");
    fp = fopen(argv[9], "wb");
    if (!fp || !write_words(fp, got.mult.data(), T) || !write_words(fp, got.missing, 2) || fclose(fp)) { fprintf(stderr, "cannot write\n"); return 2; }
    if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
    printf("OK mult p=%llu T=%llu n=%llu C=%llu order=%llu\n", (unsigned long long)p, (unsigned long long)T, (unsigned long long)n,
           (unsigned long long)C, (unsigned long long)order);
    return 0;
  }
  if (argc == 13 && !strcmp(argv[1], "quot")) {
    Shape s;
    s.p = strtoull(argv[2], nullptr, 0); s.g = strtoull(argv[3], nullptr, 0); s.w = strtoull(argv[4], nullptr, 0);
    s.log2n = (u32)atoi(argv[5]); s.log2b = (u32)atoi(argv[6]); s.shift = strtoull(argv[7], nullptr, 0);
    Inputs in;
    in.C = (u32)atoi(argv[8]); in.with_mult = atoi(argv[9]) != 0; in.with_tin = atoi(argv[10]) != 0;
    if (s.p < 3 || !(s.p & 1) || !ext2_non_residue(s.p, s.w) || !shape_ok(s) || in.C < 1 || in.C > LOOKUP_MAX_COLUMNS) {
      fprintf(stderr, "a shape the library refuses\n");
      return 2;
    }
    const u64 M = s.M();
    g_rng = s.p ^ M;
    FILE* fp = fopen(argv[11], "rb");
    std::vector<u64> ch;
    if (!fp || !read_words(fp, in.vals, in.C * M) || (in.with_mult && !read_words(fp, in.mult, in.C * M)) || !read_words(fp, in.S, 2 * M) ||
        !read_words(fp, ch, 6) || (in.with_tin && !read_words(fp, in.Tin, 2 * M))) {
      fprintf(stderr, "cannot read %s\n", argv[11]);
      return 2;
    }
    fclose(fp);
    for (int j = 0; j < 2; j++) in.alpha[j] = ch[j];
    for (int j = 0; j < 4; j++) in.lambda[j] = ch[2 + j];
    const auto results = run_quotient(s, in);
    fp = fopen(argv[12], "wb");
    bool ok = fp != nullptr;
    for (size_t r = 0; ok && r < results.size(); r++) ok = write_words(fp, results[r].data(), 2 * M);
    if (fp) ok = fclose(fp) == 0 && ok;
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[12]); return 2; }
    if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
    printf("OK quot p=%llu M=%llu C=%u results=%zu\n", (unsigned long long)s.p, (unsigned long long)M, in.C, results.size());
    return 0;
  }
  if (argc != 4) { fprintf(stderr, "usage: emu_lookup p g w | mult ... | quot ... (see the head of the file)\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0), w = strtoull(argv[3], nullptr, 0);
  if (p < 3 || !(p & 1) || !ext2_non_residue(p, w)) { fprintf(stderr, "p must be an odd prime, w a quadratic non-residue\n"); return 2; }
  g_rng = p ^ w ^ 19;
  battery_mult(p);
  battery_quotient(p, g, w);
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu w=%llu\n", (unsigned long long)p, (unsigned long long)w);
  return 0;
}
