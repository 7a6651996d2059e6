// emu_air_per.cpp -- the bodies of csrc/air_kernels.h with periodic columns (operand kind PER: the check, the tables air_per_build
// makes, the operand reader) compiled for the host and run lane by lane over the whole grid of the kernel, as emu_air.cpp does for
// the programs without them.  Test infrastructure only; never part of the product library.
//
//   emu_air_per <p> <g> <w>
//       generated programs that read periodic columns of every period 1 .. N at rotations that cross the tables' ends in both
//       directions, over a list of shapes (M = 2 .. 2^12, B = 1, 2, 4, 8, so that P B < M and P B = M both occur), table words at
//       and above p, checked against a plain `unsigned __int128 % p` restatement in this file that evaluates q_k(x^(N/P)) directly
//       at x_i w_N^rot and never builds a table;
//   emu_air_per <p> <g> <w> <log2_n> <log2_blowup> <in> <out>
//       the case of <in> (little-endian u64: the 16 words of emu_air.cpp's header, n_per, log2_period[16]; then ops, imm,
//       per_values, the groups, the extension columns, chal, lambda, T_in), T (2M words) of every policy that serves the field
//       written to <out> one after the other, for tests/test_emu_air_per.py.
//   The last line is "OK ..." on success.  Goldilocks runs the Goldilocks policy, its W = 7 form when w = 7, AND the Montgomery
//   policy.  The coset shift is g.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/air_kernels.h"
using namespace ronk;
#include "emu_ref.h"
#include "emu_census.h"

struct Shape {
  u64 p, g, w;
  u32 log2n, log2b;
  u64 N() const { return (u64)1 << log2n; }
  u64 B() const { return (u64)1 << log2b; }
  u64 M() const { return (u64)1 << (log2n + log2b); }
};
struct Case {
  std::vector<u32> groups, log2_period;
  u32 n_ext = 0, n_chal = 0, n_regs = 0, J = 0, tin = 0;
  std::vector<u64> ops, imm, per_values, chal, lam, T_in;
  std::vector<std::vector<u64>> base, ext;   // [C_g M], [2 M]
};

// ---------------------------------------------------------------------------------------------------- the restatement
// q_k by the P^2 products of the inverse transform, one vector per column
static std::vector<std::vector<u64>> restated_coefficients(const Shape& s, const Case& c) {
  const u64 p = s.p;
  std::vector<std::vector<u64>> out;
  size_t at = 0;
  for (u32 lp : c.log2_period) {
    const u64 P = (u64)1 << lp, wpi = r_pow(r_pow(s.g % p, (p - 1) / P, p), p - 2, p), pinv = r_pow(P % p, p - 2, p);
    std::vector<u64> q(P);
    for (u64 j = 0; j < P; j++) {
      u64 sum = 0;
      for (u64 k = 0; k < P; k++) sum = r_add(sum, r_mul(c.per_values[at + k] % p, r_pow(wpi, j * k % P, p), p), p);
      q[j] = r_mul(sum, pinv, p);
    }
    at += P;
    out.push_back(q);
  }
  return out;
}

static R2 restated_row(const Shape& s, const Case& c, const std::vector<std::vector<u64>>& q, u64 i) {
  const u64 p = s.p, M = s.M(), w = s.w % p;
  const u64 wM = r_pow(s.g, (p - 1) / M, p), x = r_mul(s.g % p, r_pow(wM, i, p), p);
  const u64 wN = r_pow(wM, s.B(), p), wl = r_pow(wN, p - 2, p), ninv = r_pow(s.N() % p, p - 2, p);
  R2 reg[AIR_MAX_REGS] = {}, acc[4] = {};
  auto read = [&](u32 o) {
    const u32 kind = air_kind(o), idx = air_index(o);
    const u64 r = (u64)(((int64_t)i + (int64_t)air_rot(o) * (int64_t)s.B() + (int64_t)M * 4096) % (int64_t)M);
    if (kind == AIR_REG) return reg[idx];
    if (kind == AIR_BASE) {
      u32 g = 0, col = idx;
      while (col >= c.groups[g]) col -= c.groups[g++];
      return R2{c.base[g][col * M + r] % p, 0};
    }
    if (kind == AIR_EXT) return R2{c.ext[idx][r] % p, c.ext[idx][M + r] % p};
    if (kind == AIR_CHAL) return R2{c.chal[2 * idx] % p, c.chal[2 * idx + 1] % p};
    if (kind == AIR_IMM) return R2{c.imm[idx] % p, 0};
    if (kind == AIR_PER) {   // q((x_i w_N^rot)^(N/P)) by Horner's rule
      const u64 rot = (u64)(((int64_t)air_rot(o) + (int64_t)s.N()) % (int64_t)s.N());
      const u64 y = r_pow(r_mul(x, r_pow(wN, rot, p), p), s.N() >> c.log2_period[idx], p);
      u64 v = 0;
      for (size_t j = q[idx].size(); j-- > 0;) v = r_add(r_mul(v, y, p), q[idx][j], p);
      return R2{v, 0};
    }
    return R2{x, 0};
  };
  for (u64 op : c.ops) {
    const u32 code = air_opcode(op);
    const R2 a = read(air_a(op));
    if (code == AIR_EMIT) {
      const u32 j = air_b(op);
      acc[air_dst(op)] = x_add(acc[air_dst(op)], x_mul(R2{c.lam[2 * j] % p, c.lam[2 * j + 1] % p}, a, w, p), p);
    } else if (code == AIR_MOV) reg[air_dst(op)] = a;
    else if (code == AIR_NEG) reg[air_dst(op)] = x_sub(R2{0, 0}, a, p);
    else {
      const R2 b = read(air_b(op));
      reg[air_dst(op)] = code == AIR_ADD ? x_add(a, b, p) : code == AIR_SUB ? x_sub(a, b, p) : x_mul(a, b, w, p);
    }
  }
  const u64 vinv = r_pow(r_sub(r_pow(x, s.N(), p), 1, p), p - 2, p), xl = r_sub(x, wl, p);
  R2 t = x_scale(x_add(acc[AIR_ALL], x_scale(acc[AIR_EXCEPT_LAST], xl, p), p), vinv, p);
  t = x_add(t, x_scale(acc[AIR_FIRST], r_mul(ninv, r_pow(r_sub(x, 1, p), p - 2, p), p), p), p);
  t = x_add(t, x_scale(acc[AIR_LAST], r_mul(r_mul(ninv, wl, p), r_pow(xl, p - 2, p), p), p), p);
  if (c.tin) t = x_add(t, R2{c.T_in[i] % p, c.T_in[M + i] % p}, p);
  return t;
}

// ---------------------------------------------------------------------------------------------------- the kernel, lane by lane
template <class F>
static std::vector<u64> emu_quotient(bool mont, const Shape& s, const Case& c) {
  const u64 p = s.p, M = s.M();
  const u32 log2m = s.log2n + s.log2b;
  const F f(ext2_host_consts(mont, p));
  const Ext2<F> x(f, ext2_reg_form(mont, p, s.w));
  // the domain handle
  const u32 kb = deep_kbits(log2m);
  std::vector<u64> dom(((size_t)1 << kb) + ((size_t)1 << (log2m - kb))), vinv((size_t)s.B());
  DeepDomain dm{};
  deep_host_domain(mont, p, s.g % p, s.g, log2m, dom.data(), dom.data() + ((size_t)1 << kb), &dm.iota, &dm.sinv);
  dm.lo = dom.data(); dm.hi = dom.data() + ((size_t)1 << kb); dm.kbits = kb; dm.log2n = log2m;
  plonk_host_vanishing(mont, p, s.g % p, s.g, s.log2n, s.log2b, vinv.data());
  PlonkTab tab{};
  tab.vinv = vinv.data(); tab.log2b = s.log2b;
  tab.ninv = ext2_reg_form(mont, p, r_pow(s.N() % p, p - 2, p));
  tab.rho = ext2_reg_form(mont, p, log2m >= 3 ? r_pow(s.g % p, (p - 1) >> 3, p) : 1);
  // the program handle
  const u32 n_per = (u32)c.log2_period.size();
  const AirShape sh{s.log2n, (u32)c.groups.size(), c.groups.data(), c.n_ext, c.n_chal, (u32)c.imm.size(), c.n_regs, c.J,
                    n_per,   c.log2_period.data()};
  std::vector<u64> tape, imm, coef, per;
  std::vector<u32> cells;
  u32 boundary = 0;
  const AirStatus st = air_compile(sh, c.ops.data(), (u32)c.ops.size(), &tape, &boundary, &cells);
  CHECK(st == AIR_OK, "the program does not pass the check: %d", (int)st);
  if (st != AIR_OK) return std::vector<u64>(2 * M, 0);
  for (u32 o : cells) CHECK(air_kind(o) != AIR_PER, "a periodic operand among the cells");
  for (u64 v : c.imm) imm.push_back(ext2_reg_form(mont, p, v));
  if (n_per) air_per_build(mont, p, s.g % p, s.g, s.log2n, s.log2b, n_per, c.log2_period.data(), c.per_values.data(), &coef, &per);
  per.push_back(0xDEADBEEFDEADBEEFull);   // nothing reads past the tables
  u64 words = 2 * (u64)n_per;
  for (u32 k = 0; k < n_per; k++) {
    CHECK(per[2 * k] == words && per[2 * k + 1] == (((u64)1 << (c.log2_period[k] + s.log2b)) - 1), "the descriptor of column %u", k);
    words += per[2 * k + 1] + 1;
  }
  CHECK(words + 1 == per.size(), "the tables take sum P B words");
  const u64 wl = r_pow(r_pow(s.g % p, (p - 1) >> s.log2n, p), p - 2, p);
  AirProg pg{};
  pg.tape = tape.data(); pg.imm = imm.data(); pg.n_ops = (u32)tape.size(); pg.n_regs = c.n_regs; pg.boundary = boundary;
  pg.wl = ext2_reg_form(mont, p, wl);
  pg.wln = ext2_reg_form(mont, p, r_mul(wl, r_pow(s.N() % p, p - 2, p), p));
  pg.per = n_per ? per.data() : nullptr;
  std::vector<u64> T(2 * M, ~(u64)0), written(M, 0);
  if (c.tin == 2) T = c.T_in;   // in place
  AirCall call{};
  for (size_t g = 0; g < c.groups.size(); g++) call.base[g] = c.base[g].data();
  for (u32 e = 0; e < c.n_ext; e++) call.ext[e] = c.ext[e].data();
  call.chal = c.chal.data(); call.lambda = c.lam.data();
  call.T_in = c.tin == 0 ? nullptr : c.tin == 1 ? c.T_in.data() : T.data();
  auto run = [&](auto PP) {
    constexpr int PTS = decltype(PP)::value;
    const u32 lanes = air_lanes(c.n_regs, boundary != 0, PTS), slots = air_slots(c.n_regs, boundary != 0, PTS);
    CHECK((u64)slots * 8 * lanes <= AIR_LDS_MAX && lanes >= 64, "the LDS of a workgroup: %u slots, %u lanes", slots, lanes);
    const u64 q = M / PTS, grid = (q + lanes - 1) / lanes;
    std::vector<u64> lds((size_t)slots * lanes + 1);
    for (u64 blk = 0; blk < grid; blk++) {
      for (auto& v : lds) v = 0xDEADBEEFDEADBEEFull;   // what a workgroup finds in LDS is not defined
      for (u32 lane = 0; lane < lanes; lane++) {
        const u64 i = blk * lanes + lane;
        if (i >= q) continue;
        const AirSlots regs{lds.data(), lanes, lane};
        air_lane<F, PTS>(x, dm, tab, pg, call, regs, i, [&](u64 row, E2 v) {
          CHECK(row < M && !written[row], "row %llu out of range or written twice", (unsigned long long)row);
          if (row < M) { T[row] = v.c0; T[M + row] = v.c1; written[row] = 1; }
        });
      }
      CHECK(lds.back() == 0xDEADBEEFDEADBEEFull, "a lane wrote past its slots");
    }
  };
  census_stage("air");   // (emu_census.h: the interpreter's lanes are the one body here)
  if (log2m < PlonkRows<F>::LOG2) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 1 << PlonkRows<F>::LOG2>{});
  census_stage(nullptr);
  for (u64 r = 0; r < M; r++) CHECK(written[r], "row %llu never written", (unsigned long long)r);
  return T;
}

// the policies that serve the field, each against the restatement and against the first
static int run_case(const Shape& s, const Case& c, std::vector<std::vector<u64>>& results) {
  const u64 p = s.p, M = s.M();
  const Case before = c;
  int policies = 0;
  results.clear();
  if (p == gl64::P) {
    census_policy("gl.");
    results.push_back(emu_quotient<FriGl>(false, s, c)); policies |= 1;
    census_policy("w7.");
    if (s.w % p == 7) { results.push_back(emu_quotient<FriGlW7>(false, s, c)); policies |= 2; }
  }
  census_policy("mont.");
  results.push_back(emu_quotient<FriMont>(true, s, c)); policies |= 4;
  CHECK(before.base == c.base && before.ext == c.ext && before.chal == c.chal && before.lam == c.lam && before.T_in == c.T_in &&
            before.per_values == c.per_values,
        "an input changed");
  const std::vector<std::vector<u64>> q = restated_coefficients(s, c);
  std::vector<u64> rows;
  if (M <= 512) {
    for (u64 i = 0; i < M; i++) rows.push_back(i);
  } else {   // both ends of every eighth (a lane's rows are M / 8 or M / 4 apart), and random rows
    for (u64 e = 0; e < 8; e++)
      for (u64 d = 0; d < 2; d++) { rows.push_back(e * (M / 8) + d); rows.push_back((e + 1) * (M / 8) - 1 - d); }
    for (int j = 0; j < 48; j++) rows.push_back(rnd() % M);
  }
  for (u64 i : rows) {
    const R2 want = restated_row(s, c, q, i);
    for (size_t r = 0; r < results.size(); r++)
      CHECK(results[r][i] == want.c0 && results[r][M + i] == want.c1, "policy %zu row %llu", r, (unsigned long long)i);
  }
  for (size_t r = 1; r < results.size(); r++) CHECK(results[r] == results[0], "policy %zu differs from the first", r);
  return policies;
}

// ---------------------------------------------------------------------------------------------------- generated cases
static u64 operand(u32 kind, u32 index, int rot) { return kind | index << 4 | ((u32)rot & 0xfff) << 12; }
static u64 make_op(u32 code, u32 dst, u64 a, u64 b) { return code | (u64)dst << 8 | a << 16 | b << 40; }

// n_per periodic columns of the periods 1, 2, 4, .. capped at N and then N again; two base columns, one extension column, one
// challenge.  Every periodic column is read at every rotation of the list; the reads are chained through four registers with MUL,
// ADD and SUB, so a register holds a base value at one op and an extension value at another; four constraints, one of each kind.
static void generate(const Shape& s, Case& c, u32 n_per, u32 tin) {
  const u64 p = s.p, M = s.M();
  const int N = (int)s.N(), far = N - 1 < 2047 ? N - 1 : 2047;
  const int rots_all[6] = {0, 1, -1, 2, far, -far};
  std::vector<int> rots;
  for (int r : rots_all) if (r < N && -r < N) rots.push_back(r);
  c = Case();
  c.groups.assign(1, 2);
  c.n_ext = 1; c.n_chal = 1; c.n_regs = 4; c.J = 4; c.tin = tin;
  for (u32 k = 0; k < n_per; k++) {
    const u32 lp = k == n_per - 1 ? s.log2n : k < s.log2n ? k : s.log2n;
    c.log2_period.push_back(lp);
    for (u64 j = 0; j < ((u64)1 << lp); j++) c.per_values.push_back(edge_word(p));
  }
  c.ops.push_back(make_op(AIR_MOV, 0, operand(AIR_BASE, 0, 0), 0));
  c.ops.push_back(make_op(AIR_MOV, 1, operand(AIR_EXT, 0, rots.back()), 0));
  c.ops.push_back(make_op(AIR_NEG, 2, operand(AIR_PER, n_per - 1, rots.back()), 0));
  c.ops.push_back(make_op(AIR_MOV, 3, operand(AIR_CHAL, 0, 0), 0));
  u32 k = 0;
  for (u32 col = 0; col < n_per; col++)
    for (int r : rots) {
      const u32 codes[3] = {AIR_MUL, AIR_ADD, AIR_SUB};
      const u64 per = operand(AIR_PER, col, r), prev = operand(AIR_REG, (k + 3) % 4, 0);
      c.ops.push_back(k % 2 ? make_op(codes[k % 3], k % 4, per, prev) : make_op(codes[k % 3], k % 4, prev, per));
      k++;
    }
  c.ops.push_back(make_op(AIR_MUL, 0, operand(AIR_PER, 0, 0), operand(AIR_BASE, 1, 1)));   // base times base
  for (u32 j = 0; j < 4; j++) c.ops.push_back(make_op(AIR_EMIT, j, operand(AIR_REG, j, 0), j));
  c.base.assign(1, std::vector<u64>(2 * M));
  c.ext.assign(1, std::vector<u64>(2 * M));
  for (auto& v : c.base) for (auto& t : v) t = edge_word(p);
  for (auto& v : c.ext) for (auto& t : v) t = edge_word(p);
  c.chal.resize(2); c.lam.resize(2 * c.J); c.T_in.resize(2 * M);
  for (auto* v : {&c.chal, &c.lam, &c.T_in}) for (auto& t : *v) t = edge_word(p);
}

static bool read_words(FILE* fp, std::vector<u64>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 8, n, fp) == n;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 8) { fprintf(stderr, "usage: emu_air_per p g w [log2_n log2_blowup in out]\n"); return 2; }
  Shape s{};
  s.p = strtoull(argv[1], nullptr, 0); s.g = strtoull(argv[2], nullptr, 0); s.w = strtoull(argv[3], nullptr, 0);
  const u64 p = s.p;
  if (p < 3 || !(p & 1) || !ext2_non_residue(p, s.w)) { fprintf(stderr, "p must be an odd prime, w a quadratic non-residue\n"); return 2; }
  g_rng = p ^ s.w ^ 29;
  std::vector<std::vector<u64>> results;
  if (argc == 8) {
    s.log2n = (u32)atoi(argv[4]); s.log2b = (u32)atoi(argv[5]);
    if (s.log2n < 1 || s.log2n + s.log2b > 24 || (p - 1) % s.M() || r_pow(s.g % p, s.M(), p) == 1) { fprintf(stderr, "a shape the domain refuses\n"); return 2; }
    const u64 M = s.M();
    Case c;
    std::vector<u64> hd;
    FILE* fp = fopen(argv[6], "rb");
    bool ok = fp && read_words(fp, hd, 33);
    if (ok) {
      for (u64 g = 0; g < hd[0] && g < 8; g++) c.groups.push_back((u32)hd[1 + g]);
      c.n_ext = (u32)hd[9]; c.n_chal = (u32)hd[10]; c.n_regs = (u32)hd[12]; c.J = (u32)hd[13]; c.tin = (u32)hd[15];
      ok = c.n_ext <= AIR_MAX_EXT && hd[14] <= AIR_MAX_OPS && hd[11] <= AIR_MAX_IMM && c.n_chal <= AIR_MAX_CHAL && c.J <= AIR_MAX_CONSTRAINTS &&
           hd[16] <= AIR_MAX_PER;
      size_t per_words = 0;
      for (u64 k = 0; ok && k < hd[16]; k++) {
        ok = hd[17 + k] <= s.log2n;
        c.log2_period.push_back((u32)hd[17 + k]);
        per_words += (size_t)1 << (hd[17 + k] & 31);
      }
      ok = ok && read_words(fp, c.ops, hd[14]) && read_words(fp, c.imm, hd[11]) && read_words(fp, c.per_values, per_words);
      c.base.resize(c.groups.size()); c.ext.resize(c.n_ext);
      for (size_t g = 0; ok && g < c.groups.size(); g++) ok = c.groups[g] <= AIR_MAX_BASE && read_words(fp, c.base[g], c.groups[g] * M);
      for (u32 e = 0; ok && e < c.n_ext; e++) ok = read_words(fp, c.ext[e], 2 * M);
      ok = ok && read_words(fp, c.chal, 2 * c.n_chal) && read_words(fp, c.lam, 2 * c.J) && read_words(fp, c.T_in, c.tin ? 2 * M : 0);
    }
    if (fp) fclose(fp);
    if (!ok) { fprintf(stderr, "cannot read the case from %s\n", argv[6]); return 2; }
    const int policies = run_case(s, c, results);
    fp = fopen(argv[7], "wb");
    ok = fp != nullptr;
    for (size_t r = 0; ok && r < results.size(); r++) ok = fwrite(results[r].data(), 8, 2 * M, fp) == 2 * M;
    if (fp) ok = fclose(fp) == 0 && ok;
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
    if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
    printf("OK p=%llu w=%llu M=%llu policies=%d results=%zu\n", (unsigned long long)p, (unsigned long long)s.w, (unsigned long long)M, policies,
           results.size());
    return 0;
  }
  // log2_n, log2_b, periodic columns, T_in
  struct Gen { u32 log2n, log2b, n_per, tin; };
  const std::vector<Gen> gens = {{1, 0, 1, 0}, {1, 1, 2, 1}, {2, 1, 3, 2}, {1, 2, 2, 0}, {3, 0, 4, 1},  {2, 2, 3, 2},
                                 {4, 2, 16, 0}, {5, 1, 6, 1}, {6, 3, 7, 2}, {10, 2, 4, 0}, {9, 3, 16, 1}, {11, 1, 5, 2}};
  int cases = 0, policies = 0;
  for (const Gen& gn : gens) {
    s.log2n = gn.log2n; s.log2b = gn.log2b;
    if ((p - 1) % s.M() || r_pow(s.g % p, s.M(), p) == 1) continue;   // a small field has no such domain
    Case c;
    generate(s, c, gn.n_per, gn.tin);
    const int before = g_fail;
    policies = run_case(s, c, results);
    if (g_fail != before) printf("in the case N=2^%u B=2^%u n_per=%u\n", gn.log2n, gn.log2b, gn.n_per);
    cases++;
  }
  // the check itself, in its order
  {
    const u32 cols[1] = {2}, fine[2] = {3, 0}, wide[2] = {0, 4}, many[17] = {};
    const u64 ok_ops[2] = {make_op(AIR_MOV, 0, operand(AIR_PER, 1, -7), 0), make_op(AIR_EMIT, 0, operand(AIR_REG, 0, 0), 0)};
    const u64 past[2] = {make_op(AIR_MOV, 0, operand(AIR_PER, 2, 0), 0), ok_ops[1]};
    const u64 far[2] = {make_op(AIR_MOV, 0, operand(AIR_PER, 1, 8), 0), ok_ops[1]};
    auto shape = [&](u32 n_per, const u32* lp) { return AirShape{3, 1, cols, 1, 1, 1, 2, 1, n_per, lp}; };
    CHECK(air_compile(shape(2, fine), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_OK, "a periodic operand at rot = -(N - 1)");
    CHECK(air_compile(shape(17, many), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_UNSUPPORTED, "seventeen periodic columns");
    CHECK(air_compile(shape(17, nullptr), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_UNSUPPORTED, "seventeen columns before the NULL array");
    CHECK(air_compile(shape(2, wide), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_UNSUPPORTED, "a period above N");
    CHECK(air_compile(shape(2, nullptr), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_INVALID, "a NULL array of periods");
    CHECK(air_compile(shape(2, fine), past, 2, nullptr, nullptr, nullptr) == AIR_INVALID, "a periodic index past n_per");
    CHECK(air_compile(shape(0, nullptr), ok_ops, 2, nullptr, nullptr, nullptr) == AIR_INVALID, "a periodic operand without columns");
    CHECK(air_compile(shape(2, fine), far, 2, nullptr, nullptr, nullptr) == AIR_INVALID, "rot = N on a periodic operand");
    CHECK(air_compile(shape(2, wide), past, 0, nullptr, nullptr, nullptr) == AIR_INVALID, "no ops comes before the periods");
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu w=%llu cases=%d policies=%d\n", (unsigned long long)p, (unsigned long long)s.w, cases, policies);
  return 0;
}
