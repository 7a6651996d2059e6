// emu_stark.cpp -- the bodies of csrc/stark_kernels.h (the quotient split, the coset scaling of a round's coefficients, the
// transcript steps, the weights and the points) compiled for the host and run lane by lane over a grid, against a plain
// `unsigned __int128 % p` restatement in this file.  The Poseidon setup and the sponge restatement are those of emu_fri.cpp.  Test
// infrastructure only; never part of the product library.
//
//   emu_stark <p> <g>
//       M = 2 .. 2^12 with B = 1, 2, 8 (where B <= M), the shift s = g and s = p - 1 (order two), inputs with 0, p - 1 and words
//       >= p mixed in, grids of one lane, of 64 lanes and of the launch's 256-lane workgroups (so a lane owns one residue, or
//       several).  The split needs no root of unity, so F_17 and F_97 run every size.  Fields above 2^32 also run the transcript
//       steps against the sponge restatement.  Goldilocks runs its own policy, the W = 7 form AND the Montgomery policy.
//   The last line is "OK ..." on success.
#define main emu_fri_main
#include "emu_fri.cpp"
#undef main

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/stark_kernels.h"

static int g_cases = 0;

// ---------------------------------------------------------------------------------------------------- split and shift
template <class F>
static void run_split(bool mont, u64 p, u64 s, u32 log2m, u32 log2b) {
  const FriConsts k = ext2_host_consts(mont, p);
  const F f(k);
  const u32 log2n = log2m - log2b;
  const u64 N = (u64)1 << log2n, B = (u64)1 << log2b, M = (u64)1 << log2m;
  const u64 sinv = r_pow(s, p - 2, p);
  std::vector<u64> cin(2 * M);
  for (auto& v : cin) v = edge_word(p);
  // the restatement: c_j = c'_j s^-j; piece i, plane pl, word k
  std::vector<u64> want_coef(2 * M), want_msg(2 * M);
  for (u64 pl = 0; pl < 2; pl++)
    for (u64 j = 0; j < M; j++) {
      const u64 i = j >> log2n, kk = j & (N - 1), c = cin[pl * M + j] % p;
      want_coef[(2 * i + pl) * N + kk] = r_mul(c, r_pow(sinv, j, p), p);
      want_msg[(2 * i + pl) * N + kk] = r_mul(c, r_pow(sinv, i * N, p), p);
    }
  const u64 launch = (u64)256 * ((N + 255) / 256 > 8192 ? 8192 : (N + 255) / 256);
  for (u64 lanes : {(u64)1, (u64)64, launch, (u64)3}) {
    const StarkShift sh{ext2_reg_form(mont, p, sinv), ext2_reg_form(mont, p, r_pow(sinv, N, p)), ext2_reg_form(mont, p, r_pow(sinv, lanes, p))};
    std::vector<u64> coef(2 * M, ~(u64)0), msg(2 * M, ~(u64)0);
    for (u64 lane = 0; lane < lanes; lane++) stark_split_lane(f, sh, log2n, log2b, lane, lanes, cin.data(), coef.data(), msg.data());
    CHECK(coef == want_coef, "split coef p=%llu s=%llu M=2^%u B=%llu lanes=%llu", (unsigned long long)p, (unsigned long long)s, log2m,
          (unsigned long long)B, (unsigned long long)lanes);
    CHECK(msg == want_msg, "split msg p=%llu s=%llu M=2^%u B=%llu lanes=%llu", (unsigned long long)p, (unsigned long long)s, log2m,
          (unsigned long long)B, (unsigned long long)lanes);
  }
  // the trace rounds' scaling on the same sizes: C = 1, 3 rows of N words times s^k
  for (u32 C : {1u, 3u}) {
    std::vector<u64> co(C * N), want(C * N);
    for (auto& v : co) v = edge_word(p);
    for (u64 c = 0; c < C; c++)
      for (u64 kk = 0; kk < N; kk++) want[c * N + kk] = r_mul(co[c * N + kk] % p, r_pow(s, kk, p), p);
    for (u64 lanes : {(u64)1, launch, (u64)5}) {
      const StarkShift sh{ext2_reg_form(mont, p, s % p), 0, ext2_reg_form(mont, p, r_pow(s, lanes, p))};
      std::vector<u64> msg(C * N, ~(u64)0);
      for (u64 lane = 0; lane < lanes; lane++) stark_shift_lane(f, sh, log2n, C, lane, lanes, co.data(), msg.data());
      CHECK(msg == want, "shift p=%llu N=2^%u C=%u lanes=%llu", (unsigned long long)p, log2n, C, (unsigned long long)lanes);
    }
  }
  g_cases++;
}

template <class F>
static void run_sizes(bool mont, u64 p, u64 g) {
  for (u32 log2m = 1; log2m <= 12; log2m++)
    for (u32 log2b : {0u, 1u, 3u}) {
      if (log2b > log2m) continue;
      for (u64 s : {g % p, p - 1}) run_split<F>(mont, p, s, log2m, log2b);
    }
}

// ---------------------------------------------------------------------------------------------------- weights and points
template <class F>
static void run_small(bool mont, u64 p, u64 g) {
  const FriConsts k = ext2_host_consts(mont, p);
  const F f(k);
  const u64 w = g % p;
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  for (int it = 0; it < 20; it++) {
    const u64 lam[2] = {edge_word(p), edge_word(p)};
    const u32 J = it == 0 ? 1 : 1 + (u32)(rnd() % STARK_MAX_J);
    std::vector<u64> out(2 * J, ~(u64)0);
    stark_weights(x, lam, J, out.data());
    R2 a{1 % p, 0};
    for (u32 j = 0; j < J; j++) {
      CHECK(out[2 * j] == a.c0 && out[2 * j + 1] == a.c1, "weight %u", j);
      a = x_mul(a, red(R2{lam[0], lam[1]}, p), w, p);
    }
    StarkRots r{};
    r.K = 1 + (u32)(rnd() % STARK_MAX_K);
    u64 plain[STARK_MAX_K];
    for (u32 kk = 0; kk < r.K; kk++) { plain[kk] = kk ? rnd() % p : 1 % p; r.m[kk] = ext2_reg_form(mont, p, plain[kk]); }
    u64 z[2 * STARK_MAX_K];
    stark_points(f, lam, r, z);
    for (u32 kk = 0; kk < r.K; kk++)
      CHECK(z[kk] == r_mul(lam[0] % p, plain[kk], p) && z[r.K + kk] == r_mul(lam[1] % p, plain[kk], p), "point %u", kk);
  }
}

// ---------------------------------------------------------------------------------------------------- transcript
template <class PF, int W>
static void run_transcript(u64 p, const Setup2& S) {
  const PF pf(S.sp);
  for (u32 d : {1u, 2u, 3u})
    for (u32 n_pub : {0u, 1u, 5u}) {
      std::vector<u64> seed(d), pub(2 * n_pub + 1), t(d, 7), chal(2 * n_pub + 1, 9), in;
      for (auto& v : seed) v = edge_word(p);
      for (auto& v : pub) v = edge_word(p);
      stark_begin<PF, W>(pf, S.sp, d, seed.data(), pub.data(), n_pub, t.data(), chal.data());
      in = seed;
      in.insert(in.end(), pub.begin(), pub.begin() + 2 * n_pub);
      std::vector<u64> want(d);
      ref_sponge(S.P, in.data(), in.size(), 1, want.data(), d);
      CHECK(t == want, "begin d=%u n_pub=%u", d, n_pub);
      for (u32 j = 0; j < 2 * n_pub; j++) CHECK(chal[j] == pub[j] % p, "public pair word %u", j);
      CHECK(chal[2 * n_pub] == 9, "begin writes the public pairs only");
      for (u32 n_draw : {0u, 2u, 8u}) {
        std::vector<u64> root(d), draw(n_draw + 1, 5), tt(t), full(d + n_draw);
        for (auto& v : root) v = edge_word(p);
        in = t;
        in.insert(in.end(), root.begin(), root.end());
        ref_sponge(S.P, in.data(), in.size(), 1, full.data(), d + n_draw);
        stark_draw<PF, W>(pf, S.sp, d, tt.data(), root.data(), n_draw, draw.data());
        CHECK(std::vector<u64>(full.begin(), full.begin() + d) == tt, "draw t d=%u n=%u", d, n_draw);
        CHECK(std::vector<u64>(full.begin() + d, full.end()) == std::vector<u64>(draw.begin(), draw.begin() + n_draw), "draw d=%u n=%u", d, n_draw);
        CHECK(draw[n_draw] == 5, "draw writes n_draw words");
      }
    }
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_stark p g\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0);
  if (!(p & 1) || p < 5) { fprintf(stderr, "p must be an odd prime above 3\n"); return 2; }
  g_rng = p ^ g ^ 23;
  int policies = 0;
  if (p == gl64::P) {
    run_sizes<FriGl>(false, p, g); run_small<FriGl>(false, p, g); policies++;
    if (g % p == 7) { run_sizes<FriGlW7>(false, p, g); run_small<FriGlW7>(false, p, g); policies++; }
  }
  run_sizes<FriMont>(true, p, g);
  if (ext2_non_residue(p, g)) run_small<FriMont>(true, p, g);
  policies++;
  if (p > ((u64)1 << 32)) {
    Setup2 S;
    make_poseidon(S, p);
    if (p == gl64::P) run_transcript<PosGl, 8>(p, S);
    else run_transcript<PosMont, 8>(p, S);
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu g=%llu policies=%d cases=%d\n", (unsigned long long)p, (unsigned long long)g, policies, g_cases);
  return 0;
}
