// emu_pow.cpp -- the proof-of-work bodies of csrc/pow_kernels.h (prefix, candidate, search step, the verifier's squeeze) compiled
// for the host and run over the search kernel's grid for a given number of lanes T, in three execution orders: every lane to
// completion in forward order, in reverse order, and all lanes stepped round-robin one candidate at a time.  The found word is
// a plain variable here (one host thread): a load is a read, a hit a minimum.  The three nonces are compared with a sequential
// search on the `unsigned __int128 % p` sponge of emu_poseidon.cpp.  The Poseidon constants are those of
// tests/poseidon_ref.py derive_params (seed 1), restated here, so that tests/test_emu_pow.py can compare the nonce with
// tests/pow_ref.py.  Test infrastructure only; never part of the product library.
//
//   emu_pow <p> <width> <alpha> <num_p> <num_f> <rate> <bits> <log2_limit> <T> [seed words ...]
//   last line "OK nonce=<n> ..." on success (n = 18446744073709551615 when there is none below the limit)
#define EMU_POSEIDON_LIB
#include "emu_poseidon.cpp"

#include "../../ronkathon_amd/csrc/pow_kernels.h"
using namespace ronk;

struct Setup3 {
  RefParams P;
  std::vector<u64> rc, mds, tab;
  PoseidonConsts sp;
};
// poseidon_ref.derive_params: rc from SplitMix64(seed * 1000003 + width * 131 + alpha), mds[i][j] = 1 / (i + width + j)
static void make_params(Setup3& S, u64 p, u32 width, u64 alpha, u32 num_p, u32 num_f, u32 rate) {
  const u32 rounds = num_p + num_f;
  g_rng = 1 * 1000003ull + width * 131ull + alpha;
  S.rc.resize((size_t)rounds * width);
  for (auto& c : S.rc) c = rnd() % p;
  S.mds.resize((size_t)width * width);
  for (u32 i = 0; i < width; i++)
    for (u32 j = 0; j < width; j++) S.mds[i * width + j] = r_pow((i + width + j) % p, p - 2, p);
  S.P = RefParams{p, width, num_p, num_f, rate, alpha, S.rc.data(), S.mds.data()};
  const u32 W = poseidon_padded_width(width);
  const size_t nrc = (size_t)rounds * W, nm = (size_t)W * W;
  S.tab.assign(2 * (nrc + nm), 0);
  poseidon_host_tables(p, width, rate, rounds, S.rc.data(), S.mds.data(), S.tab.data());
  PoseidonConsts k{};
  k.alpha = alpha; k.rounds = rounds; k.full_lo = num_f / 2; k.full_from = num_p + num_f / 2; k.rate = rate;
  if (p != gl64::P) {
    const mont64::Field mf = mont64::make_field(p);
    k.p = p; k.pinv = mf.pinv; k.r2 = mf.r2;
  }
  S.sp = k; S.sp.rc = S.tab.data() + nrc + nm; S.sp.mds = S.tab.data() + 2 * nrc + nm;
}

struct Run { u64 nonce, candidates; };

// order 0: lanes forward, each to completion; 1: lanes in reverse; 2: round-robin, one candidate per lane and turn
template <class PF, int W>
static Run run_grid(const Setup3& S, const std::vector<u64>& seed, u32 bits, u32 log2_limit, u64 T, int order) {
  const PF pf(S.sp);
  u64 state0[POW_WORK_WORDS], found = 12345;   // the prefix must overwrite the found word
  for (auto& v : state0) v = ~(u64)0;
  pow_prefix<PF, W>(pf, S.sp, (u32)seed.size(), seed.data(), state0, &found);
  u64 s0[W];
  for (int i = 0; i < W; i++) s0[i] = state0[i];
  const u32 slot = pow_slot((u32)seed.size(), S.sp.rate);
  const u64 mask = ((u64)1 << bits) - 1, limit = (u64)1 << log2_limit;
  const u64 lanes = (T + 255) / 256 * 256;   // the grid: whole workgroups of 256
  Run r{0, 0};
  auto load = [&]() { return found; };
  auto hit = [&](u64 n) { if (n < found) found = n; };
  auto step = [&](u64& n) {
    if (n < found && n < limit) r.candidates++;   // the step will hash this candidate (one thread: `found` is what it loads)
    return pow_search_step<PF, W>(pf, S.sp, s0, slot, mask, limit, T, n, load, hit);
  };
  if (order < 2) {
    for (u64 i = 0; i < lanes; i++) {
      u64 n = order == 0 ? i : lanes - 1 - i;
      if (n >= T) continue;   // the kernel's guard
      while (step(n)) {}
    }
  } else {
    std::vector<u64> next(lanes);
    std::vector<char> alive(lanes);
    u64 left = 0;
    for (u64 g = 0; g < lanes; g++) { next[g] = g; alive[g] = g < T; left += alive[g]; }
    while (left)
      for (u64 g = 0; g < lanes; g++)
        if (alive[g] && !step(next[g])) { alive[g] = 0; left--; }
  }
  r.nonce = found;
  return r;
}

template <class PF, int W>
static int run_all(const Setup3& S, const std::vector<u64>& seed, u32 bits, u32 log2_limit, u64 T) {
  const u64 p = S.P.p;
  // the sequential search of the restatement
  u64 want = POW_NONE;
  std::vector<u64> item(seed);
  item.push_back(0);
  for (u64 n = 0; n < ((u64)1 << log2_limit); n++) {
    item.back() = n;
    u64 word;
    ref_sponge(S.P, item.data(), item.size(), 1, &word, 1);
    if ((word & (((u64)1 << bits) - 1)) == 0) { want = n; break; }
  }
  Run r[3];
  for (int o = 0; o < 3; o++) {
    r[o] = run_grid<PF, W>(S, seed, bits, log2_limit, T, o);
    CHECK(r[o].nonce == want, "order %d: nonce %llu, the restatement %llu", o, (unsigned long long)r[o].nonce, (unsigned long long)want);
  }
  // the verifier's squeeze: the honest nonce, nonce + 1 by the restated condition, the limit, the not-found word
  const PF pf(S.sp);
  const u32 d = S.sp.rate < 4 ? S.sp.rate : 4;
  const u64 tries[] = {want, want + 1, (u64)1 << log2_limit, POW_NONE, p + 3};
  for (u64 n : tries) {
    std::vector<u64> got(d, 7), ref(d, 9);
    const int ok = pow_squeeze<PF, W>(pf, S.sp, (u32)seed.size(), seed.data(), n, bits, log2_limit, d, got.data());
    item.back() = n;
    ref_sponge(S.P, item.data(), item.size(), 1, ref.data(), d);
    CHECK(got == ref, "squeeze of nonce %llu", (unsigned long long)n);
    const int ok_ref = n < ((u64)1 << log2_limit) && (ref[0] & (((u64)1 << bits) - 1)) == 0;
    CHECK(ok == ok_ref, "condition of nonce %llu: %d, the restatement %d", (unsigned long long)n, ok, ok_ref);
  }
  // in place, as FRI replaces u by u'
  if (seed.size() >= d && want != POW_NONE) {
    std::vector<u64> buf(seed), ref(d);
    item.back() = want;
    ref_sponge(S.P, item.data(), item.size(), 1, ref.data(), d);
    pow_squeeze<PF, W>(pf, S.sp, (u32)seed.size(), buf.data(), want, bits, log2_limit, d, buf.data());
    CHECK(std::vector<u64>(buf.begin(), buf.begin() + d) == ref, "in-place squeeze");
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK nonce=%llu T=%llu candidates forward=%llu reverse=%llu round_robin=%llu\n", (unsigned long long)want, (unsigned long long)T,
         (unsigned long long)r[0].candidates, (unsigned long long)r[1].candidates, (unsigned long long)r[2].candidates);
  return 0;
}

template <class PF>
static int run_w(u32 W, const Setup3& S, const std::vector<u64>& seed, u32 bits, u32 log2_limit, u64 T) {
  switch (W) {
    case 4: return run_all<PF, 4>(S, seed, bits, log2_limit, T);
    case 8: return run_all<PF, 8>(S, seed, bits, log2_limit, T);
    case 12: return run_all<PF, 12>(S, seed, bits, log2_limit, T);
    default: return run_all<PF, 16>(S, seed, bits, log2_limit, T);
  }
}

int main(int argc, char** argv) {
  if (argc < 10) { fprintf(stderr, "usage: emu_pow p width alpha num_p num_f rate bits log2_limit T [seed words]\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0);
  const u32 width = (u32)strtoul(argv[2], nullptr, 0);
  const u64 alpha = strtoull(argv[3], nullptr, 0);
  const u32 num_p = (u32)strtoul(argv[4], nullptr, 0), num_f = (u32)strtoul(argv[5], nullptr, 0), rate = (u32)strtoul(argv[6], nullptr, 0);
  const u32 bits = (u32)strtoul(argv[7], nullptr, 0), log2_limit = (u32)strtoul(argv[8], nullptr, 0);
  const u64 T = strtoull(argv[9], nullptr, 0);
  std::vector<u64> seed;
  for (int i = 10; i < argc; i++) seed.push_back(strtoull(argv[i], nullptr, 0));
  if (p < 3 || !(p & 1) || width < 2 || width > 16 || rate < 1 || rate >= width || !T || T > ((u64)1 << 24) ||
      pow_host_check(p, seed.size(), bits, log2_limit) || log2_limit > 24) {
    fprintf(stderr, "arguments out of range\n");
    return 2;
  }
  Setup3 S;
  make_params(S, p, width, alpha, num_p, num_f, rate);
  const u32 W = poseidon_padded_width(width);
  return p == gl64::P ? run_w<PosGl>(W, S, seed, bits, log2_limit, T) : run_w<PosMont>(W, S, seed, bits, log2_limit, T);
}
