// emu_fri.cpp -- the FRI bodies of csrc/fri_kernels.h (fold, transcript, query check, final-degree sum) compiled for the host and
// compared with a plain `unsigned __int128 % p` restatement in this file; the sponge and the tree of the restatement are those of
// emu_poseidon.cpp.  Test infrastructure only; never part of the product library.
//
//   emu_fri <p> <g>     last line "OK ..." on success.  Goldilocks with g = 7 runs the shift policy AND the Montgomery policy.
#define EMU_POSEIDON_LIB
#include "emu_poseidon.cpp"

#include "../../ronkathon_amd/csrc/fri_kernels.h"
#include "emu_census.h"
using namespace ronk;


// ---------------------------------------------------------------------------------------------------- the restatement
// f'[i] = (a + b) / 2 + beta (a - b) / (2 x_i), x_i = s w^i
static std::vector<u64> ref_fold2(u64 p, const std::vector<u64>& f, u64 beta, u64 s, u64 w) {
  const size_t h = f.size() / 2;
  const u64 inv2 = r_pow(2, p - 2, p);
  std::vector<u64> out(h);
  for (size_t i = 0; i < h; i++) {
    const u64 a = f[i] % p, b = f[i + h] % p;
    const u64 x2inv = r_pow(r_mul(2, r_mul(s, r_pow(w, i, p), p), p), p - 2, p);
    out[i] = r_add(r_mul(r_add(a, b, p), inv2, p), r_mul(r_mul(beta % p, r_sub(a, b, p), p), x2inv, p), p);
  }
  return out;
}
static std::vector<u64> ref_fold(u64 p, u64 g, std::vector<u64> f, u64 beta, u64 s, u32 eta) {
  u64 w = r_pow(g, (p - 1) / f.size(), p), b = beta % p;
  for (u32 e = 0; e < eta; e++) {
    f = ref_fold2(p, f, b, s, w);
    s = r_mul(s, s, p); w = r_mul(w, w, p); b = r_mul(b, b, p);
  }
  return f;
}

struct Tables {
  FriShape sh;
  FriConsts k;
  std::vector<std::vector<u64>> lo, hi;
  std::vector<FriLayer> layers;
  std::vector<u64> wfin;
};
static void make_tables(Tables& T, bool mont, u64 p, u64 g, u64 shift, u32 n, u32 eta, u32 log2_final, u64 queries, u64 d) {
  T.sh = FriShape{n, eta, log2_final, (n - log2_final) / eta, queries, d};
  T.k = fri_host_consts(mont, p, g, eta);
  const u32 L = T.sh.layers;
  T.lo.resize(L); T.hi.resize(L); T.layers.resize(L);
  for (u32 l = 0; l < L; l++) {
    const u32 lm = T.sh.log2m(l), kb = fri_kbits(lm);
    T.lo[l].assign((size_t)1 << kb, ~(u64)0); T.hi[l].assign((size_t)1 << (lm - kb), ~(u64)0);
    fri_host_layer_table(mont, p, g, shift, T.sh, l, T.lo[l].data(), T.hi[l].data());
    T.layers[l] = FriLayer{T.hi[l].data(), T.lo[l].data(), kb, lm, T.sh.leaf_off(l), T.sh.path_off(l)};
  }
  T.wfin.resize(T.sh.size(L));
  fri_host_final_table(mont, p, g, T.sh, T.wfin.data());
}

// ---------------------------------------------------------------------------------------------------- fold
template <class F, int ETA>
static void run_fold(bool mont, u64 p, u64 g) {
  const u32 ns[] = {ETA, ETA + 1, 5 + ETA, 9};
  const u64 shifts[] = {1, g, p - 1, rnd() % (p - 1) + 1};
  static const char* const stage[] = {"", "fold_base_eta1", "fold_base_eta2", "fold_base_eta3"};
  census_stage(stage[ETA]);
  for (u32 n : ns)
    for (u64 shift : shifts) {
      // every layer of a chain down to one word
      Tables T;
      make_tables(T, mont, p, g, shift, n, ETA, n % ETA, 1, 1);
      const F f(T.k);
      u64 s = shift;
      for (u32 l = 0; l < T.sh.layers; l++) {
        const u64 N = T.sh.size(l), m = N >> ETA;
        std::vector<u64> in(N);
        for (auto& v : in) v = edge_word(p);
        const u64 betas[] = {0, 1, p - 1, rnd() % p, p + 1};
        for (u64 beta : betas) {
          const std::vector<u64> want = ref_fold(p, g, in, beta, s, ETA);
          for (u64 i = 0; i < m; i++) {
            const u64 got = fri_fold_leaf<F, ETA>(f, fri_gamma(f, T.layers[l], i, f.in(beta)), [&](int t) { return in[i + (u64)t * m]; });
            CHECK(got == want[i], "fold eta=%d n=%u layer=%u i=%llu beta=%llu", ETA, n, l, (unsigned long long)i, (unsigned long long)beta);
          }
        }
        for (int e = 0; e < ETA; e++) s = r_mul(s, s, p);
      }
    }
}

// ---------------------------------------------------------------------------------------------------- transcript and verifier
struct Setup2 {
  RefParams P;
  std::vector<u64> rc, mds, tab;
  PoseidonConsts sp;
  u32 W;
};
static void make_poseidon(Setup2& S, u64 p) {
  const u32 width = 5, rate = 3, num_p = 2, num_f = 4, rounds = num_p + num_f;
  S.rc.resize((size_t)rounds * width); S.mds.resize((size_t)width * width);
  for (auto& c : S.rc) c = rnd() % p;
  for (auto& c : S.mds) c = rnd() % p;
  S.P = RefParams{p, width, num_p, num_f, rate, 5, S.rc.data(), S.mds.data()};
  S.W = poseidon_padded_width(width);
  const size_t nrc = (size_t)rounds * S.W, nm = (size_t)S.W * S.W;
  S.tab.assign(2 * (nrc + nm), 0);
  poseidon_host_tables(p, width, rate, rounds, S.rc.data(), S.mds.data(), S.tab.data());
  PoseidonConsts k{};
  k.alpha = 5; k.rounds = rounds; k.full_lo = num_f / 2; k.full_from = num_p + num_f / 2; k.rate = rate;
  if (p != gl64::P) {
    const mont64::Field mf = mont64::make_field(p);
    k.p = p; k.pinv = mf.pinv; k.r2 = mf.r2;
  }
  S.sp = k; S.sp.rc = S.tab.data() + nrc + nm; S.sp.mds = S.tab.data() + 2 * nrc + nm;
}

template <class F, int ETA, class PF, int W>
static void run_proof(bool mont, u64 p, u64 g, const Setup2& S) {
  const u32 n = 2 * ETA + 2, log2_final = 2, log2_blowup = 1;
  const u64 Q = 6, D = 2, A = (u64)1 << ETA, shift = g;
  census_stage(nullptr);   // a composition of the bodies counted on their own
  Tables T;
  make_tables(T, mont, p, g, shift, n, ETA, log2_final, Q, D);
  const FriShape& sh = T.sh;
  const u32 L = sh.layers;
  const F f(T.k);
  const PF pf(S.sp);
  // a codeword of degree < N_0 / 2 by direct evaluation
  const u64 N0 = sh.size(0), w0 = r_pow(g, (p - 1) / N0, p);
  std::vector<u64> coeffs(N0 >> log2_blowup), cur(N0);
  for (auto& c : coeffs) c = rnd() % p;
  for (u64 i = 0; i < N0; i++) {
    const u64 x = r_mul(shift, r_pow(w0, i, p), p);
    u64 acc = 0;
    for (size_t k = coeffs.size(); k-- > 0;) acc = r_add(r_mul(acc, x, p), coeffs[k], p);
    cur[i] = acc;
  }
  // the restatement's prover
  std::vector<u64> seed = {rnd(), p - 1}, proof(sh.proof_words(), ~(u64)0), c(seed), betas(L);
  std::vector<std::vector<u64>> vals(L + 1), trees(L);
  u64 s = shift;
  for (u32 l = 0; l < L; l++) {
    const u64 m = (u64)1 << sh.log2m(l);
    vals[l] = cur;
    trees[l].resize(ref_tree_words(m, D));
    ref_merkle(S.P, cur.data(), m, A, 1, m, D, trees[l].data());
    std::vector<u64> in(c);
    for (u64 j = 0; j < D; j++) { in.push_back(trees[l][trees[l].size() - D + j]); proof[l * D + j] = in.back(); }
    ref_sponge(S.P, in.data(), 2 * D, 1, c.data(), D);
    betas[l] = c[0];
    cur = ref_fold(p, g, cur, betas[l], s, ETA);
    for (int e = 0; e < ETA; e++) s = r_mul(s, s, p);
  }
  const u64 NL = sh.size(L), final_off = L * D;
  for (u64 i = 0; i < NL; i++) proof[final_off + i] = cur[i];
  std::vector<u64> in(c), u(D), idx(L * Q);
  in.insert(in.end(), cur.begin(), cur.end());
  ref_sponge(S.P, in.data(), D + NL, 1, u.data(), D);
  for (u64 q = 0; q < Q; q++) {
    std::vector<u64> iq(u);
    iq.push_back(q);
    u64 word;
    ref_sponge(S.P, iq.data(), D + 1, 1, &word, 1);
    for (u32 l = 0; l < L; l++) {
      const u64 m = (u64)1 << sh.log2m(l), j = word & (((u64)1 << sh.log2m(0)) - 1) & (m - 1);
      idx[l * Q + q] = j;
      for (u64 t = 0; t < A; t++) proof[sh.leaf_off(l) + q * A + t] = vals[l][j + t * m] % p;
      const int bad = merkle_open_one(trees[l].data(), m, D, j, proof.data() + sh.path_off(l) + q * sh.log2m(l) * D);
      CHECK(!bad, "open");
    }
  }
  // the bodies: the transcript in one go and layer by layer, the indices
  std::vector<u64> chain((L + 1) * D, 7), chain2((L + 1) * D, 9), bt(L, 7), bt2(L, 9), u1(D, 7), u2(D, 9), ix(L * Q, 7);
  fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain.data(), proof.data(), 0, L, bt.data(), proof.data() + final_off, NL, u1.data());
  for (u32 l = 0; l < L; l++)
    fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain2.data(), proof.data(), l, l + 1, bt2.data(), nullptr, NL, u2.data());
  fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain2.data(), proof.data(), L, L, bt2.data(), proof.data() + final_off, NL, u2.data());
  CHECK(bt == betas && bt2 == betas, "betas");
  CHECK(u1 == u && u2 == u && chain == chain2, "u / chain");
  for (u64 q = 0; q < Q; q++) fri_query_indices<PF, W>(pf, S.sp, (u32)D, u1.data(), T.layers.data(), L, Q, q, ix.data());
  CHECK(ix == idx, "indices");
  // the verifier's bodies on the honest proof
  std::vector<u64> h(3 * D);
  for (u64 q = 0; q < Q; q++) {
    CHECK((fri_check_query<F, ETA>(f, T.layers.data(), L, Q, proof.data(), final_off, bt.data(), ix.data(), q) == 1), "honest query %llu",
          (unsigned long long)q);
    for (u32 l = 0; l < L; l++) {
      const u64* leaf = proof.data() + sh.leaf_off(l) + q * A;
      CHECK((merkle_verify_one<PF, W>(pf, S.sp, A, [&](u64 j) { return leaf[j]; }, ix[l * Q + q],
                                      proof.data() + sh.path_off(l) + q * sh.log2m(l) * D, (u64)1 << sh.log2m(l), (u32)D,
                                      proof.data() + l * D, h.data()) == 1), "honest path");
    }
  }
  for (u32 k = 0; k < NL; k++) {
    const bool zero = fri_final_coeff(f, T.wfin.data(), proof.data() + final_off, (u32)NL, k) == 0;
    CHECK(zero || k < (NL >> log2_blowup), "final coefficient %u of a low-degree layer", k);
  }
  // tampering: a leaf value (every layer), a final word, a word >= p in the place of its residue
  for (u32 l = 0; l < L; l++) {
    u64& wd = proof[sh.leaf_off(l) + 3 * A + (A - 1)];
    wd ^= 2;
    CHECK((fri_check_query<F, ETA>(f, T.layers.data(), L, Q, proof.data(), final_off, bt.data(), ix.data(), 3) == 0), "leaf layer %u", l);
    wd ^= 2;
  }
  {
    u64& wd = proof[final_off + ix[(L - 1) * Q + 1]];
    const u64 keep = wd;
    wd = keep ^ 1;
    CHECK((fri_check_query<F, ETA>(f, T.layers.data(), L, Q, proof.data(), final_off, bt.data(), ix.data(), 1) == 0), "final word");
    bool any = false;
    for (u32 k = (u32)(NL >> log2_blowup); k < NL; k++) any |= fri_final_coeff(f, T.wfin.data(), proof.data() + final_off, (u32)NL, k) != 0;
    CHECK(any, "final degree");
    if (keep < ~(u64)0 - p) {
      wd = keep + p;
      CHECK((fri_check_query<F, ETA>(f, T.layers.data(), L, Q, proof.data(), final_off, bt.data(), ix.data(), 1) == 0), "word >= p");
    }
    wd = keep;
  }
  // the final sum against the restatement on arbitrary words
  std::vector<u64> fw(NL);
  for (auto& v : fw) v = edge_word(p);
  const u64 wl_inv = r_pow(r_pow(g, (p - 1) / NL, p), p - 2, p);
  for (u32 k = 0; k < NL; k++) {
    u64 acc = 0;
    for (u64 i = 0; i < NL; i++) acc = r_add(acc, r_mul(fw[i] % p, r_pow(wl_inv, i * k, p), p), p);
    const u64 got = f.out(fri_final_coeff(f, T.wfin.data(), fw.data(), (u32)NL, k));
    CHECK(got == acc, "final sum k=%u", k);
  }
}

template <class F, class PF, int W>
static void run_all(bool mont, u64 p, u64 g, const Setup2& S) {
  run_fold<F, 1>(mont, p, g); run_fold<F, 2>(mont, p, g); run_fold<F, 3>(mont, p, g);
  run_proof<F, 1, PF, W>(mont, p, g, S); run_proof<F, 2, PF, W>(mont, p, g, S); run_proof<F, 3, PF, W>(mont, p, g, S);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_fri p g\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0);
  if (!(p & 1) || ((p - 1) & 511)) { fprintf(stderr, "p - 1 must be a multiple of 2^9\n"); return 2; }
  g_rng = p ^ g;
  Setup2 S;
  make_poseidon(S, p);
  int shift_policy = 0;
  if (p == gl64::P) {
    bool ok = true;
    for (u32 eta = 1; eta <= 3; eta++) ok = ok && fri_gl_shift_roots(p, g, eta);
    census_policy("gl.");
    if (ok) { run_all<FriGl, PosGl, 8>(false, p, g, S); shift_policy = 1; }
    census_policy("mont.");
    run_all<FriMont, PosGl, 8>(true, p, g, S);
  } else {
    run_all<FriMont, PosMont, 8>(true, p, g, S);
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu g=%llu shift_policy=%d\n", (unsigned long long)p, (unsigned long long)g, shift_policy);
  return 0;
}
