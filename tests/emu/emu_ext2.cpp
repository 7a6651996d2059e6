// emu_ext2.cpp -- the quadratic extension of csrc/ext2.h and the extension FRI bodies of csrc/fri_kernels.h (fold, transcript,
// query check, final-degree sums) compiled for the host and compared with a plain `unsigned __int128 % p` restatement in this
// file.  The tables and Poseidon setup are those of emu_fri.cpp, the arithmetic of the restatement that of emu_ref.h.  W is the
// field's generator g.  Test infrastructure only; never part of the product library.
//
//   emu_ext2 <p> <g>     last line "OK ..." on success.  Goldilocks with g = 7 runs the shift policy, its W = 7 form (shift_policy=2)
//                        AND the Montgomery policy.
//
// RONK_EMU_INPUT=<file> (Goldilocks only) is the file mode of the folds: little-endian words, case after case, each
//   form (0 base, 1 base layer with an extension challenge, 2 planar pairs), eta, n, shift, beta0, beta1, then layer 0: 2^n words
//   (2^(n+1) for form 2).  Every case goes through the fold bodies of the Goldilocks policy (and of its W = 7 form) and is compared
//   with the restatement; nothing else runs.  tests/gl_directed.py fold_case writes such inputs.
#define main emu_fri_main
#include "emu_fri.cpp"
#undef main

// ---------------------------------------------------------------------------------------------------- the restatement
static R2 x_pow(R2 a, u64 e, u64 w, u64 p) {   // multiply e's bits from the top: another order than the body's
  R2 r{1 % p, 0};
  for (int b = 63; b >= 0; b--) {
    r = x_mul(r, r, w, p);
    if ((e >> b) & 1) r = x_mul(r, a, w, p);
  }
  return r;
}
static std::vector<R2> x_fold2(u64 p, u64 w, const std::vector<R2>& f, R2 beta, u64 s, u64 wn) {
  const size_t h = f.size() / 2;
  const u64 inv2 = r_pow(2, p - 2, p);
  std::vector<R2> out(h);
  for (size_t i = 0; i < h; i++) {
    const R2 a = red(f[i], p), b = red(f[i + h], p);
    const u64 x2inv = r_pow(r_mul(2, r_mul(s, r_pow(wn, i, p), p), p), p - 2, p);
    out[i] = x_add(x_scale(x_add(a, b, p), inv2, p), x_mul(red(beta, p), x_scale(x_sub(a, b, p), x2inv, p), w, p), p);
  }
  return out;
}
static std::vector<R2> x_fold(u64 p, u64 g, u64 w, std::vector<R2> f, R2 beta, u64 s, u32 eta) {
  u64 wn = r_pow(g, (p - 1) / f.size(), p);
  R2 b = red(beta, p);
  for (u32 e = 0; e < eta; e++) {
    f = x_fold2(p, w, f, b, s, wn);
    s = r_mul(s, s, p); wn = r_mul(wn, wn, p); b = x_mul(b, b, w, p);
  }
  return f;
}

// ---------------------------------------------------------------------------------------------------- the element type
template <class F>
static void run_arith(bool mont, u64 p, u64 g) {
  const FriConsts k = fri_host_consts(mont, p, g, 1);
  const F f(k);
  const u64 w = g % p;
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  CHECK(ext2_non_residue(p, w), "the generator is a non-residue");
  CHECK(!ext2_non_residue(p, r_mul(w, w, p)) && !ext2_non_residue(p, 0) && !ext2_non_residue(p, p), "residues and zero are refused");
  auto in = [&](R2 a) { return E2{f.in(a.c0), f.in(a.c1)}; };
  auto out = [&](E2 a) { return R2{f.out(a.c0), f.out(a.c1)}; };
  const u64 exps[] = {0, 1, 2, p, ~(u64)0, rnd()};
  for (int it = 0; it < 400; it++) {
    R2 a{edge_word(p), edge_word(p)}, b{edge_word(p), edge_word(p)};
    if (it == 0) a = R2{0, 0};
    if (it == 1) a = R2{p - 1, p - 1};
    if (it == 2) a = R2{p, p + 1};   // zero and one as words >= p
    if (emu_small() && it % 4 == 3) a.c0 = r_mul((u64)1 << 48, a.c0, p);   // (2^48)^2 = -1: a0^2 + W a1^2 is a small DIFFERENCE
    const u64 s = edge_word(p);
    const R2 ar = red(a, p), br = red(b, p);
    census_stage("ext2_add");
    CHECK(out(x.add(in(a), in(b))) == x_add(ar, br, p), "add %d", it);
    census_stage("ext2_sub");
    CHECK(out(x.sub(in(a), in(b))) == x_sub(ar, br, p), "sub %d", it);
    census_stage("ext2_neg");
    CHECK(out(x.neg(in(a))) == x_sub(R2{0, 0}, ar, p), "neg %d", it);
    census_stage("ext2_mul");
    CHECK(out(x.mul(in(a), in(b))) == x_mul(ar, br, w, p), "mul %d", it);
    census_stage("ext2_sqr");
    CHECK(out(x.sqr(in(a))) == x_mul(ar, ar, w, p), "sqr %d", it);
    census_stage("ext2_mul_base");
    CHECK(out(x.mul_base(in(a), f.in(s))) == x_scale(ar, s % p, p), "mul_base %d", it);
    census_stage("ext2_norm");
    CHECK(f.out(x.norm(in(a))) == x_mul(ar, R2{ar.c0, r_sub(0, ar.c1, p)}, w, p).c0, "norm %d", it);
    census_stage("ext2_inv");
    const R2 ai = out(x.inv(in(a)));
    CHECK(ai == x_inv(ar, w, p), "inv %d", it);
    if (ar.c0 | ar.c1) CHECK((x_mul(ai, ar, w, p) == R2{1, 0}), "a * a^-1 %d", it);
    else CHECK((ai == R2{0, 0}), "the inverse of zero is written as zero");
    census_stage("ext2_pow");
    if (it < 40)
      for (u64 e : exps) CHECK(out(x.pow(in(a), e)) == x_pow(ar, e, w, p), "pow %d e=%llu", it, (unsigned long long)e);
  }
  census_stage(nullptr);
  // Frobenius: a^p = (a0, -a1)
  const R2 a{rnd() % p, rnd() % p};
  CHECK((out(x.pow(in(a), p)) == R2{a.c0, r_sub(0, a.c1, p)}), "frobenius");
  CHECK((out(x.one()) == R2{1, 0}), "one");
}

// ---------------------------------------------------------------------------------------------------- fold
static u64 beta_word(u64 p, int c) { return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? p - 1 : c == 3 ? p + 1 + rnd() % 3 : rnd() % p; }

template <class F, int ETA, bool EXT_IN>
static void run_fold_ext(bool mont, u64 p, u64 g) {
  const u64 w = g % p;
  const u32 ns[] = {ETA, ETA + 1, 5 + ETA, 9};
  const u64 shifts[] = {1, g, p - 1};
  static const char* const stage[2][4] = {{"", "fold_mix_eta1", "fold_mix_eta2", "fold_mix_eta3"}, {"", "fold_ext_eta1", "fold_ext_eta2", "fold_ext_eta3"}};
  census_stage(stage[EXT_IN][ETA]);
  for (u32 n : ns)
    for (u64 shift : shifts) {
      Tables T;
      make_tables(T, mont, p, g, shift, n, ETA, n % ETA, 1, 2);
      const F f(T.k);
      const Ext2<F> x(f, ext2_reg_form(mont, p, w));
      u64 s = shift;
      for (u32 l = 0; l < T.sh.layers; l++) {
        const u64 N = T.sh.size(l), m = N >> ETA;
        std::vector<u64> in((EXT_IN ? 2 : 1) * N);
        for (auto& v : in) v = edge_word(p);
        std::vector<R2> fin(N);
        for (u64 i = 0; i < N; i++) fin[i] = R2{in[i], EXT_IN ? in[N + i] : 0};
        for (int bc = 0; bc < 25; bc++) {
          if (n == 9 && bc % 6) continue;
          const R2 beta{beta_word(p, bc / 5), beta_word(p, bc % 5)};
          const std::vector<R2> want = x_fold(p, g, w, fin, beta, s, ETA);
          const E2 b{f.in(beta.c0), f.in(beta.c1)};
          for (u64 i = 0; i < m; i++) {
            const E2 got = fri_fold_leaf_ext<F, ETA, EXT_IN>(x, fri_gamma_ext(x, T.layers[l], i, b), [&](int t) { return in[i + (u64)t * m]; });
            CHECK(got.c0 == want[i].c0 && got.c1 == want[i].c1, "fold ext_in=%d eta=%d n=%u layer=%u i=%llu beta=%d", (int)EXT_IN, ETA, n, l,
                  (unsigned long long)i, bc);
          }
        }
        for (int e = 0; e < ETA; e++) s = r_mul(s, s, p);
      }
    }
}

// one case of the file mode
template <class F, int ETA>
static void run_fold_file(u64 p, u64 g, u32 form, u32 n, u64 shift, R2 beta, const std::vector<u64>& in) {
  static const char* const stage[3][4] = {{"", "fold_base_eta1", "fold_base_eta2", "fold_base_eta3"},
                                          {"", "fold_mix_eta1", "fold_mix_eta2", "fold_mix_eta3"},
                                          {"", "fold_ext_eta1", "fold_ext_eta2", "fold_ext_eta3"}};
  const u64 w = g % p;
  Tables T;
  make_tables(T, false, p, g, shift, n, ETA, n % ETA, 1, form ? 2 : 1);
  const F f(T.k);
  const u64 N = T.sh.size(0), m = N >> ETA;
  if (form == 0) {
    const std::vector<u64> want = ref_fold(p, g, in, beta.c0, shift % p, ETA);
    census_stage(stage[0][ETA]);
    for (u64 i = 0; i < m; i++) {
      const u64 got = fri_fold_leaf<F, ETA>(f, fri_gamma(f, T.layers[0], i, f.in(beta.c0)), [&](int t) { return in[i + (u64)t * m]; });
      CHECK(got == want[i], "file fold eta=%d n=%u i=%llu", ETA, n, (unsigned long long)i);
    }
  } else {
    const Ext2<F> x(f, ext2_reg_form(false, p, w));
    std::vector<R2> fin(N);
    for (u64 i = 0; i < N; i++) fin[i] = R2{in[i], form == 2 ? in[N + i] : 0};
    const std::vector<R2> want = x_fold(p, g, w, fin, beta, shift % p, ETA);
    const E2 b{f.in(beta.c0), f.in(beta.c1)};
    census_stage(stage[form][ETA]);
    for (u64 i = 0; i < m; i++) {
      const E2 gm = fri_gamma_ext(x, T.layers[0], i, b);
      const E2 got = form == 2 ? fri_fold_leaf_ext<F, ETA, true>(x, gm, [&](int t) { return in[i + (u64)t * m]; })
                               : fri_fold_leaf_ext<F, ETA, false>(x, gm, [&](int t) { return in[i + (u64)t * m]; });
      CHECK(got.c0 == want[i].c0 && got.c1 == want[i].c1, "file fold form=%u eta=%d n=%u i=%llu", form, ETA, n, (unsigned long long)i);
    }
  }
  census_stage(nullptr);
}
template <class F>
static bool run_fold_cases(u64 p, u64 g, const std::vector<u64>& file, bool with_base, int* cases) {   // (the base form has no product with W)
  size_t at = 0;
  while (at < file.size()) {
    if (file.size() - at < 6) return false;
    const u64 form = file[at], eta = file[at + 1], n = file[at + 2], shift = file[at + 3];
    const R2 beta{file[at + 4], file[at + 5]};
    at += 6;
    if (form > 2 || eta < 1 || eta > 3 || n < eta || n > 9 || shift % p == 0) return false;
    const size_t len = (size_t)(form == 2 ? 2 : 1) << n;
    if (file.size() - at < len) return false;
    const std::vector<u64> in(file.begin() + at, file.begin() + at + len);
    at += len;
    if (form == 0 && !with_base) continue;
    if (eta == 1) run_fold_file<F, 1>(p, g, (u32)form, (u32)n, shift, beta, in);
    if (eta == 2) run_fold_file<F, 2>(p, g, (u32)form, (u32)n, shift, beta, in);
    if (eta == 3) run_fold_file<F, 3>(p, g, (u32)form, (u32)n, shift, beta, in);
    ++*cases;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------- transcript and verifier
template <class F, int ETA, class PF, int W>
static void run_proof_ext(bool mont, u64 p, u64 g, const Setup2& S, u32 in_ext) {
  const u32 n = 2 * ETA + 2, log2_final = 2, log2_blowup = 1;
  const u64 Q = 6, D = 2, A = (u64)1 << ETA, shift = g, w = g % p;
  census_stage(nullptr);   // a composition of the bodies counted on their own
  Tables T;
  make_tables(T, mont, p, g, shift, n, ETA, log2_final, Q, D);
  T.sh.ext = 1; T.sh.in_ext = in_ext;
  const FriShape& sh = T.sh;
  const u32 L = sh.layers;
  for (u32 l = 0; l < L; l++) { T.layers[l].leaf_off = sh.leaf_off(l); T.layers[l].path_off = sh.path_off(l); }
  const F f(T.k);
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  const PF pf(S.sp);
  // a codeword of degree < N_0 / 2 by direct evaluation: base coefficients, or extension coefficients plane by plane
  const u64 N0 = sh.size(0), w0 = r_pow(g, (p - 1) / N0, p);
  std::vector<R2> coeffs(N0 >> log2_blowup), cur(N0);
  for (auto& c : coeffs) c = R2{rnd() % p, in_ext ? rnd() % p : 0};
  for (u64 i = 0; i < N0; i++) {
    const u64 xi = r_mul(shift, r_pow(w0, i, p), p);
    R2 acc{0, 0};
    for (size_t k = coeffs.size(); k-- > 0;) acc = x_add(x_scale(acc, xi, p), coeffs[k], p);
    cur[i] = acc;
  }
  // the restatement's prover
  auto planar = [&](const std::vector<R2>& v, u64 vw) {
    std::vector<u64> o(vw * v.size());
    for (size_t i = 0; i < v.size(); i++) { o[i] = v[i].c0; if (vw == 2) o[v.size() + i] = v[i].c1; }
    return o;
  };
  std::vector<u64> seed = {rnd(), p - 1}, proof(sh.proof_words(), ~(u64)0), c(seed);
  std::vector<R2> betas(L);
  std::vector<std::vector<u64>> vals(L + 1), trees(L);
  u64 s = shift;
  for (u32 l = 0; l < L; l++) {
    const u64 m = (u64)1 << sh.log2m(l);
    vals[l] = planar(cur, sh.vw(l));
    trees[l].resize(ref_tree_words(m, D));
    ref_merkle(S.P, vals[l].data(), m, sh.leaf_len(l), 1, m, D, trees[l].data());
    std::vector<u64> in(c);
    for (u64 j = 0; j < D; j++) { in.push_back(trees[l][trees[l].size() - D + j]); proof[l * D + j] = in.back(); }
    ref_sponge(S.P, in.data(), 2 * D, 1, c.data(), D);
    betas[l] = R2{c[0], c[1]};
    cur = x_fold(p, g, w, cur, betas[l], s, ETA);
    for (int e = 0; e < ETA; e++) s = r_mul(s, s, p);
  }
  const u64 NL = sh.size(L), final_off = L * D;
  vals[L] = planar(cur, 2);
  for (u64 i = 0; i < 2 * NL; i++) proof[final_off + i] = vals[L][i];
  std::vector<u64> in(c), u(D), idx(L * Q);
  in.insert(in.end(), vals[L].begin(), vals[L].end());
  ref_sponge(S.P, in.data(), D + 2 * NL, 1, u.data(), D);
  for (u64 q = 0; q < Q; q++) {
    std::vector<u64> iq(u);
    iq.push_back(q);
    u64 word;
    ref_sponge(S.P, iq.data(), D + 1, 1, &word, 1);
    for (u32 l = 0; l < L; l++) {
      const u64 m = (u64)1 << sh.log2m(l), j = word & (((u64)1 << sh.log2m(0)) - 1) & (m - 1), ll = sh.leaf_len(l);
      idx[l * Q + q] = j;
      for (u64 t = 0; t < ll; t++) proof[sh.leaf_off(l) + q * ll + t] = vals[l][j + t * m] % p;
      const int bad = merkle_open_one(trees[l].data(), m, D, j, proof.data() + sh.path_off(l) + q * sh.log2m(l) * D);
      CHECK(!bad, "open");
    }
  }
  CHECK(sh.path_off(L - 1) + Q * sh.log2m(L - 1) * D == sh.proof_words(), "proof size");
  // the bodies: the transcript in one go and layer by layer, the indices
  std::vector<u64> chain((L + 1) * D, 7), chain2((L + 1) * D, 9), bt(2 * L, 7), bt2(2 * L, 9), u1(D, 7), u2(D, 9), ix(L * Q, 7), bw(2 * L);
  for (u32 l = 0; l < L; l++) { bw[2 * l] = betas[l].c0; bw[2 * l + 1] = betas[l].c1; }
  fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain.data(), proof.data(), 0, L, bt.data(), proof.data() + final_off, 2 * NL, u1.data(), 2);
  for (u32 l = 0; l < L; l++)
    fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain2.data(), proof.data(), l, l + 1, bt2.data(), nullptr, 2 * NL, u2.data(), 2);
  fri_transcript<PF, W>(pf, S.sp, (u32)D, seed.data(), chain2.data(), proof.data(), L, L, bt2.data(), proof.data() + final_off, 2 * NL, u2.data(), 2);
  CHECK(bt == bw && bt2 == bw, "betas");
  CHECK(u1 == u && u2 == u && chain == chain2, "u / chain");
  for (u64 q = 0; q < Q; q++) fri_query_indices<PF, W>(pf, S.sp, (u32)D, u1.data(), T.layers.data(), L, Q, q, ix.data());
  CHECK(ix == idx, "indices");
  // the verifier's bodies on the honest proof
  auto check = [&](u64 q) { return fri_check_query_ext<F, ETA>(x, T.layers.data(), L, Q, proof.data(), final_off, NL, in_ext != 0, bt.data(), ix.data(), q); };
  std::vector<u64> h(3 * D);
  for (u64 q = 0; q < Q; q++) {
    CHECK(check(q) == 1, "honest query %llu", (unsigned long long)q);
    for (u32 l = 0; l < L; l++) {
      const u64 ll = sh.leaf_len(l);
      const u64* leaf = proof.data() + sh.leaf_off(l) + q * ll;
      CHECK((merkle_verify_one<PF, W>(pf, S.sp, ll, [&](u64 j) { return leaf[j]; }, ix[l * Q + q],
                                      proof.data() + sh.path_off(l) + q * sh.log2m(l) * D, (u64)1 << sh.log2m(l), (u32)D,
                                      proof.data() + l * D, h.data()) == 1), "honest path");
    }
  }
  for (u32 pl = 0; pl < 2; pl++)
    for (u32 k = 0; k < NL; k++) {
      const bool zero = fri_final_coeff(f, T.wfin.data(), proof.data() + final_off + pl * NL, (u32)NL, k) == 0;
      CHECK(zero || k < (NL >> log2_blowup), "final coefficient %u of plane %u of a low-degree layer", k, pl);
    }
  // tampering: a leaf word of every layer in the c0 half and in the c1 half, a final word of either plane, a word >= p
  for (u32 l = 0; l < L; l++) {
    const u64 ll = sh.leaf_len(l);
    for (u64 at : {A - 1, ll - 1}) {
      u64& wd = proof[sh.leaf_off(l) + 3 * ll + at];
      wd ^= 2;
      CHECK(check(3) == 0, "leaf layer %u word %llu", l, (unsigned long long)at);
      wd ^= 2;
    }
  }
  for (u32 pl = 0; pl < 2; pl++) {
    u64& wd = proof[final_off + pl * NL + ix[(L - 1) * Q + 1]];
    const u64 keep = wd;
    wd = keep ^ 1;
    CHECK(check(1) == 0, "final word plane %u", pl);
    bool any = false;
    for (u32 k = (u32)(NL >> log2_blowup); k < NL; k++) any |= fri_final_coeff(f, T.wfin.data(), proof.data() + final_off + pl * NL, (u32)NL, k) != 0;
    CHECK(any, "final degree plane %u", pl);
    if (keep < ~(u64)0 - p) {
      wd = keep + p;
      CHECK(check(1) == 0, "word >= p plane %u", pl);
    }
    wd = keep;
  }
  CHECK(check(1) == 1 && check(3) == 1, "restored");
}

template <class F, class PF, int W>
static void run_all_ext(bool mont, u64 p, u64 g, const Setup2& S) {
  run_arith<F>(mont, p, g);
  run_fold_ext<F, 1, false>(mont, p, g); run_fold_ext<F, 2, false>(mont, p, g); run_fold_ext<F, 3, false>(mont, p, g);
  run_fold_ext<F, 1, true>(mont, p, g); run_fold_ext<F, 2, true>(mont, p, g); run_fold_ext<F, 3, true>(mont, p, g);
  for (u32 in_ext = 0; in_ext < 2; in_ext++) {
    run_proof_ext<F, 1, PF, W>(mont, p, g, S, in_ext); run_proof_ext<F, 2, PF, W>(mont, p, g, S, in_ext);
    run_proof_ext<F, 3, PF, W>(mont, p, g, S, in_ext);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_ext2 p g\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0);
  if (!(p & 1) || ((p - 1) & 511)) { fprintf(stderr, "p - 1 must be a multiple of 2^9\n"); return 2; }
  g_rng = p ^ g ^ 2;
  if (const char* path = getenv("RONK_EMU_INPUT")) {
    bool ok = p == gl64::P;
    for (u32 eta = 1; eta <= 3; eta++) ok = ok && fri_gl_shift_roots(p, g, eta);
    std::vector<u64> file;
    FILE* fp = ok ? fopen(path, "rb") : nullptr;
    u64 word;
    while (fp && fread(&word, 8, 1, fp) == 1) file.push_back(word);
    if (fp) fclose(fp);
    int cases = 0;
    census_policy("gl.");
    ok = fp && run_fold_cases<FriGl>(p, g, file, true, &cases);
    census_policy("w7.");
    if (ok && g % p == 7) ok = run_fold_cases<FriGlW7>(p, g, file, false, &cases);
    if (!ok) { fprintf(stderr, "the file mode needs Goldilocks, a generator with shift roots and a well-formed %s\n", path); return 2; }
    if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
    printf("OK p=%llu g=%llu fold cases from the file: %d\n", (unsigned long long)p, (unsigned long long)g, cases);
    return 0;
  }
  Setup2 S;
  make_poseidon(S, p);
  int shift_policy = 0;
  if (p == gl64::P) {
    bool ok = true;
    for (u32 eta = 1; eta <= 3; eta++) ok = ok && fri_gl_shift_roots(p, g, eta);
    census_policy("gl.");
    if (ok) { run_all_ext<FriGl, PosGl, 8>(false, p, g, S); shift_policy = 1; }
    census_policy("w7.");
    if (ok && g % p == 7) { run_all_ext<FriGlW7, PosGl, 8>(false, p, g, S); shift_policy = 2; }   // W = g = 7: the shift form of the product with W
    census_policy("mont.");
    run_all_ext<FriMont, PosGl, 8>(true, p, g, S);
  } else {
    run_all_ext<FriMont, PosMont, 8>(true, p, g, S);
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu g=%llu w=%llu shift_policy=%d\n", (unsigned long long)p, (unsigned long long)g, (unsigned long long)(g % p), shift_policy);
  return 0;
}
