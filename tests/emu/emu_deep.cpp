// emu_deep.cpp -- the bodies that ronk_pcs_* runs, compiled for the host: the one-round case of csrc/mpcs_kernels.h (one matrix of C
// columns under mpcs_full_mask(K), the mapping of csrc/ronk_pcs.hip: the table of a call, the DEEP combination of a lane's points
// for the one-round combine kernel's four points, mpcs_one_round_lane, and the check kernel's one, mpcs_combine_lane<F, K, 1>) and the evaluation at extension points of csrc/deep_kernels.h,
// compared with a plain `unsigned __int128 % p` restatement in this file: the double sum of the definition and Horner's rule, over
// the arithmetic of emu_ref.h (which emu_fri.cpp brings in).  Test infrastructure only; never part of the product library.
//
//   emu_deep <p> <g> [w]   last line "OK ..." on success; w defaults to g.  Goldilocks runs the Goldilocks policy, its W = 7 form
//                          when w = 7, AND the Montgomery policy.
#define main emu_fri_main
#include "emu_fri.cpp"
#undef main

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/mpcs_kernels.h"

// ---------------------------------------------------------------------------------------------------- the restatement
// G at the point x from the column values there: sum_k sum_c alpha^(k C + c) (col[c] - y[k][c]) / (x - z_k), term by term
static R2 ref_point(u64 p, u64 w, const std::vector<u64>& col, u64 x, const std::vector<R2>& ys, const std::vector<R2>& zs, R2 alpha) {
  const size_t C = col.size(), K = zs.size();
  R2 g{0, 0}, ap{1 % p, 0};
  for (size_t k = 0; k < K; k++) {
    const R2 q = x_inv(x_sub(R2{x, 0}, red(zs[k], p), p), w, p);
    for (size_t c = 0; c < C; c++) {
      g = x_add(g, x_mul(ap, x_mul(x_sub(R2{col[c] % p, 0}, red(ys[k * C + c], p), p), q, w, p), w, p), p);
      ap = x_mul(ap, red(alpha, p), w, p);
    }
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------- table and combination
struct Domain {
  std::vector<u64> tab;
  DeepDomain dm;
};
static void make_domain(Domain& D, bool mont, u64 p, u64 g, u64 shift, u32 n) {
  const u32 kb = deep_kbits(n);
  D.tab.assign(((size_t)1 << kb) + ((size_t)1 << (n - kb)), ~(u64)0);
  deep_host_domain(mont, p, g, shift, n, D.tab.data(), D.tab.data() + ((size_t)1 << kb), &D.dm.iota, &D.dm.sinv);
  D.dm.lo = D.tab.data(); D.dm.hi = D.tab.data() + ((size_t)1 << kb); D.dm.kbits = kb; D.dm.log2n = n;
}

static u64 pair_word(u64 p, int c) { return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? p - 1 : c == 3 ? p + 1 + rnd() % 3 : challenge_word(p); }

template <class F, int K>
static void run_combine(bool mont, u64 p, u64 g, u64 w) {
  const FriConsts k = ext2_host_consts(mont, p);
  const F f(k);
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  const u32 ns[] = {2, 3, 6};
  const u32 Cs[] = {1, 2, 5};
  const u64 shifts[] = {1, g};
  for (u32 n : ns)
    for (u32 C : Cs)
      for (u64 shift : shifts) {
        const u64 N = (u64)1 << n, q = N >> 2, wn = r_pow(g, (p - 1) >> n, p);
        const u32 mask = mpcs_full_mask(K);
        MpcsShape sh;
        CHECK(mpcs_host_shape(K, 1, &C, &mask, &sh) && sh.Y == (u32)K * C, "shape K=%d C=%u refused", K, C);
        Domain D;
        make_domain(D, mont, p, g, shift, n);
        std::vector<u64> M(C * N);
        for (auto& v : M) v = edge_word(p);
        for (int variant = 0; variant < 6; variant++) {
          std::vector<R2> zs(K), ys((size_t)K * C);
          for (auto& z : zs) z = R2{rnd() % p, rnd() % p};
          for (auto& y : ys) y = R2{edge_word(p), edge_word(p)};
          bool want_on = false;
          if (variant == 1) zs[0] = R2{r_mul(shift, r_pow(wn, N - 1, p), p), 0}, want_on = true;   // the last domain point
          if (variant == 2) zs[K - 1] = R2{rnd() % p, 0};                                           // z1 = 0, off the domain
          if (variant == 3 && p < ~(u64)0 - p) zs[0] = R2{zs[0].c0 + p, zs[0].c1 + p};              // words >= p
          if (variant == 4) zs[K - 1] = R2{shift % p + (shift % p < ~(u64)0 - p ? p : 0), 0}, want_on = true;   // x_0, maybe as a word >= p
          const R2 alpha{pair_word(p, variant % 5), pair_word(p, (variant * 3 + 1) % 5)};
          // the table
          std::vector<u64> tab(mpcs_tab_words(1, K, C), ~(u64)0), zw(2 * K), yw(2 * (size_t)K * C), aw = {alpha.c0, alpha.c1};
          u64 *tab_y = tab.data() + (size_t)MPCS_KW * K, *tab_ap = tab_y + 2 * (size_t)K;
          for (u32 j = 0; j < (u32)K; j++) { zw[j] = zs[j].c0; zw[K + j] = zs[j].c1; }
          for (size_t j = 0; j < ys.size(); j++) { yw[j] = ys[j].c0; yw[ys.size() + j] = ys[j].c1; }
          const E2 a{f.in(aw[0]), f.in(aw[1])};
          int bits = 0;
          census_stage("deep_prep");
          for (u32 c = 0; c < C; c++) deep_prep_column(x, a, c, tab_ap);
          for (u32 j = 0; j < (u32)K; j++) bits |= mpcs_prep_point(x, D.dm, a, zw.data(), sh, j, tab.data() + (size_t)MPCS_KW * j);
          for (u32 j = 0; j < (u32)K; j++) mpcs_prep_claims(x, a, yw.data(), sh, 0, j, tab_y + 2 * (size_t)j);
          CHECK(bits == (want_on ? 32 : 0), "status K=%d n=%u C=%u variant=%d bits=%d", K, n, C, variant, bits);
          const MpcsTab T{tab.data(), tab_y, tab_ap};
          census_stage(nullptr);
          // the restatement
          std::vector<R2> want(N);
          for (u64 i = 0; i < N; i++) {
            std::vector<u64> col(C);
            for (u32 c = 0; c < C; c++) col[c] = M[c * N + i];
            want[i] = ref_point(p, w, col, r_mul(shift, r_pow(wn, i, p), p), ys, zs, alpha);
          }
          // the combine kernel's lanes: four points at stride N / 4
          census_stage("deep_combine");
          for (u64 i = 0; i < q; i++) {
            E2 out[4];
            mpcs_one_round_lane<F, K>(x, D.dm, T, sh.C[0], i, [&](u32 c, int t) { return M[c * N + i + (u64)t * q]; }, out);
            for (int t = 0; t < 4; t++)
              CHECK((R2{out[t].c0, out[t].c1} == want[i + t * q]), "combine K=%d n=%u C=%u shift=%llu variant=%d i=%llu t=%d", K, n, C,
                    (unsigned long long)shift, variant, (unsigned long long)i, t);
          }
          // the check kernel's lanes: one point, from a gathered leaf
          census_stage("deep_check");
          for (u64 i = 0; i < N; i += (n == 6 ? 5 : 1)) {
            E2 out[1];
            mpcs_combine_lane<F, K, 1>(x, D.dm, T, sh, i, [&](u32, u32 c, int) { return M[c * N + i]; }, out);
            CHECK((R2{out[0].c0, out[0].c1} == want[i]), "check K=%d n=%u C=%u variant=%d i=%llu", K, n, C, variant, (unsigned long long)i);
          }
        }
      }
}

// ---------------------------------------------------------------------------------------------------- evaluation
template <class F>
static void run_eval(bool mont, u64 p, u64 w) {
  const FriConsts k = ext2_host_consts(mont, p);
  const F f(k);
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  const u64 ds[] = {1, 2, 255, 256, 257, 700};
  const u32 Ks[] = {1, 3, 8};
  census_stage("deep_eval");
  for (u64 d : ds)
    for (u32 K : Ks) {
      std::vector<u64> coef(d);
      for (auto& c : coef) c = edge_word(p);
      std::vector<R2> zs(K);
      for (u32 j = 0; j < K; j++) zs[j] = R2{pair_word(p, (int)((j + d) % 5)), pair_word(p, (int)((2 * j + d + 1) % 5))};
      E2 zr[DEEP_MAX_K];
      for (u32 j = 0; j < DEEP_MAX_K; j++) zr[j] = j < K ? E2{f.in(zs[j].c0), f.in(zs[j].c1)} : x.zero();
      std::vector<E2> sum(K, x.zero());
      for (u32 lane = 0; lane < DEEP_EVAL_LANES; lane++) {
        E2 share[DEEP_MAX_K];
        deep_eval_lane(x, d, lane, DEEP_EVAL_LANES, zr, K, [&](u64 j) { return coef[j]; }, share);
        for (u32 j = 0; j < K; j++) sum[j] = x.add(sum[j], share[j]);
      }
      for (u32 j = 0; j < K; j++) {
        R2 acc{0, 0};
        for (u64 i = d; i-- > 0;) acc = x_add(x_mul(acc, red(zs[j], p), w, p), R2{coef[i] % p, 0}, p);
        CHECK((R2{f.out(sum[j].c0), f.out(sum[j].c1)} == acc), "eval d=%llu K=%u k=%u", (unsigned long long)d, K, j);
      }
    }
}

template <class F>
static void run_all_deep(bool mont, u64 p, u64 g, u64 w) {
  run_combine<F, 1>(mont, p, g, w); run_combine<F, 2>(mont, p, g, w); run_combine<F, 3>(mont, p, g, w); run_combine<F, 8>(mont, p, g, w);
  run_eval<F>(mont, p, w);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_deep p g [w]\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0), w = argc > 3 ? strtoull(argv[3], nullptr, 0) : g;
  if (!(p & 1) || ((p - 1) & 63)) { fprintf(stderr, "p - 1 must be a multiple of 2^6\n"); return 2; }
  if (!ext2_non_residue(p, w)) { fprintf(stderr, "w must be a quadratic non-residue\n"); return 2; }
  g_rng = p ^ g ^ w ^ 3;
  int policies = 0;
  if (p == gl64::P) {
    census_policy("gl.");
    run_all_deep<FriGl>(false, p, g, w); policies |= 1;
    census_policy("w7.");
    if (w % p == 7) { run_all_deep<FriGlW7>(false, p, g, w); policies |= 2; }
  }
  census_policy("mont.");
  run_all_deep<FriMont>(true, p, g, w); policies |= 4;
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu g=%llu w=%llu policies=%d\n", (unsigned long long)p, (unsigned long long)g, (unsigned long long)w, policies);
  return 0;
}
