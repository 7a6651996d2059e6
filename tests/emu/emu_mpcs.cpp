// emu_mpcs.cpp -- the bodies of csrc/mpcs_kernels.h (the table of a call, the combination of R matrices at per-matrix points for
// the combine kernel's four points per lane and the check kernel's one) compiled for the host and compared with a plain
// `unsigned __int128 % p` restatement in this file: the triple sum of the definition, every (r, k, c) term with its own power of
// alpha, over the arithmetic of emu_ref.h (which emu_fri.cpp brings in).  Test infrastructure only; never part of the product
// library.
//
//   emu_mpcs <p> <g> [w]   last line "OK ..." on success; w defaults to g.  Goldilocks runs the Goldilocks policy, its W = 7 form
//                          when w = 7, AND the Montgomery policy.
#define main emu_fri_main
#include "emu_fri.cpp"
#undef main

#include "../../ronkathon_amd/csrc/ext2_kernels.h"
#include "../../ronkathon_amd/csrc/mpcs_kernels.h"

// ---------------------------------------------------------------------------------------------------- the restatement
struct Shape {
  u32 K;
  std::vector<u32> C, mask;
};
static R2 x_pow(R2 a, u64 e, u64 w, u64 p) {
  R2 r{1 % p, 0};
  for (; e; e >>= 1) {
    if (e & 1) r = x_mul(r, a, w, p);
    a = x_mul(a, a, w, p);
  }
  return r;
}
// G at the point x from the column values there; ys in proof order: by round, by the set bits of the mask ascending, by column
static R2 ref_point(u64 p, u64 w, const Shape& s, const std::vector<std::vector<u64>>& col, u64 x, const std::vector<R2>& ys,
                    const std::vector<R2>& zs, R2 alpha) {
  u64 ctot = 0;
  for (u32 c : s.C) ctot += c;
  R2 g{0, 0};
  size_t at = 0, off = 0;
  for (size_t r = 0; r < s.C.size(); r++) {
    for (u32 k = 0; k < s.K; k++) {
      if (!((s.mask[r] >> k) & 1)) continue;
      const R2 q = x_inv(x_sub(R2{x, 0}, red(zs[k], p), p), w, p);
      for (u32 c = 0; c < s.C[r]; c++) {
        const R2 a = x_pow(red(alpha, p), (u64)k * ctot + off + c, w, p);
        g = x_add(g, x_mul(a, x_mul(x_sub(R2{col[r][c] % p, 0}, red(ys[at + c], p), p), q, w, p), w, p), p);
      }
      at += s.C[r];
    }
    off += s.C[r];
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
static void run_shape(bool mont, u64 p, u64 g, u64 w, const Shape& s) {
  const FriConsts k = ext2_host_consts(mont, p);
  const F f(k);
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  MpcsShape sh;
  CHECK(mpcs_host_shape(s.K, (u32)s.C.size(), s.C.data(), s.mask.data(), &sh), "shape K=%d R=%zu refused", K, s.C.size());
  const u32 R = sh.R;
  const u32 ns[] = {2, 3, 6};
  const u64 shifts[] = {1, g};
  for (u32 n : ns)
    for (u64 shift : shifts) {
      const u64 N = (u64)1 << n, q = N >> 2, wn = r_pow(g, (p - 1) >> n, p);
      Domain D;
      make_domain(D, mont, p, g, shift, n);
      std::vector<std::vector<u64>> M(R);
      for (u32 r = 0; r < R; r++) {
        M[r].resize(sh.C[r] * N);
        for (auto& v : M[r]) v = edge_word(p);
      }
      for (int variant = 0; variant < 6; variant++) {
        std::vector<R2> zs(K), ys(sh.Y);
        for (auto& z : zs) z = R2{rnd() % p, rnd() % p};
        for (auto& y : ys) y = R2{edge_word(p), edge_word(p)};
        bool want_on = false;
        if (variant == 1) zs[0] = R2{r_mul(shift, r_pow(wn, N - 1, p), p), 0}, want_on = true;   // the last domain point
        if (variant == 2) zs[K - 1] = R2{rnd() % p, 0};                                           // z1 = 0, off the domain
        if (variant == 3 && p < ~(u64)0 - p) zs[0] = R2{zs[0].c0 + p, zs[0].c1 + p};              // words >= p
        if (variant == 4) zs[K - 1] = R2{shift % p + (shift % p < ~(u64)0 - p ? p : 0), 0}, want_on = true;   // x_0, maybe as a word >= p
        const R2 alpha{pair_word(p, variant % 5), pair_word(p, (variant * 3 + 1) % 5)};
        // the table, as the prep kernel's lanes write it
        std::vector<u64> tab(mpcs_tab_words(R, K, sh.Ctot), ~(u64)0), zw(2 * K), yw(2 * (size_t)sh.Y), aw = {alpha.c0, alpha.c1};
        for (u32 j = 0; j < (u32)K; j++) { zw[j] = zs[j].c0; zw[K + j] = zs[j].c1; }
        for (size_t j = 0; j < ys.size(); j++) { yw[j] = ys[j].c0; yw[ys.size() + j] = ys[j].c1; }
        u64* tab_y = tab.data() + (size_t)MPCS_KW * K;
        u64* tab_ap = tab_y + 2 * (size_t)R * K;
        const E2 a{f.in(aw[0]), f.in(aw[1])};
        int bits = 0;
        census_stage("mpcs_prep");
        for (u32 c = 0; c < sh.Ctot; c++) deep_prep_column(x, a, c, tab_ap);
        for (u32 j = 0; j < (u32)K; j++) bits |= mpcs_prep_point(x, D.dm, a, zw.data(), sh, j, tab.data() + (size_t)MPCS_KW * j);
        for (u32 j = 0; j < R * (u32)K; j++) mpcs_prep_claims(x, a, yw.data(), sh, j / K, j % K, tab_y + 2 * (size_t)j);
        census_stage(nullptr);
        CHECK(bits == (want_on ? 32 : 0), "status K=%d R=%u n=%u variant=%d bits=%d", K, R, n, variant, bits);
        for (u64 v : tab) CHECK(v != ~(u64)0 || p == ~(u64)0, "a table word is left unwritten K=%d R=%u", K, R);
        const MpcsTab T{tab.data(), tab_y, tab_ap};
        // the restatement
        std::vector<R2> want(N);
        for (u64 i = 0; i < N; i++) {
          std::vector<std::vector<u64>> col(R);
          for (u32 r = 0; r < R; r++)
            for (u32 c = 0; c < sh.C[r]; c++) col[r].push_back(M[r][c * N + i]);
          want[i] = ref_point(p, w, s, col, r_mul(shift, r_pow(wn, i, p), p), ys, zs, alpha);
        }
        // the combine kernel's lanes: four points at stride N / 4
        census_stage("mpcs_combine");
        for (u64 i = 0; i < q; i++) {
          E2 out[4];
          mpcs_combine_lane<F, K, 4>(x, D.dm, T, sh, i, [&](u32 r, u32 c, int t) { return M[r][c * N + i + (u64)t * q]; }, out);
          for (int t = 0; t < 4; t++)
            CHECK((R2{out[t].c0, out[t].c1} == want[i + t * q]), "combine K=%d R=%u n=%u shift=%llu variant=%d i=%llu t=%d", K, R, n,
                  (unsigned long long)shift, variant, (unsigned long long)i, t);
        }
        // the check kernel's lanes: one point, from the gathered leaves
        census_stage("mpcs_check");
        for (u64 i = 0; i < N; i += (n == 6 ? 5 : 1)) {
          E2 out[1];
          mpcs_combine_lane<F, K, 1>(x, D.dm, T, sh, i, [&](u32 r, u32 c, int) { return M[r][c * N + i]; }, out);
          CHECK((R2{out[0].c0, out[0].c1} == want[i]), "check K=%d R=%u n=%u variant=%d i=%llu", K, R, n, variant, (unsigned long long)i);
        }
      }
    }
}

template <class F>
static void run_all_mpcs(bool mont, u64 p, u64 g, u64 w) {
  // one round: full masks (the batched commitment's shape)
  run_shape<F, 1>(mont, p, g, w, Shape{1, {1}, {1}});
  run_shape<F, 2>(mont, p, g, w, Shape{2, {5}, {3}});
  run_shape<F, 3>(mont, p, g, w, Shape{3, {2}, {7}});
  // two rounds: full, disjoint
  run_shape<F, 2>(mont, p, g, w, Shape{2, {2, 3}, {3, 3}});
  run_shape<F, 2>(mont, p, g, w, Shape{2, {3, 1}, {1, 2}});
  // three rounds: nested
  run_shape<F, 2>(mont, p, g, w, Shape{2, {1, 5, 2}, {3, 1, 3}});
  // eight points, the second round at the last only
  run_shape<F, 8>(mont, p, g, w, Shape{8, {2, 3}, {0xFF, 0x80}});
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_mpcs p g [w]\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), g = strtoull(argv[2], nullptr, 0), w = argc > 3 ? strtoull(argv[3], nullptr, 0) : g;
  if (!(p & 1) || ((p - 1) & 63)) { fprintf(stderr, "p - 1 must be a multiple of 2^6\n"); return 2; }
  if (!ext2_non_residue(p, w)) { fprintf(stderr, "w must be a quadratic non-residue\n"); return 2; }
  g_rng = p ^ g ^ w ^ 5;
  int policies = 0;
  if (p == gl64::P) {
    census_policy("gl.");
    run_all_mpcs<FriGl>(false, p, g, w); policies |= 1;
    census_policy("w7.");
    if (w % p == 7) { run_all_mpcs<FriGlW7>(false, p, g, w); policies |= 2; }
  }
  census_policy("mont.");
  run_all_mpcs<FriMont>(true, p, g, w); policies |= 4;
  // what the host shape refuses
  {
    MpcsShape sh;
    const u32 c2[] = {1, 1}, m_ok[] = {1, 2}, m_gap[] = {1, 1}, m_big[] = {1, 4}, c0[] = {1, 0}, cbig[] = {1000, 25}, mfull[] = {3, 3};
    CHECK(mpcs_host_shape(2, 2, c2, m_ok, &sh) && sh.Y == 2 && sh.off[1] == 1 && sh.yoff[1] == 1, "a shape is refused");
    CHECK(!mpcs_host_shape(2, 2, c2, m_gap, &sh) && !mpcs_host_shape(2, 2, c2, m_big, &sh) && !mpcs_host_shape(2, 2, c0, m_ok, &sh),
          "a shape is accepted");
    CHECK(!mpcs_host_shape(2, 2, cbig, mfull, &sh) && !mpcs_host_shape(0, 2, c2, m_ok, &sh) && !mpcs_host_shape(2, 0, c2, m_ok, &sh),
          "a shape is accepted");
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu g=%llu w=%llu policies=%d\n", (unsigned long long)p, (unsigned long long)g, (unsigned long long)w, policies);
  return 0;
}
