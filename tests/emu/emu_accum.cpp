// emu_accum.cpp -- the bodies of csrc/accum_kernels.h (the three phases of the scans over base words and pairs, the chunk
// inversion, the permutation and logUp terms) compiled for the host, run lane by lane in the order the kernels' barriers allow, and
// compared with a plain `unsigned __int128 % p` restatement in this file.  Test infrastructure only; never part of the product
// library.
//
//   emu_accum <p> <w>   last line "OK ..." on success.  Goldilocks runs the Goldilocks policy, its W = 7 form when w = 7, AND the
//                       Montgomery policy.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ronkathon_amd/csrc/accum_kernels.h"
using namespace ronk;
#include "emu_ref.h"
#include "emu_census.h"

// ---------------------------------------------------------------------------------------------------- the kernels, lane by lane
template <class O>
static typename O::V emu_block_reduce(const O& op, std::vector<typename O::V>& buf) {
  for (u32 s = ACC_LANES / 2; s > 0; s >>= 1)
    for (u32 lane = 0; lane < ACC_LANES; lane++) acc_tree_step(op, buf.data(), lane, s);
  return buf[0];
}
template <class O>
static std::vector<typename O::V> emu_block_scan(const O& op, std::vector<typename O::V> src) {
  std::vector<typename O::V> dst(ACC_LANES);
  for (u32 s = 0; s < ACC_LOG2_LANES; s++) {
    for (u32 lane = 0; lane < ACC_LANES; lane++) dst[lane] = acc_hs_step(op, src.data(), lane, s);
    src.swap(dst);
  }
  return src;
}
template <class O>
static void emu_phase1(const O& op, const u64* a, size_t n, u64* work) {
  const u64 B = acc_blocks(n);
  for (u64 b = 0; b < B; b++) {
    std::vector<typename O::V> buf(ACC_LANES);
    for (u32 lane = 0; lane < ACC_LANES; lane++) {
      typename O::V v[ACC_EPL];
      acc_load_chunk(op, a, n, (size_t)b * ACC_BLOCK + (size_t)lane * ACC_EPL, v);
      buf[lane] = acc_chunk_total(op, v);
    }
    op.e.raw_store(work, B, b, emu_block_reduce(op, buf));
  }
}
// returns the status the kernel writes (when it is asked for one)
template <class O>
static int emu_phase2(const O& op, u64* work, u64 B, u64* total, bool flags) {
  const u64 chunk = (B + ACC_LANES - 1) / ACC_LANES;
  std::vector<typename O::V> t(ACC_LANES);
  u64 flag = 0;
  for (u32 lane = 0; lane < ACC_LANES; lane++) t[lane] = acc_totals_reduce(op, work, B, lane, chunk, flags ? work + 2 * B : nullptr, &flag);
  const std::vector<typename O::V> incl = emu_block_scan(op, t);
  for (u32 lane = 0; lane < ACC_LANES; lane++) acc_totals_rewrite(op, work, B, lane, chunk, lane ? incl[lane - 1] : op.identity());
  if (total) op.e.store(total, 1, 0, incl[ACC_LANES - 1]);
  return flag != 0;
}
template <class O>
static void emu_phase3(const O& op, const u64* a, u64* out, size_t n, int exclusive, const u64* work) {
  const u64 B = acc_blocks(n);
  for (u64 b = 0; b < B; b++) {
    std::vector<typename O::V> t(ACC_LANES);
    std::vector<std::vector<typename O::V>> chunks(ACC_LANES, std::vector<typename O::V>(ACC_EPL));
    for (u32 lane = 0; lane < ACC_LANES; lane++) {   // every lane loads before any lane writes: in place is the kernel's order
      typename O::V v[ACC_EPL];
      acc_load_chunk(op, a, n, (size_t)b * ACC_BLOCK + (size_t)lane * ACC_EPL, v);
      for (int r = 0; r < ACC_EPL; r++) chunks[lane][r] = v[r];
      t[lane] = acc_chunk_total(op, v);
    }
    const std::vector<typename O::V> incl = emu_block_scan(op, t);
    for (u32 lane = 0; lane < ACC_LANES; lane++) {
      typename O::V v[ACC_EPL];
      for (int r = 0; r < ACC_EPL; r++) v[r] = chunks[lane][r];
      typename O::V base = op.e.raw_load(work, B, b);
      if (lane) base = op.comb(base, incl[lane - 1]);
      acc_write_chunk(op, base, v, exclusive, out, n, (size_t)b * ACC_BLOCK + (size_t)lane * ACC_EPL);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- scans
// EW words per element
template <class O, int EW, bool PROD>
static void run_scan(bool mont, u64 p, u64 w, size_t n, int exclusive, bool in_place) {
  const O op(ext2_host_consts(mont, p), ext2_reg_form(mont, p, w));
  std::vector<u64> a((size_t)EW * n), out((size_t)EW * n, ~(u64)0), work(acc_work_words(n), ~(u64)0), total(EW, ~(u64)0);
  for (auto& v : a) v = PROD && rnd() % 64 ? 1 + rnd() % (p - 1) : edge_word(p);   // few zeros in a product
  if (PROD && emu_small()) {   // the directed mode: factors +-1 and a few 2's -- pairs: (+-1, 0) and a few t's, 1 + t's and 1 - t's,
    size_t k = 0;              // whose products have two non-zero components -- so that every prefix stays small
    for (size_t i = 0; i < n; i++) {
      const bool special = i % (n / 16 + 1) == n / 32;
      const int kind = !special ? 0 : EW == 1 ? (k < 10 ? 1 : 0) : k % 5 == 1 ? 2 : k % 5 == 3 ? 3 : 1;   // at most ten 2's, as in gl_directed.scan_base
      k += special;
      a[i] = kind == 0 ? (rnd() & 1 ? 1 : p - 1) : kind == 1 ? (EW == 2 ? 0 : 2) : 1;
      if (EW == 2) a[n + i] = kind == 0 ? 0 : kind == 3 ? p - 1 : 1;
    }
  }
  // the restatement
  std::vector<R2> want(n);
  R2 run = PROD ? R2{1 % p, 0} : R2{0, 0};
  for (size_t i = 0; i < n; i++) {
    const R2 v = red(R2{a[i], EW == 2 ? a[n + i] : 0}, p);
    const R2 next = PROD ? x_mul(run, v, w % p, p) : x_add(run, v, p);
    want[i] = exclusive ? run : next;
    run = next;
  }
  std::vector<u64> src = a;
  u64* o = in_place ? src.data() : out.data();
  static const char* const stage[2][2][3] = {{{"scan_sum_base_1", "scan_sum_base_2", "scan_sum_base_3"}, {"scan_prod_base_1", "scan_prod_base_2", "scan_prod_base_3"}},
                                            {{"scan_sum_ext_1", "scan_sum_ext_2", "scan_sum_ext_3"}, {"scan_prod_ext_1", "scan_prod_ext_2", "scan_prod_ext_3"}}};
  census_stage(stage[EW - 1][PROD][0]);
  emu_phase1(op, src.data(), n, work.data());
  census_stage(stage[EW - 1][PROD][1]);
  emu_phase2(op, work.data(), acc_blocks(n), total.data(), false);
  census_stage(stage[EW - 1][PROD][2]);
  emu_phase3(op, src.data(), o, n, exclusive, work.data());
  census_stage(nullptr);
  for (size_t i = 0; i < n; i++)
    CHECK(o[i] == want[i].c0 && (EW == 1 || o[n + i] == want[i].c1), "scan EW=%d prod=%d n=%zu excl=%d inplace=%d i=%zu", EW, (int)PROD, n,
          exclusive, (int)in_place, i);
  CHECK(total[0] == run.c0 && (EW == 1 || total[1] == run.c1), "total EW=%d prod=%d n=%zu", EW, (int)PROD, n);
  if (!in_place) CHECK(src == a, "the input changed");
}

// phase 2 alone over B random totals: every lane count per chunk, B below, at and above the 256 lanes
template <class O, int EW, bool PROD>
static void run_phase2(bool mont, u64 p, u64 w) {
  const O op(ext2_host_consts(mont, p), ext2_reg_form(mont, p, w));
  const u64 Bs[] = {1, 2, 255, 256, 257, 511, 512, 513, 1000};
  for (u64 B : Bs) {
    std::vector<u64> work(3 * B, 0), plain(2 * B, 0), total(2, 0);
    for (u64 j = 0; j < B; j++) {
      const R2 v{1 + rnd() % (p - 1), EW == 2 ? rnd() % p : 0};
      plain[j] = v.c0; plain[B + j] = v.c1;
      const typename O::V reg = op.e.load(plain.data(), B, j);
      op.e.raw_store(work.data(), B, j, reg);
    }
    const u64 where = rnd() % B;
    for (int with_flag = 0; with_flag < 2; with_flag++) {
      std::vector<u64> wk = work;
      if (with_flag) wk[2 * B + where] = 1;
      const int st = emu_phase2(op, wk.data(), B, total.data(), true);
      CHECK(st == with_flag, "phase 2 status B=%llu", (unsigned long long)B);
      R2 run = PROD ? R2{1 % p, 0} : R2{0, 0};
      std::vector<u64> got(2 * B, 0);
      for (u64 j = 0; j < B; j++) {
        op.e.store(got.data(), B, j, op.e.raw_load(wk.data(), B, j));
        CHECK((R2{got[j], EW == 2 ? got[B + j] : 0} == run), "phase 2 B=%llu j=%llu", (unsigned long long)B, (unsigned long long)j);
        const R2 v{plain[j], plain[B + j]};
        run = PROD ? x_mul(run, v, w % p, p) : x_add(run, v, p);
      }
      CHECK(total[0] == run.c0 && (EW == 1 || total[1] == run.c1), "phase 2 total B=%llu", (unsigned long long)B);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- chunk inversion
template <class F>
static void run_invert(bool mont, u64 p, u64 w) {
  const F f(ext2_host_consts(mont, p));
  const Ext2<F> x(f, ext2_reg_form(mont, p, w));
  // zero patterns over the 8 slots: none, first, middle, last, two, all
  const u32 patterns[] = {0, 1, 1u << 3, 1u << 7, (1u << 2) | (1u << 5), 1u | (1u << 7), 0xFF};
  for (u32 z : patterns)
    for (int rep = 0; rep < 4; rep++) {
      u64 plain[ACC_EPL], nrm[ACC_EPL];
      for (int r = 0; r < ACC_EPL; r++) {
        plain[r] = (z >> r) & 1 ? 0 : 1 + rnd() % (p - 1);
        nrm[r] = f.in(plain[r] + ((z >> r) & 1 && rep == 1 && p < ~(u64)0 - p ? p : 0));   // a zero as the word p
      }
      const bool any = acc_chunk_invert(x, nrm);
      CHECK(any == (z != 0), "invert flag pattern=%u", z);
      for (int r = 0; r < ACC_EPL; r++)
        CHECK(f.out(nrm[r]) == r_pow(plain[r], p - 2, p), "invert pattern=%u r=%d", z, r);
    }
}

// ---------------------------------------------------------------------------------------------------- the accumulators
// the fused phase 1 as the kernels run it: terms, store, the block's total and flag
template <class O, class Terms>
static void emu_terms_phase1(const O& op, size_t N, u64* out, u64* work, Terms&& terms) {
  const u64 B = acc_blocks(N);
  for (u64 b = 0; b < B; b++) {
    std::vector<E2> buf(ACC_LANES);
    bool raised = false;
    for (u32 lane = 0; lane < ACC_LANES; lane++) {
      const size_t i0 = (size_t)b * ACC_BLOCK + (size_t)lane * ACC_EPL;
      E2 term[ACC_EPL];
      raised |= terms(i0, term);
      acc_store_terms(op.e.x, term, out, N, i0);
      buf[lane] = acc_chunk_total(op, term);
    }
    op.e.raw_store(work, B, b, emu_block_reduce(op, buf));
    work[2 * B + b] = raised;
  }
}

// zeros: rows whose denominator is forced to ZERO
template <class F>
static void run_perm(bool mont, u64 p, u64 w, u32 W, size_t N, const std::vector<size_t>& zeros) {
  typedef AccOp<AccPair<F>, ACC_PROD> O;
  const O op(ext2_host_consts(mont, p), ext2_reg_form(mont, p, w));
  const Ext2<F>& x = op.e.x;
  std::vector<u64> a((size_t)W * N), ids((size_t)W * N), sg((size_t)W * N);
  for (auto& v : a) v = edge_word(p);
  for (auto& v : ids) v = edge_word(p);
  for (auto& v : sg) v = edge_word(p);
  // a + beta s + gamma = 0 for the wire value a = -(beta0 s + gamma0) when gamma1 = -beta1 s
  const R2 beta{rnd() % p, rnd() % p};
  const u64 s = rnd() % p;
  const R2 gamma{rnd() % p, r_sub(0, r_mul(beta.c1, s, p), p)};
  for (size_t i : zeros) {
    const u32 c = (u32)(rnd() % W);
    sg[(size_t)c * N + i] = s;
    a[(size_t)c * N + i] = r_sub(0, r_add(r_mul(beta.c0, s, p), gamma.c0, p), p);
  }
  // the restatement
  std::vector<R2> want(N);
  R2 run{1 % p, 0};
  int want_status = 0;
  for (size_t i = 0; i < N; i++) {
    want[i] = run;
    R2 num{1 % p, 0}, den{1 % p, 0};
    for (u32 c = 0; c < W; c++) {
      const u64 av = a[(size_t)c * N + i] % p;
      num = x_mul(num, x_add(x_add(R2{av, 0}, x_scale(beta, ids[(size_t)c * N + i] % p, p), p), gamma, p), w % p, p);
      den = x_mul(den, x_add(x_add(R2{av, 0}, x_scale(beta, sg[(size_t)c * N + i] % p, p), p), gamma, p), w % p, p);
    }
    if (den == R2{0, 0}) want_status = 1;
    run = x_mul(run, x_mul(num, x_inv(den, w % p, p), w % p, p), w % p, p);
  }
  for (size_t i : zeros) CHECK(want_status == 1 && (i + 1 >= N || want[i + 1] == R2{0, 0}), "the forced zero did not take");
  // the kernels
  const E2 br{x.f.in(beta.c0), x.f.in(beta.c1)}, gr{x.f.in(gamma.c0), x.f.in(gamma.c1)};
  std::vector<u64> Z(2 * N, ~(u64)0), work(acc_work_words(N), ~(u64)0), last(2, ~(u64)0);
  emu_terms_phase1(op, N, Z.data(), work.data(), [&](size_t i0, E2 (&term)[ACC_EPL]) {
    return acc_perm_chunk(x, br, gr, a.data(), ids.data(), sg.data(), W, N, i0, term);
  });
  const int status = emu_phase2(op, work.data(), acc_blocks(N), last.data(), true);
  emu_phase3(op, Z.data(), Z.data(), N, 1, work.data());
  CHECK(status == want_status, "perm status W=%u N=%zu got %d want %d", W, N, status, want_status);
  for (size_t i = 0; i < N; i++) CHECK((R2{Z[i], Z[N + i]} == want[i]), "perm W=%u N=%zu zeros=%zu i=%zu", W, N, zeros.size(), i);
  CHECK((R2{last[0], last[1]} == run), "perm last W=%u N=%zu", W, N);
}

template <class F>
static void run_logup(bool mont, u64 p, u64 w, u32 C, size_t N, bool with_mult, const std::vector<size_t>& zeros) {
  typedef AccOp<AccPair<F>, ACC_SUM> O;
  const O op(ext2_host_consts(mont, p), ext2_reg_form(mont, p, w));
  const Ext2<F>& x = op.e.x;
  std::vector<u64> v((size_t)C * N), m((size_t)C * N);
  for (auto& t : v) t = edge_word(p);
  for (auto& t : m) t = rnd() % 4 ? rnd() % 5 : edge_word(p);
  const R2 alpha{rnd() % p, zeros.empty() ? rnd() % p : 0};   // alpha + v = 0 needs alpha1 = 0
  for (size_t i : zeros) v[(size_t)(rnd() % C) * N + i] = r_sub(0, alpha.c0, p);
  std::vector<R2> want(N);
  R2 run{0, 0};
  int want_status = 0;
  for (size_t i = 0; i < N; i++) {
    want[i] = run;
    for (u32 c = 0; c < C; c++) {
      const R2 d = x_add(alpha, R2{v[(size_t)c * N + i] % p, 0}, p);
      if (d == R2{0, 0}) want_status = 1;
      run = x_add(run, x_scale(x_inv(d, w % p, p), with_mult ? m[(size_t)c * N + i] % p : 1 % p, p), p);
    }
  }
  if (!zeros.empty()) CHECK(want_status == 1, "the forced zero did not take");
  const E2 ar{x.f.in(alpha.c0), x.f.in(alpha.c1)};
  std::vector<u64> S(2 * N, ~(u64)0), work(acc_work_words(N), ~(u64)0), last(2, ~(u64)0);
  emu_terms_phase1(op, N, S.data(), work.data(), [&](size_t i0, E2 (&term)[ACC_EPL]) {
    return acc_logup_chunk(x, ar, v.data(), with_mult ? m.data() : nullptr, C, N, i0, term);
  });
  const int status = emu_phase2(op, work.data(), acc_blocks(N), last.data(), true);
  emu_phase3(op, S.data(), S.data(), N, 1, work.data());
  CHECK(status == want_status, "logup status C=%u N=%zu got %d want %d", C, N, status, want_status);
  for (size_t i = 0; i < N; i++) CHECK((R2{S[i], S[N + i]} == want[i]), "logup C=%u N=%zu mult=%d zeros=%zu i=%zu", C, N, (int)with_mult, zeros.size(), i);
  CHECK((R2{last[0], last[1]} == run), "logup last C=%u N=%zu", C, N);
}

template <class F>
static void run_all(bool mont, u64 p, u64 w) {
  // a lane is 8 elements, a wavefront 512, a workgroup 2048; phase 2 gives a lane two totals from 2048 * 256 + 1 elements on
  const size_t sizes[] = {1, 2, 7, 8, 9, 15, 17, 511, 512, 513, 2047, 2048, 2049, 4097, 6150};
  for (size_t n : sizes)
    for (int variant = 0; variant < 4; variant++) {
      const int excl = variant & 1;
      const bool inpl = variant >> 1;
      run_scan<AccOp<AccWord<F>, ACC_PROD>, 1, true>(mont, p, w, n, excl, inpl);
      run_scan<AccOp<AccWord<F>, ACC_SUM>, 1, false>(mont, p, w, n, excl, inpl);
      run_scan<AccOp<AccPair<F>, ACC_PROD>, 2, true>(mont, p, w, n, excl, inpl);
      run_scan<AccOp<AccPair<F>, ACC_SUM>, 2, false>(mont, p, w, n, excl, inpl);
    }
  const size_t big = (size_t)ACC_BLOCK * ACC_LANES + 1;
  run_scan<AccOp<AccPair<F>, ACC_PROD>, 2, true>(mont, p, w, big, 1, true);
  run_scan<AccOp<AccWord<F>, ACC_SUM>, 1, false>(mont, p, w, big, 0, false);
  run_phase2<AccOp<AccWord<F>, ACC_PROD>, 1, true>(mont, p, w);
  run_phase2<AccOp<AccWord<F>, ACC_SUM>, 1, false>(mont, p, w);
  run_phase2<AccOp<AccPair<F>, ACC_PROD>, 2, true>(mont, p, w);
  run_phase2<AccOp<AccPair<F>, ACC_SUM>, 2, false>(mont, p, w);
  run_invert<F>(mont, p, w);
  const u32 cols[] = {1, 3, 16};
  const size_t rows[] = {1, 5, 8, 9, 2049, 4097};
  for (u32 W : cols)
    for (size_t N : rows) {
      run_perm<F>(mont, p, w, W, N, {});
      run_logup<F>(mont, p, w, W, N, true, {});
      run_logup<F>(mont, p, w, W, N, false, {});
      // a zero denominator in the first, a middle and the last slot of a chunk, and two in one chunk
      const size_t c0 = N > 16 ? 8 * ((N - 8) / 16) : 0;   // the first row of some chunk
      std::vector<std::vector<size_t>> zs = {{c0}, {N - 1}};
      if (c0 + 7 < N) { zs.push_back({c0 + 3}); zs.push_back({c0 + 7}); zs.push_back({c0 + 1, c0 + 6}); zs.push_back({c0, c0 + 7, N - 1}); }
      for (const auto& z : zs) {
        run_perm<F>(mont, p, w, W, N, z);
        run_logup<F>(mont, p, w, W, N, W != 3, z);
      }
    }
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: emu_accum p w\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0), w = strtoull(argv[2], nullptr, 0);
  if (p < 3 || !(p & 1) || !ext2_non_residue(p, w)) { fprintf(stderr, "p must be an odd prime, w a quadratic non-residue\n"); return 2; }
  g_rng = p ^ w ^ 16;
  int policies = 0;
  if (p == gl64::P) {
    census_policy("gl.");
    run_all<FriGl>(false, p, w); policies |= 1;
    census_policy("w7.");
    if (w % p == 7) { run_all<FriGlW7>(false, p, w); policies |= 2; }
  }
  census_policy("mont.");
  run_all<FriMont>(true, p, w); policies |= 4;
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu w=%llu policies=%d\n", (unsigned long long)p, (unsigned long long)w, policies);
  return 0;
}
