// emu_multipoint.cpp -- HOST EMULATOR of multipoint evaluation and interpolation (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_emu_multipoint.py).  The tree's leaf body, the evaluation and interpolation leaf bodies (multipoint_kernels.h) run on
// ucontext fibers, one per work-item, barrier = yield; the element-wise bodies run in plain loops; the level products (in the
// library: batched NTTs) and the root's inverse series come from the oracle.  Checks:
//   - at EVERY node S of the walk down: W_S * A_S == rev_{s-1}(f mod M_S) mod z^s, the remainder from orc_poly_divrem;
//   - every output against orc_poly_eval, and the direct Horner body against the same;
//   - the interpolant of those values at distinct nodes equals f reduced to m coefficients; a repeated node sets the status.
//
// usage: emu_multipoint <m> <d> <seed> [distinct]      (RONK_EMU_P: a Montgomery prime instead of Goldilocks)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <functional>
#include <vector>

#include "../../oracle/ronk_oracle.h"
#include "../../ronkathon_amd/csrc/multipoint_kernels.h"

using namespace ronk;

static ucontext_t g_sched;
static std::vector<ucontext_t> g_ctx;
static std::vector<char> g_stacks, g_done;
static int g_cur;
static std::function<void(u32)> g_body;
static void fiber_barrier() { swapcontext(&g_ctx[g_cur], &g_sched); }
static void fiber_main(int tid) {
  g_body((u32)tid);
  g_done[tid] = 1;
  swapcontext(&g_ctx[tid], &g_sched);
}
static void run_block(u32 T) {
  const size_t STK = 64 * 1024;
  if (g_ctx.size() < T) { g_ctx.resize(T); g_stacks.resize((size_t)T * STK); g_done.resize(T); }
  for (u32 t = 0; t < T; t++) {
    getcontext(&g_ctx[t]);
    g_ctx[t].uc_stack.ss_sp = &g_stacks[(size_t)t * STK];
    g_ctx[t].uc_stack.ss_size = STK;
    g_ctx[t].uc_link = &g_sched;
    makecontext(&g_ctx[t], (void (*)())fiber_main, 1, (int)t);
    g_done[t] = 0;
  }
  for (bool any = true; any;) {
    any = false;
    for (u32 t = 0; t < T; t++) {
      if (g_done[t]) continue;
      any = true;
      g_cur = (int)t;
      swapcontext(&g_sched, &g_ctx[t]);
    }
  }
}

static u64 splitmix(u64& s) {
  s += 0x9E3779B97F4A7C15ull;
  u64 z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int g_fail = 0;
static void expect(bool ok, const char* what, size_t a, size_t b) {
  if (!ok && g_fail++ < 10) printf("MISMATCH %s at %zu / %zu\n", what, a, b);
}

typedef std::vector<u64> Vec;

// the retained tree: the spread layout of every level (level 0: the leaves), the product Z of m + 1 coefficients
struct Tree {
  std::vector<Vec> spread;
  Vec z;
};

template <class FLD>
static Tree build_tree(const FLD& f, u64 p, const Vec& xs, size_t m, u32 G, size_t M) {
  Tree t;
  const size_t leaves = M / G;
  t.z.assign(m + 1, ~(u64)0);
  t.spread.push_back(Vec(2 * M, ~(u64)0));
  RootsStore st{};
  st.out = t.spread[0].data(); st.half = M;
  Vec lds(3 * G);
  for (size_t b = 0; b < leaves; b++) {
    g_body = [&](u32 tid) { roots_leaf_body(f, p, xs.data(), (u64)m, G, st, lds.data(), tid, (u64)b, [] { fiber_barrier(); }); };
    run_block(G);
  }
  if (leaves == 1) {
    for (u64 j = 0; j < G; j++) roots_single_leaf_elem(t.spread[0].data(), (u64)(M - m), (u64)m, t.z.data(), j);
  }
  size_t d = G, count = leaves;
  while (count > 1) {
    const size_t pairs = count / 2, half = pairs * 2 * d;
    const Vec& S = t.spread.back();
    Vec prod(half, 0);
    for (size_t i = 0; i < pairs; i++) orc_poly_mul(p, S.data() + i * 2 * d, d, S.data() + half + i * 2 * d, d, prod.data() + i * 2 * d);
    Vec next(2 * M, ~(u64)0);
    RootsStore nx{};
    if (pairs == 1) { nx.out = t.z.data(); nx.final_ = 1; nx.shift = M - m; nx.m = m; }
    else { nx.out = next.data(); nx.half = M; }
    for (size_t e = 0; e < half; e++) roots_combine_elem(f, prod.data(), S.data(), (u64)pairs, (u64)d, nx, (u64)e);
    if (pairs > 1) t.spread.push_back(next);
    d *= 2;
    count = pairs;
  }
  return t;
}

// node i of the level whose nodes have d coefficients: its d low coefficients (the leading ONE implicit)
static const u64* node_of(const Tree& t, size_t level, size_t M, size_t d, size_t i) {
  return t.spread[level].data() + (i & 1) * M + (i >> 1) * 2 * d;
}

// the cyclic product of s points of v (s words) and low (s / 2 words): what the inverse transform of the library returns
static Vec cyclic_mul(u64 p, const u64* v, const u64* low, size_t s) {
  Vec full(s + s / 2 - 1 + 1, 0), out(s, 0);
  orc_poly_mul(p, v, s, low, s / 2, full.data());
  for (size_t j = 0; j < s + s / 2 - 1; j++) out[j % s] = orc_add(p, out[j % s], full[j]);
  return out;
}

// W_S * A_S == rev_{s-1}(f mod M_S) mod z^s for the node of s points whose window (reversed) is v and low coefficients `low`
static void check_window(u64 p, const Vec& fpoly, const u64* v, const u64* low, size_t s, size_t level, size_t i) {
  Vec ms(low, low + s);
  ms.push_back(1);
  Vec rem(s, 0);
  if (fpoly.size() <= s) {
    for (size_t j = 0; j < fpoly.size(); j++) rem[j] = fpoly[j];
  } else {
    Vec q(fpoly.size()), r(fpoly.size());
    if (orc_poly_divrem(p, fpoly.data(), fpoly.size(), ms.data(), s + 1, q.data(), r.data()) != 0) { expect(false, "divrem", level, i); return; }
    for (size_t j = 0; j < s; j++) rem[j] = r[j];
  }
  Vec w(s), a(s + 1);
  for (size_t k = 0; k < s; k++) w[k] = v[s - 1 - k];
  for (size_t k = 0; k <= s; k++) a[k] = ms[s - k];
  Vec wa(2 * s);
  orc_poly_mul(p, w.data(), s, a.data(), s + 1, wa.data());
  for (size_t k = 0; k < s; k++) expect(wa[k] == rem[s - 1 - k], "window identity", level * 1000 + i, k);
}

// the walk down: f (canonical) at the tree's points; checks every node's window
template <class FLD>
static Vec walk_down(const FLD& f, u64 p, const Tree& t, const Vec& fpoly, const Vec& xs, size_t m, u32 G, size_t M, bool check) {
  const size_t d = fpoly.size(), D = d > M ? d : M;
  // A_root = rev(Z); alpha = 1 / A_root mod z^D (the library: the Newton ladder)
  Vec a(D, 0), alpha(D, 0), fr(D, 0);
  for (u64 k = 0; k < D; k++) mp_reverse_elem(p, t.z.data(), (u64)m, (u64)(m + 1), a.data(), k);
  for (u64 k = 0; k < D; k++) mp_one_elem(alpha.data(), k);   // the ladder's start; the oracle loop below fills the rest
  for (size_t k = 1; k < D; k++) {
    u64 acc = 0;
    for (size_t j = 1; j <= k; j++) acc = orc_add(p, acc, orc_mul(p, a[j], alpha[k - j]));
    alpha[k] = orc_neg(p, acc);
  }
  for (u64 k = 0; k < D; k++) mp_reverse_elem(p, fpoly.data(), (u64)(D - 1), (u64)d, fr.data(), k);
  Vec q(2 * D);
  orc_poly_mul(p, fr.data(), D, alpha.data(), D, q.data());
  Vec V(M), VN(M);
  for (u64 k = 0; k < M; k++) mp_reverse_elem(p, q.data(), (u64)(D - 1), (u64)D, V.data(), k);
  const size_t levels = (size_t)__builtin_ctzll(M / G);
  if (check && levels > 0) {   // the root: x^pad * Z, its M low coefficients
    Vec low(M, 0);
    for (size_t j = M - m; j < M; j++) low[j] = t.z[j - (M - m)];
    check_window(p, fpoly, V.data(), low.data(), M, levels, 0);
  }
  for (size_t level = levels; level-- > 0;) {
    const size_t dd = (size_t)G << level, pairs = M / (2 * dd);
    Vec PL(M), PR(M);
    for (size_t r = 0; r < pairs; r++) {
      const Vec pl = cyclic_mul(p, V.data() + r * 2 * dd, node_of(t, level, M, dd, 2 * r + 1), 2 * dd);
      const Vec pr = cyclic_mul(p, V.data() + r * 2 * dd, node_of(t, level, M, dd, 2 * r), 2 * dd);
      memcpy(PL.data() + r * 2 * dd, pl.data(), 2 * dd * 8);
      memcpy(PR.data() + r * 2 * dd, pr.data(), 2 * dd * 8);
    }
    for (u64 e = 0; e < M; e++) mp_window_elem(f, V.data(), PL.data(), PR.data(), (u64)dd, VN.data(), e);
    V.swap(VN);
    if (check)
      for (size_t i = 0; i < M / dd; i++) check_window(p, fpoly, V.data() + i * dd, node_of(t, level, M, dd, i), dd, level, i);
  }
  if (check && levels == 0) check_window(p, fpoly, V.data(), node_of(t, 0, M, G, 0), G, 0, 0);
  Vec out(m, ~(u64)0), lds(3 * G);
  for (size_t b = 0; b < M / G; b++) {
    g_body = [&](u32 tid) {
      mp_eval_leaf_body(f, p, V.data(), t.spread[0].data(), xs.data(), (u64)m, (u64)M, G, out.data(), lds.data(), tid, (u64)b,
                        [] { fiber_barrier(); });
    };
    run_block(G);
  }
  return out;
}

template <class FLD>
static void run(const FLD& f, u64 p, size_t m, size_t d, u64 seed, bool distinct) {
  const u32 G = 64;
  Vec xs(m), fpoly(d);
  for (size_t i = 0; i < m; i++) {
    const u64 v = splitmix(seed);
    if (distinct) xs[i] = p > 2 * m ? (v % (p / m)) * m + i : i;   // distinct residues (needs m <= p)
    else xs[i] = (i % 7 == 3) ? 0 : (i % 5 == 4) ? xs[i / 2] : v;   // raw 64-bit values, repeats and ZERO mixed in
  }
  for (size_t j = 0; j < d; j++) fpoly[j] = splitmix(seed) % p;
  size_t M = G;
  while (M < m) M <<= 1;
  const Tree t = build_tree(f, p, xs, m, G, M);
  // evaluation: the walk down, and the direct body
  const Vec got = walk_down(f, p, t, fpoly, xs, m, G, M, true);
  Vec direct(m, ~(u64)0), hl(MP_CH);
  for (size_t b = 0; b < (m + MP_DIRECT_BLOCK - 1) / MP_DIRECT_BLOCK; b++) {
    g_body = [&](u32 tid) {
      mp_horner_body(f, p, fpoly.data(), (u64)d, xs.data(), (u64)m, direct.data(), hl.data(), tid, (u64)b, MP_DIRECT_BLOCK, [] { fiber_barrier(); });
    };
    run_block(MP_DIRECT_BLOCK);
  }
  for (size_t i = 0; i < m; i++) {
    const u64 want = orc_poly_eval(p, fpoly.data(), d, xs[i] % p);
    expect(got[i] == want, "tree value", i, m);
    expect(direct[i] == want, "direct value", i, m);
  }
  // interpolation through (xs, got): Z', its values by the same walk, the weights, the leaves, the levels
  Vec dz(m), w(M, ~(u64)0);
  for (u64 j = 0; j < m; j++) mp_deriv_elem(f, p, t.z.data(), dz.data(), j);
  const Vec dzx = walk_down(f, p, t, dz, xs, m, G, M, false);
  for (size_t i = 0; i < m; i++) expect(dzx[i] == orc_poly_eval(p, dz.data(), m, xs[i] % p), "derivative value", i, m);
  int status = 0;
  for (u64 c = 0; c < M / REC_CH; c++) mp_weights_chunk(f, p, dzx.data(), got.data(), (u64)m, w.data(), &status, -2, c);
  bool repeated = false;
  for (size_t i = 0; i < m && !repeated; i++)
    for (size_t j = 0; j < i; j++) if (xs[i] % p == xs[j] % p) { repeated = true; break; }
  expect((status == -2) == repeated, "status", (size_t)status, repeated);
  if (!repeated) {
    Vec out(m, ~(u64)0), N(2 * M, ~(u64)0), N2(2 * M, ~(u64)0), lds(G + G * (G + 1));
    const size_t leaves = M / G;
    InterpStore st{};
    if (leaves == 1) { st.out = out.data(); st.final_ = 1; st.shift = M - m; }
    else { st.out = N.data(); st.half = M; }
    for (size_t b = 0; b < leaves; b++) {
      g_body = [&](u32 tid) {
        mp_interp_leaf_body(f, p, w.data(), t.spread[0].data(), xs.data(), (u64)m, (u64)M, G, st, lds.data(), tid, (u64)b,
                            [] { fiber_barrier(); });
      };
      run_block(G);
    }
    size_t dd = G, count = leaves, level = 0;
    while (count > 1) {
      const size_t pairs = count / 2, half = pairs * 2 * dd;
      // N_L * low(M_R) + N_R * low(M_L): the library's pointwise step between the transforms (mp_interp_pointwise_elem is the same
      // sum on transform values; here on coefficients, through the oracle's products)
      Vec prod(half, 0), t1(2 * dd), t2(2 * dd);
      for (size_t i = 0; i < pairs; i++) {
        orc_poly_mul(p, N.data() + i * 2 * dd, dd, node_of(t, level, M, dd, 2 * i + 1), dd, t1.data());
        orc_poly_mul(p, N.data() + half + i * 2 * dd, dd, node_of(t, level, M, dd, 2 * i), dd, t2.data());
        t1[2 * dd - 1] = t2[2 * dd - 1] = 0;
        for (size_t j = 0; j < 2 * dd; j++) prod[i * 2 * dd + j] = orc_add(p, t1[j], t2[j]);
      }
      InterpStore nx{};
      if (pairs == 1) { nx.out = out.data(); nx.final_ = 1; nx.shift = M - m; }
      else { nx.out = N2.data(); nx.half = M; }
      for (u64 e = 0; e < half; e++) mp_interp_combine_elem(f, prod.data(), N.data(), (u64)pairs, (u64)dd, nx, e);
      N.swap(N2);
      dd *= 2;
      count = pairs;
      level++;
    }
    // the interpolant of f's values at m distinct nodes: f itself when d <= m, else f mod Z
    Vec want(m, 0);
    if (d <= m) {
      for (size_t j = 0; j < d; j++) want[j] = fpoly[j];
    } else {
      Vec q(d), r(d);
      if (orc_poly_divrem(p, fpoly.data(), d, t.z.data(), m + 1, q.data(), r.data()) != 0) expect(false, "divrem root", 0, 0);
      for (size_t j = 0; j < m; j++) want[j] = r[j];
    }
    for (size_t j = 0; j < m; j++) expect(out[j] == want[j], "interpolant", j, m);
  }
  // the reduction and status bodies of the direct interpolation
  {
    Vec red(m);
    for (u64 i = 0; i < m; i++) mp_reduce_elem(p, xs.data(), red.data(), i);
    for (size_t i = 0; i < m; i++) expect(red[i] == orc_new(p, xs[i]), "reduce", i, m);
    expect(mp_status_code(0, -2) == 0 && mp_status_code(1, -2) == -2 && mp_status_code(4, -2) == -2, "status code", 0, 0);
  }
  // the pointwise body on one pair of values, against its definition
  {
    const u64 fn[2] = {splitmix(seed) % p, splitmix(seed) % p}, tk[2] = {splitmix(seed) % p, splitmix(seed) % p};
    u64 x = 0;
    mp_interp_pointwise_elem(f, fn, tk, 1, &x, 0);
    expect(x == orc_add(p, orc_mul(p, fn[0], tk[1]), orc_mul(p, fn[1], tk[0])), "pointwise", 0, 0);
  }
  if (g_fail) { printf("FAIL %d mismatches\n", g_fail); exit(1); }
  printf("OK m=%zu d=%zu M=%zu levels=%d repeated=%d p=%llu\n", m, d, M, (int)__builtin_ctzll(M / G), (int)repeated, (unsigned long long)p);
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: emu_multipoint <m> <d> <seed> [distinct]\n"); return 2; }
  const size_t m = (size_t)atoll(argv[1]), d = (size_t)atoll(argv[2]);
  const u64 seed = (u64)strtoull(argv[3], nullptr, 0);
  const bool distinct = argc > 4 && atoi(argv[4]) != 0;
  const char* ep = getenv("RONK_EMU_P");
  if (!ep) {
    run(GlField(), gl64::P, m, d, seed, distinct);
  } else {
    const u64 p = strtoull(ep, nullptr, 0);
    const mont64::Field mf = mont64::make_field(p);
    FieldConst c{};
    c.p = p; c.pinv = mf.pinv; c.r2 = mf.r2; c.w16[0] = mf.one;
    run(MontField(c), p, m, d, seed, distinct);
  }
  return 0;
}
