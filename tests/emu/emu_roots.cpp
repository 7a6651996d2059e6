// emu_roots.cpp -- HOST EMULATOR of the product tree (TEST INFRASTRUCTURE ONLY; built and run by tests/test_emu_roots.py).
// The leaf body (roots_kernels.h roots_leaf_body) runs on ucontext fibers, one per work-item, barrier = yield; each level's
// pair products come from the oracle's schoolbook multiply (in the library: batched NTTs), and roots_combine_elem assembles
// the next level in the spread layout.  Checks, against a chain of oracle products of the linear factors (x - r_i):
//   - every node of every level: the monic combine identity (x^d + a)(x^d + b) = a*b + x^d (a + b) + x^2d;
//   - the root: every coefficient of prod (x - r_i), padding by the root ZERO undone by the final shift.
//
// usage: emu_roots <m> <G> <seed>      (RONK_EMU_P: a Montgomery prime instead of Goldilocks)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <functional>
#include <vector>

#include "../../oracle/ronk_oracle.h"
#include "../../ronkathon_amd/csrc/roots_kernels.h"

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

template <class FLD>
static void run(const FLD& f, u64 p, size_t m, u32 G, u64 seed) {
  // roots: random, with repeats and the root ZERO mixed in
  std::vector<u64> roots(m);
  for (size_t i = 0; i < m; i++) {
    const u64 v = splitmix(seed);
    roots[i] = (i % 7 == 3) ? 0 : (i % 5 == 4 && i) ? roots[i / 2] : v;   // raw 64-bit values: the leaf reduces mod p
  }
  // the reference: a chain of oracle products of (x - r_i)
  std::vector<u64> want(1, 1);
  for (size_t i = 0; i < m; i++) {
    const u64 lin[2] = {orc_neg(p, roots[i] % p), 1};
    std::vector<u64> nx(want.size() + 1);
    orc_poly_mul(p, want.data(), want.size(), lin, 2, nx.data());
    want.swap(nx);
  }
  size_t M = G;
  while (M < m) M <<= 1;
  const size_t leaves = M / G;
  std::vector<u64> S(2 * M, ~(u64)0), S2(2 * M, ~(u64)0), out(m + 1, ~(u64)0);
  RootsStore st{};
  if (leaves == 1) { st.out = out.data(); st.final_ = 1; st.shift = M - m; st.m = m; }
  else { st.out = S.data(); st.half = M; }
  std::vector<u64> lds(3 * G);
  for (size_t b = 0; b < leaves; b++) {
    g_body = [&](u32 tid) { roots_leaf_body(f, p, roots.data(), (u64)m, G, st, lds.data(), tid, (u64)b, [] { fiber_barrier(); }); };
    run_block(G);
  }
  // the leaves against the oracle (padding roots are ZERO)
  if (leaves > 1)
    for (size_t b = 0; b < leaves; b++) {
      std::vector<u64> leaf(1, 1);
      for (size_t t = 0; t < G; t++) {
        const size_t i = b * G + t;
        const u64 lin[2] = {i < m ? orc_neg(p, roots[i] % p) : 0, 1};
        std::vector<u64> nx(leaf.size() + 1);
        orc_poly_mul(p, leaf.data(), leaf.size(), lin, 2, nx.data());
        leaf.swap(nx);
      }
      const u64* node = S.data() + (b & 1) * M + (b >> 1) * 2 * G;
      for (size_t j = 0; j < G; j++) expect(node[j] == leaf[j], "leaf", b, j);
      for (size_t j = G; j < 2 * G; j++) expect(node[j] == 0, "leaf padding", b, j);
    }
  size_t d = G, count = leaves;
  while (count > 1) {
    const size_t pairs = count / 2, half = pairs * 2 * d;
    std::vector<u64> prod(half, 0);
    for (size_t i = 0; i < pairs; i++)   // a * b of the LOW coefficients (the library: NTTs of 2d points)
      orc_poly_mul(p, S.data() + i * 2 * d, d, S.data() + half + i * 2 * d, d, prod.data() + i * 2 * d);
    RootsStore nx{};
    std::vector<u64> top(2 * d, ~(u64)0);
    if (pairs == 1) { nx.out = out.data(); nx.final_ = 1; nx.shift = M - m; nx.m = m; }
    else { nx.out = S2.data(); nx.half = M; }
    for (size_t e = 0; e < half; e++) roots_combine_elem(f, prod.data(), S.data(), (u64)pairs, (u64)d, nx, (u64)e);
    // the monic identity, node by node: (x^d + a)(x^d + b) against the oracle
    if (pairs > 1)
      for (size_t i = 0; i < pairs; i++) {
        std::vector<u64> a(S.begin() + i * 2 * d, S.begin() + i * 2 * d + d), b(S.begin() + half + i * 2 * d, S.begin() + half + i * 2 * d + d);
        a.push_back(1); b.push_back(1);
        std::vector<u64> ab(2 * d + 1);
        orc_poly_mul(p, a.data(), d + 1, b.data(), d + 1, ab.data());
        const u64* node = S2.data() + (i & 1) * M + (i >> 1) * 4 * d;
        for (size_t j = 0; j < 2 * d; j++) expect(node[j] == ab[j], "combine", i, j);
        for (size_t j = 2 * d; j < 4 * d; j++) expect(node[j] == 0, "combine padding", i, j);
        expect(ab[2 * d] == 1, "monic", i, 2 * d);
      }
    S.swap(S2);
    d *= 2;
    count = pairs;
  }
  for (size_t j = 0; j <= m; j++) expect(out[j] == want[j], "root", j, m);
  if (g_fail) { printf("FAIL %d mismatches\n", g_fail); exit(1); }
  printf("OK m=%zu G=%u M=%zu levels=%d p=%llu\n", m, G, M, 0 + (int)__builtin_ctzll(M / G), (unsigned long long)p);
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: emu_roots <m> <G> <seed>\n"); return 2; }
  const size_t m = (size_t)atoll(argv[1]);
  const u32 G = (u32)atoi(argv[2]);
  const u64 seed = (u64)strtoull(argv[3], nullptr, 0);
  const char* ep = getenv("RONK_EMU_P");
  if (!ep) {
    run(GlField(), gl64::P, m, G, seed);
  } else {
    const u64 p = strtoull(ep, nullptr, 0);
    const mont64::Field mf = mont64::make_field(p);
    FieldConst c{};
    c.p = p; c.pinv = mf.pinv; c.r2 = mf.r2; c.w16[0] = mf.one;
    run(MontField(c), p, m, G, seed);
  }
  return 0;
}
