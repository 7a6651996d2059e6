// emu_fr_ntt.cpp -- HOST EMULATOR of the transform over BN254's scalar field (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_emu_fr_ntt.py and `make sanitize`).  The pass body of csrc/fr_ntt_kernels.h runs on ucontext fibers, one per
// work-item, barrier = yield, with the library's own planner and table builder (fr_build_plan) and the library's buffer
// rotation.  Checks, for `batch` rows that hold r, r + 1 and 2^256 - 1 among arbitrary 256-bit integers:
//   - the forward transform of every row, every output, against the naive O(n^2) DFT  X[k] = sum_i x[i] omega^(i k);
//   - the inverse transform of that, in place, against the rows' residues; and the inverse plan on the arbitrary rows
//     themselves, the first row against the naive (1/n) sum_i x[i] omega^(-i k);
//   - the multiply's path (padding body, forward of both operands as one batch of two, pointwise body, the inverse whose
//     table carries 2^256 / n) against the schoolbook product.
//
// usage: emu_fr_ntt <log2n> <max_log2_tile> <batch> <seed>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "../../ronkathon_amd/csrc/fr_ntt_kernels.h"

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
typedef unsigned __int128 u128;

// the reference arithmetic of the naive DFT: Montgomery product and addition on 4 x 64-bit limbs, written independently of
// bn254_fr.h (which it thereby cross-checks) and several times faster on the host
struct F4 { u64 w[4]; };
static u64 g_mod[4], g_ninv;
static void ref_init() {
  for (int i = 0; i < 4; i++) g_mod[i] = (u64)bn254::fr_mod(2 * i) | ((u64)bn254::fr_mod(2 * i + 1) << 32);
  u64 inv = 1;
  for (int i = 0; i < 6; i++) inv *= 2 - g_mod[0] * inv;   // 1 / r mod 2^64
  g_ninv = (u64)0 - inv;
}
static F4 ref_reduce(const u64* t, u64 top) {   // t < 2 r (with its carry word) -> t mod r
  F4 d;
  u64 borrow = 0;
  for (int i = 0; i < 4; i++) {
    const u128 x = (u128)t[i] - g_mod[i] - borrow;
    d.w[i] = (u64)x;
    borrow = (u64)(x >> 64) & 1;
  }
  if (top == 0 && borrow) memcpy(d.w, t, 32);
  return d;
}
static F4 ref_add(const F4& a, const F4& b) {
  u64 t[4];
  u128 c = 0;
  for (int i = 0; i < 4; i++) { c += (u128)a.w[i] + b.w[i]; t[i] = (u64)c; c >>= 64; }
  return ref_reduce(t, (u64)c);
}
static F4 ref_mul(const F4& a, const F4& b) {   // a b / 2^256 mod r
  u64 t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) { const u128 s = (u128)a.w[j] * b.w[i] + t[j] + c; t[j] = (u64)s; c = s >> 64; }
    u128 s = (u128)t[4] + c;
    t[4] = (u64)s; t[5] = (u64)(s >> 64);
    const u64 m = t[0] * g_ninv;
    c = ((u128)m * g_mod[0] + t[0]) >> 64;
    for (int j = 1; j < 4; j++) { s = (u128)m * g_mod[j] + t[j] + c; t[j - 1] = (u64)s; c = s >> 64; }
    s = (u128)t[4] + c;
    t[3] = (u64)s; t[4] = t[5] + (u64)(s >> 64);
  }
  return ref_reduce(t, t[4]);
}

// out[o] = scale * sum_i c[i] omega^(+-i o): c canonical, W4[t] = omega^t and scale (may be null) in Montgomery form.  The n
// products of an output are summed as plain 512-bit integers (n <= 2^13 terms below 2^510: nine words hold the sum) and
// reduced once: with V = L0 + 2^256 L1 + 2^512 L2,  V / 2^256 = L0 / 2^256 + L1 + 2^256 L2  (mod r).
static void naive_dft(const std::vector<F4>& c, const std::vector<F4>& W4, bool inverse, const F4* scale, u64* out) {
  const size_t n = c.size();
  F4 one = {{1, 0, 0, 0}}, one_m, r2;
  bn254::fr_store(one_m.w, bn254::fr_const_one_mont());
  bn254::fr_store(r2.w, bn254::fr_const_r2());
  // outputs are independent: up to 8 host threads share them (plain threads, outside the fibers)
  const size_t nthr = n < 1024 ? 1 : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
  auto work = [&](size_t t) {
  for (size_t o = t; o < n; o += nthr) {
    u64 v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const size_t step = inverse ? (n - o) & (n - 1) : o;
    for (size_t i = 0, e = 0; i < n; i++, e = (e + step) & (n - 1)) {
      const u64 *x = c[i].w, *y = W4[e].w;
      u64 p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int a = 0; a < 4; a++) {
        u128 cy = 0;
        for (int b = 0; b < 4; b++) { const u128 t = (u128)x[a] * y[b] + p[a + b] + cy; p[a + b] = (u64)t; cy = t >> 64; }
        p[a + 4] = (u64)cy;
      }
      u128 cy = 0;
      for (int a = 0; a < 8; a++) { cy += (u128)v[a] + p[a]; v[a] = (u64)cy; cy >>= 64; }
      v[8] += (u64)cy;
    }
    F4 l0, l1, l2 = {{v[8], 0, 0, 0}};
    memcpy(l0.w, v, 32);
    memcpy(l1.w, v + 4, 32);
    F4 acc = ref_add(ref_add(ref_mul(l0, one), ref_mul(l1, one_m)), ref_mul(l2, r2));
    if (scale) acc = ref_mul(acc, *scale);
    memcpy(out + 4 * o, acc.w, 32);
  }
  };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nthr; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
}

// every pass of `pd` over `batch` rows, buffers rotated as the library does (ronk_fr_ntt.hip FrCompiled::run)
static void run_plan(const FrPlanDesc& pd, const u64* in, u64* out, size_t batch) {
  const size_t n = (size_t)1 << pd.log2n, P = pd.passes.size();
  Vec t1(P >= 2 ? 4 * n * batch : 0, ~(u64)0), t2(P >= 3 ? 4 * n * batch : 0, ~(u64)0);
  const u64* src = in;
  for (size_t t = 0; t < P; t++) {
    const FrPassDesc& ps = pd.passes[t];
    u64* dst = t + 1 == P ? out : ((t & 1) ? t2.data() : t1.data());
    FrPassArgs a;
    a.g = ps.g; a.in = src; a.out = dst; a.wr = ps.wr.data(); a.tw = ps.tw.data();
    const u32 T = fr_pass_threads(ps.g);
    Vec lds(fr_pass_lds_bytes(ps.g) / 8);
    for (u64 row = 0; row < batch; row++)
      for (u64 tile = 0; tile < fr_pass_blocks(ps.g); tile++) {
        g_body = [&](u32 tid) { fr_ntt_pass_body(a, lds.data(), tid, T, tile, row, [] { fiber_barrier(); }); };
        run_block(T);
      }
    src = dst;
  }
}

int main(int argc, char** argv) {
  using namespace bn254;
  if (argc < 5) { fprintf(stderr, "usage: emu_fr_ntt <log2n> <max_log2_tile> <batch> <seed>\n"); return 2; }
  const u32 k = (u32)atoi(argv[1]), cap = (u32)atoi(argv[2]);
  const size_t batch = (size_t)atoll(argv[3]);
  u64 seed = strtoull(argv[4], nullptr, 0);
  const size_t n = (size_t)1 << k;
  FrPlanDesc fwd, inv, invm;
  const Fr sc = fr_to_mont(fr_inv(fr_from_u64((u64)n))), scm = fr_to_mont(sc);
  if (!fr_build_plan(k, cap, false, nullptr, &fwd) || !fr_build_plan(k, cap, true, &sc, &inv) || !fr_build_plan(k, cap, true, &scm, &invm)) {
    printf("FAIL no plan\n");
    return 1;
  }
  // the table budget: no n-entry table from 2^20 up (checked here on whatever size runs: direct tables hold <= n / 16)
  for (auto& ps : fwd.passes) expect(ps.tw.size() <= (n >> FR_DIRECT_SHIFT) || ps.g.tw_mode != FR_TW_DIRECT, "table size", ps.tw.size(), n);

  // rows of arbitrary 256-bit integers, r, r + 1 and 2^256 - 1 among them
  Vec x(4 * n * batch);
  for (auto& w : x) w = splitmix(seed);
  const Fr rr = fr_mod_minus(0);
  Fr r1 = rr;
  r1.l[0] += 1;   // r is odd-limbed at the bottom (…0001): no carry
  for (size_t b = 0; b < batch; b++) {
    u64* row = x.data() + 4 * n * b;
    fr_store(row + 4 * ((0 + b) % n), rr);
    if (n > 1) fr_store(row + 4 * ((n / 2 + b) % n), r1);
    if (n > 2) for (int w = 0; w < 4; w++) row[4 * ((n - 1 - b) % n) + w] = ~(u64)0;
  }
  // naive DFT, on the reference arithmetic above (its own Montgomery product, not the library's)
  std::vector<Fr> W(n);
  {
    const Fr w = fr_root_of_unity_mont(k);
    Fr p = fr_const_one_mont();
    for (size_t t = 0; t < n; t++) { W[t] = p; p = fr_mul(p, w); }
    expect(fr_eq(p, fr_const_one_mont()), "omega^n", 0, 0);
    if (n > 1) expect(fr_eq(fr_from_mont(W[n / 2]), fr_mod_minus(1)), "omega^(n/2)", 0, 0);
  }
  ref_init();
  std::vector<F4> W4(n);
  for (size_t t = 0; t < n; t++) fr_store(W4[t].w, W[t]);
  Vec want(4 * n * batch), res(4 * n * batch);
  for (size_t b = 0; b < batch; b++) {
    std::vector<F4> c(n);
    for (size_t i = 0; i < n; i++) {
      fr_store(c[i].w, fr_canon(fr_load(x.data() + 4 * (n * b + i))));
      memcpy(res.data() + 4 * (n * b + i), c[i].w, 32);
    }
    naive_dft(c, W4, false, nullptr, want.data() + 4 * n * b);
  }
  Vec y(4 * n * batch, ~(u64)0);
  run_plan(fwd, x.data(), y.data(), batch);
  for (size_t i = 0; i < n * batch; i++) expect(memcmp(&y[4 * i], &want[4 * i], 32) == 0, "forward", i / n, i % n);
  run_plan(inv, y.data(), y.data(), batch);   // in place
  for (size_t i = 0; i < n * batch; i++) expect(memcmp(&y[4 * i], &res[4 * i], 32) == 0, "inverse of forward", i / n, i % n);
  // the inverse plan on the arbitrary rows themselves; the first row against (1/n) sum_i x[i] omega^(-i k)
  {
    run_plan(inv, x.data(), y.data(), batch);
    std::vector<F4> c(n);
    for (size_t i = 0; i < n; i++) memcpy(c[i].w, res.data() + 4 * i, 32);
    F4 ninv;
    fr_store(ninv.w, sc);
    Vec wi(4 * n);
    naive_dft(c, W4, true, &ninv, wi.data());
    for (size_t i = 0; i < n; i++) expect(memcmp(&y[4 * i], &wi[4 * i], 32) == 0, "inverse", 0, i);
  }

  // the multiply: d + d2 - 1 <= n
  {
    const size_t d = n >= 2 ? n / 2 : 1, d2 = n >= 2 ? n / 2 + 1 : 1, len = d + d2 - 1;
    Vec a(4 * d), b(4 * d2), ab(8 * n, ~(u64)0), prod(4 * n, ~(u64)0);
    for (auto& w : a) w = splitmix(seed);
    for (auto& w : b) w = splitmix(seed);
    for (int w = 0; w < 4; w++) b[w] = ~(u64)0;
    for (u64 i = 0; i < n; i++) { fr_pad_elem(a.data(), d, ab.data(), i); fr_pad_elem(b.data(), d2, ab.data() + 4 * n, i); }
    run_plan(fwd, ab.data(), ab.data(), 2);
    for (u64 i = 0; i < n; i++) fr_pointwise_elem(ab.data(), ab.data() + 4 * n, ab.data(), i);
    run_plan(invm, ab.data(), prod.data(), 1);
    std::vector<F4> acc(len, F4{{0, 0, 0, 0}}), ca(d);
    for (size_t i = 0; i < d; i++) fr_store(ca[i].w, fr_canon(fr_load(a.data() + 4 * i)));
    for (size_t j = 0; j < d2; j++) {
      F4 bm;
      fr_store(bm.w, fr_to_mont(fr_load(b.data() + 4 * j)));
      for (size_t i = 0; i < d; i++) acc[i + j] = ref_add(acc[i + j], ref_mul(ca[i], bm));
    }
    for (size_t i = 0; i < len; i++) expect(memcmp(acc[i].w, &prod[4 * i], 32) == 0, "product", i, len);
  }
  if (g_fail) { printf("FAIL %d mismatches\n", g_fail); return 1; }
  printf("OK log2n=%u passes=%zu rows=", k, fwd.passes.size());
  for (auto& ps : fwd.passes) printf("%u,", ps.g.logr);
  printf(" batch=%zu table_bytes=%zu\n", batch, fwd.table_bytes());
  return 0;
}
