// emu_sharded_mul.cpp -- HOST EMULATOR of the sharded polynomial multiply (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_emu_sharded_mul.py).  All W ranks in one process, the two exchanges as memcpy, the per-rank passes as the very same
// tile bodies the library launches (ntt_tile.h; the fused middle = ntt_mul.h mul_mid_body with the dist instantiation's template
// arguments) on ucontext fibers, one per work-item, barrier = yield.  Checks every coefficient against the oracle's NTT product,
// and that the swapped-split index maps put the forward's output block exactly where the inverse reads it.
//
// usage: emu_sharded_mul <log2n> <world> <chunks> <fused 0|1>      (RONK_EMU_P / RONK_EMU_G: a Montgomery prime)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <functional>
#include <vector>

#include "../../oracle/ronk_oracle.h"
#include "../../ronkathon_amd/csrc/ntt_mul.h"
#include "../../ronkathon_amd/csrc/plan_dist_mul.h"

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

static u64 g_p = gl64::P, g_g = gl64::GENERATOR;
static bool g_mont = false;
static HostField g_hf;

static u64 splitmix(u64& s) {
  s += 0x9E3779B97F4A7C15ull;
  u64 z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static u64 rnd_elem(u64& s) {
  if (g_p < ((u64)1 << 63)) return splitmix(s) % g_p;
  u64 v; do v = splitmix(s); while (v >= g_p); return v;
}

static TileArgs bind_pass(const PlanDesc& pd, size_t idx, const u64* in, const u64* in2, u64* out, u64* tmp) {
  const PassDesc& p = pd.passes[idx];
  TileArgs a = p.args;
  const u64* bufs_in[3] = {in, out, tmp};
  u64* bufs_out[3] = {nullptr, out, tmp};
  a.in = bufs_in[p.in_buf];
  a.in2 = p.in_buf == BUF_IN ? in2 : nullptr;
  a.out = bufs_out[p.out_buf];
  a.wr = pd.wr[p.wr_id].data();
  if (p.tw_id >= 0) { a.tw_lo = pd.tw[p.tw_id].lo.data(); a.tw_hi = pd.tw[p.tw_id].hi.data(); }
  if (p.twf_id >= 0) a.tw_full = pd.twf[p.twf_id].data();
  return a;
}

template <int LR, bool INV, class FLD>
static void generic(const TileArgs& a, u64* lds, u32 tid, u32 bid) { tile_body<LR, INV, 0, TileCfg<-1, 0>, FLD>(a, lds, tid, bid, fiber_barrier); }
template <bool INV, class FLD>
static void generic_any(int logr, const TileArgs& a, u64* lds, u32 tid, u32 bid) {
  switch (logr) {
    case 4: generic<4, INV, FLD>(a, lds, tid, bid); break;
    case 5: generic<5, INV, FLD>(a, lds, tid, bid); break;
    case 6: generic<6, INV, FLD>(a, lds, tid, bid); break;
    case 7: generic<7, INV, FLD>(a, lds, tid, bid); break;
    case 8: generic<8, INV, FLD>(a, lds, tid, bid); break;
    case 9: generic<9, INV, FLD>(a, lds, tid, bid); break;
    case 10: generic<10, INV, FLD>(a, lds, tid, bid); break;
    default: abort();
  }
}
// every pass of a plan with the generic body (the library's specialised kernels are checked by tests/emu/emu_tile.cpp)
// x0_add: the chunk's column offset (CompiledPlan::launch)
static void run_plan(const PlanDesc& pd, const u64* in, const u64* in2, u64* out, u64* tmp, u64 x0_add = 0) {
  std::vector<u64> lds;
  for (size_t i = 0; i < pd.passes.size(); i++) {
    const PassDesc& p = pd.passes[i];
    TileArgs a = bind_pass(pd, i, in, in2, out, tmp);
    if (x0_add && a.tw_log && a.xc) a.x0 += x0_add * a.xc;
    lds.assign(p.lds_bytes / 8 + 1, 0);
    for (u32 bid = 0; bid < p.grid; bid++) {
      g_body = [&](u32 tid) {
        if (g_mont) { if (pd.inverse) generic_any<true, MontField>(p.logr, a, lds.data(), tid, bid); else generic_any<false, MontField>(p.logr, a, lds.data(), tid, bid); }
        else if (pd.inverse) generic_any<true, GlField>(p.logr, a, lds.data(), tid, bid); else generic_any<false, GlField>(p.logr, a, lds.data(), tid, bid);
      };
      run_block(p.block);
    }
  }
}

template <int LR, int LC>
static void mid(const TileArgs& fa, const TileArgs& ia, u64* lds, u32 tid, u32 bid) {
  if (g_mont) mul_mid_body<LR, LC, 4, MontField>(fa, ia, lds, tid, bid, fiber_barrier);
  else mul_mid_body<LR, LC, 4, GlField>(fa, ia, lds, tid, bid, fiber_barrier);
}

int main(int argc, char** argv) {
  if (argc < 5) { printf("usage: emu_sharded_mul <log2n> <world> <chunks> <fused 0|1>\n"); return 2; }
  if (const char* e = getenv("RONK_EMU_P")) {
    g_p = strtoull(e, 0, 0);
    g_g = getenv("RONK_EMU_G") ? strtoull(getenv("RONK_EMU_G"), 0, 0) : 0;
    if (!g_g && orc_find_primitive_element(g_p, &g_g)) { printf("no generator\n"); return 2; }
    g_mont = true;
    g_hf = HostField::montgomery(g_p, g_g);
  }
  const int log2n = atoi(argv[1]), W = atoi(argv[2]), chunks = atoi(argv[3]);
  const bool want_fused = atoi(argv[4]) != 0;
  DistShape sh, ish;
  if (!dist_shape(log2n, W, &sh) || !dist_shape_mul(log2n, W, &ish, true) || !dist_chunks_ok(sh, chunks) || !dist_chunks_ok(ish, chunks)) {
    printf("bad shape\n");
    return 2;
  }
  const u64 n = sh.n, per = n / sh.W, Cwc = sh.Cw / chunks, cc = ish.Cw / chunks, blk = sh.Rw * Cwc, blk2 = ish.Rw * cc;

  // the layout argument: forward rank h's output element (k2, k1l) = X[(h*Rw + k1l) + R*k2] sits at k2*Rw + k1l; the swapped
  // inverse's rank h reads its input element (r', c'l) = X'[r'*C' + h*Cw' + c'l] at r'*Cw' + c'l -- the same element must be there
  if (ish.R != sh.C || ish.C != sh.R || ish.Cw != sh.Rw) { printf("LAYOUT MISMATCH (shape)\n"); return 1; }
  for (int h = 0; h < W; h++)
    for (u64 k2 = 0; k2 < sh.C; k2++)
      for (u64 k1l = 0; k1l < sh.Rw; k1l += 7) {
        const u64 fwd_pos = k2 * sh.Rw + k1l, fwd_idx = (h * sh.Rw + k1l) + sh.R * k2;
        const u64 r = fwd_pos / ish.Cw, cl = fwd_pos % ish.Cw, inv_idx = r * ish.C + h * ish.Cw + cl;
        if (inv_idx != fwd_idx) { printf("LAYOUT MISMATCH at rank %d k2=%llu k1l=%llu\n", h, (unsigned long long)k2, (unsigned long long)k1l); return 1; }
      }

  std::vector<u64> a(n), b(n), got(n);
  u64 s = 0x5EED0D00ull + log2n * 16 + W;
  for (u64 i = 0; i < n; i++) { a[i] = rnd_elem(s); b[i] = rnd_elem(s); }
  a[0] = g_p - 1; b[n - 1] = g_p - 1;
  std::vector<std::vector<u64>> loc(W), snd(W), rcv(W), tmp(W), spec(W), snd2(W), rcv2(W), res(W);
  std::vector<PlanDesc> p1(W), p2(W), q1(W), q2(W);
  bool fused = want_fused;
  for (int g = 0; g < W; g++) {
    loc[g].resize(2 * per); snd[g].assign(2 * per, 1); rcv[g].assign(2 * per, 2); tmp[g].assign(2 * per, 3); spec[g].assign(2 * per, 4);
    snd2[g].assign(per, 5); rcv2[g].assign(per, 6); res[g].assign(per, 7);
    for (u64 r = 0; r < sh.R; r++)
      for (u64 cl = 0; cl < sh.Cw; cl++) {
        loc[g][r * sh.Cw + cl] = a[r * sh.C + g * sh.Cw + cl];
        loc[g][per + r * sh.Cw + cl] = b[r * sh.C + g * sh.Cw + cl];
      }
    p1[g] = build_dist_phase1(log2n, false, g, W, 4, 0, 0, chunks, g_hf);
    p2[g] = build_dist_mul_phase2(log2n, false, g, W, 4, 0, chunks, g_hf, false, 2);
    q1[g] = build_dist_mul_phase1(log2n, true, g, W, 4, 0, 0, chunks, g_hf, true);
    q2[g] = build_dist_mul_phase2(log2n, true, g, W, 4, 0, chunks, g_hf, true);
    if (p1[g].passes.empty() || p2[g].passes.empty() || q1[g].passes.empty() || q2[g].passes.empty()) { printf("no plan\n"); return 2; }
    fused = fused && p2[g].passes.size() == 1 && q1[g].passes.size() == 1;
  }
  // forward phase 1 of a and b, first exchange
  for (int g = 0; g < W; g++)
    for (int j = 0; j < chunks; j++)
      for (int b1 = 0; b1 < 2; b1++)
        run_plan(p1[g], loc[g].data() + b1 * per + j * Cwc, nullptr, snd[g].data() + b1 * per + j * sh.R * Cwc, tmp[g].data(), j * Cwc);
  for (int g = 0; g < W; g++)
    for (int j = 0; j < chunks; j++)
      for (int h = 0; h < W; h++)
        for (int b1 = 0; b1 < 2; b1++)
          memcpy(&rcv[h][b1 * per + ((u64)g * chunks + j) * blk], &snd[g][b1 * per + j * sh.R * Cwc + h * blk], blk * 8);
  // the middle, per inverse column chunk
  int fused_tiles = 0;
  for (int h = 0; h < W; h++) {
    if (!fused) run_plan(p2[h], rcv[h].data(), nullptr, spec[h].data(), tmp[h].data());
    for (int j = 0; j < chunks; j++) {
      if (!fused) {
        run_plan(q1[h], spec[h].data() + j * cc, spec[h].data() + per + j * cc, snd2[h].data() + j * ish.R * cc, tmp[h].data(), j * cc);
        continue;
      }
      // ronk_dist.hip mul_mid_args
      TileArgs fa = bind_pass(p2[h], 0, rcv[h].data(), nullptr, nullptr, tmp[h].data());
      TileArgs ia = bind_pass(q1[h], 0, nullptr, nullptr, snd2[h].data(), tmp[h].data());
      fa.in += (i64)(j * cc) * fa.in_sc;
      fa.ncols = cc;
      fa.tiles = (u32)(cc >> fa.logc);
      ia.x0 += j * cc * ia.xc;
      ia.out += j * ish.R * cc;
      const PassDesc& fp = p2[h].passes[0];
      if (!mul_mid_matches_dist(fa, ia, fp.logr, (int)fa.logc)) { printf("passes do not fuse (logr %d logc %u)\n", fp.logr, fa.logc); return 2; }
      std::vector<u64> lds(fp.lds_bytes / 8 + 1, 0);
      for (u32 bid = 0; bid < fa.tiles; bid++) {
        g_body = [&](u32 tid) {
          const int lr = fp.logr, lc = (int)fa.logc;
          if (lr == 9 && lc == 4) mid<9, 4>(fa, ia, lds.data(), tid, bid);
          else if (lr == 10 && lc == 4) mid<10, 4>(fa, ia, lds.data(), tid, bid);
          else if (lr == 11 && lc == 3) mid<11, 3>(fa, ia, lds.data(), tid, bid);
          else if (lr == 12 && lc == 2) mid<12, 2>(fa, ia, lds.data(), tid, bid);
          else abort();
        };
        run_block(fp.block);
        fused_tiles++;
      }
    }
  }
  // second exchange, inverse phase 2
  for (int g = 0; g < W; g++)
    for (int j = 0; j < chunks; j++)
      for (int h = 0; h < W; h++)
        memcpy(&rcv2[h][((u64)g * chunks + j) * blk2], &snd2[g][j * ish.R * cc + h * blk2], blk2 * 8);
  for (int h = 0; h < W; h++) {
    run_plan(q2[h], rcv2[h].data(), nullptr, res[h].data(), tmp[h].data());
    for (u64 r = 0; r < sh.R; r++)   // the product in the operands' layout: [R][C/W] column block of rank h
      for (u64 cl = 0; cl < sh.Cw; cl++) got[r * sh.C + h * sh.Cw + cl] = res[h][r * sh.Cw + cl];
  }
  std::vector<u64> fa_(n), fb_(n), ref(n);
  if (orc_fft(g_p, g_g, a.data(), fa_.data(), n) || orc_fft(g_p, g_g, b.data(), fb_.data(), n)) return 1;
  for (u64 i = 0; i < n; i++) fa_[i] = orc_mul(g_p, fa_[i], fb_[i]);
  if (orc_ifft(g_p, g_g, fa_.data(), ref.data(), n)) return 1;
  for (u64 i = 0; i < n; i++)
    if (got[i] != ref[i]) { printf("SHARDED MUL MISMATCH at %llu: got %llu want %llu\n", (unsigned long long)i, (unsigned long long)got[i], (unsigned long long)ref[i]); return 1; }
  printf("OK sharded mul log2n=%d world=%d chunks=%d middle=%s fused_tiles=%d\n", log2n, W, chunks, fused ? "fused" : "composed", fused_tiles);
  return 0;
}
