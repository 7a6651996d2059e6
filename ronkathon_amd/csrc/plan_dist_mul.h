// plan_dist_mul.h -- the per-rank phases of the SHARDED polynomial multiply (ronk_dist.hip ronk_poly_mul_sharded_dev): plan.h's
// four-step phase builders (build_dist_phase1 / 2) with two options the transform does not have --
//   swapped  the other split of an odd log2n, R = 2^floor, C = 2^ceil: the multiply's inverse, whose input layout [R][C/W] is then
//            exactly the forward's output block [C][R/W] (r = k2, c = k1), so nothing is redistributed between the transforms;
//   batch    phase 2 over several polynomials n/W elements apart (the operand pair a, b: one receive buffer of 2 x n/W).
// With swapped = false and batch = 1 they build exactly what plan.h builds.  (A separate header rather than options of plan.h's
// builders: plan.h is one of the kernel sources whose hash the committed counter files record, bench.py KERNEL_SOURCES.)
#pragma once
#include "plan.h"

namespace ronk {

// swapped: the other split of an odd log2n, R = 2^floor, C = 2^ceil (the inverse of a sharded multiply, ronk_dist.hip: its input
// layout [R][C/W] is then exactly the forward's output block [C][R/W]; for an even log2n both splits are the same)
inline bool dist_shape_mul(int log2n, int world, DistShape* s, bool swapped) {
  int lw = 0;
  while ((1 << lw) < world) lw++;
  if ((1 << lw) != world) return false;
  s->log2n = log2n; s->logC = swapped ? log2n - log2n / 2 : log2n / 2; s->logR = log2n - s->logC; s->logW = lw;
  s->n = (u64)1 << log2n; s->R = (u64)1 << s->logR; s->C = (u64)1 << s->logC; s->W = (u64)world;
  if (s->logC < lw + 4 || s->logR > 24 || s->logC > 24) return false;  // >= 16 columns and rows per rank
  if (swapped && s->logR < lw + 4) return false;                        // (R <= C here: the rows need their own check)
  // two-pass phase 2 (logC > 12) splits the received row index at logC - logW - kb bits, kb = floor(logC/2)
  if (s->logC > 12 && s->logC - lw < s->logC / 2) return false;
  s->Rw = s->R / s->W; s->Cw = s->C / s->W;
  return true;
}

inline PlanDesc build_dist_mul_phase1(int log2n, bool inverse, int rank, int world, int max_logc = 4, int twf_max_log = 0,
                                  int chunk = 0, int chunks = 1, const HostField& hf = HostField(), bool swapped = false) {
  DistShape sh;
  PlanBuilder b;
  b.hf = hf;
  b.twf_max_log = twf_max_log;
  b.d.log2n = log2n; b.d.inverse = inverse;
  if (!dist_shape_mul(log2n, world, &sh, swapped) || !dist_chunks_ok(sh, chunks) || chunk < 0 || chunk >= chunks) return b.d;
  const u64 Cw = sh.Cw, Cwc = Cw / (u64)chunks;       // input row stride / columns of this chunk = output row stride
  const u64 g0 = (u64)rank * Cw + (u64)chunk * Cwc;   // global index of the chunk's first column
  const u64 scale = inverse ? hf.inv(sh.n % hf.p) : 1;   // folded into the global twiddle of phase 1
  // the launcher adds chunk*Cwc to the input pointer and chunk*R*Cwc to the output pointer (ronk_dist.hip)
  if (sh.logR <= 12) {
    PassDesc& p = b.add_pass(sh.logR, Cwc, max_logc);
    p.args.in_sj = (i64)Cw; p.args.in_sc = 1; p.args.out_sk = (i64)Cwc; p.args.out_sc = 1;
    p.tw_id = b.tw_table(log2n, scale);
    p.args.tw_log = log2n; p.args.tw_lo_bits = b.d.tw[p.tw_id].lo_bits;
    p.args.xc = 1; p.args.x0 = g0; p.args.yk = 1;            // omega_n^{(g0 + cl) * k1}
    p.in_buf = BUF_IN; p.out_buf = BUF_OUT;
    b.finish(p);
  } else {
    const int ka = (sh.logR + 1) / 2, kb = sh.logR - ka;
    const u64 A = (u64)1 << ka, B = (u64)1 << kb;
    {
      PassDesc& p = b.add_pass(ka, Cwc, max_logc);            // r = a*B + b: A-point over a, batch b; tmp is [R][Cwc]
      p.args.in_sj = (i64)(B * Cw); p.args.in_sc = 1; p.args.out_sk = (i64)(B * Cwc); p.args.out_sc = 1;
      p.args.nb2 = (u32)B; p.args.in_sb2 = (i64)Cw; p.args.out_sb2 = (i64)Cwc;
      p.tw_id = b.tw_table(sh.logR);
      p.args.tw_log = sh.logR; p.args.tw_lo_bits = b.d.tw[p.tw_id].lo_bits;
      p.args.xb2 = 1; p.args.yk = 1;                          // omega_R^{b * ka}
      p.in_buf = BUF_IN; p.out_buf = BUF_TMP;
      b.finish(p);
    }
    {
      PassDesc& p = b.add_pass(kb, Cwc, max_logc);            // B-point over b, batch ka; k1 = ka + A*kb
      p.args.in_sj = (i64)Cwc; p.args.in_sc = 1; p.args.out_sk = (i64)(A * Cwc); p.args.out_sc = 1;
      p.args.nb2 = (u32)A; p.args.in_sb2 = (i64)(B * Cwc); p.args.out_sb2 = (i64)Cwc;
      p.tw_id = b.tw_table(log2n, scale);
      p.args.tw_log = log2n; p.args.tw_lo_bits = b.d.tw[p.tw_id].lo_bits;
      p.args.xc = 1; p.args.x0 = g0; p.args.yk = A; p.args.yb2 = 1;   // omega_n^{c * (ka + A*kb)}
      p.in_buf = BUF_TMP; p.out_buf = BUF_OUT;
      b.finish(p);
    }
    b.d.needs_tmp = true;
  }
  return b.d;
}

inline PlanDesc build_dist_mul_phase2(int log2n, bool inverse, int rank, int world, int max_logc = 4, int twf_max_log = 0,
                                  int chunks = 1, const HostField& hf = HostField(), bool swapped = false, u32 batch = 1) {
  (void)rank;
  DistShape sh;
  PlanBuilder b;
  b.hf = hf;
  b.twf_max_log = twf_max_log;
  b.d.log2n = log2n; b.d.inverse = inverse;
  if (!dist_shape_mul(log2n, world, &sh, swapped) || !dist_chunks_ok(sh, chunks)) return b.d;
  const u64 Cw = sh.Cw, Rw = sh.Rw, C = sh.C, Cwc = Cw / (u64)chunks;
  int lcwc = 0; while (((u64)1 << lcwc) < Cwc) lcwc++;
  const u64 scale = 1;  // the inverse's n^-1 is applied by phase 1 (folded into its global twiddle)
  if (sh.logC <= 12) {
    PassDesc& p = b.add_pass(sh.logC, Rw, max_logc);          // columns = local rows k1, rows j = c (blocked)
    p.args.in_sc = (i64)Cwc; p.args.in_sj = 1;
    p.args.js_log = (u32)lcwc; p.args.in_sj_hi = (i64)(Rw * Cwc);
    p.args.out_sk = (i64)Rw; p.args.out_sc = 1;
    p.args.scale = scale;
    p.in_buf = BUF_IN; p.out_buf = BUF_OUT;
    b.finish(p);
  } else {
    const int ka = (sh.logC + 1) / 2, kb = sh.logC - ka;
    const u64 A2 = (u64)1 << ka, B2 = (u64)1 << kb;
    {
      PassDesc& p = b.add_pass(ka, B2, max_logc);             // c = a2*B2 + b2: A2-point over a2; batch k1
      p.args.in_sc = 1; p.args.in_sj = (i64)B2;
      p.args.js_log = (u32)(lcwc - kb); p.args.in_sj_hi = (i64)(Rw * Cwc);
      p.args.nb2 = (u32)Rw; p.args.in_sb2 = (i64)Cwc;
      p.args.out_sb2 = (i64)C; p.args.out_sk = (i64)B2; p.args.out_sc = 1;   // tmp: natural [k1][a2][b2]
      p.tw_id = b.tw_table(sh.logC);
      p.args.tw_log = sh.logC; p.args.tw_lo_bits = b.d.tw[p.tw_id].lo_bits;
      p.args.xc = 1; p.args.yk = 1;                           // omega_C^{b2 * ka2}
      p.in_buf = BUF_IN; p.out_buf = BUF_TMP;
      b.finish(p);
    }
    {
      PassDesc& p = b.add_pass(kb, Rw, max_logc);             // B2-point over b2; columns k1; batch ka2
      p.args.in_sc = (i64)C; p.args.in_sj = 1;
      p.args.nb2 = (u32)A2; p.args.in_sb2 = (i64)B2;
      p.args.out_sc = 1; p.args.out_sb2 = (i64)Rw; p.args.out_sk = (i64)(A2 * Rw);   // k2 = ka2 + A2*kb2
      p.args.scale = scale;
      p.in_buf = BUF_TMP; p.out_buf = BUF_OUT;
      b.finish(p);
    }
    b.d.needs_tmp = true;
  }
  // batch > 1 (the operand pair of a sharded multiply): polynomial b1 of every buffer -- receive buffer, scratch, output -- starts
  // b1 * n/W elements further on
  if (batch > 1) {
    b.d.batch = batch;
    for (auto& p : b.d.passes) {
      p.args.nb1 = batch;
      p.args.in_sb1 = p.args.out_sb1 = (i64)(sh.n / sh.W);
      p.grid = p.args.tiles * p.args.nb1 * p.args.nb2;
    }
  }
  return b.d;
}

}  // namespace ronk
