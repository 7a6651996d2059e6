// bn254_probe.h -- TEST HOOK: one function of bn254.h applied to RAW limbs (no form conversion, no canonicalisation), so
// that a test can hand the field and group arithmetic any representative in [0, 2p) and read back exactly what the code
// produced.  Shared by the device probe (ronk_bn254_probe_dev, ronk_msm.hip: the only way to reach the inline assembly of
// acc_mad / acc_mad2 with chosen operands) and by its host twin (tests/emu/bn254_host.cpp, which runs the __int128
// fallback on the same vectors).  Nothing on the MSM's own path includes this file.
#pragma once
#include "bn254.h"

namespace bn254 {

// field ops: a, b, out are 4 words (b ignored by the unary ones); predicates write 1 word
// point ops: a point is 16 words (X, Y, ZZ, ZZZ), the affine operand of madd / on_curve 8 words (x, y); out 16 words, or 1
enum ProbeOp {
  PROBE_FP_MUL = 0, PROBE_FP_ADD = 1, PROBE_FP_SUB = 2, PROBE_FP_NEG = 3, PROBE_FP_CANON = 4, PROBE_FP_TO_MONT = 5,
  PROBE_FP_FROM_MONT = 6, PROBE_FP_IS_ZERO = 7, PROBE_FP_IS_ZERO_EXACT = 8, PROBE_FP_GEQ_P = 9,
  PROBE_XYZZ_ADD = 16, PROBE_XYZZ_DBL = 17, PROBE_XYZZ_MADD = 18, PROBE_XYZZ_MADD_NEG = 19, PROBE_ON_CURVE = 20
};

struct ProbeShape { int wa, wb, wo; };   // words per element of a, b (0: unused), out; wo == 0: unknown op
RONK_HD ProbeShape probe_shape(int op) {
  ProbeShape s = {0, 0, 0};
  switch (op) {
    case PROBE_FP_MUL: case PROBE_FP_ADD: case PROBE_FP_SUB: s = {4, 4, 4}; break;
    case PROBE_FP_NEG: case PROBE_FP_CANON: case PROBE_FP_TO_MONT: case PROBE_FP_FROM_MONT: s = {4, 0, 4}; break;
    case PROBE_FP_IS_ZERO: case PROBE_FP_IS_ZERO_EXACT: case PROBE_FP_GEQ_P: s = {4, 0, 1}; break;
    case PROBE_XYZZ_ADD: s = {16, 16, 16}; break;
    case PROBE_XYZZ_DBL: s = {16, 0, 16}; break;
    case PROBE_XYZZ_MADD: case PROBE_XYZZ_MADD_NEG: s = {16, 8, 16}; break;
    case PROBE_ON_CURVE: s = {8, 0, 1}; break;
    default: break;
  }
  return s;
}

RONK_HD Xyzz probe_load_xyzz(const u64* w) {
  Xyzz p;
  p.X = fp_load(w); p.Y = fp_load(w + 4); p.ZZ = fp_load(w + 8); p.ZZZ = fp_load(w + 12);
  return p;
}
RONK_HD void probe_store_xyzz(u64* w, const Xyzz& p) {
  fp_store(w, p.X); fp_store(w + 4, p.Y); fp_store(w + 8, p.ZZ); fp_store(w + 12, p.ZZZ);
}

// one element: a, b, out point at this element's words
template <int OP>
RONK_HD void probe_apply(const u64* a, const u64* b, u64* out) {
  if (OP == PROBE_FP_MUL) fp_store(out, fp_mul(fp_load(a), fp_load(b)));
  else if (OP == PROBE_FP_ADD) fp_store(out, fp_add(fp_load(a), fp_load(b)));
  else if (OP == PROBE_FP_SUB) fp_store(out, fp_sub(fp_load(a), fp_load(b)));
  else if (OP == PROBE_FP_NEG) fp_store(out, fp_neg(fp_load(a)));
  else if (OP == PROBE_FP_CANON) fp_store(out, fp_canon(fp_load(a)));
  else if (OP == PROBE_FP_TO_MONT) fp_store(out, fp_to_mont(fp_load(a)));
  else if (OP == PROBE_FP_FROM_MONT) fp_store(out, fp_from_mont(fp_load(a)));
  else if (OP == PROBE_FP_IS_ZERO) out[0] = fp_is_zero(fp_load(a)) ? 1 : 0;
  else if (OP == PROBE_FP_IS_ZERO_EXACT) out[0] = fp_is_zero_exact(fp_load(a)) ? 1 : 0;
  else if (OP == PROBE_FP_GEQ_P) out[0] = fp_geq_p(fp_load(a)) ? 1 : 0;
  else if (OP == PROBE_XYZZ_ADD) probe_store_xyzz(out, xyzz_add(probe_load_xyzz(a), probe_load_xyzz(b)));
  else if (OP == PROBE_XYZZ_DBL) probe_store_xyzz(out, xyzz_dbl(probe_load_xyzz(a)));
  else if (OP == PROBE_XYZZ_MADD || OP == PROBE_XYZZ_MADD_NEG) {
    Xyzz acc = probe_load_xyzz(a);
    Affine q;
    q.x = fp_load(b); q.y = fp_load(b + 4);
    xyzz_madd(acc, q, OP == PROBE_XYZZ_MADD_NEG);
    probe_store_xyzz(out, acc);
  } else if (OP == PROBE_ON_CURVE) {
    Affine q;
    q.x = fp_load(a); q.y = fp_load(a + 4);
    out[0] = affine_on_curve(q) ? 1 : 0;
  }
}

// run X(OP) for the compile-time constant matching `op` (a known one: probe_shape(op).wo != 0)
#define BN254_PROBE_DISPATCH(op, X)                                                                                    \
  switch (op) {                                                                                                        \
    case bn254::PROBE_FP_MUL: X(bn254::PROBE_FP_MUL); break;                                                           \
    case bn254::PROBE_FP_ADD: X(bn254::PROBE_FP_ADD); break;                                                           \
    case bn254::PROBE_FP_SUB: X(bn254::PROBE_FP_SUB); break;                                                           \
    case bn254::PROBE_FP_NEG: X(bn254::PROBE_FP_NEG); break;                                                           \
    case bn254::PROBE_FP_CANON: X(bn254::PROBE_FP_CANON); break;                                                       \
    case bn254::PROBE_FP_TO_MONT: X(bn254::PROBE_FP_TO_MONT); break;                                                   \
    case bn254::PROBE_FP_FROM_MONT: X(bn254::PROBE_FP_FROM_MONT); break;                                               \
    case bn254::PROBE_FP_IS_ZERO: X(bn254::PROBE_FP_IS_ZERO); break;                                                   \
    case bn254::PROBE_FP_IS_ZERO_EXACT: X(bn254::PROBE_FP_IS_ZERO_EXACT); break;                                       \
    case bn254::PROBE_FP_GEQ_P: X(bn254::PROBE_FP_GEQ_P); break;                                                       \
    case bn254::PROBE_XYZZ_ADD: X(bn254::PROBE_XYZZ_ADD); break;                                                       \
    case bn254::PROBE_XYZZ_DBL: X(bn254::PROBE_XYZZ_DBL); break;                                                       \
    case bn254::PROBE_XYZZ_MADD: X(bn254::PROBE_XYZZ_MADD); break;                                                     \
    case bn254::PROBE_XYZZ_MADD_NEG: X(bn254::PROBE_XYZZ_MADD_NEG); break;                                             \
    case bn254::PROBE_ON_CURVE: X(bn254::PROBE_ON_CURVE); break;                                                       \
    default: break;                                                                                                    \
  }

}  // namespace bn254
