// bn254_san.cpp -- TEST INFRASTRUCTURE (make sanitize): csrc/bn254.h under ASan + UBSan on the host: field identities and
// the group law driven through every branch (infinity operands, P + P, P - P), order of the generator.
#include <stdio.h>

#include "../../ronkathon_amd/csrc/bn254.h"

using namespace bn254;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)

// raw 256-bit helpers (no reduction): the weakly reduced representatives the kernels work on
static Fp p_raw() { Fp r; for (int i = 0; i < 8; i++) r.l[i] = P_limb(i); return r; }
static Fp minus_one_raw() { Fp r; for (int i = 0; i < 8; i++) r.l[i] = 0xFFFFFFFFu; return r; }   // + (2^256 - 1) == - 1
static Fp raw_add(const Fp& a, const Fp& b) {
  Fp r; u64 c = 0;
  for (int i = 0; i < 8; i++) { const u64 t = (u64)a.l[i] + b.l[i] + c; r.l[i] = (u32)t; c = t >> 32; }
  return r;
}
static bool raw_eq(const Fp& a, const Fp& b) { for (int i = 0; i < 8; i++) if (a.l[i] != b.l[i]) return false; return true; }
static bool raw_less(const Fp& a, const Fp& b) {
  for (int i = 7; i >= 0; i--) if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
  return false;
}
// (X l^2, Y l^3, ZZ l^2, ZZZ l^3): the same point
static Xyzz scaled(const Xyzz& v, u32 l) {
  Fp lm = fp_zero(); lm.l[0] = l; lm = fp_to_mont(lm);
  const Fp l2 = fp_sqr(lm), l3 = fp_mul(l2, lm);
  Xyzz r;
  r.X = fp_mul(v.X, l2); r.Y = fp_mul(v.Y, l3); r.ZZ = fp_mul(v.ZZ, l2); r.ZZZ = fp_mul(v.ZZZ, l3);
  return r;
}

int main() {
  // field: (a*b) * b^-1 == a, a - a == 0, a + (p - a) == 0 for a few values incl. the edges
  u64 seed = 0x9E3779B97F4A7C15ull;
  for (int it = 0; it < 50; it++) {
    Fp a, b;
    for (int i = 0; i < 8; i++) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; a.l[i] = (u32)(seed >> 32); seed = seed * 6364136223846793005ull + 1; b.l[i] = (u32)(seed >> 33); }
    a.l[7] &= 0x1FFFFFFF; b.l[7] &= 0x1FFFFFFF;   // < 2^253 < p
    if (it == 0) { a = fp_zero(); a.l[0] = 1; }
    if (it == 1) { for (int i = 0; i < 8; i++) a.l[i] = P_limb(i); a.l[0] -= 1; }   // p - 1
    if (fp_is_zero_exact(b)) b.l[0] = 7;
    const Fp am = fp_to_mont(a), bm = fp_to_mont(b);
    CHECK(fp_eq(fp_from_mont(fp_mul(fp_mul(am, bm), fp_inv(bm))), a));
    CHECK(fp_is_zero(fp_sub(am, am)));
    CHECK(fp_is_zero(fp_add(am, fp_neg(am))));
    CHECK(fp_eq(fp_sqr(am), fp_mul(am, am)));
  }
  // group: G = (1, 2); r * G == infinity, (r - 1) * G == -G, branches of madd / add / dbl
  Affine g;
  g.x = fp_zero(); g.x.l[0] = 1; g.y = fp_zero(); g.y.l[0] = 2;
  g.x = fp_to_mont(g.x); g.y = fp_to_mont(g.y);
  CHECK(affine_on_curve(g));
  const u64 r[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};   // group order
  Xyzz acc = xyzz_inf();
  for (int i = 255; i >= 0; i--) { acc = xyzz_dbl(acc); if ((r[i >> 6] >> (i & 63)) & 1) xyzz_madd(acc, g, false); }
  CHECK(xyzz_is_inf(acc));
  Xyzz two = xyzz_inf();
  xyzz_madd(two, g, false); xyzz_madd(two, g, false);            // P + P inside the mixed addition
  u64 out[8];
  xyzz_store_affine(two, out);
  CHECK(out[0] != 0 || out[4] != 0);                             // an affine point, not infinity
  Xyzz z = two;
  Affine ng = g; ng.y = fp_neg(g.y);
  xyzz_madd(z, ng, false); xyzz_madd(z, g, true);                // 2G - G - G
  CHECK(xyzz_is_inf(z));
  CHECK(xyzz_is_inf(xyzz_add(two, xyzz_inf())) == false && xyzz_is_inf(xyzz_add(xyzz_inf(), xyzz_inf())));
  Xyzz four_a = xyzz_dbl(two), four_b = xyzz_add(two, two);      // dbl vs add's equal-operand branch
  u64 oa[8], ob[8];
  xyzz_store_affine(four_a, oa); xyzz_store_affine(four_b, ob);
  for (int i = 0; i < 8; i++) CHECK(oa[i] == ob[i]);
  // raw, weakly reduced operands: every representative below 2p must act as its residue (the kernels never canonicalise
  // between operations), results stay below 2p, and the zero tests accept 0 and p
  {
    const Fp pm1 = raw_add(p_raw(), minus_one_raw()), two_p_m1 = raw_add(raw_add(p_raw(), p_raw()), minus_one_raw());
    Fp one = fp_zero(); one.l[0] = 1;
    Fp low7 = fp_zero(); for (int i = 0; i < 7; i++) low7.l[i] = 0xFFFFFFFFu; low7.l[7] = P2_limb(7) - 1;
    const Fp edge[] = {fp_zero(), one, pm1, p_raw(), raw_add(p_raw(), one), two_p_m1, fp_const_one(), fp_const_r2(), low7,
                       raw_add(fp_const_one(), p_raw()), raw_add(fp_const_r2(), p_raw())};
    const int ne = (int)(sizeof edge / sizeof edge[0]);
    for (int i = 0; i < ne; i++) {
      const Fp a = edge[i], ac = fp_canon(a);
      CHECK(raw_less(a, raw_add(p_raw(), p_raw())) && !fp_geq_p(ac));
      CHECK(fp_is_zero(a) == fp_is_zero_exact(ac));
      CHECK(raw_eq(fp_canon(fp_neg(a)), fp_canon(fp_neg(ac))));
      for (int j = 0; j < ne; j++) {
        const Fp b = edge[j], bc = fp_canon(b);
        const Fp m = fp_mul(a, b), s = fp_add(a, b), d = fp_sub(a, b);
        CHECK(raw_less(m, raw_add(p_raw(), p_raw())) && raw_less(s, raw_add(p_raw(), p_raw())) && raw_less(d, raw_add(p_raw(), p_raw())));
        CHECK(raw_eq(fp_canon(m), fp_canon(fp_mul(ac, bc))));
        CHECK(raw_eq(fp_canon(s), fp_canon(fp_add(ac, bc))));
        CHECK(raw_eq(fp_canon(d), fp_canon(fp_sub(ac, bc))));
      }
    }
  }
  // one addition P + P whose operands differ in scaling and in the representative of X and ZZ: U2 - U1 comes out as exactly
  // 0, as p (U2 = U1 + p) and as p through fp_sub's borrow branch (U2 = U1 - p); each time the result must be 2P
  {
    int seen[3] = {0, 0, 0};
    u64 want[8], got[8];
    xyzz_store_affine(four_a, want);                               // 2 * (2G)
    for (u32 l1 = 1; l1 < 12; l1++)
      for (u32 l2 = 1; l2 < 12; l2++)
        for (int mask = 0; mask < 16; mask++) {
          Xyzz a = scaled(two, l1), b = scaled(two, l2);
          if (mask & 1) a.X = raw_add(a.X, p_raw());
          if (mask & 2) a.ZZ = raw_add(a.ZZ, p_raw());
          if (mask & 4) b.X = raw_add(b.X, p_raw());
          if (mask & 8) b.ZZ = raw_add(b.ZZ, p_raw());
          const Fp U1 = fp_mul(a.X, b.ZZ), U2 = fp_mul(b.X, a.ZZ);
          const int cls = raw_eq(U1, U2) ? 0 : raw_less(U1, U2) ? 1 : 2;
          CHECK(fp_is_zero(fp_sub(U2, U1)));
          if (seen[cls]++ >= 8) continue;                          // a few of each class through the whole addition
          const Xyzz r = xyzz_add(a, b);
          xyzz_store_affine(r, got);
          for (int i = 0; i < 8; i++) CHECK(got[i] == want[i]);
          CHECK(fp_eq(fp_mul(fp_sqr(r.ZZ), r.ZZ), fp_sqr(r.ZZZ)));
        }
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0);
  }
  printf(fails ? "bn254 sanitize run: %d failure(s)\n" : "bn254 sanitize run ok\n", fails);
  return fails ? 1 : 0;
}
