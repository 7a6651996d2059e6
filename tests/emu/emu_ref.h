// emu_ref.h -- what the host emulators of the field-policy families share: the SplitMix64 draws, the failure count, and the plain
// `unsigned __int128 % p` restatement of the base field and of its quadratic extension F_p[t] / (t^2 - w) that the kernel bodies
// are compared with.  Test infrastructure only; never part of the product library.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef uint64_t u64;
typedef unsigned __int128 u128;

static u64 g_rng;
static inline u64 rnd() {   // SplitMix64
  u64 z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
[[maybe_unused]] static int g_fail = 0;   // the restatement alone (emu_poseidon.cpp as a library) checks nothing
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 10) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---------------------------------------------------------------------------------------------------- the base field; a, b < p
static inline u64 r_mul(u64 a, u64 b, u64 p) { return (u64)(((u128)a * b) % p); }
static inline u64 r_add(u64 a, u64 b, u64 p) { const u128 s = (u128)a + b; return (u64)(s >= p ? s - p : s); }
static inline u64 r_sub(u64 a, u64 b, u64 p) { return a >= b ? a - b : a + (p - b); }
static inline u64 r_pow(u64 a, u64 e, u64 p) {
  u64 r = 1 % p;
  while (e) { if (e & 1) r = r_mul(r, a, p); a = r_mul(a, a, p); e >>= 1; }
  return r;
}
// The directed mode (tests/test_emu_gl_directed.py): with RONK_EMU_SMALL=B in the environment every input word is SMALL SIGNED,
// t mod p for t uniform in [-B, B], and so is every challenge drawn through challenge_word; sums and products of such words
// land in [p, 2^64) all the time, which uniform residues never do.  Unset, every draw is what it was.
static inline u64 emu_small() {
  static long b = -1;
  if (b < 0) { const char* e = getenv("RONK_EMU_SMALL"); b = e ? atol(e) : 0; }
  return (u64)b;
}
static inline u64 small_word(u64 p, u64 B) { const u64 r = rnd() % (2 * B + 1); return r <= B ? r : p - (r - B); }
// an input word: p - 1, 0, a word just above p, or any word
static inline u64 edge_word(u64 p) {
  if (emu_small()) return small_word(p, emu_small());
  const u64 c = rnd() % 8;
  return c == 0 ? p - 1 : c == 1 ? 0 : c == 2 && p < ~(u64)0 - 5 ? p + rnd() % 5 : rnd();
}
// a challenge: any residue
static inline u64 challenge_word(u64 p) { return emu_small() ? small_word(p, emu_small()) : rnd() % p; }

// ---------------------------------------------------------------------------------------------------- the extension
struct R2 { u64 c0, c1; };
static inline bool operator==(R2 a, R2 b) { return a.c0 == b.c0 && a.c1 == b.c1; }
static inline R2 x_add(R2 a, R2 b, u64 p) { return R2{r_add(a.c0, b.c0, p), r_add(a.c1, b.c1, p)}; }
static inline R2 x_sub(R2 a, R2 b, u64 p) { return R2{r_sub(a.c0, b.c0, p), r_sub(a.c1, b.c1, p)}; }
static inline R2 x_scale(R2 a, u64 s, u64 p) { return R2{r_mul(a.c0, s, p), r_mul(a.c1, s, p)}; }
// schoolbook, reduced modulo t^2 - w
static inline R2 x_mul(R2 a, R2 b, u64 w, u64 p) {
  return R2{r_add(r_mul(a.c0, b.c0, p), r_mul(w, r_mul(a.c1, b.c1, p), p), p), r_add(r_mul(a.c0, b.c1, p), r_mul(a.c1, b.c0, p), p)};
}
// (a0, -a1) / norm; zero for the zero element
static inline R2 x_inv(R2 a, u64 w, u64 p) {
  const u64 n = r_sub(r_mul(a.c0, a.c0, p), r_mul(w, r_mul(a.c1, a.c1, p), p), p);
  return x_scale(R2{a.c0, r_sub(0, a.c1, p)}, r_pow(n, p - 2, p), p);
}
static inline R2 red(R2 a, u64 p) { return R2{a.c0 % p, a.c1 % p}; }
