// pow_kernels.h -- proof-of-work grinding on the Poseidon sponge (csrc/ronk_pow.hip, csrc/ronk_fri.hip; include/ronk_ntt.h
// "proof of work"): the smallest nonce n < 2^log2_limit for which the first word of the one-shot
// sponge(seed || [n]) has its low `bits` bits zero.
//
// The item seed || [n] has seed_len + 1 words, so the sponge absorbs floor(seed_len / rate) + 1 chunks and only the last one holds
// the nonce.  Everything before the nonce is the same for every candidate: the PREFIX runs the floor(seed_len / rate) seed-only
// permutations and adds the seed_len mod rate words that share the last chunk, once, in one lane, and leaves the state in
// register form.  A candidate is then a copy of that state, one addition at slot 1 + seed_len mod rate, ONE permutation and a
// mask of internal[1], the sponge's first output (poseidon_kernels.h: internal[1 .. rate] are the rate elements).  No memory is
// read per candidate but the found word, and nothing is written except by a hit.
//
// The search: T lanes, lane g tries n = g, g + T, g + 2 T, ... in increasing order.  Before each candidate it loads the found
// word (2^64 - 1 until a hit) and stops when n >= found or n >= 2^log2_limit; a hit lowers the found word to n by a 64-bit
// atomic minimum, and the lane stops at its next check.  The result is the global minimum whatever the order in which lanes run: let n* be the smallest
// solution.  The found word only ever holds 2^64 - 1 or a solution, so it is never below n*.  The lane g* = n* mod T meets only
// non-solutions below n* on its way (they are smaller than n*, hence smaller than every value the found word takes, and below the
// limit), so it is never stopped before n*, reaches it, and writes it; nothing smaller is ever written, and a minimum is never
// undone.  Without a solution below the limit no lane writes and the word stays 2^64 - 1.  No lane waits for another.
//
// Plain C++ on uint32 / uint64, so tests/emu/emu_pow.cpp compiles the same bodies for the host.
#pragma once
#include "poseidon_kernels.h"

namespace ronk {

static constexpr u64 POW_NONE = ~(u64)0;        // the nonce word of a search that found nothing
static constexpr u32 POW_MAX_BITS = 40;         // bits and log2_limit
static constexpr u32 POW_MAX_SEED = 4096;       // seed words
static constexpr u32 POW_WORK_WORDS = 16;       // the prefix state, W <= 16 words in register form

// the slot of the nonce in the internal layout
RONK_HD u32 pow_slot(u32 seed_len, u32 rate) { return 1 + seed_len % rate; }

// One lane: state0[0 .. W) = the sponge's state, register form, after every seed word is absorbed and before the nonce is;
// *nonce = POW_NONE.  seed: any 64-bit words.
template <class PF, int W>
RONK_HD void pow_prefix(const PF& pf, const PoseidonConsts& k, u32 seed_len, const u64* seed, u64* state0, u64* nonce) {
  u64 s[W];
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = 0;
  const u32 rate = k.rate, chunks = seed_len / rate + 1;
  for (u32 t = 0; t < chunks; t++) {
    const u32 base = t * rate;
#pragma unroll
    for (int i = 0; i < W - 1; i++)
      if ((u32)i < rate && base + i < seed_len) s[1 + i] = pf.add(s[1 + i], pf.in(seed[base + i]));
    if (t + 1 < chunks) poseidon_permute<PF, W>(pf, k, s);
  }
#pragma unroll
  for (int i = 0; i < W; i++) state0[i] = s[i];
  *nonce = POW_NONE;
}

// the sponge's first output word for the candidate n, canonical: s0 with n added at `slot`, one permutation
template <class PF, int W>
RONK_HD u64 pow_candidate(const PF& pf, const PoseidonConsts& k, const u64 (&s0)[W], u32 slot, u64 n) {
  const u64 x = pf.in(n);
  u64 s[W];
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = (u32)i == slot ? pf.add(s0[i], x) : s0[i];
  poseidon_permute<PF, W>(pf, k, s);
  return pf.out(s[1]);
}

// One candidate of a lane: false when the lane is done.  found(): the found word, a real read of memory every time; hit(n): the
// atomic minimum.  n: the lane's next candidate, advanced by T.  A lane that hits publishes INSIDE the iteration and leaves at its
// next check (n + T is above the word it has just lowered): a lane that left the loop on its hit would carry the atomic to where
// its wavefront reconverges, behind the loop, and the word would stay 2^64 - 1 until the other 63 lanes had run to the limit --
// measured: every call then took 2^log2_limit / T candidates per lane whatever the nonce.
template <class PF, int W, class Found, class Hit>
RONK_HD bool pow_search_step(const PF& pf, const PoseidonConsts& k, const u64 (&s0)[W], u32 slot, u64 mask, u64 limit, u64 T, u64& n,
                             Found&& found, Hit&& hit) {
  if (n >= found() || n >= limit) return false;
  if ((pow_candidate<PF, W>(pf, k, s0, slot, n) & mask) == 0) hit(n);
  n += T;
  return true;
}

// The first d words of sponge(seed || [nonce]) -- word 0 is the word the condition is about -- by the ordinary sponge (the
// verifier's side shares nothing with the prefix and the search but the permutation).  Returns 1 when nonce < 2^log2_limit and
// the low `bits` bits of word 0 are zero.  The nonce is absorbed as it stands, reduced on input like every word; out may be the
// seed (every word is absorbed before the first is stored).
template <class PF, int W>
RONK_HD int pow_squeeze(const PF& pf, const PoseidonConsts& k, u32 seed_len, const u64* seed, u64 nonce, u32 bits, u32 log2_limit, u32 d,
                        u64* out) {
  u64 first = 0;
  poseidon_sponge<PF, W>(pf, k, (u64)seed_len + 1, d, [&](u64 j) { return j < seed_len ? seed[j] : nonce; },
                         [&](u64 q, u64 v) { if (q == 0) first = v; out[q] = v; });
  return nonce < ((u64)1 << log2_limit) && (first & (((u64)1 << bits) - 1)) == 0;
}

// ---------------------------------------------------------------------------------------------------- host: arguments
// 0, or 1: 2^bits >= p or 2^log2_limit >= p (a nonce must be a canonical, distinct field element), or 2: beyond the limits
inline int pow_host_check(u64 p, size_t seed_len, u32 bits, u32 log2_limit) {
  if (bits > 63 || log2_limit > 63 || ((u64)1 << bits) >= p || ((u64)1 << log2_limit) >= p) return 1;
  if (bits > POW_MAX_BITS || log2_limit > POW_MAX_BITS || seed_len > POW_MAX_SEED) return 2;
  return 0;
}
}  // namespace ronk
