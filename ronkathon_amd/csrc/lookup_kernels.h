// lookup_kernels.h -- the two missing steps of the lookup argument around the logUp running sum (csrc/ronk_lookup.hip;
// include/ronk_ntt.h "lookup multiplicities and the logUp quotient").
//
// A. Multiplicities.  m[j] = #{(c, i) : f_c[i] = t[j]} for a table t[T] and C lookup columns f_c[n], every comparison between the
//    words reduced mod p, counted at the smallest index of each table value.  An open-addressing hash table in the caller's
//    workspace: CAP slots, CAP the power of two with 2 T <= CAP, one KEY word (the canonical value; the sentinel 2^64 - 1 is never
//    canonical) and one INFO word per slot, INFO = index << 34 | count (index < 2^28, count <= 16 * 2^28 = 2^32).  FOUR launches:
//      clear     keys <- sentinel, info <- all ones, m <- 0, missing <- (0, 2^64 - 1)
//      build     one lane per table entry: linear probing from a multiplicative hash, atomicCAS on the key; on "was empty" or "was
//                my key" atomicMin of index << 34 into the info word, so the smallest index wins for duplicates
//      count     one lane per lookup word, flat index c n + i (a wavefront's loads are contiguous): probe until the key or an empty
//                slot; found adds 1 to the info word, empty adds 1 to missing[0] and takes atomicMin of the flat index into
//                missing[1].  Equal slots are combined inside the wavefront first, and the most common one is carried from pass
//                to pass of the wavefront over the grid (Atomics::add_combined); the missing count is one add per wavefront.
//      finalise  one lane per slot: an occupied slot writes field(count), or its negation, to m[index]
//    No lane or workgroup ever waits for another: every probe loop is bounded by CAP (and ends sooner, the table is at most half
//    full), there is no flag, no spin and no grid barrier.  What one launch writes only later launches read.  Integer atomics
//    commute, so every word written is a function of the inputs alone.
//    Reduction mod p is the field policy's f.out(f.in(x)): gl64::canon over Goldilocks, a Montgomery product with R^2 and one with
//    1 over any other odd prime -- exact for every 64-bit word and every odd p < 2^64, p = 17 included.
//
// B. The logUp quotient on the evaluation coset, the sibling of the PLONK quotient (plonk_kernels.h) on the same lane:
//      D_c = alpha + v_c[i],  P = prod_c D_c,  Q = sum_c m_c[i] prod_(c' != c) D_c'
//      R   = (S_((i + B) mod M) - S_i) P - Q
//      T_out_i = T_in_i + lambda0 R / (x_i^N - 1) + lambda1 S_i / (N (x_i - 1))
//    P and Q stream: Q <- Q D_c + m_c P; P <- P D_c.  No per-column arrays, no division by D_c, no status word.
//
// Plain C++ on uint64 with the atomic operations behind a policy, so tests/emu/emu_lookup.cpp compiles the same bodies for the
// host and runs the lanes in any order.
#pragma once
#include "plonk_kernels.h"

namespace ronk {

constexpr u32 LOOKUP_LANES = 256;
constexpr u64 LOOKUP_MAX_N = (u64)1 << 28;      // table entries, and rows of a lookup column
constexpr u32 LOOKUP_MAX_COLUMNS = 16;
constexpr u64 LOOKUP_EMPTY = ~(u64)0;           // never canonical: p < 2^64
constexpr u32 LOOKUP_COUNT_BITS = 34;           // counts reach 16 * 2^28 = 2^32
constexpr u64 LOOKUP_COUNT_MASK = ((u64)1 << LOOKUP_COUNT_BITS) - 1;
constexpr u64 LOOKUP_GRID_MAX = (u64)1 << 20;   // workgroups of a grid-stride launch
// ... and of the count launch: 8 per CU of the MI355X's 256 (a fixed number, not queried: fewer CUs only mean more waves per CU),
// so a wavefront makes several passes over the column and carries its first slot
constexpr u64 LOOKUP_COUNT_GRID = 2048;

// log2 of the capacity CAP: the smallest power of two with 2 T <= CAP (so CAP >= 2, its log2 >= 1)
RONK_HD u32 lookup_log2_cap(u64 T) {
  u32 l = 1;
  while (((u64)1 << l) < 2 * T) l++;
  return l;
}
// the workspace of one call: CAP keys, CAP info words
RONK_HD u64 lookup_work_words(u64 T) { return (T == 0 || T > LOOKUP_MAX_N) ? 0 : (u64)2 << lookup_log2_cap(T); }

// the table as the kernels see it
struct LookupTab {
  u64* keys;     // [CAP]
  u64* info;     // [CAP]: index << 34 | count
  u32 log2cap;
};
RONK_HD u64 lookup_cap(const LookupTab& t) { return (u64)1 << t.log2cap; }
RONK_HD u64 lookup_hash(const LookupTab& t, u64 key) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - t.log2cap); }
template <class F>
RONK_HD u64 lookup_canon(const F& f, u64 word) { return f.out(f.in(word)); }

// ---------------------------------------------------------------------------------------------------- the four bodies
// element e of the clear launch, e < max(CAP, T, 2)
RONK_HD void lookup_clear(const LookupTab& t, u64 T, u64* mult, u64* missing, u64 e) {
  if (e < lookup_cap(t)) { t.keys[e] = LOOKUP_EMPTY; t.info[e] = ~(u64)0; }
  if (e < T) mult[e] = 0;
  if (e < 2) missing[e] = e ? ~(u64)0 : 0;
}

// table entry j: A supplies cas(ptr, expected, desired) -> old and min(ptr, value)
template <class F, class A>
RONK_HD void lookup_build(const F& f, A& at, const LookupTab& t, const u64* table, u64 j) {
  const u64 key = lookup_canon(f, table[j]), mask = lookup_cap(t) - 1;
  u64 s = lookup_hash(t, key);
  for (u64 probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
    const u64 old = at.cas(&t.keys[s], LOOKUP_EMPTY, key);
    if (old == LOOKUP_EMPTY || old == key) {
      at.min(&t.info[s], j << LOOKUP_COUNT_BITS);
      return;
    }
  }
}

// the slot of a lookup word, or CAP when the table does not hold it.  The keys were written by an earlier launch.
template <class F>
RONK_HD u64 lookup_probe(const F& f, const LookupTab& t, u64 word) {
  const u64 key = lookup_canon(f, word), mask = lookup_cap(t) - 1;
  u64 s = lookup_hash(t, key);
  for (u64 probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
    const u64 k = t.keys[s];
    if (k == key) return s;
    if (k == LOOKUP_EMPTY) break;
  }
  return mask + 1;
}

// lookup word e of the C n (lanes past the end take part with e >= total: a wavefront combines as a whole).
// A supplies add_combined(base, slot, active): info[slot] += 1 for every active lane, at once or owed until its flush(base), and
// missing(ptr, is_missing, e).
template <class F, class A>
RONK_HD void lookup_count(const F& f, A& at, const LookupTab& t, const u64* vals, u64 total, u64* missing, u64 e) {
  const bool live = e < total;
  const u64 s = live ? lookup_probe(f, t, vals[e]) : 0;
  const bool found = live && s < lookup_cap(t);
  at.add_combined(t.info, (u32)(found ? s : 0), found);
  at.missing(missing, live && !found, e);
}

// slot s: an occupied slot writes the field element of its count, or the negation, to its index
template <class F>
RONK_HD void lookup_finalise(const F& f, const LookupTab& t, int negate, u64* mult, u64 s) {
  if (t.keys[s] == LOOKUP_EMPTY) return;
  const u64 info = t.info[s];
  const u64 v = lookup_canon(f, info & LOOKUP_COUNT_MASK);
  mult[info >> LOOKUP_COUNT_BITS] = negate && v ? f.order() - v : v;
}

// ---------------------------------------------------------------------------------------------------- the logUp quotient
// the arrays of a call
struct LogupCols {
  const u64* vals;     // [C][M]
  const u64* mult;     // [C][M] or NULL: all ones
  u32 C;
  const u64* S;        // planar [2][M]
  const u64* alpha;    // two words
  const u64* lambda;   // lambda0, lambda1: four words
  const u64* Tin;      // planar [2][M] or NULL: zero
};
// the challenges as a row uses them
struct LogupChal {
  E2 alpha, l0;
  E2 l1n;   // lambda1 / N
};
template <class F>
RONK_HD LogupChal logup_challenges(const Ext2<F>& x, const PlonkTab& tab, const u64* alpha, const u64* lambda) {
  const F& f = x.f;
  LogupChal ch;
  ch.alpha = E2{f.in(alpha[0]), f.in(alpha[1])};
  ch.l0 = E2{f.in(lambda[0]), f.in(lambda[1])};
  ch.l1n = x.mul_base(E2{f.in(lambda[2]), f.in(lambda[3])}, tab.ninv);
  return ch;
}

// T_out at row i, canonical: dinv = 1 / (x_i - 1), vinv = 1 / (x_i^N - 1), register form.  The columns are read here, one
// word per column and pass of the runtime loop.
template <class F>
RONK_HD E2 logup_row(const Ext2<F>& x, const LogupChal& ch, const LogupCols& c, u64 M, u64 B, u64 i, u64 dinv, u64 vinv) {
  const F& f = x.f;
  const u64 in = (i + B) & (M - 1);
  E2 P = x.one(), Q = x.zero();
  for (u32 col = 0; col < c.C; col++) {
    const E2 D{f.add(ch.alpha.c0, f.in(c.vals[(u64)col * M + i])), ch.alpha.c1};
    Q = x.mul(Q, D);
    Q = x.add(Q, c.mult ? x.mul_base(P, f.in(c.mult[(u64)col * M + i])) : P);
    P = x.mul(P, D);
  }
  const E2 S{f.in(c.S[i]), f.in(c.S[M + i])}, Sn{f.in(c.S[in]), f.in(c.S[M + in])};
  const E2 R = x.sub(x.mul(x.sub(Sn, S), P), Q);
  E2 t = x.mul_base(x.mul(ch.l0, R), vinv);
  t = x.add(t, x.mul(ch.l1n, x.mul_base(S, dinv)));
  if (c.Tin) t = x.add(t, E2{f.in(c.Tin[i]), f.in(c.Tin[M + i])});
  return E2{f.out(t.c0), f.out(t.c1)};
}

// The sibling of plonk_lane (left as it is: its kernels keep their resource lines): the lane that owns the rows i + t q, t < PTS
// (q = M / PTS), keeps the differences x - 1 of its rows instead of the points, inverts their product once and unwinds;
// store(row, T) takes the canonical pair.
template <class F, int PTS, class Store>
RONK_HD void logup_lane(const Ext2<F>& x, const DeepDomain& dm, const PlonkTab& tab, const LogupChal& ch, const LogupCols& c, u64 i,
                        Store&& store) {
  static_assert(PTS == 1 || PTS == 4 || PTS == 8, "a lane owns one row, or the rows x rho^t of an eighth or a fourth root rho");
  const F& f = x.f;
  const u64 M = (u64)1 << dm.log2n, B = (u64)1 << tab.log2b, q = M / PTS;
  const FriTable vinv = (FriTable)tab.vinv;
  u64 d[PTS], pre[PTS];
  d[0] = deep_point(f, dm, i);
  if constexpr (PTS == 4) {
    d[1] = f.mul(d[0], dm.iota);
    d[2] = f.neg(d[0]);
    d[3] = f.neg(d[1]);
  }
  if constexpr (PTS == 8) {
    d[1] = f.mul(d[0], tab.rho);
    d[2] = f.mul(d[0], dm.iota);
    d[3] = f.mul(d[1], dm.iota);
    deep_for<0, 4>([&](auto J) { constexpr int j = decltype(J)::value; d[4 + j] = f.neg(d[j]); });
  }
  u64 run = f.one();
  deep_for<0, PTS>([&](auto T) {
    constexpr int t = decltype(T)::value;
    d[t] = f.sub(d[t], f.one());
    pre[t] = run;
    run = f.mul(run, d[t]);
  });
  u64 inv = deep_inverse(x, run);
  deep_for<0, PTS>([&](auto T) {
    constexpr int t = PTS - 1 - decltype(T)::value;
    const u64 row = i + (u64)t * q;
    const u64 dinv = f.mul(inv, pre[t]);
    inv = f.mul(inv, d[t]);
    store(row, logup_row(x, ch, c, M, B, row, dinv, vinv[row & (B - 1)]));
  });
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------- kernels
// The atomics of the device.  add_combined: lanes of a wavefront that hit the same slot are counted by one of them -- up to
// LOOKUP_PEEL rounds take the slot of the first pending lane and retire every lane that shares it (a skewed column, where a few
// values take most of the lanes, is done in as many rounds; an all-equal one in a single round); whoever is still pending adds
// for itself.  What the FIRST round retires is not added at once: the wavefront carries it (slot and count, wave-uniform) into
// its next pass over the grid and adds it only when the first slot changes, or in flush() at the end -- a column of one value
// costs one atomic per wavefront for the whole launch, not one per 64 words.  Every lane of the wavefront must call
// add_combined and flush (the rounds are wave-uniform).
constexpr int LOOKUP_PEEL = 8;
struct LookupDeviceAtomics {
  u32 carried_slot = 0;
  u64 carried = 0;   // the adds owed to carried_slot; 0: nothing carried
  __device__ u64 cas(u64* p, u64 expected, u64 desired) const {
    return atomicCAS((unsigned long long*)p, (unsigned long long)expected, (unsigned long long)desired);
  }
  __device__ void min(u64* p, u64 v) const { atomicMin((unsigned long long*)p, (unsigned long long)v); }
  __device__ void flush(u64* base) {
    if (carried && __lane_id() == 0) atomicAdd((unsigned long long*)&base[carried_slot], (unsigned long long)carried);
    carried = 0;
  }
  __device__ void add_combined(u64* base, u32 slot, bool active) {
    const u32 lane = __lane_id();
    bool pending = active;
    for (int round = 0; round < LOOKUP_PEEL; round++) {
      const u64 m = __ballot(pending);
      if (!m) break;
      const u32 leader = (u32)__ffsll((unsigned long long)m) - 1;
      const u32 ls = (u32)__shfl((int)slot, (int)leader);
      const bool mine = pending && slot == ls;
      const u64 k = (u64)__popcll(__ballot(mine));
      if (round == 0) {
        if (carried && carried_slot != ls) flush(base);
        carried_slot = ls;
        carried += k;
      } else if (lane == leader) {
        atomicAdd((unsigned long long*)&base[ls], (unsigned long long)k);
      }
      if (mine) pending = false;
    }
    if (pending) atomicAdd((unsigned long long*)&base[slot], 1ull);
  }
  // one add and one min per wavefront and pass: the lanes of a wavefront hold consecutive flat indices, the first missing lane
  // the least
  __device__ void missing(u64* out, bool is_missing, u64 e) const {
    const u64 m = __ballot(is_missing);
    if (!m) return;
    if (__lane_id() == (u32)__ffsll((unsigned long long)m) - 1) {
      atomicAdd((unsigned long long*)&out[0], (unsigned long long)__popcll(m));
      atomicMin((unsigned long long*)&out[1], (unsigned long long)e);
    }
  }
};

__global__ void __launch_bounds__(LOOKUP_LANES) lookup_clear_kernel(LookupTab t, u64 T, u64* __restrict__ mult, u64* __restrict__ missing,
                                                                    u64 count) {
  for (u64 e = blockIdx.x * (u64)LOOKUP_LANES + threadIdx.x; e < count; e += (u64)gridDim.x * LOOKUP_LANES)
    lookup_clear(t, T, mult, missing, e);
}

template <class F>
__global__ void __launch_bounds__(LOOKUP_LANES) lookup_build_kernel(FriConsts k, LookupTab t, const u64* __restrict__ table, u64 T) {
  const F f(k);
  LookupDeviceAtomics at;
  for (u64 j = blockIdx.x * (u64)LOOKUP_LANES + threadIdx.x; j < T; j += (u64)gridDim.x * LOOKUP_LANES) lookup_build(f, at, t, table, j);
}

// `rounds` = ceil(total / lanes of the grid), the same for every lane, so a wavefront stays whole through add_combined
template <class F>
__global__ void __launch_bounds__(LOOKUP_LANES) lookup_count_kernel(FriConsts k, LookupTab t, const u64* __restrict__ vals, u64 total,
                                                                    u64 rounds, u64* __restrict__ missing) {
  const F f(k);
  LookupDeviceAtomics at;
  u64 e = blockIdx.x * (u64)LOOKUP_LANES + threadIdx.x;
  for (u64 r = 0; r < rounds; r++, e += (u64)gridDim.x * LOOKUP_LANES) lookup_count(f, at, t, vals, total, missing, e);
  at.flush(t.info);
}

template <class F>
__global__ void __launch_bounds__(LOOKUP_LANES) lookup_finalise_kernel(FriConsts k, LookupTab t, int negate, u64* __restrict__ mult) {
  const F f(k);
  const u64 cap = lookup_cap(t);
  for (u64 s = blockIdx.x * (u64)LOOKUP_LANES + threadIdx.x; s < cap; s += (u64)gridDim.x * LOOKUP_LANES)
    lookup_finalise(f, t, negate, mult, s);
}

// one lane per PTS rows i + t M / PTS, as plonk_quotient_kernel.  No __restrict__ on T_out: it may be T_in.
template <class F, int PTS>
__global__ void __launch_bounds__(PLONK_LANES) logup_quotient_kernel(FriConsts k, u64 w, DeepDomain dm, PlonkTab tab, LogupCols cols,
                                                                     u64* T) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 M = (u64)1 << dm.log2n, q = M / PTS;
  const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= q) return;
  const LogupChal ch = logup_challenges(x, tab, cols.alpha, cols.lambda);
  logup_lane<F, PTS>(x, dm, tab, ch, cols, i, [&](u64 row, E2 v) { T[row] = v.c0; T[M + row] = v.c1; });
}
#endif

}  // namespace ronk
