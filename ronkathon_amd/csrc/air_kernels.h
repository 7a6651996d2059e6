// air_kernels.h -- the bodies of the constraint-program quotient on the evaluation coset (csrc/ronk_air.hip; include/ronk_ntt.h
// "constraint programs").  A straight-line program over up to 16 registers is fixed at handle creation; one
// launch runs it at every row of the coset x_i = s w_M^i of a ronk_plonk handle and adds
//
//   sum_j lambda_j C_j D_kind(j)(x_i),   D_ALL = 1 / (x^N - 1),   D_FIRST = 1 / (N (x - 1)),   D_LAST = w_l / (N (x - w_l)),
//                                        D_EXCEPT_LAST = (x - w_l) / (x^N - 1),   w_l = w_N^-1
//
// onto T.  The interpreter: every lane of a launch runs the same op at the same time, so the op word, the immediates, the
// challenges and the weights are read at wave-uniform indices through the constant address space (the scalar path) and every
// switch is a uniform branch.  The registers are indexed by the op word, so they cannot be a VGPR array: they live in LDS as
// [register][plane][lane], 8 bytes per lane and slot, every access lane-contiguous and conflict-free; a launch asks for as many
// slots as the program has registers.  ronk_air_create types every value statically (base or extension: the program is
// straight-line) and writes the types into the tape, so base values take base arithmetic and plane 0 only.  The four sums, one
// per kind, are VGPRs.
//
// A lane owns PTS rows at stride M / PTS (plonk_kernels.h) and runs the tape once per row in a runtime loop.  A program with a
// FIRST or LAST constraint needs 1 / (x - 1) and 1 / (x - w_l): the 2 PTS differences of a lane are multiplied up, inverted ONCE
// (deep_inverse) and unwound with Montgomery's trick before the loop, and parked in LDS behind the registers; a program without
// those kinds skips all of it (a flag of the handle, wave-uniform).  ronk_plonk_check refuses s^M = 1, so nothing vanishes.
//
// A periodic column (operand kind PER) is never an input of a call: the handle owns its values on the coset, P B words per column
// (the coset values of a column of period P repeat after P B rows), built once at creation by air_per_build below.  The kernel
// reads the table's offset and mask at a wave-uniform index through the scalar path, then one word per lane, adjacent lanes
// adjacent words.
//
// Plain C++ on uint64 behind a small accessor for the register file, so tests/emu/emu_air.cpp compiles the same bodies for the
// host.
#pragma once
#include <vector>

#include "plonk_kernels.h"

namespace ronk {

constexpr u32 AIR_MAX_GROUPS = 8, AIR_MAX_BASE = 64, AIR_MAX_EXT = 8, AIR_MAX_CHAL = 32, AIR_MAX_IMM = 256, AIR_MAX_REGS = 16;
constexpr u32 AIR_MAX_CONSTRAINTS = 64, AIR_MAX_OPS = 4096, AIR_MAX_PER = 16;
constexpr u32 AIR_LANES = 256;              // lanes of a workgroup; halved while the LDS of a workgroup would pass AIR_LDS_MAX
constexpr u32 AIR_LDS_MAX = 64 * 1024;
enum AirOp : u32 { AIR_MOV, AIR_ADD, AIR_SUB, AIR_MUL, AIR_NEG, AIR_EMIT };
enum AirOperand : u32 { AIR_REG, AIR_BASE, AIR_EXT, AIR_CHAL, AIR_IMM, AIR_X, AIR_PER };
enum AirKind : u32 { AIR_ALL, AIR_FIRST, AIR_LAST, AIR_EXCEPT_LAST };

// ---- the op word as the caller writes it (include/ronk_ntt.h)
RONK_HD u32 air_opcode(u64 op) { return (u32)(op & 0xff); }
RONK_HD u32 air_dst(u64 op) { return (u32)((op >> 8) & 0xff); }
RONK_HD u32 air_a(u64 op) { return (u32)((op >> 16) & 0xffffff); }
RONK_HD u32 air_b(u64 op) { return (u32)((op >> 40) & 0xffffff); }
RONK_HD u32 air_kind(u32 o) { return o & 0xf; }
RONK_HD u32 air_index(u32 o) { return (o >> 4) & 0xff; }
RONK_HD int air_rot(u32 o) { return (int)(((o >> 12) & 0xfff) ^ 0x800) - 0x800; }   // the signed 12 bits

// ---- the typed tape the kernel reads: the same fields with
//        bits 0-2 the opcode, bit 3 operand a is an extension value, bit 4 operand b is, bits 5-6 the kind of an EMIT;
//        an operand: bits 0-2 its kind, bits 3-11 its index (BASE: group << 6 | column in the group; PER: the column p), bits 12-23 rot
constexpr u64 AIR_TA = 8, AIR_TB = 16;

// what the handle knows: device pointers, register form
struct AirProg {
  const u64* tape;   // [n_ops]
  const u64* imm;    // [n_imm], register form
  u32 n_ops, n_regs;
  u32 boundary;      // some constraint is FIRST or LAST
  u64 wl, wln;       // w_l = w_N^-1 and w_l / N
  const u64* per;    // periodic columns: [n_per][2] words (offset from `per`, P B - 1), then the tables, register form; or NULL
};
// the arrays of a call
struct AirCall {
  const u64* base[AIR_MAX_GROUPS];   // [C_g][M]
  const u64* ext[AIR_MAX_EXT];       // planar [2][M]
  const u64* chal;                   // [n_chal][2]
  const u64* lambda;                 // [J][2]
  const u64* T_in;                   // planar [2][M] or NULL; may be the output
};

// Read-only words at wave-uniform indices (the tape, the immediates, the challenges, the weights): the constant address space
// lets the device take them through the scalar path.  Nothing of a call writes them (the output overlaps no input but T_in).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) u64* AirUniform;
#else
typedef const u64* AirUniform;
#endif

// The register file of one lane: slot s of lane l is word s * lanes + l.  Slots 2 r and 2 r + 1 are the planes of register r; the
// parked inverses follow the registers.
struct AirSlots {
  u64* words;
  u32 lanes, lane;
  RONK_HD u64 get(u32 slot) const { return words[(size_t)slot * lanes + lane]; }
  RONK_HD void put(u32 slot, u64 v) const { words[(size_t)slot * lanes + lane] = v; }
};
RONK_HD u32 air_slots(u32 n_regs, bool boundary, u32 pts) { return 2 * n_regs + (boundary ? 2 * pts : 0); }

// row (i + rot B) mod M
RONK_HD u64 air_rotated(u64 row, u32 o, u64 M, u32 log2b) {
  const int64_t by = (int64_t)air_rot(o) * ((int64_t)1 << log2b);
  return (row + (u64)by) & (M - 1);
}

// one operand in register form; `ext`: its static type (a base value has c1 = 0 and never reads plane 1)
template <class F, class R>
RONK_HD E2 air_operand(const F& f, const AirProg& pg, const AirCall& c, const R& regs, u32 o, bool ext, u64 row, u64 M, u32 log2b,
                       u64 xi) {
  const u32 kind = o & 7, idx = (o >> 3) & 0x1ff;
  switch (kind) {
    case AIR_REG: return E2{regs.get(2 * idx), ext ? regs.get(2 * idx + 1) : 0};
    case AIR_BASE: {
      const FriTable col = (FriTable)c.base[idx >> 6];
      return E2{f.in(col[(u64)(idx & 63) * M + air_rotated(row, o, M, log2b)]), 0};
    }
    case AIR_EXT: {
      const FriTable col = (FriTable)c.ext[idx];
      const u64 r = air_rotated(row, o, M, log2b);
      return E2{f.in(col[r]), f.in(col[M + r])};
    }
    case AIR_CHAL: {
      const AirUniform ch = (AirUniform)c.chal;
      return E2{f.in(ch[2 * idx]), f.in(ch[2 * idx + 1])};
    }
    case AIR_IMM: return E2{((AirUniform)pg.imm)[idx], 0};
    case AIR_PER: {
      const AirUniform d = (AirUniform)pg.per;
      const u64 off = d[2 * idx], mask = d[2 * idx + 1];
      const int64_t by = (int64_t)air_rot(o) * ((int64_t)1 << log2b);
      return E2{((FriTable)pg.per)[off + ((row + (u64)by) & mask)], 0};
    }
    default: return E2{xi, 0};
  }
}

// the tape at one row: acc[kind] = sum over the constraints of that kind of lambda_j C_j, register form
template <class F, class R>
RONK_HD void air_row(const Ext2<F>& x, const AirProg& pg, const AirCall& c, const R& regs, u64 row, u64 M, u32 log2b, u64 xi,
                     E2 (&acc)[4]) {
  const F& f = x.f;
  const AirUniform tape = (AirUniform)pg.tape, lam = (AirUniform)c.lambda;
  acc[0] = acc[1] = acc[2] = acc[3] = x.zero();
#pragma unroll 1
  for (u32 pc = 0; pc < pg.n_ops; pc++) {
    const u64 op = tape[pc];
    const u32 code = (u32)(op & 7);
    const bool ta = (op & AIR_TA) != 0, tb = (op & AIR_TB) != 0;
    const E2 a = air_operand(f, pg, c, regs, air_a(op), ta, row, M, log2b, xi);
    if (code == AIR_EMIT) {
      const u32 j = air_b(op), kind = (u32)((op >> 5) & 3);
      const E2 l{f.in(lam[2 * j]), f.in(lam[2 * j + 1])};
      const E2 t = ta ? x.mul(l, a) : x.mul_base(l, a.c0);
      if (kind == AIR_ALL) acc[0] = x.add(acc[0], t);
      else if (kind == AIR_FIRST) acc[1] = x.add(acc[1], t);
      else if (kind == AIR_LAST) acc[2] = x.add(acc[2], t);
      else acc[3] = x.add(acc[3], t);
      continue;
    }
    E2 r = a;
    if (code == AIR_NEG) {
      r = E2{f.neg(a.c0), ta ? f.neg(a.c1) : 0};
    } else if (code != AIR_MOV) {
      const E2 b = air_operand(f, pg, c, regs, air_b(op), tb, row, M, log2b, xi);
      if (code == AIR_ADD) r = E2{f.add(a.c0, b.c0), ta && tb ? f.add(a.c1, b.c1) : ta ? a.c1 : b.c1};
      else if (code == AIR_SUB) r = E2{f.sub(a.c0, b.c0), ta && tb ? f.sub(a.c1, b.c1) : ta ? a.c1 : tb ? f.neg(b.c1) : 0};
      else r = ta && tb ? x.mul(a, b) : ta ? x.mul_base(a, b.c0) : tb ? x.mul_base(b, a.c0) : E2{f.mul(a.c0, b.c0), 0};
    }
    const u32 dst = air_dst(op);
    regs.put(2 * dst, r.c0);
    if (ta || tb) regs.put(2 * dst + 1, r.c1);
  }
}

// The lane that owns the rows i + t q, t < PTS (q = M / PTS; PTS = 8 or 4, or 1 with q unused): store(row, T) takes the canonical
// pair.  regs: air_slots(n_regs, boundary, PTS) slots.
template <class F, int PTS, class R, class Store>
RONK_HD void air_lane(const Ext2<F>& x, const DeepDomain& dm, const PlonkTab& tab, const AirProg& pg, const AirCall& c, const R& regs,
                      u64 i, Store&& store) {
  static_assert(PTS == 1 || PTS == 4 || PTS == 8, "a lane owns one row, or the rows x rho^t of an eighth or a fourth root rho");
  const F& f = x.f;
  const u64 M = (u64)1 << dm.log2n, q = M / PTS, bmask = ((u64)1 << tab.log2b) - 1;
  const FriTable vinv = (FriTable)tab.vinv;
  const u32 park = 2 * pg.n_regs;
  const u64 x0 = deep_point(f, dm, i);
  const u64 step = PTS == 4 ? dm.iota : PTS == 8 ? tab.rho : f.one();   // x_(i + q) = x_i step
  if (pg.boundary) {
    u64 xs[PTS], pre[2 * PTS];
    xs[0] = x0;
    deep_for<1, PTS>([&](auto T) { constexpr int t = decltype(T)::value; xs[t] = f.mul(xs[t - 1], step); });
    u64 run = f.one();
    deep_for<0, 2 * PTS>([&](auto J) {
      constexpr int j = decltype(J)::value;
      pre[j] = run;
      run = f.mul(run, f.sub(xs[j / 2], j % 2 ? pg.wl : f.one()));
    });
    u64 inv = deep_inverse(x, run);
    deep_for<0, 2 * PTS>([&](auto J) {
      constexpr int j = 2 * PTS - 1 - decltype(J)::value;
      regs.put(park + j, f.mul(inv, pre[j]));
      inv = f.mul(inv, f.sub(xs[j / 2], j % 2 ? pg.wl : f.one()));
    });
  }
  u64 xi = x0;
#pragma unroll 1
  for (u32 t = 0; t < (u32)PTS; t++) {
    if (t) xi = f.mul(xi, step);
    const u64 row = i + (u64)t * q;
    E2 acc[4];
    air_row(x, pg, c, regs, row, M, tab.log2b, xi, acc);
    E2 v = x.mul_base(x.add(acc[0], x.mul_base(acc[3], f.sub(xi, pg.wl))), vinv[row & bmask]);
    if (pg.boundary) {
      v = x.add(v, x.mul_base(acc[1], f.mul(regs.get(park + 2 * t), tab.ninv)));
      v = x.add(v, x.mul_base(acc[2], f.mul(regs.get(park + 2 * t + 1), pg.wln)));
    }
    if (c.T_in) v = x.add(v, E2{f.in(c.T_in[row]), f.in(c.T_in[M + row])});
    store(row, E2{f.out(v.c0), f.out(v.c1)});
  }
}

// ---------------------------------------------------------------------------------------------------- host: checking and typing
struct AirShape {
  u32 log2n, n_groups;
  const u32* n_columns;   // [n_groups]
  u32 n_ext, n_chal, n_imm, n_regs, n_constraints;
  u32 n_per = 0;
  const u32* log2_period = nullptr;   // [n_per]
};
enum AirStatus { AIR_OK = 0, AIR_INVALID = 1, AIR_UNSUPPORTED = 2 };

// The codes of ronk_air_check_per in their order (ronk_air_check: n_per = 0).  With `tape` the typed tape, `boundary` and the cells (the distinct BASE and EXT
// operands as the caller wrote them, in first-use order) are written as well.
inline AirStatus air_compile(const AirShape& s, const u64* ops, u32 n_ops, std::vector<u64>* tape, u32* boundary,
                             std::vector<u32>* cells) {
  if (!ops || (s.n_groups && !s.n_columns) || n_ops == 0 || s.n_constraints == 0) return AIR_INVALID;
  if (s.n_groups > AIR_MAX_GROUPS) return AIR_UNSUPPORTED;
  u32 total = 0;
  for (u32 g = 0; g < s.n_groups; g++) {
    if (s.n_columns[g] == 0) return AIR_INVALID;
    if (s.n_columns[g] > AIR_MAX_BASE) return AIR_UNSUPPORTED;
    total += s.n_columns[g];
  }
  if (total > AIR_MAX_BASE || s.n_ext > AIR_MAX_EXT || s.n_chal > AIR_MAX_CHAL || s.n_imm > AIR_MAX_IMM || s.n_regs > AIR_MAX_REGS ||
      s.n_constraints > AIR_MAX_CONSTRAINTS || n_ops > AIR_MAX_OPS || s.log2n < 1 || s.log2n > PLONK_MAX_LOG2M)
    return AIR_UNSUPPORTED;
  if (s.n_per > AIR_MAX_PER) return AIR_UNSUPPORTED;
  for (u32 k = 0; k < s.n_per && s.log2_period; k++)
    if (s.log2_period[k] > s.log2n) return AIR_UNSUPPORTED;
  if (s.n_per && !s.log2_period) return AIR_INVALID;
  int rtype[AIR_MAX_REGS];
  for (u32 r = 0; r < AIR_MAX_REGS; r++) rtype[r] = -1;
  bool emitted[AIR_MAX_CONSTRAINTS] = {};
  u32 n_emitted = 0, bnd = 0;
  const int64_t N = (int64_t)1 << s.log2n;
  // -> the typed operand and its type, or false
  auto operand = [&](u32 o, u32* typed, int* type) {
    const u32 kind = air_kind(o), idx = air_index(o);
    const int rot = air_rot(o);
    if (kind > AIR_PER) return false;
    if (kind != AIR_BASE && kind != AIR_EXT && kind != AIR_PER && rot != 0) return false;
    if (rot >= N || -rot >= N) return false;
    u32 tidx = idx;
    switch (kind) {
      case AIR_REG:
        if (idx >= s.n_regs || rtype[idx] < 0) return false;
        *type = rtype[idx];
        break;
      case AIR_BASE: {
        if (idx >= total) return false;
        u32 g = 0, col = idx;
        while (col >= s.n_columns[g]) col -= s.n_columns[g++];
        tidx = g << 6 | col;
        *type = 0;
        break;
      }
      case AIR_EXT: if (idx >= s.n_ext) return false; *type = 1; break;
      case AIR_CHAL: if (idx >= s.n_chal) return false; *type = 1; break;
      case AIR_IMM: if (idx >= s.n_imm) return false; *type = 0; break;
      case AIR_PER: if (idx >= s.n_per) return false; *type = 0; break;
      default: if (idx != 0) return false; *type = 0; break;
    }
    if (cells && (kind == AIR_BASE || kind == AIR_EXT)) {
      bool seen = false;
      for (u32 v : *cells) seen = seen || v == o;
      if (!seen) cells->push_back(o);
    }
    *typed = kind | tidx << 3 | (o & 0xfff000);
    return true;
  };
  if (tape) tape->clear();
  for (u32 pc = 0; pc < n_ops; pc++) {
    const u64 op = ops[pc];
    const u32 code = air_opcode(op), dst = air_dst(op);
    if (code > AIR_EMIT) return AIR_INVALID;
    u32 a = 0, b = 0;
    int ta = 0, tb = 0;
    if (!operand(air_a(op), &a, &ta)) return AIR_INVALID;
    u64 word = code | (ta ? AIR_TA : 0) | (u64)a << 16;
    if (code == AIR_EMIT) {
      const u32 j = air_b(op);
      if (dst > AIR_EXCEPT_LAST || j >= s.n_constraints || emitted[j]) return AIR_INVALID;
      emitted[j] = true;
      n_emitted++;
      if (dst == AIR_FIRST || dst == AIR_LAST) bnd = 1;
      word |= (u64)dst << 5 | (u64)j << 40;
    } else {
      if (dst >= s.n_regs) return AIR_INVALID;
      if (code == AIR_MOV || code == AIR_NEG) {
        if (air_b(op) != 0) return AIR_INVALID;
      } else {
        if (!operand(air_b(op), &b, &tb)) return AIR_INVALID;
        word |= (tb ? AIR_TB : 0) | (u64)b << 40;
      }
      rtype[dst] = ta | tb;
      word |= (u64)dst << 8;
    }
    if (tape) tape->push_back(word);
  }
  if (n_emitted != s.n_constraints) return AIR_INVALID;
  if (boundary) *boundary = bnd;
  return AIR_OK;
}

// ---------------------------------------------------------------------------------------------------- host: the periodic columns
// in-place transform of a[0 .. 2^log2len) on plain residues: a[k] <- sum_j a[j] root^(j k), root of order 2^log2len
inline void air_host_ntt(u64 p, u64 root, u32 log2len, u64* a) {
  const u64 n = (u64)1 << log2len;
  for (u64 i = 1, j = 0; i < n; i++) {
    u64 bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { const u64 t = a[i]; a[i] = a[j]; a[j] = t; }
  }
  for (u32 l = 1; l <= log2len; l++) {
    const u64 half = (u64)1 << (l - 1), wl = fri_powmod(root, n >> l, p);
    for (u64 b = 0; b < n; b += 2 * half) {
      u64 w = 1 % p;
      for (u64 k = 0; k < half; k++) {
        const u64 u = a[b + k], v = fri_mulmod(a[b + k + half], w, p);
        a[b + k] = (u64)(((unsigned __int128)u + v) % p);
        a[b + k + half] = (u64)(((unsigned __int128)u + p - v) % p);
        w = fri_mulmod(w, wl, p);
      }
    }
  }
}

// Column k of period P = 2^log2_period[k] with the values vals (any words): q of degree below P with q(w_P^j) = vals[j], and
// tab[j] = q(s^(N/P) w_M^(j N/P)), j < P B: the inverse transform over <w_P>, the scaling by (s^(N/P))^k, the zero padding to P B
// and the transform over <w_M^(N/P)>.  coef receives the n_per coefficient vectors one after the other (plain residues, for the
// evaluation at a point); words receives [n_per][2] (offset, mask) and then the tables in register form: what AirProg::per points to.
inline void air_per_build(bool mont, u64 p, u64 g, u64 shift, u32 log2n, u32 log2b, u32 n_per, const u32* log2_period,
                          const u64* vals, std::vector<u64>* coef, std::vector<u64>* words) {
  coef->clear();
  words->assign(2 * (size_t)n_per, 0);
  for (u32 k = 0; k < n_per; k++) {
    const u32 lp = log2_period[k];
    const u64 P = (u64)1 << lp, PB = P << log2b;
    std::vector<u64> q(P), t(PB, 0);
    for (u64 j = 0; j < P; j++) q[j] = vals[j] % p;
    vals += P;
    const u64 wp = fri_powmod(g, (p - 1) >> lp, p), pinv = fri_powmod(P % p, p - 2, p);
    air_host_ntt(p, fri_powmod(wp, p - 2, p), lp, q.data());
    u64 sp = shift % p, run = 1 % p;
    for (u32 j = lp; j < log2n; j++) sp = fri_mulmod(sp, sp, p);   // s^(N/P)
    for (u64 j = 0; j < P; j++) {
      q[j] = fri_mulmod(q[j], pinv, p);
      t[j] = fri_mulmod(q[j], run, p);
      run = fri_mulmod(run, sp, p);
    }
    air_host_ntt(p, fri_powmod(g, (p - 1) >> (lp + log2b), p), lp + log2b, t.data());
    (*words)[2 * k] = words->size();
    (*words)[2 * k + 1] = PB - 1;
    for (u64 v : t) words->push_back(fri_reg_form(mont, p, v));
    coef->insert(coef->end(), q.begin(), q.end());
  }
}

// lanes of a workgroup and its LDS bytes for a program on PTS rows per lane
inline u32 air_lanes(u32 n_regs, bool boundary, u32 pts) {
  u32 lanes = AIR_LANES;
  while (lanes > 64 && (u64)air_slots(n_regs, boundary, pts) * 8 * lanes > AIR_LDS_MAX) lanes /= 2;
  return lanes;
}

#if defined(__HIPCC__)
// one lane per PTS rows i + t M / PTS, as plonk_quotient_kernel.  No __restrict__ on T: it may be T_in.
template <class F, int PTS>
__global__ void __launch_bounds__(AIR_LANES) air_quotient_kernel(FriConsts k, u64 w, DeepDomain dm, PlonkTab tab, AirProg pg, AirCall c,
                                                                 u64* T) {
  extern __shared__ __attribute__((aligned(16))) u64 air_lds[];
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 M = (u64)1 << dm.log2n, q = M / PTS;
  const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= q) return;
  const AirSlots regs{air_lds, blockDim.x, threadIdx.x};
  air_lane<F, PTS>(x, dm, tab, pg, c, regs, i, [&](u64 row, E2 v) { T[row] = v.c0; T[M + row] = v.c1; });
}
#endif

}  // namespace ronk
