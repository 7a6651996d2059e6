// ronk_air.hip -- C ABI of libronk_ntt.so, part 17: constraint programs on the evaluation coset (csrc/air_kernels.h;
// include/ronk_ntt.h "constraint programs").  A handle holds the checked and typed tape of one program on the
// domain of a ronk_plonk handle; a quotient call is one launch with no host round trip and no library workspace, legal under
// stream capture.  ronk_air_cells and ronk_air_eval_point are the verifier's side: host-side integer logic, no device.
#include "runtime.h"
#include "hip_launch.h"
#include "ext2_launch.h"
#include "plonk_handle.h"
#include "air_kernels.h"

struct ronk_air {
  const ronk_plonk* dom = nullptr;   // borrowed
  AirProg pg{};
  u64* d_tape = nullptr;
  u64* d_imm = nullptr;
  u64* d_per = nullptr;              // the descriptors and the coset tables of the periodic columns
  // the program as the caller wrote it, for the host-side evaluation
  std::vector<u64> ops, imm;         // imm reduced mod p
  std::vector<u32> cells, n_columns;
  u32 log2n = 0, n_ext = 0, n_chal = 0, n_constraints = 0;
  std::vector<u32> log2_period;      // the periodic columns: column k has the coefficients per_coef[per_at[k] ..], plain residues
  std::vector<u64> per_coef;
  std::vector<size_t> per_at;
};

static int air_code(AirStatus s) { return s == AIR_OK ? RONK_OK : s == AIR_INVALID ? RONK_ERR_INVALID : RONK_ERR_UNSUPPORTED; }

extern "C" int ronk_air_check_per(uint32_t log2_n, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext, uint32_t n_chal,
                                  uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                                  uint32_t n_per, const uint32_t* log2_period) {
  const AirShape s{log2_n, n_groups, n_columns, n_ext, n_chal, n_imm, n_regs, n_constraints, n_per, log2_period};
  return air_code(air_compile(s, ops, n_ops, nullptr, nullptr, nullptr));
}

extern "C" int ronk_air_check(uint32_t log2_n, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext, uint32_t n_chal,
                              uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops) {
  return ronk_air_check_per(log2_n, n_groups, n_columns, n_ext, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, 0, nullptr);
}

extern "C" int ronk_air_destroy(ronk_air* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->d_tape) (void)hipFree(h->d_tape);
  if (h->d_imm) (void)hipFree(h->d_imm);
  if (h->d_per) (void)hipFree(h->d_per);
  delete h;
  return RONK_OK;
}

extern "C" int ronk_air_create_per(ronk_air** out, const ronk_plonk* domain, uint32_t n_groups, const uint32_t* n_columns,
                                   uint32_t n_ext, uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints,
                                   const uint64_t* ops, uint32_t n_ops, const uint64_t* imm, uint32_t n_per,
                                   const uint32_t* log2_period, const uint64_t* per_values) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!domain || (n_imm && !imm)) return RONK_ERR_INVALID;
  const u32 log2n = domain->log2m - domain->tab.log2b;
  const AirShape s{log2n, n_groups, n_columns, n_ext, n_chal, n_imm, n_regs, n_constraints, n_per, log2_period};
  std::vector<u64> tape;
  std::vector<u32> cells;
  u32 boundary = 0;
  RCHK(air_code(air_compile(s, ops, n_ops, &tape, &boundary, &cells)));
  if (n_per && !per_values) return RONK_ERR_INVALID;
  RCHK(need_device());
  ronk_air* h = new ronk_air;
  const u64 p = domain->p;
  const bool mont = domain->c.mont;
  h->dom = domain;
  h->ops.assign(ops, ops + n_ops);
  h->cells = cells;
  h->n_columns.assign(n_columns, n_columns + n_groups);
  h->log2n = log2n; h->n_ext = n_ext; h->n_chal = n_chal; h->n_constraints = n_constraints;
  std::vector<u64> reg(n_imm);
  for (u32 j = 0; j < n_imm; j++) { h->imm.push_back(imm[j] % p); reg[j] = ext2_reg_form(mont, p, imm[j]); }
  int rc = upload(tape, &h->d_tape);
  if (rc == RONK_OK) rc = upload(reg, &h->d_imm);
  if (rc == RONK_OK && n_per) {
    std::vector<u64> words;
    air_per_build(mont, p, domain->g, domain->s, log2n, domain->tab.log2b, n_per, log2_period, per_values, &h->per_coef, &words);
    h->log2_period.assign(log2_period, log2_period + n_per);
    size_t at = 0;
    for (u32 k = 0; k < n_per; k++) { h->per_at.push_back(at); at += (size_t)1 << log2_period[k]; }
    rc = upload(words, &h->d_per);
  }
  if (rc != RONK_OK) { ronk_air_destroy(h); return rc; }
  const u64 wn = h_powmod(domain->g, (p - 1) >> log2n, p), wl = h_powmod(wn, p - 2, p);
  h->pg.tape = h->d_tape; h->pg.imm = h->d_imm; h->pg.per = h->d_per;
  h->pg.n_ops = n_ops; h->pg.n_regs = n_regs; h->pg.boundary = boundary;
  h->pg.wl = ext2_reg_form(mont, p, wl);
  h->pg.wln = ext2_reg_form(mont, p, h_mulmod(wl, h_powmod(((u64)1 << log2n) % p, p - 2, p), p));
  *out = h;
  return RONK_OK;
}

extern "C" int ronk_air_create(ronk_air** out, const ronk_plonk* domain, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext,
                               uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops,
                               uint32_t n_ops, const uint64_t* imm) {
  return ronk_air_create_per(out, domain, n_groups, n_columns, n_ext, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, imm, 0, nullptr,
                             nullptr);
}

// one launch with the rows per lane of the field policy, or one row per lane below that many rows (as plonk_launch); the LDS of a
// workgroup is what the program's registers take, and the parked inverses of a program with boundary constraints
template <class FF>
static void air_launch(const ronk_air* h, const AirCall& c, u64* d_T, hipStream_t s) {
  constexpr u32 LP = PlonkRows<FF>::LOG2;
  const ronk_plonk* d = h->dom;
  const u64 M = (u64)1 << d->log2m;
  const u32 pts = d->log2m < LP ? 1 : 1u << LP;
  const u32 lanes = air_lanes(h->pg.n_regs, h->pg.boundary != 0, pts);
  const u32 lds = air_slots(h->pg.n_regs, h->pg.boundary != 0, pts) * 8 * lanes;
  const u32 grid = (u32)((M / pts + lanes - 1) / lanes);
  if (pts == 1)
    hipLaunchKernelGGL((air_quotient_kernel<FF, 1>), dim3(grid), dim3(lanes), lds, s, d->c.k, d->c.w, d->dm, d->tab, h->pg, c, d_T);
  else
    hipLaunchKernelGGL((air_quotient_kernel<FF, 1 << LP>), dim3(grid), dim3(lanes), lds, s, d->c.k, d->c.w, d->dm, d->tab, h->pg, c, d_T);
}

extern "C" int ronk_air_quotient_dev(const ronk_air* h, const uint64_t* const* d_base, const uint64_t* const* d_ext,
                                     const uint64_t* d_chal, const uint64_t* d_lambda, const uint64_t* d_T_in, uint64_t* d_T_out,
                                     void* stream) {
  if (!h || !d_lambda || !d_T_out || (!h->n_columns.empty() && !d_base) || (h->n_ext && !d_ext) || (h->n_chal && !d_chal))
    return RONK_ERR_INVALID;
  AirCall c{};
  for (size_t g = 0; g < h->n_columns.size(); g++)
    if (!(c.base[g] = d_base[g])) return RONK_ERR_INVALID;
  for (u32 e = 0; e < h->n_ext; e++)
    if (!(c.ext[e] = d_ext[e])) return RONK_ERR_INVALID;
  c.chal = d_chal; c.lambda = d_lambda; c.T_in = d_T_in;
  EXT2_DISPATCH3(h->dom->c, air_launch<FF>(h, c, d_T_out, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_air_quotient(const ronk_air* h, const uint64_t* const* base, const uint64_t* const* ext, const uint64_t* chal,
                                 const uint64_t* lambda, const uint64_t* T_in, uint64_t* T_out) {
  if (!h || !lambda || !T_out || (!h->n_columns.empty() && !base) || (h->n_ext && !ext) || (h->n_chal && !chal)) return RONK_ERR_INVALID;
  for (size_t g = 0; g < h->n_columns.size(); g++)
    if (!base[g]) return RONK_ERR_INVALID;
  for (u32 e = 0; e < h->n_ext; e++)
    if (!ext[e]) return RONK_ERR_INVALID;
  const size_t M = (size_t)1 << h->dom->log2m;
  HostCall hc;
  const u64 *db[AIR_MAX_GROUPS] = {}, *de[AIR_MAX_EXT] = {};
  for (size_t g = 0; g < h->n_columns.size(); g++) db[g] = hc.in(base[g], h->n_columns[g] * M);
  for (u32 e = 0; e < h->n_ext; e++) de[e] = hc.in(ext[e], 2 * M);
  const u64 *dc = hc.in(h->n_chal ? chal : nullptr, 2 * (size_t)h->n_chal), *dl = hc.in(lambda, 2 * (size_t)h->n_constraints);
  const u64* dTin = hc.in(T_in, 2 * M);   // optional
  u64* dT = hc.out(2 * M);
  RCHK(hc.rc);
  RCHK(ronk_air_quotient_dev(h, db, de, dc, dl, dTin, dT, nullptr));
  return hc.get(T_out, dT, 2 * M * 8);
}

// ---------------------------------------------------------------------------------------------------- the verifier's side
extern "C" uint32_t ronk_air_cells(const ronk_air* h, uint32_t* cells, uint32_t cap) {
  if (!h) return 0;
  for (size_t j = 0; j < h->cells.size() && j < cap && cells; j++) cells[j] = h->cells[j];
  return (uint32_t)h->cells.size();
}

namespace {
// F_p[t] / (t^2 - w) on plain residues
struct HostExt {
  u64 p, w;
  typedef E2 V;
  V add(V a, V b) const { return V{(u64)(((u128)a.c0 + b.c0) % p), (u64)(((u128)a.c1 + b.c1) % p)}; }
  V neg(V a) const { return V{a.c0 ? p - a.c0 : 0, a.c1 ? p - a.c1 : 0}; }
  V sub(V a, V b) const { return add(a, neg(b)); }
  V mul(V a, V b) const {
    const u64 c0 = (u64)(((u128)h_mulmod(a.c0, b.c0, p) + h_mulmod(w, h_mulmod(a.c1, b.c1, p), p)) % p);
    return V{c0, (u64)(((u128)h_mulmod(a.c0, b.c1, p) + h_mulmod(a.c1, b.c0, p)) % p)};
  }
  V inv(V a) const {   // a != 0
    const u64 n = (u64)(((u128)h_mulmod(a.c0, a.c0, p) + p - h_mulmod(w, h_mulmod(a.c1, a.c1, p), p)) % p);
    const u64 ni = h_powmod(n, p - 2, p);
    return V{h_mulmod(a.c0, ni, p), h_mulmod(a.c1 ? p - a.c1 : 0, ni, p)};
  }
};
}  // namespace

extern "C" int ronk_air_eval_point(const ronk_air* h, const uint64_t z[2], const uint64_t* cell_values, const uint64_t* chal,
                                   const uint64_t* lambda, uint64_t out[2]) {
  if (!h || !z || !lambda || !out || (!h->cells.empty() && !cell_values) || (h->n_chal && !chal)) return RONK_ERR_INVALID;
  const u64 p = h->dom->p;
  const HostExt x{p, h->dom->w};
  const E2 zz{z[0] % p, z[1] % p}, one{1 % p, 0};
  E2 zn = zz;
  for (u32 b = 0; b < h->log2n; b++) zn = x.mul(zn, zn);
  if (zn.c0 == one.c0 && zn.c1 == 0) return RONK_ERR_INVALID;   // z lies on H: every divisor vanishes or is undefined
  const u64 wn = h_powmod(h->dom->g, (p - 1) >> h->log2n, p), wl = h_powmod(wn, p - 2, p);
  const u64 ninv = h_powmod(((u64)1 << h->log2n) % p, p - 2, p);
  E2 reg[AIR_MAX_REGS] = {}, acc[4] = {};
  // q_k((z w_N^rot)^(N/P)) by Horner's rule on the coefficients the handle keeps
  auto periodic = [&](u32 k, int rot) {
    const u64 N = (u64)1 << h->log2n, P = (u64)1 << h->log2_period[k];
    const u64 turn = h_powmod(wn, (u64)((int64_t)rot + (int64_t)N) % N, p);
    E2 y = x.mul(zz, E2{turn, 0});
    for (u32 b = h->log2_period[k]; b < h->log2n; b++) y = x.mul(y, y);
    const u64* q = h->per_coef.data() + h->per_at[k];
    E2 r{0, 0};
    for (u64 j = P; j-- > 0;) r = x.add(x.mul(r, y), E2{q[j], 0});
    return r;
  };
  auto operand = [&](u32 o) {
    const u32 kind = air_kind(o), idx = air_index(o);
    switch (kind) {
      case AIR_PER: return periodic(idx, air_rot(o));
      case AIR_REG: return reg[idx];
      case AIR_CHAL: return E2{chal[2 * idx] % p, chal[2 * idx + 1] % p};
      case AIR_IMM: return E2{h->imm[idx], 0};
      case AIR_X: return zz;
      default: {
        size_t j = 0;
        while (h->cells[j] != o) j++;
        return E2{cell_values[2 * j] % p, cell_values[2 * j + 1] % p};
      }
    }
  };
  for (u64 op : h->ops) {
    const u32 code = air_opcode(op);
    const E2 a = operand(air_a(op));
    if (code == AIR_EMIT) {
      const u32 j = air_b(op);
      acc[air_dst(op)] = x.add(acc[air_dst(op)], x.mul(E2{lambda[2 * j] % p, lambda[2 * j + 1] % p}, a));
      continue;
    }
    E2 r = a;
    if (code == AIR_NEG) r = x.neg(a);
    else if (code != AIR_MOV) {
      const E2 b = operand(air_b(op));
      r = code == AIR_ADD ? x.add(a, b) : code == AIR_SUB ? x.sub(a, b) : x.mul(a, b);
    }
    reg[air_dst(op)] = r;
  }
  const E2 zl = x.sub(zz, E2{wl, 0});
  const E2 vinv = x.inv(x.sub(zn, one));
  E2 v = x.mul(x.add(acc[AIR_ALL], x.mul(acc[AIR_EXCEPT_LAST], zl)), vinv);
  const E2 first = x.mul(acc[AIR_FIRST], x.inv(x.sub(zz, one)));
  const E2 last = x.mul(x.mul(acc[AIR_LAST], E2{wl, 0}), x.inv(zl));
  v = x.add(v, x.mul(x.add(first, last), E2{ninv, 0}));
  out[0] = v.c0; out[1] = v.c1;
  return RONK_OK;
}
