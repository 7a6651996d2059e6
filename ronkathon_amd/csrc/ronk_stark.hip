// ronk_stark.hip -- C ABI of libronk_ntt.so, part 18: the STARK layer (include/ronk_ntt.h "STARK"; csrc/stark_kernels.h; DESIGN.md
// section 23).  A handle joins the merged stages through their own entry points -- the transforms of ronk_plan, the constraint
// program of ronk_air on the domain of ronk_plonk, the multi-matrix commitment of ronk_mpcs -- and adds what lies between them: the
// transcript that ties commitments to challenges, the coset scaling of a round's coefficients, and the quotient split.  The prover
// is staged and never leaves the stream; the verifier enqueues its device part, synchronises once and closes the out-of-domain
// identity on the host with ronk_air_eval_point.
#include "runtime.h"
#include "hip_launch.h"
#include "poseidon_handle.h"
#include "ext2_launch.h"
#include "air_kernels.h"
#include "mpcs_kernels.h"
#include "pow_kernels.h"
#include "stark_kernels.h"

// ------------------------------------------------------------------------------------- shape
namespace {
// what the rounds and the program imply: the AIR's groups, the points and the masks
struct StarkShape {
  u32 R = 0, K = 0, J = 0, n_pub = 0, n_chal = 0, n_ext = 0, log2n = 0, log2b = 0;
  u32 F = 0, fo = 0;                  // the fixed round's columns; 1 when there is one: trace round r is round fo + r of the commitment
  u32 C[STARK_MAX_R] = {}, E[STARK_MAX_R] = {}, draw[STARK_MAX_R] = {};
  u32 base[STARK_MAX_R] = {}, boff[STARK_MAX_R] = {}, eoff[STARK_MAX_R] = {};
  std::vector<u32> groups;            // the non-empty base parts, in round order
  std::vector<u32> cells, rots;       // rots[k]: point k is zeta w_N^rots[k]; rots[0] = 0
  // the inner commitment's rounds: the fixed round if there is one, the trace rounds, then the quotient
  u32 cols[STARK_MAX_R + 2] = {}, masks[STARK_MAX_R + 2] = {};
  u32 rounds() const { return fo + R + 1; }
  // the round of the inner commitment that holds a column cell, and the cell's first row there
  bool where(u32 kind, u32 index, u32* round, u32* row) const {
    if (kind == AIR_BASE && index < F) { *round = 0; *row = index; return true; }
    for (u32 r = 0; r < R; r++) {
      if (kind == AIR_BASE && index >= boff[r] && index < boff[r] + base[r]) { *round = fo + r; *row = index - boff[r]; return true; }
      if (kind == AIR_EXT && index >= eoff[r] && index < eoff[r] + E[r]) { *round = fo + r; *row = base[r] + 2 * (index - eoff[r]); return true; }
    }
    return false;
  }
  u32 rot_mod_n(int rot) const {
    const int64_t N = (int64_t)1 << log2n;
    return (u32)(((int64_t)rot % N + N) % N);
  }
  // the point of a rotation, or the number of points when there is none yet
  u32 point_of(int rot) const {
    const u32 m = rot_mod_n(rot);
    for (u32 k = 0; k < rots.size(); k++)
      if (rots[k] == m) return k;
    return (u32)rots.size();
  }
};

int air_code(AirStatus s) { return s == AIR_OK ? RONK_OK : s == AIR_INVALID ? RONK_ERR_INVALID : RONK_ERR_UNSUPPORTED; }

// The codes of ronk_stark_check_fixed in their order; fills *s for a shape that passes.  Where the arrays or R are refused only at the
// end, the earlier checks run on what can be derived: the first four rounds, E_r clamped to C_r / 2, no rounds for a NULL array.
int stark_check(u64 p, u32 rate, u64 g, u64 w, u32 log2_n, u32 log2_b, u64 shift, u32 log2_arity, u32 log2_final, u32 n_queries,
                u32 digest_len, u32 R, const u32* n_columns, const u32* n_ext, u32 n_pub, const u32* n_draw, u32 n_chal, u32 n_imm,
                u32 n_regs, u32 J, const u64* ops, u32 n_ops, u32 n_fixed, u32 n_per, const u32* log2_period, StarkShape* s) {
  const bool arrays = n_columns && n_ext && n_draw;
  s->R = arrays ? (R < STARK_MAX_R ? R : STARK_MAX_R) : 0;
  s->J = J; s->n_pub = n_pub; s->n_chal = n_chal; s->log2n = log2_n; s->log2b = log2_b;
  s->F = n_fixed; s->fo = n_fixed ? 1 : 0;
  if (n_fixed) s->groups.push_back(n_fixed);   // the fixed round is group 0 and takes the first flat base indices
  u32 bo = n_fixed, eo = 0;
  for (u32 r = 0; r < s->R; r++) {
    s->C[r] = n_columns[r];
    s->E[r] = n_ext[r] < n_columns[r] / 2 ? n_ext[r] : n_columns[r] / 2;
    s->draw[r] = n_draw[r];
    s->base[r] = s->C[r] - 2 * s->E[r];
    s->boff[r] = bo; s->eoff[r] = eo;
    bo += s->base[r]; eo += s->E[r];
    if (s->base[r]) s->groups.push_back(s->base[r]);
  }
  s->n_ext = eo;
  // 1. the program, as ronk_air_check sees it
  const AirShape as{log2_n, (u32)s->groups.size(), s->groups.data(), s->n_ext, n_chal, n_imm, n_regs, J, n_per, log2_period};
  std::vector<u64> tape;
  u32 boundary = 0;
  RCHK(air_code(air_compile(as, ops, n_ops, &tape, &boundary, &s->cells)));
  // the points: zeta, then every distinct non-zero rot mod N in the cells' order; the masks
  s->rots.assign(1, 0);
  const u32 fo = s->fo, RQ = fo + s->R;   // the quotient's round
  if (fo) { s->cols[0] = n_fixed; s->masks[0] = 1; }
  for (u32 r = 0; r < s->R; r++) { s->cols[fo + r] = s->C[r]; s->masks[fo + r] = 1; }
  for (u32 o : s->cells) {
    u32 k = s->point_of(air_rot(o)), r = 0, row = 0;
    if (k == s->rots.size()) s->rots.push_back(s->rot_mod_n(air_rot(o)));
    if (s->where(air_kind(o), air_index(o), &r, &row) && k < STARK_MAX_K) s->masks[r] |= 1u << k;
  }
  s->K = (u32)s->rots.size();
  s->cols[RQ] = 2u << (log2_b < 20 ? log2_b : 20);
  s->masks[RQ] = 1;
  // 2. the inner commitment on the derived shape (more than eight points are refused at the end)
  RCHK(ronk_mpcs_check(p, rate, g, w, log2_n + log2_b, shift, log2_arity, log2_final, log2_b, n_queries, digest_len,
                       s->K < STARK_MAX_K ? s->K : STARK_MAX_K, RQ + 1, arrays ? s->cols : nullptr, s->masks));
  // 3. the domain
  const u64 labels[3] = {1, 2, 3};
  RCHK(ronk_plonk_check(p, g, w, log2_n, log2_b, shift, labels));
  // 4. this family's own
  if (!arrays || R == 0) return RONK_ERR_INVALID;
  u64 chal = n_pub;
  for (u32 r = 0; r < s->R; r++) {
    if (2 * (u64)n_ext[r] > n_columns[r]) return RONK_ERR_INVALID;
    chal += n_draw[r];
  }
  if (chal != n_chal) return RONK_ERR_INVALID;
  if (R > STARK_MAX_R || s->K > STARK_MAX_K) return RONK_ERR_UNSUPPORTED;
  return RONK_OK;
}

struct StarkPlan {
  u32 log2n;
  u64 batch;
  ronk_plan* pl;
};
}  // namespace

extern "C" int ronk_stark_check_fixed(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                                      uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                      uint32_t digest_len, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext,
                                      uint32_t n_pub, const uint32_t* n_draw, uint32_t n_chal, uint32_t n_imm, uint32_t n_regs,
                                      uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops, uint32_t n_fixed, uint32_t n_per,
                                      const uint32_t* log2_period) {
  StarkShape s;
  return stark_check(p, rate, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len, n_rounds, n_columns,
                     n_ext, n_pub, n_draw, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, n_fixed, n_per, log2_period, &s);
}

extern "C" int ronk_stark_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                                uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw,
                                uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops,
                                uint32_t n_ops) {
  return ronk_stark_check_fixed(p, rate, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len, n_rounds,
                                n_columns, n_ext, n_pub, n_draw, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, 0, 0, nullptr);
}

// ------------------------------------------------------------------------------------- handle
struct ronk_stark {
  const ronk_poseidon* pos = nullptr;   // borrowed
  ronk_plonk* dom = nullptr;            // owned, with everything below
  ronk_air* air = nullptr;
  ronk_mpcs* mpcs = nullptr;
  std::vector<StarkPlan> plans;
  StarkShape s;
  Ext2Launch c;
  u64 p = 0, w = 0, shift = 0, sinv = 0, wn = 0;   // plain residues
  u32 D = 0, Q = 0, log2_arity = 0, pow_bits = 0;
  u64 tree_words = 0;
  StarkRots rots{};
  u64* d_vs = nullptr;                  // the verifier's transcript state (the layout of the workspace's head), its status word, and
                                        // with a fixed round the root list of the inner verifier, [R + 2][D]
  const u64* fixed = nullptr;           // borrowed: the whole buffer of ronk_stark_fixed_commit_dev, or NULL
  const u64* fixed_root = nullptr;      // borrowed: the fixed round's root (inside `fixed` when that is set), or NULL
  u64* own_fixed = nullptr;             // owned: what ronk_stark_set_fixed copied to the device
  int stage = -1;                       // the trace round the prover expects next, R for finish, -1 before begin
  const u64* work = nullptr;            // the workspace of the sequence in flight

  u64 N() const { return (u64)1 << s.log2n; }
  u64 M() const { return (u64)1 << (s.log2n + s.log2b); }
  // the head of a workspace: t [D], the challenge table [n_chal][2] with lambda [2] right behind it (the last round's draw is one
  // squeeze), the weights [J][2], zeta [2], the points [2][K]
  u64 off_chal() const { return D; }
  u64 off_lambda() const { return off_chal() + 2 * (u64)s.n_chal; }
  u64 off_weights() const { return off_lambda() + 2; }
  u64 off_zeta() const { return off_weights() + 2 * (u64)s.J; }
  u64 off_z() const { return off_zeta() + 2; }
  u64 head_words() const { return off_z() + 2 * (u64)s.K; }
  // then per round of the inner commitment but the fixed one, which lives in the caller's d_fixed (the quotient last): the extended
  // matrix [C][M], the coefficients [C][N], the tree.  r counts the inner commitment's rounds.
  u64 round_words(u32 r) const { return s.cols[r] * (M() + N()) + tree_words; }
  u64 off_round(u32 r) const {
    u64 o = head_words();
    for (u32 q = s.fo; q < r; q++) o += round_words(q);
    return o;
  }
  u64 off_T() const { return off_round(s.rounds()); }
  u64 msg_rows() const {
    u64 m = 0;
    for (u32 r = s.fo; r < s.rounds(); r++) m = s.cols[r] > m ? s.cols[r] : m;
    return m;
  }
  // d_fixed: the extended matrix [F][M], the coefficients [F][N], the tree, the coset-basis scratch [F][N]
  u64 fixed_words() const { return s.F ? s.F * (M() + 2 * N()) + tree_words : 0; }
  const u64* root_in(const u64* d_fixed) const { return d_fixed + s.F * (M() + N()) + tree_words - D; }
  u64 off_msg() const { return off_T() + 2 * M(); }
  u64 off_inner() const { return off_msg() + msg_rows() * N(); }
  u64 workspace_words() const { return off_inner() + ronk_mpcs_handle_workspace_words(mpcs); }
  u64 roots_words() const { return (u64)(s.R + 1) * D; }
  u64 proof_words() const { return roots_words() + ronk_mpcs_handle_proof_words(mpcs); }
  u64 claims() const {
    u64 y = 0;
    for (u32 r = 0; r < s.rounds(); r++) y += (u64)mpcs_popcount(s.masks[r]) * s.cols[r];
    return y;
  }
  ronk_plan* plan(u32 log2n, u64 batch) const {
    for (const StarkPlan& e : plans)
      if (e.log2n == log2n && e.batch == batch) return e.pl;
    return nullptr;
  }
};

extern "C" int ronk_stark_destroy(ronk_stark* h) {
  if (!h) return RONK_ERR_INVALID;
  for (StarkPlan& e : h->plans) (void)ronk_plan_destroy(e.pl);
  if (h->mpcs) (void)ronk_mpcs_destroy(h->mpcs);
  if (h->air) (void)ronk_air_destroy(h->air);
  if (h->dom) (void)ronk_plonk_destroy(h->dom);
  if (h->d_vs) (void)hipFree(h->d_vs);
  if (h->own_fixed) (void)hipFree(h->own_fixed);
  delete h;
  return RONK_OK;
}

static int stark_add_plan(ronk_stark* h, u64 g, u32 log2n, u64 batch) {
  if (h->plan(log2n, batch)) return RONK_OK;
  ronk_plan* pl = nullptr;
  RCHK(ronk_plan_create(&pl, h->p, g, log2n, batch, -1));
  h->plans.push_back(StarkPlan{log2n, batch, pl});
  return RONK_OK;
}

extern "C" int ronk_stark_create_fixed(ronk_stark** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n,
                                       uint32_t log2_blowup, uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final,
                                       uint32_t n_queries, uint32_t digest_len, uint32_t n_rounds, const uint32_t* n_columns,
                                       const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw, uint32_t n_chal, uint32_t n_imm,
                                       uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops, const uint64_t* imm,
                                       uint32_t n_fixed, uint32_t n_per, const uint32_t* log2_period, const uint64_t* per_values) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!pos || (n_imm && !imm)) return RONK_ERR_INVALID;
  ronk_stark* h = new ronk_stark;
  int rc = stark_check(pos->p, pos->rate, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len, n_rounds,
                       n_columns, n_ext, n_pub, n_draw, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, n_fixed, n_per, log2_period,
                       &h->s);
  if (rc == RONK_OK && n_per && !per_values) rc = RONK_ERR_INVALID;
  if (rc == RONK_OK) rc = need_device();
  if (rc != RONK_OK) { delete h; return rc; }
  const StarkShape& s = h->s;
  const u64 p = pos->p;
  h->pos = pos; h->p = p; h->D = digest_len; h->Q = n_queries; h->log2_arity = log2_arity;
  h->shift = coset_shift % p;
  h->w = w % p;
  h->sinv = h_powmod(h->shift, p - 2, p);
  h->wn = h_powmod(g, (p - 1) >> log2_n, p);
  h->c = ext2_launch(p, w);
  h->tree_words = ronk_merkle_tree_words((size_t)1 << (log2_n + log2_blowup - log2_arity), digest_len);
  h->rots.K = s.K;
  for (u32 k = 0; k < s.K; k++) h->rots.m[k] = ext2_reg_form(h->c.mont, p, h_powmod(h->wn, s.rots[k], p));
  const u64 labels[3] = {1, 2, 3};
  rc = ronk_plonk_create(&h->dom, p, g, w, log2_n, log2_blowup, coset_shift, labels);
  if (rc == RONK_OK)
    rc = ronk_air_create_per(&h->air, h->dom, (u32)s.groups.size(), s.groups.data(), s.n_ext, n_chal, n_imm, n_regs, n_constraints, ops,
                             n_ops, imm, n_per, log2_period, per_values);
  if (rc == RONK_OK)
    rc = ronk_mpcs_create(&h->mpcs, pos, g, w, log2_n + log2_blowup, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len,
                          s.K, s.rounds(), s.cols, s.masks);
  // a trace round: the inverse transform on H and the encode on the coset's group, both of its batch; the quotient: the inverse
  // transform of the two planes of T and the encode of the 2 B pieces; the fixed round goes the way of a trace round
  for (u32 r = 0; r < s.fo + s.R && rc == RONK_OK; r++) {
    rc = stark_add_plan(h, g, log2_n, s.cols[r]);
    if (rc == RONK_OK) rc = stark_add_plan(h, g, log2_n + log2_blowup, s.cols[r]);
  }
  if (rc == RONK_OK) rc = stark_add_plan(h, g, log2_n + log2_blowup, 2);
  if (rc == RONK_OK) rc = stark_add_plan(h, g, log2_n + log2_blowup, s.cols[s.fo + s.R]);
  if (rc == RONK_OK) {
    const hipError_t e = hipMalloc((void**)&h->d_vs, (h->head_words() + 1 + (s.fo ? (u64)s.rounds() * digest_len : 0)) * 8);
    if (e != hipSuccess) rc = hip_fail(e, "ronk_stark_create");
  }
  if (rc != RONK_OK) { ronk_stark_destroy(h); return rc; }
  *out = h;
  return RONK_OK;
}

extern "C" int ronk_stark_create(ronk_stark** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                                 uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                 uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw,
                                 uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops,
                                 uint32_t n_ops, const uint64_t* imm) {
  return ronk_stark_create_fixed(out, pos, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len, n_rounds,
                                 n_columns, n_ext, n_pub, n_draw, n_chal, n_imm, n_regs, n_constraints, ops, n_ops, imm, 0, 0, nullptr,
                                 nullptr);
}

extern "C" int ronk_stark_set_pow(ronk_stark* h, uint32_t bits, uint32_t log2_limit) {
  if (!h) return RONK_ERR_INVALID;
  RCHK(ronk_mpcs_set_pow(h->mpcs, bits, log2_limit));
  h->pow_bits = bits;
  return RONK_OK;
}
extern "C" size_t ronk_stark_proof_words(const ronk_stark* h) { return h ? (size_t)h->proof_words() : 0; }
extern "C" size_t ronk_stark_workspace_words(const ronk_stark* h) { return h ? (size_t)h->workspace_words() : 0; }
extern "C" size_t ronk_stark_fixed_words(const ronk_stark* h) { return h ? (size_t)h->fixed_words() : 0; }

// ------------------------------------------------------------------------------------- transcript steps
// t <- sponge(seed || pub), the public pairs into the table at `head`
static int stark_begin_launch(const ronk_stark* h, const u64* d_seed, const u64* d_pub, u64* head, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((stark_begin_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, h->D, d_seed, d_pub, h->s.n_pub, head,
                                       head + h->off_chal()));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
// the step after the commitment of trace round r: its draws into the table, and after the last round lambda and the weights
static int stark_round_launch(const ronk_stark* h, u32 r, const u64* d_root, u64* head, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  const StarkShape& sh = h->s;
  u64 at = sh.n_pub;
  for (u32 q = 0; q < r; q++) at += sh.draw[q];
  const bool last = r + 1 == sh.R;
  const u32 n = 2 * (sh.draw[r] + (last ? 1 : 0));
  POS_DISPATCH(pos, hipLaunchKernelGGL((stark_draw_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, h->D, head, d_root, n,
                                       head + h->off_chal() + 2 * at));
  HIPCHK(hipGetLastError());
  if (last) {
    EXT2_DISPATCH3(h->c, hipLaunchKernelGGL((stark_weights_kernel<FF>), dim3(1), dim3(64), 0, s, h->c.k, h->c.w, head + h->off_lambda(), sh.J,
                                            head + h->off_weights()));
    HIPCHK(hipGetLastError());
  }
  return RONK_OK;
}
// the step after the quotient's commitment: zeta and the points
static int stark_points_launch(const ronk_stark* h, const u64* d_root, u64* head, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((stark_draw_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, h->D, head, d_root, 2u,
                                       head + h->off_zeta()));
  HIPCHK(hipGetLastError());
  EXT2_DISPATCH2(h->c, hipLaunchKernelGGL((stark_points_kernel<FF>), dim3(1), dim3(64), 0, s, h->c.k, head + h->off_zeta(), h->rots,
                                          head + h->off_z()));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// the step that binds the fixed round: t <- sponge(t || root_F), the draw step with no draw
static int stark_fixed_launch(const ronk_stark* h, u64* head, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((stark_draw_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, h->D, head, h->fixed_root, 0u,
                                       head + h->off_chal()));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- the fixed round
// a round's matrix on H into its extension on the coset, its coefficients and its tree: what a trace round and the fixed round share
static int stark_commit_matrix(const ronk_stark* h, u32 round, const u64* d_evals, u64* d_ext, u64* d_coef, u64* d_tree, u64* d_msg,
                               void* stream) {
  const StarkShape& sh = h->s;
  const u32 C = sh.cols[round], log2m = sh.log2n + sh.log2b;
  const u64 N = h->N(), p = h->p;
  RCHK(ronk_ntt_inverse_dev(h->plan(sh.log2n, C), d_evals, d_coef, stream));
  const u32 grid = grid_for(N);
  const bool mont = h->c.mont;
  const StarkShift sf{ext2_reg_form(mont, p, h->shift), 0, ext2_reg_form(mont, p, h_powmod(h->shift, (u64)grid * 256, p))};
  EXT2_DISPATCH2(h->c, hipLaunchKernelGGL((stark_shift_kernel<FF>), dim3(grid), dim3(256), 0, (hipStream_t)stream, h->c.k, sf, sh.log2n, C,
                                          d_coef, d_msg));
  HIPCHK(hipGetLastError());
  RCHK(ronk_rs_encode_batch_dev(h->plan(log2m, C), d_msg, N, d_ext, stream));
  return ronk_mpcs_commit_dev(h->mpcs, round, d_ext, d_tree, stream);
}

extern "C" int ronk_stark_fixed_commit_dev(const ronk_stark* h, const uint64_t* d_evals, uint64_t* d_fixed, void* stream) {
  if (!h || !h->s.F || !d_evals || !d_fixed) return RONK_ERR_INVALID;
  const u64 F = h->s.F, N = h->N(), M = h->M();
  u64* d_coef = d_fixed + F * M;
  u64* d_tree = d_coef + F * N;
  return stark_commit_matrix(h, 0, d_evals, d_fixed, d_coef, d_tree, d_tree + h->tree_words, stream);
}

extern "C" const uint64_t* ronk_stark_fixed_root_dev(const ronk_stark* h, const uint64_t* d_fixed) {
  return h && h->s.F && d_fixed ? h->root_in(d_fixed) : nullptr;
}

static void stark_drop_fixed(ronk_stark* h) {
  if (h->own_fixed) (void)hipFree(h->own_fixed);
  h->own_fixed = nullptr; h->fixed = nullptr; h->fixed_root = nullptr;
  h->stage = -1;   // a sequence in flight was bound to the old round
}

extern "C" int ronk_stark_set_fixed_dev(ronk_stark* h, const uint64_t* d_fixed) {
  if (!h || !h->s.F || !d_fixed) return RONK_ERR_INVALID;
  stark_drop_fixed(h);
  h->fixed = d_fixed;
  h->fixed_root = h->root_in(d_fixed);
  return RONK_OK;
}

extern "C" int ronk_stark_set_fixed_root_dev(ronk_stark* h, const uint64_t* d_root) {
  if (!h || !h->s.F || !d_root) return RONK_ERR_INVALID;
  stark_drop_fixed(h);
  h->fixed_root = d_root;
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- prover
extern "C" int ronk_stark_begin_dev(ronk_stark* h, const uint64_t* d_seed, const uint64_t* d_pub, uint64_t* d_work, void* stream) {
  if (!h || !d_seed || !d_work || (h->s.n_pub && !d_pub)) return RONK_ERR_INVALID;
  if (h->s.F && !h->fixed) return RONK_ERR_INVALID;   // no fixed round is set, or its root only: that serves a verifier
  RCHK(stark_begin_launch(h, d_seed, d_pub, d_work, (hipStream_t)stream));
  if (h->s.F) RCHK(stark_fixed_launch(h, d_work, (hipStream_t)stream));
  h->stage = 0;
  h->work = d_work;
  return RONK_OK;
}

extern "C" const uint64_t* ronk_stark_challenges_dev(const ronk_stark* h, const uint64_t* d_work) {
  return h && d_work ? d_work + h->off_chal() : nullptr;
}

extern "C" int ronk_stark_commit_round_dev(ronk_stark* h, uint32_t round, const uint64_t* d_evals, uint64_t* d_work, void* stream) {
  if (!h || !d_evals || !d_work) return RONK_ERR_INVALID;
  if (round >= h->s.R || h->stage != (int)round || h->work != d_work) return RONK_ERR_INVALID;   // rounds go in order, after begin
  const StarkShape& sh = h->s;
  const u32 C = sh.C[round];
  const u64 N = h->N(), M = h->M();
  u64* d_ext = d_work + h->off_round(sh.fo + round);
  u64* d_coef = d_ext + C * M;
  u64* d_tree = d_coef + C * N;
  h->stage = -1;   // a failed step ends the sequence
  RCHK(stark_commit_matrix(h, sh.fo + round, d_evals, d_ext, d_coef, d_tree, d_work + h->off_msg(), stream));
  RCHK(stark_round_launch(h, round, d_tree + h->tree_words - h->D, d_work, (hipStream_t)stream));
  h->stage = (int)round + 1;
  return RONK_OK;
}

// the split as a building block: d_c planar [2][M], what the inverse transform of T's planes leaves; d_coef, d_msg: [2B][N]
extern "C" int ronk_stark_split_dev(const ronk_stark* h, const uint64_t* d_c, uint64_t* d_coef, uint64_t* d_msg, void* stream) {
  if (!h || !d_c || !d_coef || !d_msg) return RONK_ERR_INVALID;
  const u64 N = h->N(), p = h->p;
  const u32 grid = grid_for(N);
  const bool mont = h->c.mont;
  const StarkShift sf{ext2_reg_form(mont, p, h->sinv), ext2_reg_form(mont, p, h_powmod(h->sinv, N, p)),
                      ext2_reg_form(mont, p, h_powmod(h->sinv, (u64)grid * 256, p))};
  EXT2_DISPATCH3(h->c, hipLaunchKernelGGL((stark_split_kernel<FF>), dim3(grid), dim3(256), 0, (hipStream_t)stream, h->c.k, sf, h->s.log2n,
                                          h->s.log2b, d_c, d_coef, d_msg));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_stark_finish_dev(ronk_stark* h, uint64_t* d_work, uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || !d_work || !d_proof || !d_status) return RONK_ERR_INVALID;
  if (h->stage != (int)h->s.R || h->work != d_work) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const StarkShape& sh = h->s;
  const u32 fo = sh.fo, R = fo + sh.R, log2m = sh.log2n + sh.log2b, CQ = sh.cols[R];   // R: the quotient's round of the inner commitment
  const u64 N = h->N(), M = h->M();
  h->stage = -1;
  if (fo && !h->fixed) return RONK_ERR_INVALID;
  const u64 *d_M[STARK_MAX_R + 2], *d_tree[STARK_MAX_R + 2], *d_coef[STARK_MAX_R + 2];
  const u64 *d_base[AIR_MAX_GROUPS] = {}, *d_ext[AIR_MAX_EXT] = {};
  u32 ng = 0, ne = 0;
  if (fo) d_base[ng++] = h->fixed;
  for (u32 r = 0; r <= R; r++) {
    d_M[r] = fo && r == 0 ? h->fixed : d_work + h->off_round(r);
    d_coef[r] = d_M[r] + sh.cols[r] * M;
    d_tree[r] = d_coef[r] + sh.cols[r] * N;
    if (r == R || r < fo) continue;
    const u32 tr = r - fo;
    if (sh.base[tr]) d_base[ng++] = d_M[r];
    for (u32 e = 0; e < sh.E[tr]; e++) d_ext[ne++] = d_M[r] + (sh.base[tr] + 2 * (u64)e) * M;
  }
  u64* d_T = d_work + h->off_T();
  u64* d_msg = d_work + h->off_msg();
  u64* d_MQ = d_work + h->off_round(R);
  u64* d_coefQ = d_MQ + CQ * M;
  u64* d_treeQ = d_coefQ + CQ * N;
  // the quotient on the extended rounds, its coefficients in the coset basis (both planes in one batch of two, in place)
  RCHK(ronk_air_quotient_dev(h->air, d_base, d_ext, d_work + h->off_chal(), d_work + h->off_weights(), nullptr, d_T, stream));
  RCHK(ronk_ntt_inverse_dev(h->plan(log2m, 2), d_T, d_T, stream));
  // the split, the pieces back on the coset, their commitment
  RCHK(ronk_stark_split_dev(h, d_T, d_coefQ, d_msg, stream));
  RCHK(ronk_rs_encode_batch_dev(h->plan(log2m, CQ), d_msg, N, d_MQ, stream));
  RCHK(ronk_mpcs_commit_dev(h->mpcs, R, d_MQ, d_treeQ, stream));
  RCHK(stark_points_launch(h, d_treeQ + h->tree_words - h->D, d_work, s));
  // the opening under the transcript's last state; then bit 128 beside its status, and the roots in front of its proof
  RCHK(ronk_mpcs_open_dev(h->mpcs, d_M, d_tree, d_coef, d_work + h->off_z(), d_work, d_work + h->off_inner(), d_proof + h->roots_words(),
                          d_status, stream));
  hipLaunchKernelGGL(stark_flag_kernel, dim3(1), dim3(64), 0, s, d_work + h->off_zeta(), d_status);
  HIPCHK(hipGetLastError());
  for (u32 r = fo; r <= R; r++)   // the fixed root is the verifier's own: the proof does not carry it
    HIPCHK(hipMemcpyAsync(d_proof + (u64)(r - fo) * h->D, d_tree[r] + h->tree_words - h->D, h->D * 8, hipMemcpyDeviceToDevice, s));
  return RONK_OK;
}

extern "C" int ronk_stark_prove_dev(ronk_stark* h, const uint64_t* d_seed, const uint64_t* d_pub, const uint64_t* d_evals, uint64_t* d_work,
                                    uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || h->s.R != 1) return RONK_ERR_INVALID;
  if (!d_evals || !d_proof || !d_status) return RONK_ERR_INVALID;
  RCHK(ronk_stark_begin_dev(h, d_seed, d_pub, d_work, stream));
  RCHK(ronk_stark_commit_round_dev(h, 0, d_evals, d_work, stream));
  return ronk_stark_finish_dev(h, d_work, d_proof, d_status, stream);
}

// ------------------------------------------------------------------------------------- verifier
namespace {
// F_p[t] / (t^2 - w) on plain residues
struct HostPair {
  u64 p, w;
  E2 add(E2 a, E2 b) const { return E2{(u64)(((u128)a.c0 + b.c0) % p), (u64)(((u128)a.c1 + b.c1) % p)}; }
  E2 mul(E2 a, E2 b) const {
    const u64 c0 = (u64)(((u128)h_mulmod(a.c0, b.c0, p) + h_mulmod(w, h_mulmod(a.c1, b.c1, p), p)) % p);
    return E2{c0, (u64)(((u128)h_mulmod(a.c0, b.c1, p) + h_mulmod(a.c1, b.c0, p)) % p)};
  }
  // a + t b
  E2 join(E2 a, E2 b) const { return add(a, mul(E2{0, 1 % p}, b)); }
};
}  // namespace

extern "C" int ronk_stark_verify_dev(ronk_stark* h, const uint64_t* d_seed, const uint64_t* d_pub, const uint64_t* d_proof, int* status,
                                     void* stream) {
  if (!h || !d_seed || !d_proof || !status || (h->s.n_pub && !d_pub)) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const StarkShape& sh = h->s;
  if (sh.F && !h->fixed_root) return RONK_ERR_INVALID;
  const u32 R = sh.fo + sh.R;   // the quotient's round of the inner commitment
  const u64 p = h->p, Y = h->claims();
  u64* head = h->d_vs;
  int* d_st = (int*)(head + h->head_words());
  const u64* d_inner = d_proof + h->roots_words();
  // the transcript from the seed, the public inputs, the verifier's own fixed root and the proof's roots
  RCHK(stark_begin_launch(h, d_seed, d_pub, head, s));
  if (sh.F) RCHK(stark_fixed_launch(h, head, s));
  for (u32 r = 0; r < sh.R; r++) RCHK(stark_round_launch(h, r, d_proof + (u64)r * h->D, head, s));
  RCHK(stark_points_launch(h, d_proof + (u64)sh.R * h->D, head, s));
  // the inner opening's root list: the proof's, after the fixed root when there is one
  const u64* d_roots = d_proof;
  if (sh.F) {
    u64* d_list = head + h->head_words() + 1;
    HIPCHK(hipMemcpyAsync(d_list, h->fixed_root, h->D * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(d_list + h->D, d_proof, h->roots_words() * 8, hipMemcpyDeviceToDevice, s));
    d_roots = d_list;
  }
  RCHK(ronk_mpcs_verify_dev(h->mpcs, d_roots, head + h->off_z(), head, d_inner, d_st, stream));
  hipLaunchKernelGGL(stark_flag_kernel, dim3(1), dim3(64), 0, s, head + h->off_zeta(), d_st);
  HIPCHK(hipGetLastError());
  // what the host needs, then the one synchronisation
  std::vector<u64> hv(h->head_words() + 1), y(2 * Y);
  HIPCHK(hipMemcpyAsync(hv.data(), head, hv.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(y.data(), d_inner, y.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int st = 0;
  memcpy(&st, &hv[h->head_words()], sizeof(int));
  // the out-of-domain identity: sum_i zeta^(i N) (y_Q[2 i] + t y_Q[2 i + 1]) against the program at zeta on the opened cells
  const HostPair x{p, h->w};
  MpcsShape ms{};
  ms.R = R + 1; ms.K = sh.K;
  u32 yo = 0;
  for (u32 r = 0; r <= R; r++) { ms.C[r] = sh.cols[r]; ms.mask[r] = sh.masks[r]; ms.yoff[r] = yo; yo += mpcs_popcount(sh.masks[r]) * sh.cols[r]; }
  auto claim = [&](u32 r, u32 k, u32 c) {
    const u32 i = mpcs_claim_index(ms, r, k, c);
    return E2{y[i] % p, y[Y + i] % p};
  };
  std::vector<u64> cv(2 * sh.cells.size() + 2);
  for (size_t j = 0; j < sh.cells.size(); j++) {
    const u32 o = sh.cells[j], k = sh.point_of(air_rot(o));
    u32 r = 0, row = 0;
    (void)sh.where(air_kind(o), air_index(o), &r, &row);
    const E2 v = air_kind(o) == AIR_BASE ? claim(r, k, row) : x.join(claim(r, k, row), claim(r, k, row + 1));
    cv[2 * j] = v.c0; cv[2 * j + 1] = v.c1;
  }
  const u64* zeta = &hv[h->off_zeta()];
  E2 zn{zeta[0] % p, zeta[1] % p}, lhs{0, 0};
  for (u32 b = 0; b < sh.log2n; b++) zn = x.mul(zn, zn);
  for (u32 i = (u32)1 << sh.log2b; i-- > 0;) lhs = x.add(x.mul(lhs, zn), x.join(claim(R, 0, 2 * i), claim(R, 0, 2 * i + 1)));
  u64 rhs[2] = {0, 0};
  const int rc = ronk_air_eval_point(h->air, zeta, cv.data(), &hv[h->off_chal()], &hv[h->off_weights()], rhs);
  if (rc != RONK_OK || rhs[0] != lhs.c0 || rhs[1] != lhs.c1) st |= 256;   // zeta^N = 1: the identity cannot be evaluated
  *status = st;
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
extern "C" int ronk_stark_prove(ronk_stark* h, const uint64_t* seed, const uint64_t* pub, const uint64_t* evals, uint64_t* proof,
                                int* status) {
  if (!h || h->s.R != 1 || !seed || !evals || !proof || !status || (h->s.n_pub && !pub)) return RONK_ERR_INVALID;
  HostCall hc;
  const u64 *ds = hc.in(seed, h->D), *dp = hc.in(h->s.n_pub ? pub : nullptr, 2 * (size_t)h->s.n_pub),
            *de = hc.in(evals, (size_t)h->s.C[0] * h->N());
  u64 *dw = hc.out(h->workspace_words()), *dpr = hc.out(h->proof_words()), *dst = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_stark_prove_dev(h, ds, dp, de, dw, dpr, (int*)dst, nullptr));
  RCHK(hc.get(proof, dpr, h->proof_words() * 8));
  RCHK(hc.get(status, dst, sizeof(int)));
  if (!h->pow_bits) return RONK_OK;
  // the embedded FRI proof's last word is the nonce: the search found nothing below the limit
  u64 rounds = 0;
  const u64 A = (u64)1 << h->log2_arity, depth = h->s.log2n + h->s.log2b - h->log2_arity;
  for (u32 r = 0; r < h->s.rounds(); r++) rounds += h->Q * h->s.cols[r] * A + h->Q * depth * h->D;
  return proof[h->proof_words() - rounds - 1] == POW_NONE ? RONK_ERR_INDEX : RONK_OK;
}

// The host-pointer forms of the fixed round: the commit into a host buffer of ronk_stark_fixed_words words, and a host buffer (or,
// root_only, its D root words alone) onto the device, where the handle owns the copy.
extern "C" int ronk_stark_fixed_commit(const ronk_stark* h, const uint64_t* evals, uint64_t* fixed) {
  if (!h || !h->s.F || !evals || !fixed) return RONK_ERR_INVALID;
  HostCall hc;
  const u64* de = hc.in(evals, (size_t)h->s.F * h->N());
  u64* df = hc.out(h->fixed_words());
  RCHK(hc.rc);
  RCHK(ronk_stark_fixed_commit_dev(h, de, df, nullptr));
  return hc.get(fixed, df, h->fixed_words() * 8);
}

extern "C" int ronk_stark_set_fixed(ronk_stark* h, const uint64_t* fixed, int root_only) {
  if (!h || !h->s.F || !fixed) return RONK_ERR_INVALID;
  const u64 words = root_only ? h->D : h->fixed_words();
  u64* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, words * 8);
  if (e == hipSuccess) e = hipMemcpy(d, fixed, words * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (d) (void)hipFree(d); return hip_fail(e, "ronk_stark_set_fixed"); }
  const int rc = root_only ? ronk_stark_set_fixed_root_dev(h, d) : ronk_stark_set_fixed_dev(h, d);
  if (rc != RONK_OK) { (void)hipFree(d); return rc; }
  h->own_fixed = d;
  return RONK_OK;
}

extern "C" int ronk_stark_verify(ronk_stark* h, const uint64_t* seed, const uint64_t* pub, const uint64_t* proof, int* status) {
  if (!h || !seed || !proof || !status || (h->s.n_pub && !pub)) return RONK_ERR_INVALID;
  HostCall hc;
  const u64 *ds = hc.in(seed, h->D), *dp = hc.in(h->s.n_pub ? pub : nullptr, 2 * (size_t)h->s.n_pub), *dpr = hc.in(proof, h->proof_words());
  RCHK(hc.rc);
  return ronk_stark_verify_dev(h, ds, dp, dpr, status, nullptr);
}
