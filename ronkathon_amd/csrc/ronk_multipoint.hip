// ronk_multipoint.hip -- C ABI of libronk_ntt.so, part 8: one polynomial at many arbitrary points, and the interpolating
// polynomial through arbitrary nodes, in O(m log^2 m) on the retained product tree (csrc/multipoint_kernels.h; DESIGN.md
// "Multipoint evaluation and interpolation"), with a direct O(m d) / O(m^2) form for small sizes and primes without the
// tree's 2-adicity.
#include "roots_host.h"
#include "multipoint_kernels.h"

// ------------------------------------------------------------------------------------- kernels
template <class FLD>
__global__ void __launch_bounds__(MP_DIRECT_BLOCK) mp_horner_kernel(FieldConst fc, u64 p, const u64* __restrict__ c, u64 d,
                                                                    const u64* __restrict__ xs, u64 m, u64* __restrict__ out) {
  __shared__ u64 lds[MP_CH];
  const FLD f(fc);
  mp_horner_body(f, p, c, d, xs, m, out, lds, threadIdx.x, blockIdx.x, MP_DIRECT_BLOCK, [] { __syncthreads(); });
}
__global__ void __launch_bounds__(256) mp_reverse_kernel(u64 p, const u64* __restrict__ z, u64 top, u64 have, u64* __restrict__ a, u64 len) {
  for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < len; k += (u64)gridDim.x * blockDim.x) mp_reverse_elem(p, z, top, have, a, k);
}
__global__ void __launch_bounds__(256) mp_one_kernel(u64* __restrict__ g, u64 len) {
  for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < len; k += (u64)gridDim.x * blockDim.x) mp_one_elem(g, k);
}
template <class FLD>
__global__ void __launch_bounds__(256) mp_window_kernel(FieldConst fc, const u64* __restrict__ v, const u64* __restrict__ pl,
                                                        const u64* __restrict__ pr, u64 d, u64* __restrict__ vn, u64 M) {
  const FLD f(fc);
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < M; e += (u64)gridDim.x * blockDim.x) mp_window_elem(f, v, pl, pr, d, vn, e);
}
template <class FLD>
__global__ void __launch_bounds__(64) mp_eval_leaf_kernel(FieldConst fc, u64 p, const u64* __restrict__ v, const u64* __restrict__ leaves,
                                                          const u64* __restrict__ xs, u64 m, u64 M, u64* __restrict__ out) {
  __shared__ u64 lds[3 * RONK_ROOTS_LEAF];
  const FLD f(fc);
  mp_eval_leaf_body(f, p, v, leaves, xs, m, M, RONK_ROOTS_LEAF, out, lds, threadIdx.x, blockIdx.x, [] { __syncthreads(); });
}
template <class FLD>
__global__ void __launch_bounds__(256) mp_deriv_kernel(FieldConst fc, u64 p, const u64* __restrict__ z, u64* __restrict__ dz, u64 m) {
  const FLD f(fc);
  for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) mp_deriv_elem(f, p, z, dz, j);
}
template <class FLD>
__global__ void __launch_bounds__(256) mp_weights_kernel(FieldConst fc, u64 p, const u64* __restrict__ dzx, const u64* __restrict__ ys, u64 m,
                                                         u64* __restrict__ w, int* status, u64 chunks) {
  const FLD f(fc);
  for (u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x; c < chunks; c += (u64)gridDim.x * blockDim.x)
    mp_weights_chunk(f, p, dzx, ys, m, w, status, RONK_ERR_ZERO_INVERSE, c);
}
template <class FLD>
__global__ void __launch_bounds__(64) mp_interp_leaf_kernel(FieldConst fc, u64 p, const u64* __restrict__ w, const u64* __restrict__ leaves,
                                                            const u64* __restrict__ xs, u64 m, u64 M, InterpStore st) {
  __shared__ u64 lds[RONK_ROOTS_LEAF + RONK_ROOTS_LEAF * (RONK_ROOTS_LEAF + 1)];
  const FLD f(fc);
  mp_interp_leaf_body(f, p, w, leaves, xs, m, M, RONK_ROOTS_LEAF, st, lds, threadIdx.x, blockIdx.x, [] { __syncthreads(); });
}
template <class FLD>
__global__ void __launch_bounds__(256) mp_interp_pointwise_kernel(FieldConst fc, const u64* __restrict__ fn, const u64* __restrict__ tk, u64 M,
                                                                  u64* __restrict__ x) {
  const FLD f(fc);
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < M; e += (u64)gridDim.x * blockDim.x) mp_interp_pointwise_elem(f, fn, tk, M, x, e);
}
template <class FLD>
__global__ void __launch_bounds__(256) mp_interp_combine_kernel(FieldConst fc, const u64* __restrict__ prod, const u64* __restrict__ spread,
                                                                u64 pairs, u64 d, InterpStore st) {
  const FLD f(fc);
  const u64 total = pairs * 2 * d;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x)
    mp_interp_combine_elem(f, prod, spread, pairs, d, st, e);
}
// x[i] %= p on the way into the O(m^2) interpolation kernels, which take canonical residues
__global__ void __launch_bounds__(256) mp_reduce_kernel(u64 p, const u64* __restrict__ in, u64* __restrict__ out, u64 n) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) mp_reduce_elem(p, in, out, i);
}
__global__ void mp_status_kernel(const int* __restrict__ flag, int* __restrict__ status) { *status = mp_status_code(*flag, RONK_ERR_ZERO_INVERSE); }

// ------------------------------------------------------------------------------------- which form runs
// RONK_MULTIPOINT_FORM = direct | tree forces one form (the A/B of the tests and of tools/multipoint_time.py; read at every
// call).  A forced form that does not serve the call is RONK_ERR_UNSUPPORTED.
enum { FORM_AUTO = 0, FORM_DIRECT = 1, FORM_TREE = 2 };
static int mp_forced_form() {
  const char* e = getenv("RONK_MULTIPOINT_FORM");
  if (!e) return FORM_AUTO;
  return !strcmp(e, "direct") ? FORM_DIRECT : !strcmp(e, "tree") ? FORM_TREE : FORM_AUTO;
}
static const size_t MP_MAX_M = (size_t)1 << 24;
static const double MP_DIRECT_MAX_WORK = 17179869184.0;   // 2^34 field products
// The measured crossovers (profiles/multipoint_crossover_mi355x.jsonl).  Evaluation: the direct kernel is one
// serial Horner chain per lane, 0.153 us per coefficient whatever m is while the points fit one wave of lanes over the device
// (2^16), and the tree form costs 0.2 .. 1.6 ms for m <= 2^14 -- they meet at d = 2^13.  Interpolation: the O(m^2) kernels lose
// from m = 512 on (0.86 ms against 0.80 ms; 0.43 against 0.58 ms at 256).
static const size_t MP_EVAL_TREE_MIN_D = 8192;
static const size_t MP_DIRECT_LANES = 65536;
static const size_t MP_INTERP_TREE_MIN_M = 512;
static const size_t MP_INTERP_DIRECT_MAX_M = (size_t)1 << 14;   // the O(m^2) kernels of ronk_rs_decode_dev

static size_t pow2_at_least(size_t n) { size_t v = 1; while (v < n) v <<= 1; return v; }

// the chosen form of one call with what the tree form needs: decided ONCE per call (the host-pointer entry points hand it to
// the device-pointer work), after ONE primality test of the caller's p
struct MpForm {
  int form = FORM_AUTO;
  u64 gtree = 0, gz = 0;   // the transform roots of the tree's plans and of the root's products
  FieldCtx fld;
};

// does the tree form serve (p, m points, d coefficients)?  p: an odd prime (mp_check_prime).  The 2-adicity of the largest
// product is looked at first, so a field that cannot serve costs no further primality test and no search for a root.
static bool mp_tree_field(u64 p, size_t m, size_t d, MpForm* f) {
  if (roots_leaf() != RONK_ROOTS_LEAF || m > MP_MAX_M) return false;
  const size_t M = roots_padded(m, RONK_ROOTS_LEAF), Lp = pow2_at_least(d > M ? d : M);
  const int need = ilog2(Lp) + 1;
  if (need > 30 || (p - 1) % ((u64)1 << need) != 0) return false;
  if (roots_field(p, m, &f->gtree) != RONK_OK || make_field(p, &f->fld) != RONK_OK) return false;
  return newton_field(f->fld, Lp, &f->gz);
}

// words of workspace (M = m padded to RONK_ROOTS_LEAF * 2^t, levels = t, Lp = the power of two >= max(d, M)):
//   the tree 6 M (reused by the windows of the walk down), its leaves 2 M, its transforms 2 levels M, Z: M + 8, the root 10 Lp
static size_t mp_eval_ws_words(size_t M, size_t Lp) {
  const size_t levels = (size_t)ilog2(M / RONK_ROOTS_LEAF);
  return 6 * M + 2 * M + 2 * levels * M + (M + 8) + 10 * Lp;
}

struct MpTree {
  FieldConst fc;
  FieldCtx fld;
  u64 p, gtree, gz;
  size_t m, M, levels;
  u64 *tree_ws, *leaves, *transforms, *z, *newton;
  RootsKeep keep;
  void carve(u64* ws, size_t m_, size_t M_) {
    m = m_; M = M_;
    levels = (size_t)ilog2(M / RONK_ROOTS_LEAF);
    tree_ws = ws;
    leaves = ws + 6 * M;
    transforms = leaves + 2 * M;
    z = transforms + 2 * levels * M;
    newton = z + M + 8;
    keep.leaves = leaves; keep.transforms = transforms;
  }
};

// f (d coefficients) at the tree's m points -> d_out[0 .. m).  t.newton: 10 Lp words.  g_roots_mu held, the tree built.
static int mp_walk_down(const MpTree& t, const u64* d_f, size_t d, const u64* d_xs, u64* d_out, RootsPins& pins, hipStream_t s) {
  const size_t M = t.M, m = t.m, D = d > M ? d : M, Lp = pow2_at_least(D);
  const u32 G = RONK_ROOTS_LEAF;
  const FieldConst& fc = t.fc;
  u64* fa = t.newton;          // A_root = rev(Z) mod z^Lp
  u64* g = fa + Lp;            // 1 / A_root (2 Lp)
  u64* e = g + 2 * Lp;         // 4 Lp: ladder scratch, then the root product (2 D - 1)
  u64* h = e + 4 * Lp;         // Lp
  u64* t1 = h + Lp;            // 2 Lp: ladder scratch, then rev_{D-1}(f)
  hipLaunchKernelGGL(mp_reverse_kernel, dim3(grid_for(Lp)), dim3(256), 0, s, t.p, (const u64*)t.z, (u64)m, (u64)(m + 1), fa, (u64)Lp);
  hipLaunchKernelGGL(mp_one_kernel, dim3(grid_for(2 * Lp)), dim3(256), 0, s, g, (u64)(2 * Lp));
  HIPCHK(hipGetLastError());
  RCHK(newton_ladder_dev(t.fld, t.gz, fa, Lp, g, e, h, t1, s));
  hipLaunchKernelGGL(mp_reverse_kernel, dim3(grid_for(D)), dim3(256), 0, s, t.p, d_f, (u64)(D - 1), (u64)d, t1, (u64)D);
  HIPCHK(hipGetLastError());
  RCHK(ronk_poly_mul_dev(t.p, t.gz, t1, D, g, D, e, s));
  // the windows, in the tree's workspace: V (this level), F (its transforms), PL / PR (the two products), VN (the children)
  u64* V = t.tree_ws;
  u64* F = V + M;
  u64* PL = F + M;
  u64* PR = PL + M;
  u64* VN = PR + M;
  // V_root[t] = coefficient D - 1 - t of the product, t < M
  hipLaunchKernelGGL(mp_reverse_kernel, dim3(grid_for(M)), dim3(256), 0, s, t.p, (const u64*)e, (u64)(D - 1), (u64)D, V, (u64)M);
  HIPCHK(hipGetLastError());
  for (size_t level = t.levels; level-- > 0;) {
    const size_t dd = (size_t)G << level, pairs = M / (2 * dd);
    const u64* Tl = t.transforms + level * 2 * M;
    ronk_plan* pl = nullptr;
    RCHK(pins.get(t.p, t.gtree, (u32)ilog2(2 * dd), pairs, true, &pl));
    RCHK(transform_dev(pl, false, V, nullptr, F, s));
    RCHK(transform_dev(pl, true, F, Tl + M, PL, s));   // V_S * low(M_R): the b half multiplied on load
    RCHK(transform_dev(pl, true, F, Tl, PR, s));       // V_S * low(M_L)
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_window_kernel<decltype(f)>), dim3(grid_for(M)), dim3(256), 0, s, fc, (const u64*)V,
                                            (const u64*)PL, (const u64*)PR, (u64)dd, VN, (u64)M); });
    HIPCHK(hipGetLastError());
    std::swap(V, VN);
  }
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_eval_leaf_kernel<decltype(f)>), dim3((u32)(M / G)), dim3(G), 0, s, fc, t.p, (const u64*)V,
                                          (const u64*)t.leaves, d_xs, (u64)m, (u64)M, d_out); });
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

static int mp_eval_direct(u64 p, const u64* d_c, size_t d, const u64* d_xs, size_t m, u64* d_out, hipStream_t s) {
  if ((double)m * (double)d > MP_DIRECT_MAX_WORK) return RONK_ERR_UNSUPPORTED;
  const FieldConst fc = roots_consts(p);
  const u32 blocks = (u32)((m + MP_DIRECT_BLOCK - 1) / MP_DIRECT_BLOCK);
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_horner_kernel<decltype(f)>), dim3(blocks), dim3(MP_DIRECT_BLOCK), 0, s, fc, p, d_c, (u64)d, d_xs,
                                          (u64)m, d_out); });
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// argument and field checks shared by the two forms of each entry point, before any device work
static int mp_check_prime(u64 p) {
  if (p < 3 || !(p & 1)) return p == 2 ? RONK_ERR_UNSUPPORTED : RONK_ERR_NOT_PRIME;
  return ronk_check_prime(p);
}

// which form evaluates (p, d, m); RONK_ERR_UNSUPPORTED when none does.  A call the measured rule gives to the direct form
// does not look at the tree's field at all.
static int mp_eval_form(u64 p, size_t d, size_t m, MpForm* f) {
  RCHK(mp_check_prime(p));
  const int forced = mp_forced_form();
  const bool direct_ok = (double)m * (double)d <= MP_DIRECT_MAX_WORK;
  if (forced == FORM_DIRECT) { f->form = FORM_DIRECT; return direct_ok ? RONK_OK : RONK_ERR_UNSUPPORTED; }
  const double chain = (double)d * (m > MP_DIRECT_LANES ? (double)m / (double)MP_DIRECT_LANES : 1.0);   // coefficients per lane slot
  if (forced == FORM_AUTO && direct_ok && chain <= (double)MP_EVAL_TREE_MIN_D) { f->form = FORM_DIRECT; return RONK_OK; }
  if (mp_tree_field(p, m, d, f)) { f->form = FORM_TREE; return RONK_OK; }
  f->form = FORM_DIRECT;
  return forced == FORM_AUTO && direct_ok ? RONK_OK : RONK_ERR_UNSUPPORTED;
}

static int mp_eval_run(u64 p, const u64* d_c, size_t d, const u64* d_xs, size_t m, u64* d_out, hipStream_t s, const MpForm& fm) {
  if (stream_capturing(s)) return RONK_ERR_UNSUPPORTED;
  if (fm.form == FORM_DIRECT) return mp_eval_direct(p, d_c, d, d_xs, m, d_out, s);
  const size_t M = roots_padded(m, RONK_ROOTS_LEAF), Lp = pow2_at_least(d > M ? d : M);
  std::lock_guard<std::mutex> lk(g_roots_mu);
  RootsPins pins;
  pins.s = s;
  WsLease ws;
  RCHK(ws.acquire(mp_eval_ws_words(M, Lp) * 8, s));
  MpTree t;
  t.fc = roots_consts(p); t.fld = fm.fld; t.p = p; t.gtree = fm.gtree; t.gz = fm.gz;
  t.carve(ws.u(), m, M);
  RCHK(roots_tree(t.fc, p, t.gtree, d_xs, m, t.z, t.tree_ws, pins, s, &t.keep));
  return mp_walk_down(t, d_c, d, d_xs, d_out, pins, s);
}

extern "C" int ronk_poly_eval_many_dev(uint64_t p, const uint64_t* d_c, size_t d, const uint64_t* d_xs, size_t m, uint64_t* d_out,
                                       void* stream) {
  if (!d_c || !d_xs || !d_out || d == 0 || m == 0) return RONK_ERR_INVALID;
  MpForm fm;
  RCHK(mp_eval_form(p, d, m, &fm));
  RCHK(need_device());
  return mp_eval_run(p, d_c, d, d_xs, m, d_out, (hipStream_t)stream, fm);
}

extern "C" int ronk_poly_eval_many(uint64_t p, const uint64_t* c, size_t d, const uint64_t* xs, size_t m, uint64_t* out) {
  if (!c || !xs || !out || d == 0 || m == 0) return RONK_ERR_INVALID;
  MpForm fm;
  RCHK(mp_eval_form(p, d, m, &fm));
  RCHK(need_device());
  HostCall hc;
  const u64 *dc = hc.in(c, d), *dx = hc.in(xs, m);
  u64* dout = hc.out(m);
  RCHK(hc.rc);
  RCHK(mp_eval_run(p, dc, d, dx, m, dout, nullptr, fm));   // the _dev form past its checks: the form is decided once per call
  return hc.get(out, dout, m * 8);
}

// ------------------------------------------------------------------------------------- interpolation
static int mp_interp_form(u64 p, size_t m, MpForm* f) {
  RCHK(mp_check_prime(p));
  const int forced = mp_forced_form();
  const bool direct_ok = m <= MP_INTERP_DIRECT_MAX_M;
  if (forced == FORM_DIRECT) { f->form = FORM_DIRECT; return direct_ok ? RONK_OK : RONK_ERR_UNSUPPORTED; }
  if (forced == FORM_AUTO && m < MP_INTERP_TREE_MIN_M) { f->form = FORM_DIRECT; return RONK_OK; }
  if (mp_tree_field(p, m, m, f)) { f->form = FORM_TREE; return RONK_OK; }
  f->form = FORM_DIRECT;
  return forced == FORM_AUTO && direct_ok ? RONK_OK : RONK_ERR_UNSUPPORTED;
}

// the O(m^2) kernels behind ronk_rs_decode_dev, on reduced copies of the nodes and values.  The status relies on that entry
// point's contract for k <= 2^14 with a status word given: the word is written ONLY by the weights kernel, for coincident nodes
// (the "not a geometric sequence" bit of its O(k log k) attempt, which Goldilocks calls of k >= 1024 make first, goes to a word
// of its own) -- so any non-zero value is RONK_ERR_ZERO_INVERSE.
static int mp_interp_direct(u64 p, const u64* d_xs, const u64* d_ys, size_t m, u64* d_out, int* d_status, hipStream_t s) {
  WsLease ws;
  RCHK(ws.acquire((2 * m + 8) * 8, s));
  Carve c{ws.u()};
  int* flag = (int*)c.take(8);
  u64 *x = c.take(m), *y = c.take(m);
  HIPCHK(hipMemsetAsync(flag, 0, 64, s));
  hipLaunchKernelGGL(mp_reduce_kernel, dim3(grid_for(m)), dim3(256), 0, s, p, d_xs, x, (u64)m);
  hipLaunchKernelGGL(mp_reduce_kernel, dim3(grid_for(m)), dim3(256), 0, s, p, d_ys, y, (u64)m);
  HIPCHK(hipGetLastError());
  RCHK(ronk_rs_decode_dev(p, x, y, m, d_out, flag, s));
  hipLaunchKernelGGL(mp_status_kernel, dim3(1), dim3(1), 0, s, (const int*)flag, d_status);
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

static int mp_interp_run(u64 p, const u64* d_xs, const u64* d_ys, size_t m, u64* d_out, int* d_status, hipStream_t s, const MpForm& fm) {
  if (stream_capturing(s)) return RONK_ERR_UNSUPPORTED;
  if (fm.form == FORM_DIRECT) return mp_interp_direct(p, d_xs, d_ys, m, d_out, d_status, s);
  const u64 gtree = fm.gtree;
  const u32 G = RONK_ROOTS_LEAF;
  const size_t M = roots_padded(m, G);
  std::lock_guard<std::mutex> lk(g_roots_mu);
  RootsPins pins;
  pins.s = s;
  // the evaluation's workspace (d = m: Lp = M) and two more arrays of M: Z' and its values
  WsLease ws;
  RCHK(ws.acquire((mp_eval_ws_words(M, M) + 2 * M) * 8, s));
  MpTree t;
  t.fc = roots_consts(p); t.fld = fm.fld; t.p = p; t.gtree = gtree; t.gz = fm.gz;
  t.carve(ws.u(), m, M);
  const FieldConst& fc = t.fc;
  u64* dz = t.newton + 10 * M;
  u64* dzx = dz + M;
  HIPCHK(hipMemsetAsync(d_status, 0, 4, s));
  RCHK(roots_tree(fc, p, gtree, d_xs, m, t.z, t.tree_ws, pins, s, &t.keep));
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_deriv_kernel<decltype(f)>), dim3(grid_for(m)), dim3(256), 0, s, fc, p, (const u64*)t.z, dz, (u64)m); });
  HIPCHK(hipGetLastError());
  RCHK(mp_walk_down(t, dz, m, d_xs, dzx, pins, s));
  // the walk up, in the root's (now free) 10 M words: the weights, N spread (this level, the next), its transforms, the product
  u64* w = t.newton;
  u64* N = w + M;
  u64* N2 = N + 2 * M;
  u64* FN = N2 + 2 * M;
  u64* X = FN + 2 * M;
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_weights_kernel<decltype(f)>), dim3(grid_for(M / REC_CH)), dim3(256), 0, s, fc, p, (const u64*)dzx,
                                          d_ys, (u64)m, w, d_status, (u64)(M / REC_CH)); });
  const size_t leaves = M / G;
  InterpStore st{};
  if (leaves == 1) { st.out = d_out; st.final_ = 1; st.shift = M - m; }
  else { st.out = N; st.half = M; }
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_interp_leaf_kernel<decltype(f)>), dim3((u32)leaves), dim3(G), 0, s, fc, p, (const u64*)w,
                                          (const u64*)t.leaves, d_xs, (u64)m, (u64)M, st); });
  HIPCHK(hipGetLastError());
  size_t d = G, count = leaves, level = 0;
  while (count > 1) {
    const size_t pairs = count / 2, half = pairs * 2 * d;   // half == M
    ronk_plan* pl = nullptr;
    RCHK(pins.get(p, gtree, (u32)ilog2(2 * d), pairs, true, &pl));
    RCHK(transform_dev(pl, false, N, nullptr, FN, s));
    RCHK(transform_dev(pl, false, N + half, nullptr, FN + half, s));
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_interp_pointwise_kernel<decltype(f)>), dim3(grid_for(M)), dim3(256), 0, s, fc, (const u64*)FN,
                                            (const u64*)(t.transforms + level * 2 * M), (u64)M, X); });
    HIPCHK(hipGetLastError());
    RCHK(transform_dev(pl, true, X, nullptr, X, s));
    InterpStore nx{};
    if (pairs == 1) { nx.out = d_out; nx.final_ = 1; nx.shift = M - m; }
    else { nx.out = N2; nx.half = M; }
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((mp_interp_combine_kernel<decltype(f)>), dim3(grid_for(half)), dim3(256), 0, s, fc, (const u64*)X,
                                            (const u64*)N, (u64)pairs, (u64)d, nx); });
    HIPCHK(hipGetLastError());
    std::swap(N, N2);
    d *= 2;
    count = pairs;
    level++;
  }
  return RONK_OK;
}

extern "C" int ronk_poly_interpolate_dev(uint64_t p, const uint64_t* d_xs, const uint64_t* d_ys, size_t m, uint64_t* d_out, int* d_status,
                                         void* stream) {
  if (!d_xs || !d_ys || !d_out || !d_status || m == 0) return RONK_ERR_INVALID;
  MpForm fm;
  RCHK(mp_interp_form(p, m, &fm));
  RCHK(need_device());
  return mp_interp_run(p, d_xs, d_ys, m, d_out, d_status, (hipStream_t)stream, fm);
}

extern "C" int ronk_poly_interpolate(uint64_t p, const uint64_t* xs, const uint64_t* ys, size_t m, uint64_t* out) {
  if (!xs || !ys || !out || m == 0) return RONK_ERR_INVALID;
  MpForm fm;
  RCHK(mp_interp_form(p, m, &fm));
  RCHK(need_device());
  HostCall hc;
  const u64 *dx = hc.in(xs, m), *dy = hc.in(ys, m);
  u64* dout = hc.out(m);
  int* dst = (int*)hc.out(1);   // (both forms write it themselves)
  RCHK(hc.rc);
  RCHK(mp_interp_run(p, dx, dy, m, dout, dst, nullptr, fm));
  int status = 0;
  RCHK(hc.get(&status, dst, 4));
  if (status) return status;
  return hc.get(out, dout, m * 8);
}
