// ronk_recover.hip -- C ABI of libronk_ntt.so, part 6: the product of linear factors on the device (a product tree,
// csrc/roots_kernels.h) and Reed-Solomon erasure recovery in O(N log N) on top of it (DESIGN.md "Erasure recovery and the
// product tree").
#include <map>

#include "roots_host.h"

// ------------------------------------------------------------------------------------- kernels
// the field a launch computes in: Goldilocks, or a Montgomery prime (its constants by value: SGPRs)
FieldConst roots_consts(u64 p) {
  FieldConst c{};
  if (p == RONK_GOLDILOCKS_P) return c;
  const mont64::Field mf = mont64::make_field(p);
  c.p = p; c.pinv = mf.pinv; c.r2 = mf.r2;
  c.w16[0] = mf.one;
  return c;
}

template <class FLD>
__global__ void __launch_bounds__(256) roots_leaf_kernel(FieldConst fc, u64 p, const u64* __restrict__ roots, u64 m, u32 G,
                                                         RootsStore st) {
  __shared__ u64 lds[3 * 256];
  const FLD f(fc);
  roots_leaf_body(f, p, roots, m, G, st, lds, threadIdx.x, blockIdx.x, [] { __syncthreads(); });
}
template <class FLD>
__global__ void __launch_bounds__(256) roots_combine_kernel(FieldConst fc, const u64* __restrict__ prod, const u64* __restrict__ spread,
                                                            u64 pairs, u64 d, RootsStore st) {
  const FLD f(fc);
  const u64 total = pairs * 2 * d;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x)
    roots_combine_elem(f, prod, spread, pairs, d, st, e);
}
__global__ void __launch_bounds__(256) roots_single_leaf_kernel(const u64* __restrict__ leaf, u64 shift, u64 m, u64* __restrict__ out) {
  roots_single_leaf_elem(leaf, shift, m, out, threadIdx.x);
}
struct DevAtom {
  __device__ u32 or32(u32* a, u32 v) const { return atomicOr(a, v); }
  __device__ int or_i(int* a, int v) const { return atomicOr(a, v); }
};
template <class FLD>
__global__ void __launch_bounds__(256) rec_roots_kernel(FieldConst fc, const u64* __restrict__ erased, u64 ne, u64 n, u64 omega,
                                                        u32* bitmap, int* err, u64* __restrict__ roots) {
  const FLD f(fc);
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < ne; i += (u64)gridDim.x * blockDim.x)
    rec_roots_elem(f, DevAtom(), erased, n, omega, i, bitmap, err, roots);
}
__global__ void __launch_bounds__(256) rec_status_kernel(const int* __restrict__ err, int* __restrict__ status, u64 B) {
  for (u64 b = blockIdx.x * (u64)blockDim.x + threadIdx.x; b < B; b += (u64)gridDim.x * blockDim.x) status[b] = rec_err_code(*err);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_zprep_kernel(FieldConst fc, u64* zz, u64 n, u64 e, u64 s) {
  const FLD f(fc);
  for (u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x; c < n / REC_CH; c += (u64)gridDim.x * blockDim.x) rec_zprep_chunk(f, zz, n, e, s, c);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_batch_inv_kernel(FieldConst fc, u64 p, u64* x, u64 chunks) {
  const FLD f(fc);
  for (u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x; c < chunks; c += (u64)gridDim.x * blockDim.x) rec_batch_inv_chunk(f, p, x, c);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_mask_mul_kernel(FieldConst fc, const u64* __restrict__ y, const u64* __restrict__ zhat,
                                                           u64* __restrict__ w, u64 n, u64 total) {
  const FLD f(fc);
  for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) rec_mask_mul_elem(f, y, zhat, w, n, t);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_scale_kernel(FieldConst fc, u64* w, u64 n, u64 s, u64 chunks) {
  const FLD f(fc);
  for (u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x; c < chunks; c += (u64)gridDim.x * blockDim.x) rec_scale_chunk(f, w, n, s, c);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_div_kernel(FieldConst fc, u64* w, const u64* __restrict__ zinv, u64 n, u64 total) {
  const FLD f(fc);
  for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) rec_div_elem(f, w, zinv, n, t);
}
template <class FLD>
__global__ void __launch_bounds__(256) rec_finish_kernel(FieldConst fc, const u64* __restrict__ w, u64 n, u64 k, u64 sinv,
                                                         const int* err, u64* __restrict__ msgs, int* status, u64 chunks) {
  const FLD f(fc);
  for (u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x; c < chunks; c += (u64)gridDim.x * blockDim.x)
    rec_finish_chunk(f, w, n, k, sinv, err, msgs, status, c);
}

// ------------------------------------------------------------------------------------- plans of the tree
// One batched plan per level shape (2d points, count / 2 rows), owned by the library: a second call of the same shape builds
// no twiddle tables.  Every call holds g_roots_mu from its first lookup to its last launch, and pins what it uses; eviction
// (least recently used, unpinned, beyond ROOTS_CACHE_MAX) waits for the entry's last work first.
std::mutex g_roots_mu;
static std::vector<RootsPlan*> g_roots_plans;
static u64 g_roots_clock = 0;
static const size_t ROOTS_CACHE_MAX = 48;

static void roots_plan_free(RootsPlan* e) {
  if (e->used && e->done) (void)hipEventSynchronize(e->done);
  if (e->pl) ronk_plan_destroy(e->pl);
  if (e->done) (void)hipEventDestroy(e->done);
  delete e;
}
// g_roots_mu held
// tiled: the plan must run on the tile kernels (the tree's fused product, TileArgs::in2); otherwise RONK_ERR_UNSUPPORTED
int roots_plan_get(u64 p, u64 g, u32 log2n, u64 batch, bool tiled, RootsPlan** out) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  for (RootsPlan* e : g_roots_plans)
    if (e->p == p && e->g == g && e->log2n == log2n && e->batch == batch && e->device == dev) {
      if (tiled && ronk_plan_path(e->pl) == 0) return RONK_ERR_UNSUPPORTED;
      e->stamp = ++g_roots_clock;
      e->pins++;
      *out = e;
      return RONK_OK;
    }
  if (g_roots_plans.size() >= ROOTS_CACHE_MAX) {
    size_t lru = g_roots_plans.size();
    for (size_t i = 0; i < g_roots_plans.size(); i++)
      if (g_roots_plans[i]->pins == 0 && (lru == g_roots_plans.size() || g_roots_plans[i]->stamp < g_roots_plans[lru]->stamp)) lru = i;
    if (lru < g_roots_plans.size()) {
      roots_plan_free(g_roots_plans[lru]);
      g_roots_plans.erase(g_roots_plans.begin() + lru);
    }
  }
  RootsPlan* e = new RootsPlan();
  e->p = p; e->g = g; e->log2n = log2n; e->batch = batch; e->device = dev;
  int rc = ronk_plan_create(&e->pl, p, g, log2n, batch, dev);
  if (rc == RONK_OK && tiled && ronk_plan_path(e->pl) == 0) rc = RONK_ERR_UNSUPPORTED;
  if (rc == RONK_OK) {
    hipError_t he = hipEventCreateWithFlags(&e->done, hipEventDisableTiming);
    if (he != hipSuccess) rc = hip_fail(he, "hipEventCreate");
  }
  if (rc) { roots_plan_free(e); return rc; }
  e->stamp = ++g_roots_clock;
  e->pins = 1;
  g_roots_plans.push_back(e);
  *out = e;
  return RONK_OK;
}
// leaf size G = 2^L.  L = 6 (64 factors per leaf): the first NTT level then has 2^7 points -- see DESIGN.md for the measurement of
// L = 6 / 7 / 8.  RONK_ROOTS_LEAF_LOG2 (6 .. 8) overrides it for that A/B.
u32 roots_leaf() {
  static const u32 G = [] {
    const char* e = getenv("RONK_ROOTS_LEAF_LOG2");
    const int l = e ? atoi(e) : 6;
    return (u32)1 << (l >= 6 && l <= 8 ? l : 6);
  }();
  return G;
}
static_assert(RONK_ROOTS_LEAF == 64, "the documented leaf size");

// the transform root of the tree's plans: any element that makes the tiled plans exist (a product does not depend on it)
static bool roots_tree_root(u64 p, u64* g) {
  if (p == RONK_GOLDILOCKS_P) { *g = RONK_GOLDILOCKS_G; return true; }
  u64 z = 2 % p;
  for (int tries = 0; tries < 1000 && h_powmod(z, (p - 1) / 2, p) == 1; tries++) z = (z + 1) % p;
  if (h_powmod(z, (p - 1) / 2, p) != p - 1) return false;
  *g = z;
  return true;
}

// words of workspace the tree of m roots needs: three spread arrays of 2M (M = m padded to G * 2^t); the roots sit in the second
size_t roots_padded(size_t m, u32 G) { size_t M = G; while (M < m) M <<= 1; return M; }
size_t roots_ws_words(size_t m, u32 G) { const size_t M = roots_padded(m, G); return M > G ? 6 * M : 3 * M; }

// prod_{i < m} (x - d_roots[i]) -> d_out[0 .. m] (monic, ascending).  ws: roots_ws_words(m) words.  g_roots_mu held.
// keep (may be NULL: nothing is retained, the tree of ronk_poly_from_roots): the leaves stay in keep->leaves (2M words, the
// level-0 spread layout) and the forward transforms of level l (children of G * 2^l coefficients) in keep->transforms + l * 2M
// (a rows, then b rows) -- what the walks of ronk_multipoint.hip read.  The products and launches are the same either way.
int roots_tree(const FieldConst& fc, u64 p, u64 gtree, const u64* d_roots, size_t m, u64* d_out, u64* ws, RootsPins& pins,
               hipStream_t s, const RootsKeep* keep) {
  const u32 G = roots_leaf();
  const size_t M = roots_padded(m, G);
  const size_t leaves = M / G;
  u64* S = keep ? keep->leaves : ws;   // this level, spread
  u64* T = ws + 2 * M;         // its transforms
  u64* S2 = ws + 4 * M;        // the next level, spread
  RootsStore st{};
  if (leaves == 1 && !keep) { st.out = d_out; st.final_ = 1; st.shift = M - m; st.m = m; }
  else { st.out = S; st.half = M; }
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((roots_leaf_kernel<decltype(f)>), dim3((u32)leaves), dim3(G), 0, s, fc, p, d_roots, (u64)m, G, st); });
  HIPCHK(hipGetLastError());
  if (leaves == 1 && keep) {   // the single leaf is kept in the spread layout: its shifted copy is the product
    hipLaunchKernelGGL(roots_single_leaf_kernel, dim3(1), dim3(G), 0, s, (const u64*)S, (u64)(M - m), (u64)m, d_out);
    HIPCHK(hipGetLastError());
  }
  size_t d = G, count = leaves, level = 0;
  while (count > 1) {
    const size_t pairs = count / 2, half = pairs * 2 * d;
    ronk_plan* pl = nullptr;
    RCHK(pins.get(p, gtree, (u32)ilog2(2 * d), pairs, true, &pl));
    u64* Tl = keep ? keep->transforms + level * 2 * M : T;
    u64* prod = keep ? T : Tl;   // retained transforms are not overwritten by the product
    RCHK(transform_dev(pl, false, S, nullptr, Tl, s));
    RCHK(transform_dev(pl, false, S + half, nullptr, Tl + half, s));
    RCHK(transform_dev(pl, true, Tl, Tl + half, prod, s));     // a * b: the second half multiplied on load
    RootsStore nx{};
    if (pairs == 1) { nx.out = d_out; nx.final_ = 1; nx.shift = M - m; nx.m = m; }
    else { nx.out = S2; nx.half = M; }
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((roots_combine_kernel<decltype(f)>), dim3(grid_for(half)), dim3(256), 0, s, fc, (const u64*)prod,
                                            (const u64*)S, (u64)pairs, (u64)d, nx); });
    HIPCHK(hipGetLastError());
    if (keep && level == 0) { S = S2; S2 = ws; }   // the leaves stay where they are
    else std::swap(S, S2);
    d *= 2;
    count = pairs;
    level++;
  }
  return RONK_OK;
}

// which primes a tree of m roots serves: any odd prime up to one leaf, beyond that the 2-adicity of the top product (M points)
int roots_field(u64 p, size_t m, u64* gtree) {
  if (p < 3 || !(p & 1)) return p == 2 ? RONK_ERR_UNSUPPORTED : RONK_ERR_NOT_PRIME;
  RCHK(ronk_check_prime(p));
  const size_t M = roots_padded(m, roots_leaf());
  *gtree = 0;
  if (M == roots_leaf()) return RONK_OK;
  const int k = ilog2(M);
  if (k > 30 || (p - 1) % ((u64)1 << k) != 0 || !roots_tree_root(p, gtree)) return RONK_ERR_UNSUPPORTED;
  return RONK_OK;
}

extern "C" int ronk_poly_from_roots_dev(uint64_t p, const uint64_t* d_roots, size_t m, uint64_t* d_out, void* stream) {
  if (!d_out || (m && !d_roots)) return RONK_ERR_INVALID;
  u64 gtree = 0;
  RCHK(roots_field(p, m ? m : 1, &gtree));
  RCHK(need_device());
  hipStream_t s = (hipStream_t)stream;
  if (stream_capturing(s)) return RONK_ERR_UNSUPPORTED;
  if (m == 0) {   // the empty product: ONE
    const u64 one = 1;
    HIPCHK(hipMemcpyAsync(d_out, &one, 8, hipMemcpyHostToDevice, s));
    return hipStreamSynchronize(s) == hipSuccess ? RONK_OK : hip_fail(hipErrorUnknown, "hipStreamSynchronize");
  }
  const FieldConst fc = roots_consts(p);
  std::lock_guard<std::mutex> lk(g_roots_mu);
  RootsPins pins;
  pins.s = s;
  WsLease ws;
  RCHK(ws.acquire(roots_ws_words(m, roots_leaf()) * 8, s));
  return roots_tree(fc, p, gtree, d_roots, m, d_out, ws.u(), pins, s, nullptr);
}

extern "C" int ronk_poly_from_roots(uint64_t p, const uint64_t* roots, size_t m, uint64_t* out) {
  if (!out || (m && !roots)) return RONK_ERR_INVALID;
  u64 gtree = 0;
  RCHK(roots_field(p, m ? m : 1, &gtree));
  RCHK(need_device());
  HostCall hc;
  const u64* dr = hc.in(roots, m);
  u64* dout = hc.out(m + 1);
  RCHK(hc.rc);
  RCHK(ronk_poly_from_roots_dev(p, dr, m, dout, nullptr));
  return hc.get(out, dout, (m + 1) * 8);
}

// ------------------------------------------------------------------------------------- erasure recovery
// One erasure set E (e positions) for B rows of N values:
//   Z = prod_{i in E} (x - omega^i) (tree);  [Zhat ; Z(s omega^i)] = NTT_N of [Z ; Z(s x)] (one batch of two), the second inverted
//   P = iNTT_N(y . Zhat) = D * Z exactly (deg D + e <= N - 1);  Q = iNTT_N(NTT_N(P(s x)) / Z(s omega^i)) (s^-j)
//   Q has degree < k exactly when the survivors lie on one polynomial of degree < k, and then Q = D.
// Workspace (words): 2N (the two Z rows) + max(B N, tree) + N / 64 (bitmap) + 8; tree = 6 M, M = e padded to 64 * 2^t.
extern "C" int ronk_rs_recover_batch_dev(ronk_plan* plan, size_t k, const uint64_t* d_erased, size_t n_erased, const uint64_t* d_ys,
                                         uint64_t* d_msgs, uint64_t* d_full, int* d_status, void* stream) {
  if (!plan || !d_ys || !d_msgs || !d_status || (n_erased && !d_erased) || k == 0) return RONK_ERR_INVALID;
  const u64 N = plan->n, B = plan->batch, p = plan->p;
  if (k > N || n_erased > N - k) return RONK_ERR_INDEX;
  if (N < REC_CH || plan->field.kind == F_MOD2) return RONK_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (stream_capturing(s)) return RONK_ERR_UNSUPPORTED;
  const size_t e = n_erased;
  u64 gtree = 0, sh = 1, sinv = 1, omega = 1;
  if (e) {
    RCHK(roots_field(p, e, &gtree));
    // the coset s * <omega_N>: g itself unless g^N = 1; no coset exists when N = p - 1
    if (N == p - 1) return RONK_ERR_UNSUPPORTED;
    sh = plan->g % p;
    if (sh == 0 || h_powmod(sh, N, p) == 1) {
      sh = 0;
      for (u64 c = 2; c < 1000 && c < p; c++) if (h_powmod(c, N, p) != 1) { sh = c; break; }
      if (!sh) return RONK_ERR_UNSUPPORTED;
    }
    sinv = h_powmod(sh, p - 2, p);
    omega = h_powmod(plan->g % p, (p - 1) / N, p);
  }
  RCHK(need_device());
  const FieldConst fc = roots_consts(p);
  std::lock_guard<std::mutex> lk(g_roots_mu);
  RootsPins pins;
  pins.s = s;
  const size_t tree_w = e ? roots_ws_words(e, roots_leaf()) : 0;
  const size_t big = (size_t)B * N > tree_w ? (size_t)B * N : tree_w;
  const size_t bitmap_w = (N + 63) / 64;
  WsLease lease;
  RCHK(lease.acquire((8 + bitmap_w + (e ? 2 * N : 0) + big) * 8, s));
  u64* ws = lease.u();
  int* err = (int*)ws;
  u32* bitmap = (u32*)(ws + 8);
  u64* zz = ws + 8 + bitmap_w;
  u64* W = zz + (e ? 2 * N : 0);
  HIPCHK(hipMemsetAsync(ws, 0, (8 + bitmap_w) * 8, s));
  const u64 total = B * N, chunks = total / REC_CH;
  if (e) {
    u64* roots = W + 2 * roots_padded(e, roots_leaf());   // the tree's second array (roots_tree reads them before it is written)
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((rec_roots_kernel<decltype(f)>), dim3(grid_for(e)), dim3(256), 0, s, fc, d_erased, (u64)e, N,
                                            omega, bitmap, err, roots); });
    HIPCHK(hipGetLastError());
    RCHK(roots_tree(fc, p, gtree, roots, e, zz, W, pins, s, nullptr));
    ronk_plan* pz = nullptr;
    RCHK(pins.get(p, plan->g % p, plan->log2n, 2, false, &pz));
    ROOTS_DISPATCH(fc, {
      hipLaunchKernelGGL((rec_zprep_kernel<decltype(f)>), dim3(grid_for(N / REC_CH)), dim3(256), 0, s, fc, zz, N, (u64)e, sh);
    });
    HIPCHK(hipGetLastError());
    RCHK(transform_dev(pz, false, zz, nullptr, zz, s));
    ROOTS_DISPATCH(fc, {
      hipLaunchKernelGGL((rec_batch_inv_kernel<decltype(f)>), dim3(grid_for(N / REC_CH)), dim3(256), 0, s, fc, p, zz + N, N / REC_CH);
      hipLaunchKernelGGL((rec_mask_mul_kernel<decltype(f)>), dim3(grid_for(total)), dim3(256), 0, s, fc, d_ys, (const u64*)zz, W, N, total);
    });
    HIPCHK(hipGetLastError());
    RCHK(transform_dev(plan, true, W, nullptr, W, s));
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((rec_scale_kernel<decltype(f)>), dim3(grid_for(chunks)), dim3(256), 0, s, fc, W, N, sh, chunks); });
    HIPCHK(hipGetLastError());
    RCHK(transform_dev(plan, false, W, nullptr, W, s));
    ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((rec_div_kernel<decltype(f)>), dim3(grid_for(total)), dim3(256), 0, s, fc, W, (const u64*)(zz + N), N, total); });
    HIPCHK(hipGetLastError());
    RCHK(transform_dev(plan, true, W, nullptr, W, s));
  } else {
    RCHK(transform_dev(plan, true, d_ys, nullptr, W, s));
  }
  hipLaunchKernelGGL(rec_status_kernel, dim3(grid_for(B)), dim3(256), 0, s, (const int*)err, d_status, B);
  ROOTS_DISPATCH(fc, { hipLaunchKernelGGL((rec_finish_kernel<decltype(f)>), dim3(grid_for(chunks)), dim3(256), 0, s, fc, (const u64*)W, N, (u64)k,
                                          (u64)sinv, (const int*)err, d_msgs, d_status, chunks); });
  HIPCHK(hipGetLastError());
  if (d_full) RCHK(ronk_rs_encode_batch_dev(plan, d_msgs, k, d_full, s));
  return RONK_OK;
}

extern "C" int ronk_rs_recover(uint64_t p, uint64_t g, size_t n, size_t k, const uint64_t* erased, size_t n_erased, const uint64_t* ys,
                               uint64_t* msg, uint64_t* full) {
  if (!ys || !msg || (n_erased && !erased) || k == 0 || n == 0) return RONK_ERR_INVALID;
  if (k > n || n_erased > n - k) return RONK_ERR_INDEX;
  if (!is_pow2(n)) return RONK_ERR_NOT_POW2;
  RCHK(ronk_check_prime(p));
  if ((p - 1) % n != 0) return RONK_ERR_NO_ROOT;
  RCHK(need_device());
  std::vector<u64> hy(n);
  for (size_t i = 0; i < n; i++) hy[i] = ys[i] % p;
  ronk_plan* pl = nullptr;
  RCHK(ronk_plan_create(&pl, p, g, (u32)ilog2(n), 1, -1));
  struct Destroy { ronk_plan* pl; ~Destroy() { ronk_plan_destroy(pl); } } destroy{pl};
  HostCall hc;
  const u64 *de = hc.in(erased, n_erased), *dy = hc.in(hy.data(), n);
  u64 *dm = hc.out(k), *df = hc.out(n);
  int* dst = (int*)hc.out(1);   // (written by the call for every row: not zeroed here)
  RCHK(hc.rc);
  RCHK(ronk_rs_recover_batch_dev(pl, k, de, n_erased, dy, dm, full ? df : nullptr, dst, nullptr));
  int status = 0;
  RCHK(hc.get(&status, dst, 4));
  if (status) return status;
  RCHK(hc.get(msg, dm, k * 8));
  return full ? hc.get(full, df, n * 8) : RONK_OK;
}
