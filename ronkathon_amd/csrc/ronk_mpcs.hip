// ronk_mpcs.hip -- C ABI of libronk_ntt.so, part 16: the multi-matrix FRI polynomial commitment (include/ronk_ntt.h "multi-matrix
// polynomial commitment"; csrc/mpcs_kernels.h): R committed matrices, each opened at its own subset of K
// extension points, combined into one DEEP codeword and opened under one FRI.  The Merkle tree, the openings, the extension FRI
// prover and verifier are the merged ones, used through their own entry points; the evaluation body, the domain table and the
// inversion are those of csrc/deep_kernels.h.  The R device pointers of a call travel to the kernels by value (MpcsPtrs).
// The batched commitment of one matrix, ronk_pcs_* (csrc/ronk_pcs.hip), is this code with R = 1 and the full mask (the combine
// launch of a one-round handle walks the rows before it inverts, mpcs_one_round_kernel; everything else is shared), and
// ronk_ext2_poly_eval_batch* (include/ronk_ntt.h "batched FRI polynomial commitment") is the evaluation kernel on its own.
#include "runtime.h"
#include "hip_launch.h"
#include "poseidon_handle.h"
#include "ext2_launch.h"
#include "mpcs_kernels.h"
#include "pow_kernels.h"

// ------------------------------------------------------------------------------------- handle
struct ronk_mpcs {
  const ronk_poseidon* pos = nullptr;
  ronk_fri* fri = nullptr;      // owned: extension challenges, planar layer 0
  u64 p = 0;
  u32 log2_blowup = 0;
  MpcsShape ms{};
  FriShape sh;                  // that of the FRI handle
  Ext2Launch c;                 // the field policy, its constants, W
  DeepDomain dm{};
  u64* d_dom = nullptr;         // lo, hi of the domain
  u64* d_tab = nullptr;         // the table of the call in flight (mpcs_tab_words)
  u64* d_vs = nullptr;          // the verifier's state: a [D], ok [R][Q] ints
  u32 pow_bits = 0;             // the FRI handle's grinding bits (ronk_mpcs_set_pow)
  u64 leaf_len(u32 r) const { return (u64)ms.C[r] << sh.eta; }
  u64 claims() const { return 2 * (u64)ms.Y; }
  u64 fri_proof() const { return sh.proof_words() + (pow_bits ? 1 : 0); }
  u64 round_words(u32 r) const { return sh.queries * leaf_len(r) + sh.queries * sh.log2m(0) * sh.d; }
  u64 proof_words() const {
    u64 n = claims() + fri_proof();
    for (u32 r = 0; r < ms.R; r++) n += round_words(r);
    return n;
  }
  // a [D], open status [Q] (every round's in turn), G [2][N], then the FRI workspace (which holds the query indices)
  u64 small_words() const { return sh.d + sh.queries; }
  u64 workspace_words() const { return small_words() + 2 * sh.size(0) + sh.workspace_words() + (pow_bits ? POW_WORK_WORDS : 0); }
  MpcsTab tab() const {
    const u64* k = d_tab;
    const u64* y = k + (u64)MPCS_KW * ms.K;
    return MpcsTab{k, y, y + 2 * (u64)ms.R * ms.K};
  }
};

// run the statement with KK bound to the number of points and FF to the handle's field policy
#define MPCS_DISPATCH_K(Kv, ...)                            \
  do {                                                      \
    switch (Kv) {                                           \
      case 1: { constexpr int KK = 1; __VA_ARGS__; } break; \
      case 2: { constexpr int KK = 2; __VA_ARGS__; } break; \
      case 3: { constexpr int KK = 3; __VA_ARGS__; } break; \
      case 4: { constexpr int KK = 4; __VA_ARGS__; } break; \
      case 5: { constexpr int KK = 5; __VA_ARGS__; } break; \
      case 6: { constexpr int KK = 6; __VA_ARGS__; } break; \
      case 7: { constexpr int KK = 7; __VA_ARGS__; } break; \
      default: { constexpr int KK = 8; __VA_ARGS__; } break; \
    }                                                       \
  } while (0)
#define MPCS_DISPATCH(h, ...) EXT2_DISPATCH3((h)->c, MPCS_DISPATCH_K((h)->ms.K, __VA_ARGS__))

// ------------------------------------------------------------------------------------- kernels
// One workgroup per column of one round: lane l takes the coefficients l + 256 r, the shares meet in an LDS tree.  Slot j of the
// lane is the j-th point of the round's mask.  y0, y1: the round's claims in the two planes, element j C + c.
template <class F>
__global__ void __launch_bounds__(DEEP_EVAL_LANES) mpcs_eval_kernel(FriConsts k, u64 w, const u64* __restrict__ coef, u64 d,
                                                                    const u64* __restrict__ z, u32 K, u32 mask, u32 C,
                                                                    u64* __restrict__ y0, u64* __restrict__ y1) {
  __shared__ u64 red[2][DEEP_EVAL_LANES];
  const F f(k);
  const Ext2<F> x(f, w);
  const u32 c = blockIdx.x, lane = threadIdx.x, Kp = mpcs_popcount(mask);
  E2 zr[DEEP_MAX_K], share[DEEP_MAX_K];
  u32 rest = mask;
  deep_for<0, (int)DEEP_MAX_K>([&](auto J) {
    constexpr u32 j = decltype(J)::value;
    if (j < Kp) {
      const u32 kk = (u32)__builtin_ctz(rest);
      rest &= rest - 1;
      zr[j] = E2{f.in(z[kk]), f.in(z[K + kk])};
    } else {
      zr[j] = x.zero();
    }
  });
  const u64* col = coef + (u64)c * d;
  deep_eval_lane(x, d, lane, DEEP_EVAL_LANES, zr, Kp, [&](u64 j) { return col[j]; }, share);
  deep_for<0, (int)DEEP_MAX_K>([&](auto J) {
    constexpr u32 j = decltype(J)::value;
    if (j >= Kp) return;   // wave-uniform
    red[0][lane] = share[j].c0;
    red[1][lane] = share[j].c1;
    __syncthreads();
    for (u32 s = DEEP_EVAL_LANES / 2; s > 0; s >>= 1) {
      if (lane < s) {
        red[0][lane] = f.add(red[0][lane], red[0][lane + s]);
        red[1][lane] = f.add(red[1][lane], red[1][lane + s]);
      }
      __syncthreads();
    }
    if (lane == 0) {
      y0[(u64)j * C + c] = f.out(red[0][0]);
      y1[(u64)j * C + c] = f.out(red[1][0]);
    }
    __syncthreads();
  });
}

// a = sponge(seed || root_0 || .. || root_(R-1) || z planes || y planes) squeezing d words; one lane
template <class PF, int W>
__global__ void __launch_bounds__(64) mpcs_transcript_kernel(PoseidonConsts k, u32 d, u32 R, const u64* seed, MpcsPtrs roots, const u64* z,
                                                             u64 nz, const u64* y, u64 ny, u64* a) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  const u64 nr = (u64)R * d;
  poseidon_sponge<PF, W>(pf, k, d + nr + nz + ny, d,
                         [&](u64 j) {
                           if (j < d) return seed[j];
                           j -= d;
                           if (j < nr) return roots.p[j / d][j % d];
                           j -= nr;
                           return j < nz ? z[j] : y[j - nz];
                         },
                         [&](u64 q, u64 v) { a[q] = v; });
}

// one workgroup: the table of a call.  *status gets bit 32 when a point lies on the domain.
template <class F>
__global__ void __launch_bounds__(256) mpcs_prep_kernel(FriConsts k, u64 w, DeepDomain dm, MpcsShape sh, const u64* __restrict__ alpha,
                                                        const u64* __restrict__ z, const u64* __restrict__ y, u64* __restrict__ tab,
                                                        int* status) {
  const F f(k);
  const Ext2<F> x(f, w);
  const E2 a{f.in(alpha[0]), f.in(alpha[1])};
  u64* tab_y = tab + (u64)MPCS_KW * sh.K;
  u64* tab_ap = tab_y + 2 * (u64)sh.R * sh.K;
  for (u32 c = threadIdx.x; c < sh.Ctot; c += blockDim.x) deep_prep_column(x, a, c, tab_ap);
  if (threadIdx.x < sh.K) {
    const int bits = mpcs_prep_point(x, dm, a, z, sh, threadIdx.x, tab + (u64)MPCS_KW * threadIdx.x);
    if (bits) atomicOr(status, bits);
  }
  // the last lanes, so that the claims do not wait behind the points' lanes of the first wavefront
  const u32 back = blockDim.x - 1 - threadIdx.x;
  if (back < sh.R * sh.K) mpcs_prep_claims(x, a, y, sh, back / sh.K, back % sh.K, tab_y + 2 * (u64)back);
}

// one lane per four points i + t N/4: adjacent lanes read adjacent words of every row, and write adjacent words of both planes
template <class F, int K>
__global__ void __launch_bounds__(256) mpcs_combine_kernel(FriConsts k, u64 w, DeepDomain dm, MpcsTab tab, MpcsShape sh, MpcsPtrs M,
                                                           u64* __restrict__ G) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 N = (u64)1 << dm.log2n, q = N >> 2;
  const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= q) return;
  E2 out[DEEP_PTS];
  mpcs_combine_lane<F, K, DEEP_PTS>(x, dm, tab, sh, i, [&](u32 r, u32 c, int t) { return M.p[r][(u64)c * N + i + (u64)t * q]; }, out);
  deep_for<0, DEEP_PTS>([&](auto T) {
    constexpr int t = decltype(T)::value;
    G[i + (u64)t * q] = out[t].c0;
    G[N + i + (u64)t * q] = out[t].c1;
  });
}

// the same grid for a handle of ONE round: the lane that walks the rows first (mpcs_one_round_lane), the same words
template <class F, int K>
__global__ void __launch_bounds__(256) mpcs_one_round_kernel(FriConsts k, u64 w, DeepDomain dm, MpcsTab tab, u32 C,
                                                             const u64* __restrict__ M, u64* __restrict__ G) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 N = (u64)1 << dm.log2n, q = N >> 2;
  const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= q) return;
  E2 out[DEEP_PTS];
  mpcs_one_round_lane<F, K>(x, dm, tab, C, i, [&](u32 c, int t) { return M[(u64)c * N + i + (u64)t * q]; }, out);
  deep_for<0, DEEP_PTS>([&](auto T) {
    constexpr int t = decltype(T)::value;
    G[i + (u64)t * q] = out[t].c0;
    G[N + i + (u64)t * q] = out[t].c1;
  });
}

// The verifier: one lane per (query, t) recomputes G[j_0 + t m] from the opened leaves of every round (round r: word c A + t) with
// the body of the combine kernel and compares it with words t and A + t of the FRI proof's layer-0 leaf, as they stand.  Bit 8:
// a matrix path of the query failed in some round (ok: [R][Q]); bit 16: a mismatch.
template <class F, int K>
__global__ void __launch_bounds__(256) mpcs_check_kernel(FriConsts k, u64 w, DeepDomain dm, MpcsTab tab, MpcsShape sh, MpcsPtrs leaves,
                                                         u32 eta, u64 n_queries, const u64* __restrict__ idx,
                                                         const u64* __restrict__ fleaf, const int* __restrict__ ok, int* status) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 A = (u64)1 << eta, total = n_queries << eta;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
    const u64 q = e >> eta, t = e & (A - 1);
    const u64 i = idx[q] + (t << (dm.log2n - eta));
    E2 out[1];
    mpcs_combine_lane<F, K, 1>(x, dm, tab, sh, i, [&](u32 r, u32 c, int) { return leaves.p[r][(q * sh.C[r] + c) * A + t]; }, out);
    int bits = 0;
    if (t == 0)
      for (u32 r = 0; r < sh.R; r++)
        if (!ok[r * n_queries + q]) bits |= 8;
    if (out[0].c0 != fleaf[q * 2 * A + t] || out[0].c1 != fleaf[q * 2 * A + A + t]) bits |= 16;
    if (bits) atomicOr(status, bits);
  }
}

// the opened leaves of one matrix, canonical: out[q][j] = M[idx[q] + j m], j < leaf_len = C A
template <class F>
__global__ void __launch_bounds__(256) mpcs_gather_kernel(FriConsts k, const u64* __restrict__ M, u32 log2m, u64 leaf_len,
                                                          const u64* __restrict__ idx, u64 n_queries, u64* __restrict__ out) {
  const F f(k);
  const u64 total = n_queries * leaf_len;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
    const u64 q = e / leaf_len, j = e % leaf_len;
    out[e] = f.out(f.in(M[idx[q] + (j << log2m)]));
  }
}

// ------------------------------------------------------------------------------------- arguments and sizes
extern "C" int ronk_mpcs_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                               uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, uint32_t n_points,
                               uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks) {
  RCHK(ronk_fri_check_ext(p, rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, 1));
  if (!n_columns || !point_masks || !n_points || !n_rounds) return RONK_ERR_INVALID;
  const u64 all = n_points >= 32 ? ~(u64)0 : ((u64)1 << n_points) - 1;   // a u32 mask lies below 2^32
  u64 seen = 0, ctot = 0;
  for (u32 r = 0; r < n_rounds; r++) {
    if (!n_columns[r] || !point_masks[r] || point_masks[r] > all) return RONK_ERR_INVALID;
    seen |= point_masks[r];
    ctot += n_columns[r];
  }
  if (seen != all) return RONK_ERR_INVALID;   // a point that no mask selects
  if (n_points > DEEP_MAX_K || n_rounds > MPCS_MAX_R || ctot > DEEP_MAX_C) return RONK_ERR_UNSUPPORTED;
  if (log2_n < 2) return RONK_ERR_UNSUPPORTED;   // a lane of the combine kernel owns four points
  return RONK_OK;
}

// the FRI handle's shape (extension challenges, planar layer 0) and the rounds', false for a shape that ronk_mpcs_check refuses
static bool mpcs_shape(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len, uint32_t K,
                       uint32_t R, const uint32_t* C, const uint32_t* masks, ronk_mpcs* h) {
  if (!ronk_fri_proof_words_ext(log2_n, log2_arity, log2_final, n_queries, digest_len, 1)) return false;
  if (log2_n < 2 || n_queries > (1u << 16) || !mpcs_host_shape(K, R, C, masks, &h->ms)) return false;
  FriShape& sh = h->sh;
  sh.n = log2_n; sh.eta = log2_arity; sh.log2_final = log2_final; sh.layers = (log2_n - log2_final) / log2_arity;
  sh.queries = n_queries; sh.d = digest_len; sh.ext = 1; sh.in_ext = 1;
  return true;
}
extern "C" size_t ronk_mpcs_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                        uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks) {
  ronk_mpcs h;
  return mpcs_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, n_rounds, n_columns, point_masks, &h)
             ? (size_t)h.proof_words() : 0;
}
extern "C" size_t ronk_mpcs_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                            uint32_t digest_len, uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns,
                                            const uint32_t* point_masks) {
  ronk_mpcs h;
  return mpcs_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, n_rounds, n_columns, point_masks, &h)
             ? (size_t)h.workspace_words() : 0;
}

// ------------------------------------------------------------------------------------- handle
extern "C" int ronk_mpcs_destroy(ronk_mpcs* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->fri) (void)ronk_fri_destroy(h->fri);
  if (h->d_dom) (void)hipFree(h->d_dom);
  if (h->d_tab) (void)hipFree(h->d_tab);
  if (h->d_vs) (void)hipFree(h->d_vs);
  delete h;
  return RONK_OK;
}

extern "C" int ronk_mpcs_create(ronk_mpcs** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                                uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                                uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!pos) return RONK_ERR_INVALID;
  RCHK(ronk_mpcs_check(pos->p, pos->rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_points,
                       n_rounds, n_columns, point_masks));
  RCHK(need_device());
  ronk_mpcs* h = new ronk_mpcs;
  mpcs_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, n_rounds, n_columns, point_masks, h);
  h->pos = pos; h->p = pos->p; h->log2_blowup = log2_blowup;
  h->c = ext2_launch(h->p, w);
  int rc = ronk_fri_create_ext(&h->fri, pos, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, 1);
  if (rc != RONK_OK) { ronk_mpcs_destroy(h); return rc; }
  const u32 kb = deep_kbits(log2_n);
  std::vector<u64> dom(((size_t)1 << kb) + ((size_t)1 << (log2_n - kb)));
  deep_host_domain(h->c.mont, h->p, g % h->p, coset_shift, log2_n, dom.data(), dom.data() + ((size_t)1 << kb), &h->dm.iota, &h->dm.sinv);
  rc = upload(dom, &h->d_dom);
  if (rc != RONK_OK) { ronk_mpcs_destroy(h); return rc; }
  h->dm.lo = h->d_dom; h->dm.hi = h->d_dom + ((size_t)1 << kb); h->dm.kbits = kb; h->dm.log2n = log2_n;
  hipError_t e = hipMalloc((void**)&h->d_tab, mpcs_tab_words(h->ms.R, h->ms.K, h->ms.Ctot) * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_vs, (h->sh.d + (u64)h->ms.R * h->sh.queries) * 8);
  if (e != hipSuccess) { ronk_mpcs_destroy(h); return hip_fail(e, "ronk_mpcs_create"); }
  *out = h;
  return RONK_OK;
}

// grinding: the owned FRI handle does it; this handle only follows its sizes
extern "C" int ronk_mpcs_set_pow(ronk_mpcs* h, uint32_t bits, uint32_t log2_limit) {
  if (!h) return RONK_ERR_INVALID;
  RCHK(ronk_fri_set_pow(h->fri, bits, log2_limit));
  h->pow_bits = bits;
  return RONK_OK;
}
extern "C" size_t ronk_mpcs_handle_proof_words(const ronk_mpcs* h) { return h ? (size_t)h->proof_words() : 0; }
extern "C" size_t ronk_mpcs_handle_workspace_words(const ronk_mpcs* h) { return h ? (size_t)h->workspace_words() : 0; }

// ------------------------------------------------------------------------------------- device entry points
// C columns of d coefficients at the points of mask; y0, y1: the two planes of the claims
static int mpcs_eval_launch(const Ext2Launch& c, const u64* d_coef, u32 C, u64 d, const u64* d_z, u32 K, u32 mask, u64* d_y0, u64* d_y1,
                            hipStream_t s) {
  EXT2_DISPATCH3(c, hipLaunchKernelGGL((mpcs_eval_kernel<FF>), dim3(C), dim3(DEEP_EVAL_LANES), 0, s, c.k, c.w, d_coef, d, d_z, K, mask, C,
                                       d_y0, d_y1));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// no handle, any odd prime: every column at every point, y planar [2][K C]
extern "C" int ronk_ext2_poly_eval_batch_dev(uint64_t p, uint64_t w, const uint64_t* d_coef, uint32_t n_columns, size_t d,
                                             const uint64_t* d_z, uint32_t n_points, uint64_t* d_y, void* stream) {
  if (!d_coef || !d_z || !d_y || !n_columns || !n_points || !d) return RONK_ERR_INVALID;
  RCHK(ronk_ext2_check(p, w));
  if (n_points > DEEP_MAX_K || n_columns > (1u << 24)) return RONK_ERR_UNSUPPORTED;
  RCHK(need_device());
  return mpcs_eval_launch(ext2_launch(p, w), d_coef, n_columns, d, d_z, n_points, mpcs_full_mask(n_points), d_y,
                          d_y + (u64)n_points * n_columns, (hipStream_t)stream);
}

static bool mpcs_all(const ronk_mpcs* h, const uint64_t* const* a) {
  if (!a) return false;
  for (u32 r = 0; r < h->ms.R; r++)
    if (!a[r]) return false;
  return true;
}
static MpcsPtrs mpcs_ptrs(const ronk_mpcs* h, const uint64_t* const* a) {
  MpcsPtrs p{};
  for (u32 r = 0; r < h->ms.R; r++) p.p[r] = a[r];
  return p;
}

static int mpcs_transcript_dev(const ronk_mpcs* h, const u64* d_seed, const MpcsPtrs& roots, const u64* d_z, const u64* d_y, u64* d_a,
                               hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((mpcs_transcript_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, (u32)h->sh.d, h->ms.R, d_seed,
                                       roots, d_z, 2 * (u64)h->ms.K, d_y, h->claims(), d_a));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// the table of a call from alpha, the points and the claims; ORs bit 32 into *d_status
static int mpcs_prep_dev(const ronk_mpcs* h, const u64* d_alpha, const u64* d_z, const u64* d_y, int* d_status, hipStream_t s) {
  EXT2_DISPATCH3(h->c, hipLaunchKernelGGL((mpcs_prep_kernel<FF>), dim3(1), dim3(256), 0, s, h->c.k, h->c.w, h->dm, h->ms, d_alpha, d_z,
                                                   d_y, h->d_tab, d_status));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_mpcs_combine_dev(const ronk_mpcs* h, const uint64_t* const* d_M, const uint64_t* d_y, const uint64_t* d_z,
                                     const uint64_t* d_alpha, uint64_t* d_G, int* d_status, void* stream) {
  if (!h || !mpcs_all(h, d_M) || !d_y || !d_z || !d_alpha || !d_G || !d_status) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const u64 q = h->sh.size(0) >> 2;
  if ((q + 255) / 256 > 0x7fffffffull) return RONK_ERR_UNSUPPORTED;
  HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), s));
  RCHK(mpcs_prep_dev(h, d_alpha, d_z, d_y, d_status, s));
  const dim3 grid((u32)((q + 255) / 256));
  if (h->ms.R == 1) {   // one round has the full mask (ronk_mpcs_check): rows first
    MPCS_DISPATCH(h, hipLaunchKernelGGL((mpcs_one_round_kernel<FF, KK>), grid, dim3(256), 0, s, h->c.k, h->c.w, h->dm, h->tab(), h->ms.C[0],
                                        d_M[0], d_G));
  } else {
    const MpcsPtrs M = mpcs_ptrs(h, d_M);
    MPCS_DISPATCH(h, hipLaunchKernelGGL((mpcs_combine_kernel<FF, KK>), grid, dim3(256), 0, s, h->c.k, h->c.w, h->dm, h->tab(), h->ms, M,
                                        d_G));
  }
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_mpcs_commit_dev(const ronk_mpcs* h, uint32_t round, const uint64_t* d_M, uint64_t* d_tree, void* stream) {
  if (!h || round >= h->ms.R || !d_M || !d_tree) return RONK_ERR_INVALID;
  const u64 m = (u64)1 << h->sh.log2m(0);
  return ronk_merkle_commit_dev(h->pos, d_M, m, h->leaf_len(round), 1, m, h->sh.d, d_tree, stream);
}

extern "C" int ronk_mpcs_open_dev(const ronk_mpcs* h, const uint64_t* const* d_M, const uint64_t* const* d_tree,
                                  const uint64_t* const* d_coef, const uint64_t* d_z, const uint64_t* d_seed, uint64_t* d_work,
                                  uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || !mpcs_all(h, d_M) || !mpcs_all(h, d_tree) || !mpcs_all(h, d_coef) || !d_z || !d_seed || !d_work || !d_proof || !d_status)
    return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const FriShape& sh = h->sh;
  const MpcsShape& ms = h->ms;
  const u64 D = sh.d, Q = sh.queries, N = sh.size(0), m = (u64)1 << sh.log2m(0);
  u64* d_a = d_work;
  int* d_st = (int*)(d_a + D);
  u64* d_G = d_work + h->small_words();
  u64* d_fri_work = d_G + 2 * N;
  const u64* d_idx = d_fri_work + sh.idx_off();   // j_0 of every query, as the prover's transcript leaves them
  u64* d_claims = d_proof;
  u64* d_fri_proof = d_proof + h->claims();
  u64* d_round = d_fri_proof + h->fri_proof();
  MpcsPtrs roots{};
  for (u32 r = 0; r < ms.R; r++) {
    RCHK(mpcs_eval_launch(h->c, d_coef[r], ms.C[r], N >> h->log2_blowup, d_z, ms.K, ms.mask[r], d_claims + ms.yoff[r],
                          d_claims + ms.Y + ms.yoff[r], s));
    roots.p[r] = d_tree[r] + ronk_merkle_tree_words(m, D) - D;
  }
  RCHK(mpcs_transcript_dev(h, d_seed, roots, d_z, d_claims, d_a, s));
  RCHK(ronk_mpcs_combine_dev(h, d_M, d_claims, d_z, d_a, d_G, d_status, stream));
  RCHK(ronk_fri_prove_dev(h->fri, d_G, d_a, d_fri_work, d_fri_proof, stream));
  for (u32 r = 0; r < ms.R; r++) {
    u64* d_leaves = d_round;
    u64* d_paths = d_leaves + Q * h->leaf_len(r);
    EXT2_DISPATCH3(h->c, hipLaunchKernelGGL((mpcs_gather_kernel<FF>), dim3(grid_for(Q * h->leaf_len(r))), dim3(256), 0, s, h->c.k, d_M[r],
                                                     sh.log2m(0), h->leaf_len(r), d_idx, Q, d_leaves));
    HIPCHK(hipGetLastError());
    RCHK(ronk_merkle_open_dev(d_tree[r], m, D, d_idx, Q, d_paths, d_st, stream));
    d_round += h->round_words(r);
  }
  return RONK_OK;
}

extern "C" int ronk_mpcs_verify_dev(const ronk_mpcs* h, const uint64_t* d_roots, const uint64_t* d_z, const uint64_t* d_seed,
                                    const uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || !d_roots || !d_z || !d_seed || !d_proof || !d_status) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const FriShape& sh = h->sh;
  const MpcsShape& ms = h->ms;
  const u64 D = sh.d, Q = sh.queries, m = (u64)1 << sh.log2m(0);
  u64* d_a = h->d_vs;
  int* d_ok = (int*)(d_a + D);
  const u64* d_idx = fri_handle_indices(h->fri);   // written by ronk_fri_verify_dev below, read after it in stream order
  const u64* d_claims = d_proof;
  const u64* d_fri_proof = d_proof + h->claims();
  const u64* d_round = d_fri_proof + h->fri_proof();
  MpcsPtrs roots{}, leaves{};
  for (u32 r = 0; r < ms.R; r++) roots.p[r] = d_roots + r * D;
  RCHK(mpcs_transcript_dev(h, d_seed, roots, d_z, d_claims, d_a, s));
  RCHK(ronk_fri_verify_dev(h->fri, d_fri_proof, d_a, d_status, stream));   // writes the status: bits 1 / 2 / 4
  RCHK(mpcs_prep_dev(h, d_a, d_z, d_claims, d_status, s));
  for (u32 r = 0; r < ms.R; r++) {
    leaves.p[r] = d_round;
    const u64* d_paths = d_round + Q * h->leaf_len(r);
    RCHK(ronk_merkle_verify_dev(h->pos, leaves.p[r], Q, h->leaf_len(r), h->leaf_len(r), 1, d_idx, d_paths, m, D, roots.p[r], d_ok + r * Q,
                                stream));
    d_round += h->round_words(r);
  }
  MPCS_DISPATCH(h, hipLaunchKernelGGL((mpcs_check_kernel<FF, KK>), dim3(grid_for(Q << sh.eta)), dim3(256), 0, s, h->c.k, h->c.w, h->dm,
                                      h->tab(), ms, leaves, sh.eta, Q, d_idx, d_fri_proof + sh.leaf_off(0), d_ok, d_status));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
extern "C" int ronk_ext2_poly_eval_batch(uint64_t p, uint64_t w, const uint64_t* coef, uint32_t n_columns, size_t d, const uint64_t* z,
                                         uint32_t n_points, uint64_t* y) {
  if (!coef || !z || !y || !n_columns || !n_points || !d) return RONK_ERR_INVALID;
  RCHK(ronk_ext2_check(p, w));
  if (n_points > DEEP_MAX_K || n_columns > (1u << 24)) return RONK_ERR_UNSUPPORTED;
  RCHK(need_device());
  const size_t ny = 2 * (size_t)n_points * n_columns;
  HostCall hc;
  const u64 *dc = hc.in(coef, (size_t)n_columns * d), *dz = hc.in(z, 2 * (size_t)n_points);
  u64* dy = hc.out(ny);
  RCHK(hc.rc);
  RCHK(ronk_ext2_poly_eval_batch_dev(p, w, dc, n_columns, d, dz, n_points, dy, nullptr));
  return hc.get(y, dy, ny * 8);
}

extern "C" int ronk_mpcs_commit(const ronk_mpcs* h, uint32_t round, const uint64_t* M, uint64_t* tree) {
  if (!h || round >= h->ms.R || !M || !tree) return RONK_ERR_INVALID;
  const size_t nt = ronk_merkle_tree_words((size_t)1 << h->sh.log2m(0), h->sh.d);
  HostCall hc;
  const u64* dm = hc.in(M, (size_t)h->ms.C[round] * h->sh.size(0));
  u64* dt = hc.out(nt);
  RCHK(hc.rc);
  RCHK(ronk_mpcs_commit_dev(h, round, dm, dt, nullptr));
  return hc.get(tree, dt, nt * 8);
}

extern "C" int ronk_mpcs_open(const ronk_mpcs* h, const uint64_t* const* M, const uint64_t* const* tree, const uint64_t* const* coef,
                              const uint64_t* z, const uint64_t* seed, uint64_t* proof, int* status) {
  if (!h || !mpcs_all(h, M) || !mpcs_all(h, tree) || !mpcs_all(h, coef) || !z || !seed || !proof || !status) return RONK_ERR_INVALID;
  const FriShape& sh = h->sh;
  const size_t nt = ronk_merkle_tree_words((size_t)1 << sh.log2m(0), sh.d);
  HostCall hc;
  const u64 *dm[MPCS_MAX_R], *dt[MPCS_MAX_R], *dc[MPCS_MAX_R];
  for (u32 r = 0; r < h->ms.R; r++) {
    dm[r] = hc.in(M[r], (size_t)h->ms.C[r] * sh.size(0));
    dt[r] = hc.in(tree[r], nt);
    dc[r] = hc.in(coef[r], (size_t)h->ms.C[r] * (sh.size(0) >> h->log2_blowup));
  }
  const u64 *dz = hc.in(z, 2 * (size_t)h->ms.K), *ds = hc.in(seed, sh.d);
  u64 *dw = hc.out(h->workspace_words()), *dp = hc.out(h->proof_words()), *dst = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_mpcs_open_dev(h, dm, dt, dc, dz, ds, dw, dp, (int*)dst, nullptr));
  RCHK(hc.get(proof, dp, h->proof_words() * 8));
  RCHK(hc.get(status, dst, sizeof(int)));
  // the FRI proof's last word: the search found nothing below the limit
  return h->pow_bits && proof[h->claims() + sh.proof_words()] == POW_NONE ? RONK_ERR_INDEX : RONK_OK;
}

extern "C" int ronk_mpcs_verify(const ronk_mpcs* h, const uint64_t* roots, const uint64_t* z, const uint64_t* seed, const uint64_t* proof,
                                int* status) {
  if (!h || !roots || !z || !seed || !proof || !status) return RONK_ERR_INVALID;
  const FriShape& sh = h->sh;
  HostCall hc;
  const u64 *dr = hc.in(roots, (size_t)h->ms.R * sh.d), *dz = hc.in(z, 2 * (size_t)h->ms.K), *ds = hc.in(seed, sh.d),
            *dp = hc.in(proof, h->proof_words());
  u64* dst = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_mpcs_verify_dev(h, dr, dz, ds, dp, (int*)dst, nullptr));
  return hc.get(status, dst, sizeof(int));
}
