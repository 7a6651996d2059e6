// ronk_fri.hip -- C ABI of libronk_ntt.so, part 9: the FRI prover and verifier over the 64-bit fields, on the Poseidon sponge
// and Merkle commitment of ronk_hash.hip (csrc/fri_kernels.h), with base-field challenges
// (ronk_fri_create) or challenges and folded layers in the quadratic extension (ronk_fri_create_ext).
// The launch context and the policy dispatch are those of csrc/ext2_launch.h.
#include "runtime.h"
#include "hip_launch.h"
#include "poseidon_handle.h"
#include "fri_kernels.h"
#include "pow_kernels.h"
#include "ext2_launch.h"

// ------------------------------------------------------------------------------------- handle
struct ronk_fri {
  const ronk_poseidon* pos;
  u64 p, g, shift;
  FriShape sh;
  u32 log2_blowup;
  // mont: any prime, and Goldilocks under a root convention without shift roots; w, w7 (shift roots and W = 7: the product with
  // W is a shift, FriGlW7): extension handles (sh.ext) only
  Ext2Launch c;
  std::vector<FriLayer> layers;   // host copy; the table pointers are device pointers
  u64* d_tab = nullptr;         // per layer lo, hi; then the final layer's w^-j
  const u64* d_wfin = nullptr;
  FriLayer* d_layers = nullptr;
  u64* d_vs = nullptr;          // the verifier's state: the small words of FriShape, then ok [L][Q] ints
  // grinding between the commit and the query phase (ronk_fri_set_pow); 0 bits: none, the launches,
  // the proof and the workspace are those of a handle without it
  u32 pow_bits = 0, pow_log2_limit = 0;
  u64 proof_words() const { return sh.proof_words() + (pow_bits ? 1 : 0); }                     // the nonce is the last word
  u64 workspace_words() const { return sh.workspace_words() + (pow_bits ? POW_WORK_WORDS : 0); }   // the prefix state, at the end
};

// the small state inside a workspace
struct FriSmall {
  u64 *betas, *chain, *u, *idx;
  int* st;
  FriSmall(const FriShape& sh, u64* base) {
    betas = base;
    chain = betas + (sh.ext ? 2 : 1) * sh.layers;
    u = chain + (sh.layers + 1) * sh.d;
    idx = base + sh.idx_off();
    st = (int*)(idx + sh.layers * sh.queries);
  }
};

#define FRI_DISPATCH_E(eta, ...)                            \
  do {                                                      \
    if ((eta) == 1) { constexpr int ETA = 1; __VA_ARGS__; } \
    else if ((eta) == 2) { constexpr int ETA = 2; __VA_ARGS__; } \
    else { constexpr int ETA = 3; __VA_ARGS__; }            \
  } while (0)
// run the statement with FF and ETA bound to the handle's field policy and arity
#define FRI_DISPATCH(h, ...) EXT2_DISPATCH2((h)->c, FRI_DISPATCH_E((h)->sh.eta, __VA_ARGS__))
// the same for the extension kernels, where Goldilocks with W = 7 has a policy of its own
#define FRI_DISPATCH_X(h, ...) EXT2_DISPATCH3((h)->c, FRI_DISPATCH_E((h)->sh.eta, __VA_ARGS__))

// ------------------------------------------------------------------------------------- kernels
// one lane per output: A loads at stride m (coalesced across lanes), one store
template <class F, int ETA>
__global__ void __launch_bounds__(256) fri_fold_kernel(FriConsts k, FriLayer ly, const u64* __restrict__ in, const u64* __restrict__ beta,
                                                       u64* __restrict__ out) {
  const F f(k);
  const u64 m = (u64)1 << ly.log2m;
  const u64 b = f.in(*beta);
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x)
    out[i] = fri_fold_leaf<F, ETA>(f, fri_gamma(f, ly, i, b), [&](int t) { return in[i + (u64)t * m]; });
}

// the extension fold: in is A base words at stride m (EXT_IN = false) or the two planes of N = A m words each; out is planar [2][m]
template <class F, int ETA, bool EXT_IN>
__global__ void __launch_bounds__(256) fri_fold_ext_kernel(FriConsts k, u64 w, FriLayer ly, const u64* __restrict__ in,
                                                           const u64* __restrict__ beta, u64* __restrict__ out) {
  const F f(k);
  const Ext2<F> x(f, w);
  const u64 m = (u64)1 << ly.log2m;
  const E2 b{f.in(beta[0]), f.in(beta[1])};
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x) {
    const E2 r = fri_fold_leaf_ext<F, ETA, EXT_IN>(x, fri_gamma_ext(x, ly, i, b), [&](int t) { return in[i + (u64)t * m]; });
    out[i] = r.c0;
    out[m + i] = r.c1;
  }
}

template <class PF, int W>
__global__ void __launch_bounds__(64) fri_transcript_kernel(PoseidonConsts k, u32 d, const u64* seed, u64* chain, const u64* roots, u32 l0,
                                                            u32 l1, u64* betas, const u64* fin, u64 nl, u64* u, u32 bw) {
  if (blockIdx.x || threadIdx.x) return;
  const PF pf(k);
  fri_transcript<PF, W>(pf, k, d, seed, chain, roots, l0, l1, betas, fin, nl, u, bw);
}

template <class PF, int W>
__global__ void __launch_bounds__(256) fri_index_kernel(PoseidonConsts k, u32 d, const u64* __restrict__ u, const FriLayer* __restrict__ layers,
                                                        u32 n_layers, u64 n_queries, u64* __restrict__ idx) {
  const PF pf(k);
  for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < n_queries; q += (u64)gridDim.x * blockDim.x)
    fri_query_indices<PF, W>(pf, k, d, u, layers, n_layers, n_queries, q, idx);
}

// the opened leaves of one layer, canonical: out[q][t] = vals[idx[q] + t m]
template <class F>
__global__ void __launch_bounds__(256) fri_gather_kernel(FriConsts k, const u64* __restrict__ vals, u32 log2m, u32 eta,
                                                         const u64* __restrict__ idx, u64 n_queries, u64* __restrict__ out) {
  const F f(k);
  const u64 total = n_queries << eta;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
    const u64 q = e >> eta, t = e & (((u64)1 << eta) - 1);
    out[e] = f.out(f.in(vals[idx[q] + (t << log2m)]));
  }
}

// one lane per query: the Merkle flags of its layers (bit 1) and the fold consistency (bit 2)
template <class F, int ETA>
__global__ void __launch_bounds__(256) fri_check_kernel(FriConsts k, const FriLayer* __restrict__ layers, u32 n_layers, u64 n_queries,
                                                        const u64* __restrict__ proof, u64 final_off, const u64* __restrict__ betas,
                                                        const u64* __restrict__ idx, const int* __restrict__ ok, int* status) {
  const F f(k);
  for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < n_queries; q += (u64)gridDim.x * blockDim.x) {
    int bits = 0;
    for (u32 l = 0; l < n_layers; l++)
      if (!ok[(u64)l * n_queries + q]) bits |= 1;
    if (!fri_check_query<F, ETA>(f, layers, n_layers, n_queries, proof, final_off, betas, idx, q)) bits |= 2;
    if (bits) atomicOr(status, bits);
  }
}

template <class F, int ETA>
__global__ void __launch_bounds__(256) fri_check_ext_kernel(FriConsts k, u64 w, const FriLayer* __restrict__ layers, u32 n_layers,
                                                            u64 n_queries, const u64* __restrict__ proof, u64 final_off, u64 nl,
                                                            u32 in_ext, const u64* __restrict__ betas, const u64* __restrict__ idx,
                                                            const int* __restrict__ ok, int* status) {
  const F f(k);
  const Ext2<F> x(f, w);
  for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < n_queries; q += (u64)gridDim.x * blockDim.x) {
    int bits = 0;
    for (u32 l = 0; l < n_layers; l++)
      if (!ok[(u64)l * n_queries + q]) bits |= 1;
    if (!fri_check_query_ext<F, ETA>(x, layers, n_layers, n_queries, proof, final_off, nl, in_ext != 0, betas, idx, q)) bits |= 2;
    if (bits) atomicOr(status, bits);
  }
}

// one workgroup: lane k holds coefficient k of the final layer's interpolant; those from `first` on must vanish (bit 4)
template <class F>
__global__ void __launch_bounds__(256) fri_final_kernel(FriConsts k, const u64* __restrict__ wtab, const u64* __restrict__ fin, u32 n,
                                                        u32 first, int* status) {
  const F f(k);
  const u32 c = threadIdx.x;
  if (c >= first && c < n && fri_final_coeff(f, wtab, fin, n, c) != 0) atomicOr(status, 4);
}
// the same for a planar final layer: both planes must be of low degree (the domain is in the base field)
template <class F>
__global__ void __launch_bounds__(256) fri_final_ext_kernel(FriConsts k, const u64* __restrict__ wtab, const u64* __restrict__ fin, u32 n,
                                                            u32 first, int* status) {
  const F f(k);
  const u32 c = threadIdx.x;
  if (c >= first && c < n && (fri_final_coeff(f, wtab, fin, n, c) | fri_final_coeff(f, wtab, fin + n, n, c)) != 0) atomicOr(status, 4);
}

// ------------------------------------------------------------------------------------- arguments and sizes
extern "C" int ronk_fri_check(uint64_t p, uint32_t rate, uint64_t g, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                              uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len) {
  if (p < 3 || !(p & 1)) return RONK_ERR_INVALID;
  if (log2_arity < 1 || log2_arity > 3) return RONK_ERR_INVALID;
  if (log2_final > 8) return RONK_ERR_UNSUPPORTED;
  if (log2_blowup > log2_final) return RONK_ERR_INVALID;
  if (log2_n > 63 || ((p - 1) & (((u64)1 << log2_n) - 1))) return RONK_ERR_NO_ROOT;
  if (log2_n < log2_final + log2_arity || (log2_n - log2_final) % log2_arity) return RONK_ERR_INVALID;
  if (!n_queries || !digest_len || digest_len > rate) return RONK_ERR_INVALID;
  if (n_queries > (1u << 16)) return RONK_ERR_UNSUPPORTED;
  if (coset_shift % p == 0 || g % p == 0) return RONK_ERR_INVALID;
  // w_N = g^((p - 1) / N) must have order N exactly (g a generator, or at least of full 2-power order)
  if (fri_powmod(g, (p - 1) >> 1, p) == 1) return RONK_ERR_INVALID;
  return RONK_OK;
}

static bool fri_shape(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len, FriShape* sh,
                      uint32_t ext = 0, uint32_t input_ext = 0) {
  if (log2_arity < 1 || log2_arity > 3 || log2_final > 8 || log2_n > 63 || log2_n < log2_final + log2_arity ||
      (log2_n - log2_final) % log2_arity || !n_queries || !digest_len || (ext && (digest_len < 2 || input_ext > 1)))
    return false;
  sh->n = log2_n; sh->eta = log2_arity; sh->log2_final = log2_final; sh->layers = (log2_n - log2_final) / log2_arity;
  sh->queries = n_queries; sh->d = digest_len; sh->ext = ext; sh->in_ext = ext ? input_ext : 0;
  return true;
}
extern "C" size_t ronk_fri_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len) {
  FriShape sh;
  return fri_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, &sh) ? (size_t)sh.proof_words() : 0;
}
extern "C" size_t ronk_fri_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                           uint32_t digest_len) {
  FriShape sh;
  return fri_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, &sh) ? (size_t)sh.workspace_words() : 0;
}

extern "C" int ronk_fri_check_ext(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                                  uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                                  uint32_t input_ext) {
  RCHK(ronk_fri_check(p, rate, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len));
  RCHK(ronk_ext2_check(p, w));
  if (digest_len < 2 || input_ext > 1) return RONK_ERR_INVALID;   // a challenge takes two sponge words
  return RONK_OK;
}
extern "C" size_t ronk_fri_proof_words_ext(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                           uint32_t digest_len, uint32_t input_ext) {
  FriShape sh;
  return fri_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, &sh, 1, input_ext) ? (size_t)sh.proof_words() : 0;
}
extern "C" size_t ronk_fri_workspace_words_ext(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                               uint32_t digest_len, uint32_t input_ext) {
  FriShape sh;
  return fri_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, &sh, 1, input_ext) ? (size_t)sh.workspace_words() : 0;
}

// ------------------------------------------------------------------------------------- handle
extern "C" int ronk_fri_destroy(ronk_fri* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->d_tab) (void)hipFree(h->d_tab);
  if (h->d_layers) (void)hipFree(h->d_layers);
  if (h->d_vs) (void)hipFree(h->d_vs);
  delete h;
  return RONK_OK;
}

// ext: the handle of ronk_fri_create_ext (w, input_ext are read); the arguments have passed their check
static int fri_create(ronk_fri** out, const ronk_poseidon* pos, uint64_t g, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                      uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, bool ext, uint64_t w,
                      uint32_t input_ext) {
  RCHK(need_device());
  ronk_fri* h = new ronk_fri;
  h->pos = pos; h->p = pos->p; h->g = g % h->p; h->shift = coset_shift % h->p; h->log2_blowup = log2_blowup;
  fri_shape(log2_n, log2_arity, log2_final, n_queries, digest_len, &h->sh, ext, input_ext);
  const FriShape& sh = h->sh;
  const bool mont = !fri_gl_shift_roots(h->p, h->g, sh.eta);
  h->c = ext2_launch(mont, fri_host_consts(mont, h->p, h->g, sh.eta), h->p, ext ? w : 0);
  // tables: per layer lo then hi, then the final layer's roots
  std::vector<size_t> off(sh.layers + 1);
  size_t words = 0;
  for (u32 l = 0; l < sh.layers; l++) {
    const u32 lm = sh.log2m(l), kb = fri_kbits(lm);
    off[l] = words;
    words += ((size_t)1 << kb) + ((size_t)1 << (lm - kb));
  }
  off[sh.layers] = words;
  words += (size_t)sh.size(sh.layers);
  std::vector<u64> tab(words);
  for (u32 l = 0; l < sh.layers; l++) {
    const u32 kb = fri_kbits(sh.log2m(l));
    fri_host_layer_table(mont, h->p, h->g, h->shift, sh, l, tab.data() + off[l], tab.data() + off[l] + ((size_t)1 << kb));
  }
  fri_host_final_table(mont, h->p, h->g, sh, tab.data() + off[sh.layers]);
  int rc = upload(tab, &h->d_tab);
  if (rc != RONK_OK) { ronk_fri_destroy(h); return rc; }
  h->d_wfin = h->d_tab + off[sh.layers];
  h->layers.resize(sh.layers);
  for (u32 l = 0; l < sh.layers; l++) {
    FriLayer& ly = h->layers[l];
    ly.log2m = sh.log2m(l); ly.kbits = fri_kbits(ly.log2m);
    ly.lo = h->d_tab + off[l]; ly.hi = ly.lo + ((size_t)1 << ly.kbits);
    ly.leaf_off = sh.leaf_off(l); ly.path_off = sh.path_off(l);
  }
  hipError_t e = hipMalloc((void**)&h->d_layers, sh.layers * sizeof(FriLayer));
  if (e == hipSuccess) e = hipMemcpy(h->d_layers, h->layers.data(), sh.layers * sizeof(FriLayer), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_vs, (sh.small_words() + sh.layers * sh.queries) * 8);
  if (e != hipSuccess) { ronk_fri_destroy(h); return hip_fail(e, "ronk_fri_create"); }
  *out = h;
  return RONK_OK;
}

extern "C" int ronk_fri_create(ronk_fri** out, const ronk_poseidon* pos, uint64_t g, uint32_t log2_n, uint64_t coset_shift,
                               uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!pos) return RONK_ERR_INVALID;
  RCHK(ronk_fri_check(pos->p, pos->rate, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len));
  return fri_create(out, pos, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, false, 0, 0);
}
extern "C" int ronk_fri_create_ext(ronk_fri** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                                   uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries,
                                   uint32_t digest_len, uint32_t input_ext) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!pos) return RONK_ERR_INVALID;
  RCHK(ronk_fri_check_ext(pos->p, pos->rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len,
                          input_ext));
  return fri_create(out, pos, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, true, w, input_ext);
}

// grinding (include/ronk_ntt.h "proof of work"): set before the handle is used
extern "C" int ronk_fri_set_pow(ronk_fri* h, uint32_t bits, uint32_t log2_limit) {
  if (!h) return RONK_ERR_INVALID;
  RCHK(ronk_pow_check(h->p, h->pos->rate, h->sh.d, bits, log2_limit));
  h->pow_bits = bits; h->pow_log2_limit = log2_limit;
  return RONK_OK;
}
extern "C" size_t ronk_fri_handle_proof_words(const ronk_fri* h) { return h ? (size_t)h->proof_words() : 0; }
extern "C" size_t ronk_fri_handle_workspace_words(const ronk_fri* h) { return h ? (size_t)h->workspace_words() : 0; }

// ------------------------------------------------------------------------------------- device entry points
extern "C" int ronk_fri_fold_dev(const ronk_fri* h, uint32_t layer, const uint64_t* d_in, const uint64_t* d_beta, uint64_t* d_out,
                                 void* stream) {
  if (!h || !d_in || !d_beta || !d_out || layer >= h->sh.layers) return RONK_ERR_INVALID;
  const FriLayer& ly = h->layers[layer];
  if (h->sh.ext) {
    // d_beta: two words; d_in: layer `layer` as the handle lays it out; d_out: planar [2][N_l / A]
    if (h->sh.vw(layer) == 2)
      FRI_DISPATCH_X(h, hipLaunchKernelGGL((fri_fold_ext_kernel<FF, ETA, true>), dim3(grid_for((size_t)1 << ly.log2m)), dim3(256), 0,
                                         (hipStream_t)stream, h->c.k, h->c.w, ly, d_in, d_beta, d_out));
    else
      FRI_DISPATCH_X(h, hipLaunchKernelGGL((fri_fold_ext_kernel<FF, ETA, false>), dim3(grid_for((size_t)1 << ly.log2m)), dim3(256), 0,
                                         (hipStream_t)stream, h->c.k, h->c.w, ly, d_in, d_beta, d_out));
    HIPCHK(hipGetLastError());
    return RONK_OK;
  }
  FRI_DISPATCH(h, hipLaunchKernelGGL((fri_fold_kernel<FF, ETA>), dim3(grid_for((size_t)1 << ly.log2m)), dim3(256), 0, (hipStream_t)stream,
                                     h->c.k, ly, d_in, d_beta, d_out));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// the transcript for the layers [l0, l1) (and u when d_final is given), one lane
static int fri_transcript_dev(const ronk_fri* h, const FriSmall& sm, const u64* d_seed, const u64* d_roots, u32 l0, u32 l1,
                              const u64* d_final, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((fri_transcript_kernel<FLD, W>), dim3(1), dim3(64), 0, s, pos->sp, (u32)h->sh.d, d_seed, sm.chain,
                                       d_roots, l0, l1, sm.betas, d_final, h->sh.vw(h->sh.layers) * h->sh.size(h->sh.layers), sm.u,
                                       h->sh.ext ? 2u : 1u));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}
static int fri_indices_dev(const ronk_fri* h, const FriSmall& sm, hipStream_t s) {
  const ronk_poseidon* pos = h->pos;
  POS_DISPATCH(pos, hipLaunchKernelGGL((fri_index_kernel<FLD, W>), dim3(grid_for(h->sh.queries)), dim3(256), 0, s, pos->sp, (u32)h->sh.d,
                                       sm.u, h->d_layers, h->sh.layers, h->sh.queries, sm.idx));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_fri_prove_dev(const ronk_fri* h, const uint64_t* d_evals, const uint64_t* d_seed, uint64_t* d_work, uint64_t* d_proof,
                                  void* stream) {
  if (!h || !d_evals || !d_seed || !d_work || !d_proof) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const FriShape& sh = h->sh;
  const u32 L = sh.layers;
  const u64 D = sh.d, Q = sh.queries, BW = sh.ext ? 2 : 1;
  const FriSmall sm(sh, d_work);
  u64* next = d_work + sh.small_words();
  std::vector<const u64*> vals(L + 1), trees(L);
  vals[0] = d_evals;
  // commit phase: commit layer l, draw beta_l from its root, fold
  for (u32 l = 0; l < L; l++) {
    const u64 m = (u64)1 << sh.log2m(l);
    u64* nxt = next;
    u64* tree = nxt + sh.vw(l + 1) * sh.size(l + 1);
    next = tree + sh.tree_words(l);
    // a planar layer's leaf is its A c0 values then its A c1 values: word c A + t sits at offset i + (c A + t) m
    RCHK(ronk_merkle_commit_dev(h->pos, vals[l], m, sh.leaf_len(l), 1, m, D, tree, stream));
    HIPCHK(hipMemcpyAsync(d_proof + l * D, tree + sh.tree_words(l) - D, D * 8, hipMemcpyDeviceToDevice, s));
    RCHK(fri_transcript_dev(h, sm, d_seed, d_proof, l, l + 1, nullptr, s));
    RCHK(ronk_fri_fold_dev(h, l, vals[l], sm.betas + BW * l, nxt, stream));
    vals[l + 1] = nxt;
    trees[l] = tree;
  }
  u64* d_final = d_proof + L * D;
  HIPCHK(hipMemcpyAsync(d_final, vals[L], sh.vw(L) * sh.size(L) * 8, hipMemcpyDeviceToDevice, s));
  RCHK(fri_transcript_dev(h, sm, d_seed, d_proof, L, L, d_final, s));
  if (h->pow_bits) {
    // grinding: the nonce of the seed u into the proof's last word, then u' = sponge(u || [nonce]) in the place of u
    u64* d_nonce = d_proof + sh.proof_words();
    RCHK(pow_grind_launch(h->pos, sm.u, (u32)D, h->pow_bits, h->pow_log2_limit, 0, d_work + sh.workspace_words(), d_nonce, s));
    RCHK(pow_reseed_launch(h->pos, (u32)D, sm.u, h->pow_bits, h->pow_log2_limit, d_nonce, nullptr, s));
  }
  // query phase: the indices, then every layer's leaves and paths
  RCHK(fri_indices_dev(h, sm, s));
  for (u32 l = 0; l < L; l++) {
    const u64 m = (u64)1 << sh.log2m(l);
    RCHK(ronk_merkle_open_dev(trees[l], m, D, sm.idx + l * Q, Q, d_proof + sh.path_off(l), sm.st, stream));
    const u32 log2_leaf = sh.eta + (sh.vw(l) == 2);   // the 2 A words of a planar leaf are gathered at the same stride m
    EXT2_DISPATCH2(h->c, hipLaunchKernelGGL((fri_gather_kernel<FF>), dim3(grid_for(Q << log2_leaf)), dim3(256), 0, s, h->c.k, vals[l],
                                            sh.log2m(l), log2_leaf, sm.idx + l * Q, Q, d_proof + sh.leaf_off(l)));
    HIPCHK(hipGetLastError());
  }
  return RONK_OK;
}

extern "C" int ronk_fri_verify_dev(const ronk_fri* h, const uint64_t* d_proof, const uint64_t* d_seed, int* d_status, void* stream) {
  if (!h || !d_proof || !d_seed || !d_status) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const FriShape& sh = h->sh;
  const u32 L = sh.layers;
  const u64 D = sh.d, Q = sh.queries;
  const FriSmall sm(sh, h->d_vs);
  int* ok = (int*)(h->d_vs + sh.small_words());
  const u64* d_final = d_proof + L * D;
  HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), s));
  RCHK(fri_transcript_dev(h, sm, d_seed, d_proof, 0, L, d_final, s));
  // the nonce as it stands: bit 64 when it is out of range or fails, and u' from it either way, so that every other check runs
  if (h->pow_bits)
    RCHK(pow_reseed_launch(h->pos, (u32)D, sm.u, h->pow_bits, h->pow_log2_limit, d_proof + sh.proof_words(), d_status, s));
  RCHK(fri_indices_dev(h, sm, s));
  for (u32 l = 0; l < L; l++)
    RCHK(ronk_merkle_verify_dev(h->pos, d_proof + sh.leaf_off(l), Q, sh.leaf_len(l), sh.leaf_len(l), 1, sm.idx + l * Q, d_proof + sh.path_off(l),
                                (u64)1 << sh.log2m(l), D, d_proof + l * D, ok + l * Q, stream));
  const u32 nl = (u32)sh.size(L), first = nl >> h->log2_blowup;
  if (sh.ext) {
    FRI_DISPATCH_X(h, hipLaunchKernelGGL((fri_check_ext_kernel<FF, ETA>), dim3(grid_for(Q)), dim3(256), 0, s, h->c.k, h->c.w, h->d_layers, L,
                                       Q, d_proof, (u64)(L * D), (u64)nl, sh.in_ext, sm.betas, sm.idx, ok, d_status));
    HIPCHK(hipGetLastError());
    if (first < nl) {
      EXT2_DISPATCH2(h->c, hipLaunchKernelGGL((fri_final_ext_kernel<FF>), dim3(1), dim3(256), 0, s, h->c.k, h->d_wfin, d_final, nl, first,
                                              d_status));
      HIPCHK(hipGetLastError());
    }
    return RONK_OK;
  }
  FRI_DISPATCH(h, hipLaunchKernelGGL((fri_check_kernel<FF, ETA>), dim3(grid_for(Q)), dim3(256), 0, s, h->c.k, h->d_layers, L, Q, d_proof,
                                     (u64)(L * D), sm.betas, sm.idx, ok, d_status));
  HIPCHK(hipGetLastError());
  if (first < nl) {
    EXT2_DISPATCH2(h->c, hipLaunchKernelGGL((fri_final_kernel<FF>), dim3(1), dim3(256), 0, s, h->c.k, h->d_wfin, d_final, nl, first,
                                            d_status));
    HIPCHK(hipGetLastError());
  }
  return RONK_OK;
}

// where the last verify or query-indices call on the handle left j_0 of every query (runtime.h)
const u64* fri_handle_indices(const ronk_fri* h) { return h->d_vs + h->sh.idx_off(); }

// the transcript of a proof and its query indices, in the verifier's state; d_indices receives j_0 of every query
extern "C" int ronk_fri_query_indices_dev(const ronk_fri* h, const uint64_t* d_proof, const uint64_t* d_seed, uint64_t* d_indices,
                                          void* stream) {
  if (!h || !d_proof || !d_seed || !d_indices) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const FriShape& sh = h->sh;
  const FriSmall sm(sh, h->d_vs);
  RCHK(fri_transcript_dev(h, sm, d_seed, d_proof, 0, sh.layers, d_proof + sh.layers * sh.d, s));
  if (h->pow_bits)
    RCHK(pow_reseed_launch(h->pos, (u32)sh.d, sm.u, h->pow_bits, h->pow_log2_limit, d_proof + sh.proof_words(), nullptr, s));
  RCHK(fri_indices_dev(h, sm, s));
  HIPCHK(hipMemcpyAsync(d_indices, sm.idx, sh.queries * 8, hipMemcpyDeviceToDevice, s));   // layer 0: j_0 mod m_0 = j_0
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms
extern "C" int ronk_fri_prove(const ronk_fri* h, const uint64_t* evals, const uint64_t* seed, uint64_t* proof) {
  if (!h || !evals || !seed || !proof) return RONK_ERR_INVALID;
  RCHK(need_device());
  const FriShape& sh = h->sh;
  HostCall hc;
  const u64 *de = hc.in(evals, sh.vw(0) * sh.size(0)), *ds = hc.in(seed, sh.d);
  u64 *dw = hc.out(h->workspace_words()), *dp = hc.out(h->proof_words());
  RCHK(hc.rc);
  RCHK(ronk_fri_prove_dev(h, de, ds, dw, dp, nullptr));
  RCHK(hc.get(proof, dp, h->proof_words() * 8));
  return h->pow_bits && proof[sh.proof_words()] == POW_NONE ? RONK_ERR_INDEX : RONK_OK;   // the search found nothing below the limit
}

extern "C" int ronk_fri_verify(const ronk_fri* h, const uint64_t* proof, const uint64_t* seed, int* status) {
  if (!h || !proof || !seed || !status) return RONK_ERR_INVALID;
  RCHK(need_device());
  const FriShape& sh = h->sh;
  HostCall hc;
  const u64 *dp = hc.in(proof, h->proof_words()), *ds = hc.in(seed, sh.d);
  u64* dst = hc.out(1);
  RCHK(hc.rc);
  RCHK(ronk_fri_verify_dev(h, dp, ds, (int*)dst, nullptr));
  return hc.get(status, dst, sizeof(int));
}
