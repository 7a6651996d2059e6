// ronk_pcs.hip -- C ABI of libronk_ntt.so, part 11: the batched FRI polynomial commitment with DEEP quotients (include/ronk_ntt.h
// "batched FRI polynomial commitment").  One [C][N] matrix opened at K points is the multi-matrix commitment
// (csrc/ronk_mpcs.hip) with one round, C columns and the full mask: a handle owns such a ronk_mpcs and every
// entry point forwards to the one of the same name with arrays of length one.  No kernel, no device memory and no layout of its
// own; ronk_ext2_poly_eval_batch* lives beside the evaluation kernel in ronk_mpcs.hip.
#include "runtime.h"
#include "poseidon_handle.h"
#include "mpcs_kernels.h"

struct ronk_pcs {
  ronk_mpcs* m = nullptr;   // owned: R = 1, n_columns = {C}, point_masks = {2^K - 1}
};

// ------------------------------------------------------------------------------------- arguments and sizes
extern "C" int ronk_pcs_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                              uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, uint32_t n_columns,
                              uint32_t n_points) {
  // the FRI codes first, whatever the batch says; then no column or point before too many of either
  RCHK(ronk_fri_check_ext(p, rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, 1));
  if (!n_columns || !n_points) return RONK_ERR_INVALID;
  if (n_points > DEEP_MAX_K) return RONK_ERR_UNSUPPORTED;   // before the mask is formed
  const uint32_t mask = mpcs_full_mask(n_points);
  return ronk_mpcs_check(p, rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_points, 1,
                         &n_columns, &mask);
}

extern "C" size_t ronk_pcs_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                       uint32_t n_columns, uint32_t n_points) {
  if (!n_points || n_points > DEEP_MAX_K) return 0;
  const uint32_t mask = mpcs_full_mask(n_points);
  return ronk_mpcs_proof_words(log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, 1, &n_columns, &mask);
}
extern "C" size_t ronk_pcs_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries,
                                           uint32_t digest_len, uint32_t n_columns, uint32_t n_points) {
  if (!n_points || n_points > DEEP_MAX_K) return 0;
  const uint32_t mask = mpcs_full_mask(n_points);
  return ronk_mpcs_workspace_words(log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, 1, &n_columns, &mask);
}

// ------------------------------------------------------------------------------------- handle
extern "C" int ronk_pcs_destroy(ronk_pcs* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->m) (void)ronk_mpcs_destroy(h->m);
  delete h;
  return RONK_OK;
}

extern "C" int ronk_pcs_create(ronk_pcs** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                               uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                               uint32_t n_columns, uint32_t n_points) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!pos) return RONK_ERR_INVALID;
  RCHK(ronk_pcs_check(pos->p, pos->rate, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_columns,
                      n_points));
  const uint32_t mask = mpcs_full_mask(n_points);
  ronk_mpcs* m = nullptr;
  RCHK(ronk_mpcs_create(&m, pos, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_points, 1,
                        &n_columns, &mask));
  *out = new ronk_pcs{m};
  return RONK_OK;
}

extern "C" int ronk_pcs_set_pow(ronk_pcs* h, uint32_t bits, uint32_t log2_limit) {
  return h ? ronk_mpcs_set_pow(h->m, bits, log2_limit) : RONK_ERR_INVALID;
}
extern "C" size_t ronk_pcs_handle_proof_words(const ronk_pcs* h) { return h ? ronk_mpcs_handle_proof_words(h->m) : 0; }
extern "C" size_t ronk_pcs_handle_workspace_words(const ronk_pcs* h) { return h ? ronk_mpcs_handle_workspace_words(h->m) : 0; }

// ------------------------------------------------------------------------------------- device entry points
// Every pointer is tested here, before the handle is read; the forwarded call tests them again as the elements of its arrays.
extern "C" int ronk_deep_combine_dev(const ronk_pcs* h, const uint64_t* d_M, const uint64_t* d_y, const uint64_t* d_z,
                                     const uint64_t* d_alpha, uint64_t* d_G, int* d_status, void* stream) {
  if (!h || !d_M || !d_y || !d_z || !d_alpha || !d_G || !d_status) return RONK_ERR_INVALID;
  return ronk_mpcs_combine_dev(h->m, &d_M, d_y, d_z, d_alpha, d_G, d_status, stream);
}

extern "C" int ronk_pcs_commit_dev(const ronk_pcs* h, const uint64_t* d_M, uint64_t* d_tree, void* stream) {
  if (!h || !d_M || !d_tree) return RONK_ERR_INVALID;
  return ronk_mpcs_commit_dev(h->m, 0, d_M, d_tree, stream);
}

extern "C" int ronk_pcs_open_dev(const ronk_pcs* h, const uint64_t* d_M, const uint64_t* d_tree, const uint64_t* d_coef, const uint64_t* d_z,
                                 const uint64_t* d_seed, uint64_t* d_work, uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || !d_M || !d_tree || !d_coef || !d_z || !d_seed || !d_work || !d_proof || !d_status) return RONK_ERR_INVALID;
  return ronk_mpcs_open_dev(h->m, &d_M, &d_tree, &d_coef, d_z, d_seed, d_work, d_proof, d_status, stream);
}

// d_root is the [1][D] roots
extern "C" int ronk_pcs_verify_dev(const ronk_pcs* h, const uint64_t* d_root, const uint64_t* d_z, const uint64_t* d_seed,
                                   const uint64_t* d_proof, int* d_status, void* stream) {
  if (!h || !d_root || !d_z || !d_seed || !d_proof || !d_status) return RONK_ERR_INVALID;
  return ronk_mpcs_verify_dev(h->m, d_root, d_z, d_seed, d_proof, d_status, stream);
}

// ------------------------------------------------------------------------------------- host-pointer forms, synchronous
extern "C" int ronk_pcs_commit(const ronk_pcs* h, const uint64_t* M, uint64_t* tree) {
  if (!h || !M || !tree) return RONK_ERR_INVALID;
  return ronk_mpcs_commit(h->m, 0, M, tree);
}

extern "C" int ronk_pcs_open(const ronk_pcs* h, const uint64_t* M, const uint64_t* tree, const uint64_t* coef, const uint64_t* z,
                             const uint64_t* seed, uint64_t* proof, int* status) {
  if (!h || !M || !tree || !coef || !z || !seed || !proof || !status) return RONK_ERR_INVALID;
  return ronk_mpcs_open(h->m, &M, &tree, &coef, z, seed, proof, status);
}

extern "C" int ronk_pcs_verify(const ronk_pcs* h, const uint64_t* root, const uint64_t* z, const uint64_t* seed, const uint64_t* proof,
                               int* status) {
  if (!h || !root || !z || !seed || !proof || !status) return RONK_ERR_INVALID;
  return ronk_mpcs_verify(h->m, root, z, seed, proof, status);
}
