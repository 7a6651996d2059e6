// ronk_hash.hip -- C ABI of libronk_ntt.so, part 7: Poseidon over the 64-bit fields (permutation, sponge) and the Merkle
// commitment built on the sponge (csrc/poseidon_kernels.h; DESIGN.md "Poseidon and Merkle commitment").
#include "runtime.h"
#include "hip_launch.h"
#include "poseidon_handle.h"

// ------------------------------------------------------------------------------------- kernels
template <class F, int W>
__global__ void __launch_bounds__(256) poseidon_permute_kernel(PoseidonConsts k, u32 width, u64* __restrict__ states, u64 count) {
  const F f(k);
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < count; i += (u64)gridDim.x * blockDim.x)
    poseidon_permute_words<F, W>(f, k, width, states + i * width);
}

template <class F, int W>
__global__ void __launch_bounds__(256) poseidon_sponge_kernel(PoseidonConsts k, const u64* __restrict__ in, u64 n_items, u64 len,
                                                              u64 item_stride, u64 elem_stride, u64* __restrict__ out, u64 n_out) {
  const F f(k);
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n_items; i += (u64)gridDim.x * blockDim.x) {
    const u64* src = in + i * item_stride;
    u64* dst = out + i * n_out;
    poseidon_sponge<F, W>(f, k, len, n_out, [&](u64 j) { return src[j * elem_stride]; }, [&](u64 q, u64 v) { dst[q] = v; });
  }
}

// one level of the tree from the level below, one lane per node
template <class F, int W>
__global__ void __launch_bounds__(256) merkle_level_kernel(PoseidonConsts k, const u64* __restrict__ lvl, u64 cnt, u32 d,
                                                           u64* __restrict__ nxt) {
  const F f(k);
  const u64 cn = (cnt + 1) / 2;
  for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < cn; t += (u64)gridDim.x * blockDim.x)
    merkle_level_node<F, W>(f, k, lvl, cnt, d, nxt, t);
}

// nodes bid * 256 .. of a level that is already in the tree (at word offset `off`, n_lvl nodes): `climb` levels up inside the
// workgroup (the top of the tree: one workgroup, n_lvl <= 256, every remaining level)
template <class F, int W>
__global__ void __launch_bounds__(256) merkle_node_kernel(PoseidonConsts k, u64* __restrict__ tree, u64 off, u64 n_lvl, u32 d,
                                                          u32 climb) {
  extern __shared__ u64 merkle_lds[];
  const F f(k);
  u64* bufa = merkle_lds;
  u64* bufb = merkle_lds + (u64)MERKLE_BLOCK * d;
  const u32 tid = threadIdx.x;
  const u64 bid = blockIdx.x, first = bid * MERKLE_BLOCK;
  const u32 cnt = (u32)(n_lvl - first < MERKLE_BLOCK ? n_lvl - first : MERKLE_BLOCK);
  const u64* src = tree + off + first * d;
  for (u32 e = tid; e < cnt * d; e += MERKLE_BLOCK) bufa[e] = src[e];
  merkle_climb<F, W>(f, k, bufa, bufb, bid, cnt, d, climb, n_lvl, off + n_lvl * d, tree, [&](auto&& fn) { __syncthreads(); fn(tid); });
}

__global__ void __launch_bounds__(256) merkle_open_kernel(const u64* __restrict__ tree, u64 n, u64 d, const u64* __restrict__ indices,
                                                          u64 n_idx, u64* __restrict__ paths, int* __restrict__ status) {
  const u64 depth = merkle_levels(n) - 1;
  for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < n_idx; q += (u64)gridDim.x * blockDim.x)
    status[q] = merkle_open_one(tree, n, d, indices[q], paths + q * depth * d) ? RONK_ERR_INDEX : 0;
}

template <class F, int W>
__global__ void __launch_bounds__(256) merkle_verify_kernel(PoseidonConsts k, const u64* __restrict__ leaves, u64 n_idx, u64 leaf_len,
                                                            u64 item_stride, u64 elem_stride, const u64* __restrict__ indices,
                                                            const u64* __restrict__ paths, u64 n, u32 d, const u64* __restrict__ root,
                                                            int* __restrict__ ok) {
  extern __shared__ u64 merkle_lds[];
  const F f(k);
  const u64 depth = merkle_levels(n) - 1;
  u64* h = merkle_lds + (u64)threadIdx.x * 3 * d;   // lane-private (digest + the pair a node absorbs): no barrier
  for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < n_idx; q += (u64)gridDim.x * blockDim.x) {
    const u64* src = leaves + q * item_stride;
    ok[q] = merkle_verify_one<F, W>(f, k, leaf_len, [&](u64 j) { return src[j * elem_stride]; }, indices[q], paths + q * depth * d, n, d,
                                    root, h);
  }
}

// ------------------------------------------------------------------------------------- Poseidon
extern "C" int ronk_poseidon_create(ronk_poseidon** out, uint64_t p, uint32_t width, uint64_t alpha, uint32_t num_p, uint32_t num_f,
                                    uint32_t rate, const uint64_t* rc, const uint64_t* mds) {
  if (!out) return RONK_ERR_INVALID;
  *out = nullptr;
  if (!rc || !mds || width < 2) return RONK_ERR_INVALID;
  if (width > 16) return RONK_ERR_UNSUPPORTED;
  if (rate < 1 || rate >= width || alpha < 1 || p < 2) return RONK_ERR_INVALID;
  if ((u64)num_p + num_f > (1u << 20)) return RONK_ERR_UNSUPPORTED;
  if (p == 2) return RONK_ERR_UNSUPPORTED;
  if (!(p & 1)) return RONK_ERR_NOT_PRIME;
  RCHK(ronk_check_prime(p));
  RCHK(need_device());
  const u32 W = poseidon_padded_width(width), rounds = num_p + num_f;
  const size_t nrc = (size_t)rounds * W, nm = (size_t)W * W;
  std::vector<u64> tab(2 * (nrc + nm), 0);
  poseidon_host_tables(p, width, rate, rounds, rc, mds, tab.data());
  ronk_poseidon* h = new ronk_poseidon;
  h->p = p; h->width = width; h->W = W; h->rate = rate; h->num_p = num_p; h->num_f = num_f; h->alpha = alpha;
  const int rc_up = upload(tab, &h->d_tab);
  if (rc_up != RONK_OK) { delete h; return rc_up; }
  PoseidonConsts k{};
  k.alpha = alpha; k.rounds = rounds; k.full_lo = num_f / 2; k.full_from = num_p + num_f / 2; k.rate = rate;
  if (p != RONK_GOLDILOCKS_P) {
    const mont64::Field mf = mont64::make_field(p);
    k.p = p; k.pinv = mf.pinv; k.r2 = mf.r2;
  }
  h->nat = k; h->nat.rc = h->d_tab; h->nat.mds = h->d_tab + nrc;
  h->sp = k; h->sp.rc = h->d_tab + nrc + nm; h->sp.mds = h->d_tab + 2 * nrc + nm;
  *out = h;
  return RONK_OK;
}

extern "C" int ronk_poseidon_destroy(ronk_poseidon* h) {
  if (!h) return RONK_ERR_INVALID;
  if (h->d_tab) (void)hipFree(h->d_tab);
  delete h;
  return RONK_OK;
}

extern "C" int ronk_poseidon_permute_dev(const ronk_poseidon* h, uint64_t* d_states, size_t count, void* stream) {
  if (!h || (!d_states && count)) return RONK_ERR_INVALID;
  if (!count) return RONK_OK;
  POS_DISPATCH(h, hipLaunchKernelGGL((poseidon_permute_kernel<FLD, W>), dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream,
                                     h->nat, h->width, d_states, (u64)count));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_poseidon_hash(const ronk_poseidon* h, const uint64_t* in, size_t len, uint64_t* out_state) {
  if (!h || !out_state || (!in && len)) return RONK_ERR_INVALID;
  if (len > h->width) return RONK_ERR_INDEX;   // the reference's `width - state.len()` underflows
  RCHK(need_device());
  std::vector<u64> st(h->width, 0);
  for (size_t i = 0; i < len; i++) st[i] = in[i];
  HostCall hc;
  u64* d = hc.in(st.data(), h->width);
  RCHK(hc.rc);
  RCHK(ronk_poseidon_permute_dev(h, d, 1, nullptr));
  return hc.get(out_state, d, h->width * 8);
}

extern "C" int ronk_poseidon_sponge_dev(const ronk_poseidon* h, const uint64_t* d_in, size_t n_items, size_t len, size_t item_stride,
                                        size_t elem_stride, uint64_t* d_out, size_t n_out, void* stream) {
  if (!h || (!d_in && len && n_items) || (!d_out && n_out && n_items)) return RONK_ERR_INVALID;
  if (!n_items || !n_out) return RONK_OK;
  POS_DISPATCH(h, hipLaunchKernelGGL((poseidon_sponge_kernel<FLD, W>), dim3(grid_for(n_items)), dim3(256), 0, (hipStream_t)stream, h->sp,
                                     d_in, (u64)n_items, (u64)len, (u64)item_stride, (u64)elem_stride, d_out, (u64)n_out));
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- Merkle tree
extern "C" size_t ronk_merkle_tree_words(size_t n_leaves, size_t digest_len) {
  if (!n_leaves) return 0;
  return (size_t)merkle_level_offset(n_leaves, digest_len, merkle_levels(n_leaves));
}
extern "C" size_t ronk_merkle_level_offset(size_t n_leaves, size_t digest_len, size_t level) {
  if (!n_leaves) return 0;
  const u64 top = merkle_levels(n_leaves);
  return (size_t)merkle_level_offset(n_leaves, digest_len, level < top ? level : top);
}

// The leaf level is a sponge launch; a level of more than 256 nodes is one launch with a lane per parent node; the last
// (up to 8) levels, which fit one workgroup's LDS, finish in ONE launch.  (Climbing 8 levels inside every workgroup of the
// leaf launch measured slower: the steps are serial permutations on a shrinking number of lanes)
extern "C" int ronk_merkle_commit_dev(const ronk_poseidon* h, const uint64_t* d_leaves, size_t n_leaves, size_t leaf_len,
                                      size_t item_stride, size_t elem_stride, size_t digest_len, uint64_t* d_tree, void* stream) {
  if (!h || !d_tree || (!d_leaves && leaf_len) || !n_leaves || !digest_len || digest_len > h->rate) return RONK_ERR_INVALID;
  const hipStream_t s = (hipStream_t)stream;
  const u32 d = (u32)digest_len;
  const u64 top = merkle_levels(n_leaves) - 1;   // the root's level
  RCHK(ronk_poseidon_sponge_dev(h, d_leaves, n_leaves, leaf_len, item_stride, elem_stride, d_tree, digest_len, stream));
  u64 lvl = 0, n_lvl = n_leaves, off = 0;
  while (n_lvl > MERKLE_BLOCK) {
    const u64 cn = (n_lvl + 1) / 2;
    POS_DISPATCH(h, hipLaunchKernelGGL((merkle_level_kernel<FLD, W>), dim3(grid_for(cn)), dim3(256), 0, s, h->sp, d_tree + off, n_lvl, d,
                                       d_tree + off + n_lvl * d));
    HIPCHK(hipGetLastError());
    off += n_lvl * d;
    n_lvl = cn;
    lvl++;
  }
  if (lvl < top) {
    const size_t lds = (size_t)(MERKLE_BLOCK + MERKLE_BLOCK / 2) * d * 8;
    POS_DISPATCH(h, HIPCHK((launch_dyn<merkle_node_kernel<FLD, W>>(dim3(1), dim3(MERKLE_BLOCK), lds, s, h->sp, d_tree, off, n_lvl, d,
                                                                   (u32)(top - lvl)))));
  }
  return RONK_OK;
}

extern "C" int ronk_merkle_open_dev(const uint64_t* d_tree, size_t n_leaves, size_t digest_len, const uint64_t* d_indices, size_t n_idx,
                                    uint64_t* d_paths, int* d_status, void* stream) {
  if (!d_tree || !n_leaves || !digest_len || ((!d_indices || !d_status) && n_idx)) return RONK_ERR_INVALID;
  if (!d_paths && n_idx && n_leaves > 1) return RONK_ERR_INVALID;
  if (!n_idx) return RONK_OK;
  hipLaunchKernelGGL(merkle_open_kernel, dim3(grid_for(n_idx)), dim3(256), 0, (hipStream_t)stream, d_tree, (u64)n_leaves, (u64)digest_len,
                     d_indices, (u64)n_idx, d_paths, d_status);
  HIPCHK(hipGetLastError());
  return RONK_OK;
}

extern "C" int ronk_merkle_verify_dev(const ronk_poseidon* h, const uint64_t* d_leaves, size_t n_idx, size_t leaf_len, size_t item_stride,
                                      size_t elem_stride, const uint64_t* d_indices, const uint64_t* d_paths, size_t n_leaves,
                                      size_t digest_len, const uint64_t* d_root, int* d_ok, void* stream) {
  if (!h || !d_root || !n_leaves || !digest_len || digest_len > h->rate) return RONK_ERR_INVALID;
  if (n_idx && ((!d_leaves && leaf_len) || !d_indices || !d_ok || (!d_paths && n_leaves > 1))) return RONK_ERR_INVALID;
  if (!n_idx) return RONK_OK;
  const u32 d = (u32)digest_len;
  POS_DISPATCH(h, HIPCHK((launch_dyn<merkle_verify_kernel<FLD, W>>(dim3(grid_for(n_idx)), dim3(256), (size_t)256 * 3 * d * 8, (hipStream_t)stream,
                                                                   h->sp, d_leaves, (u64)n_idx, (u64)leaf_len, (u64)item_stride,
                                                                   (u64)elem_stride, d_indices, d_paths, (u64)n_leaves, d, d_root, d_ok))));
  return RONK_OK;
}

// ------------------------------------------------------------------------------------- host-pointer forms
extern "C" int ronk_merkle_commit(const ronk_poseidon* h, const uint64_t* leaves, size_t n_leaves, size_t leaf_len, size_t digest_len,
                                  uint64_t* tree) {
  if (!h || !tree || (!leaves && leaf_len) || !n_leaves || !digest_len || digest_len > h->rate) return RONK_ERR_INVALID;
  RCHK(need_device());
  const size_t words = ronk_merkle_tree_words(n_leaves, digest_len);
  HostCall hc;
  const u64* dl = hc.in(leaves, n_leaves * leaf_len);   // (NULL for empty leaves)
  u64* dt = hc.out(words);
  RCHK(hc.rc);
  RCHK(ronk_merkle_commit_dev(h, dl, n_leaves, leaf_len, leaf_len, 1, digest_len, dt, nullptr));
  return hc.get(tree, dt, words * 8);
}

extern "C" int ronk_merkle_open(const uint64_t* tree, size_t n_leaves, size_t digest_len, const uint64_t* indices, size_t n_idx,
                                uint64_t* paths, int* status) {
  if (!tree || !n_leaves || !digest_len || ((!indices || !status) && n_idx)) return RONK_ERR_INVALID;
  if (!paths && n_idx && n_leaves > 1) return RONK_ERR_INVALID;
  // host integer logic on a host tree (the same body as the device kernel): no device work
  const u64 depth = merkle_levels(n_leaves) - 1;
  u64 dummy = 0;
  for (size_t q = 0; q < n_idx; q++)
    status[q] = merkle_open_one(tree, n_leaves, digest_len, indices[q], paths ? paths + q * depth * digest_len : &dummy) ? RONK_ERR_INDEX : 0;
  return RONK_OK;
}

extern "C" int ronk_merkle_verify(const ronk_poseidon* h, const uint64_t* leaves, size_t n_idx, size_t leaf_len, const uint64_t* indices,
                                  const uint64_t* paths, size_t n_leaves, size_t digest_len, const uint64_t* root, int* ok) {
  if (!h || !root || !n_leaves || !digest_len || digest_len > h->rate) return RONK_ERR_INVALID;
  if (n_idx && ((!leaves && leaf_len) || !indices || !ok || (!paths && n_leaves > 1))) return RONK_ERR_INVALID;
  RCHK(need_device());
  if (!n_idx) return RONK_OK;
  const size_t depth = merkle_levels(n_leaves) - 1;
  HostCall hc;   // leaves (empty leaves) and paths (a one-leaf tree) may be NULL
  const u64 *dl = hc.in(leaves, n_idx * leaf_len), *di = hc.in(indices, n_idx), *dp = hc.in(paths, n_idx * depth * digest_len);
  const u64* dr = hc.in(root, digest_len);
  int* dk = (int*)hc.out((n_idx + 1) / 2);   // int ok[n_idx]
  RCHK(hc.rc);
  RCHK(ronk_merkle_verify_dev(h, dl, n_idx, leaf_len, leaf_len, 1, di, dp, n_leaves, digest_len, dr, dk, nullptr));
  return hc.get(ok, dk, n_idx * 4);
}
