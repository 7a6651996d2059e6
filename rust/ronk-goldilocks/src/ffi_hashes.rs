//! `extern "C"` items of Poseidon and the Merkle commitment (include/ronk_ntt.h, `ronk_poseidon_*` / `ronk_merkle_*`).
//!
//! Kept beside `ffi.rs` rather than in it, like `ffi_sharded_mul.rs`: the engine repository's header check
//! (tests/test_cpp_host_mirror.py) maps every parameter type of `ffi.rs` through a fixed table that has no entry for this handle,
//! and expects every item there to return `int`, which the two layout helpers do not.  Same conventions otherwise: 0 or a
//! negative `RONK_ERR_*`, turned into the reference's panic by [`crate::ffi::check`].
use core::ffi::{c_int, c_void};

/// `ronk_poseidon` (opaque): one Poseidon parameter set resident on a device
#[repr(C)]
pub struct RonkPoseidon {
  _private: [u8; 0],
}

extern "C" {
  // ---- Poseidon (hashes/poseidon/mod.rs:56-149, sponge.rs:69-275) and the Merkle tree over its sponge (tree/merkle.rs:31-99)
  pub fn ronk_poseidon_create(
    out: *mut *mut RonkPoseidon, p: u64, width: u32, alpha: u64, num_p: u32, num_f: u32, rate: u32, rc: *const u64, mds: *const u64,
  ) -> c_int;
  pub fn ronk_poseidon_destroy(h: *mut RonkPoseidon) -> c_int;
  pub fn ronk_poseidon_permute_dev(h: *const RonkPoseidon, d_states: *mut u64, count: usize, stream: *mut c_void) -> c_int;
  pub fn ronk_poseidon_hash(h: *const RonkPoseidon, input: *const u64, len: usize, out_state: *mut u64) -> c_int;
  /// element j of item i at `d_in[i * item_stride + j * elem_stride]`; `d_out`: n_items x n_out
  pub fn ronk_poseidon_sponge_dev(
    h: *const RonkPoseidon, d_in: *const u64, n_items: usize, len: usize, item_stride: usize, elem_stride: usize, d_out: *mut u64,
    n_out: usize, stream: *mut c_void,
  ) -> c_int;
  pub fn ronk_merkle_tree_words(n_leaves: usize, digest_len: usize) -> usize;
  pub fn ronk_merkle_level_offset(n_leaves: usize, digest_len: usize, level: usize) -> usize;
  pub fn ronk_merkle_commit_dev(
    h: *const RonkPoseidon, d_leaves: *const u64, n_leaves: usize, leaf_len: usize, item_stride: usize, elem_stride: usize,
    digest_len: usize, d_tree: *mut u64, stream: *mut c_void,
  ) -> c_int;
  pub fn ronk_merkle_open_dev(
    d_tree: *const u64, n_leaves: usize, digest_len: usize, d_indices: *const u64, n_idx: usize, d_paths: *mut u64,
    d_status: *mut c_int, stream: *mut c_void,
  ) -> c_int;
  pub fn ronk_merkle_verify_dev(
    h: *const RonkPoseidon, d_leaves: *const u64, n_idx: usize, leaf_len: usize, item_stride: usize, elem_stride: usize,
    d_indices: *const u64, d_paths: *const u64, n_leaves: usize, digest_len: usize, d_root: *const u64, d_ok: *mut c_int,
    stream: *mut c_void,
  ) -> c_int;
  pub fn ronk_merkle_commit(
    h: *const RonkPoseidon, leaves: *const u64, n_leaves: usize, leaf_len: usize, digest_len: usize, tree: *mut u64,
  ) -> c_int;
  pub fn ronk_merkle_open(
    tree: *const u64, n_leaves: usize, digest_len: usize, indices: *const u64, n_idx: usize, paths: *mut u64, status: *mut c_int,
  ) -> c_int;
  pub fn ronk_merkle_verify(
    h: *const RonkPoseidon, leaves: *const u64, n_idx: usize, leaf_len: usize, indices: *const u64, paths: *const u64,
    n_leaves: usize, digest_len: usize, root: *const u64, ok: *mut c_int,
  ) -> c_int;
}
