//! Poseidon and a Merkle tree over its sponge for Goldilocks: the shapes of ronkathon's `src/hashes/poseidon` and
//! `src/tree/merkle.rs`, bound to the GPU.
//!
//! The reference's `Poseidon<F>` / `PoseidonSponge<F, _>` are generic over `F: Field` with caller-supplied constants
//! (hashes/poseidon/mod.rs:56-149, sponge.rs:69-275); its `MerkleTree` hashes strings with SHA-256 (tree/merkle.rs:31-99).
//! Here the tree's hash is the sponge, a leaf is a slice of field elements, and a digest is `digest_len` elements.
//!
//! * [`Poseidon::hash`]          = `Poseidon::hash` (pad with ZERO, permute, `state[1]`)            -> `ronk_poseidon_hash`
//! * [`Poseidon::sponge`]        = absorb one slice, squeeze `n_out`                                -> `ronk_poseidon_sponge_dev`
//! * [`MerkleTree::new`]         = `MerkleTree::new`                                                -> `ronk_merkle_commit`
//! * [`MerkleTree::get_proof`]   = `get_proof` (panics where the reference indexes out of bounds)   -> `ronk_merkle_open`
//! * [`MerkleTree::prove`]       = `prove`                                                          -> `ronk_merkle_verify`
//!
//! The library ships no parameter set: whether (width, alpha, rounds, matrix) is secure for the field is the caller's concern.
use core::ffi::c_int;
use std::ptr;

use crate::{
  ffi::{check, ronk_dev_alloc, ronk_dev_free, ronk_memcpy_d2h, ronk_memcpy_h2d, P},
  ffi_hashes as ffi,
  field::Goldilocks,
};

/// One parameter set on the current device.
pub struct Poseidon {
  h:         *mut ffi::RonkPoseidon,
  pub width: usize,
  pub rate:  usize,
}

impl Poseidon {
  /// `Poseidon::new(width, alpha, num_p, num_f, rc, mds)` plus the sponge's rate; `mds` row-major.
  pub fn new(width: usize, alpha: usize, num_p: usize, num_f: usize, rate: usize, rc: &[Goldilocks], mds: &[Goldilocks]) -> Self {
    assert!(rc.len() == (num_p + num_f) * width && mds.len() == width * width, "constants do not match the width");
    let mut h = ptr::null_mut();
    check(unsafe {
      ffi::ronk_poseidon_create(&mut h, P, width as u32, alpha as u64, num_p as u32, num_f as u32, rate as u32,
                                rc.as_ptr() as *const u64, mds.as_ptr() as *const u64)
    });
    Poseidon { h, width, rate }
  }

  pub fn raw(&self) -> *const ffi::RonkPoseidon { self.h }

  /// mod.rs:131-149
  pub fn hash(&self, state: &[Goldilocks]) -> Goldilocks {
    let mut out = vec![0u64; self.width];
    check(unsafe { ffi::ronk_poseidon_hash(self.h, state.as_ptr() as *const u64, state.len(), out.as_mut_ptr()) });
    Goldilocks(out[1])
  }

  /// absorb `input` in one call, squeeze `n_out` (sponge.rs:110-275)
  pub fn sponge(&self, input: &[Goldilocks], n_out: usize) -> Vec<Goldilocks> {
    let mut out = vec![0u64; n_out];
    if n_out == 0 {
      return vec![];
    }
    let (mut d_in, mut d_out) = (ptr::null_mut(), ptr::null_mut());
    unsafe {
      check(ronk_dev_alloc(&mut d_in, (input.len() * 8).max(8)));
      check(ronk_dev_alloc(&mut d_out, n_out * 8));
      check(ronk_memcpy_h2d(d_in, input.as_ptr() as *const _, input.len() * 8));
      let rc = ffi::ronk_poseidon_sponge_dev(self.h, d_in as *const u64, 1, input.len(), input.len(), 1, d_out as *mut u64, n_out,
                                             ptr::null_mut());
      let rc2 = if rc == 0 { ronk_memcpy_d2h(out.as_mut_ptr() as *mut _, d_out, n_out * 8) } else { rc };
      ronk_dev_free(d_in);
      ronk_dev_free(d_out);
      check(rc2);
    }
    out.into_iter().map(Goldilocks).collect()
  }
}

impl Drop for Poseidon {
  fn drop(&mut self) { unsafe { ffi::ronk_poseidon_destroy(self.h) }; }
}

/// merkle.rs:11-15 (`LeftOrRight`)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum LeftOrRight {
  Left,
  Right,
}

/// merkle.rs:25-26: sibling digests from the bottom up
#[derive(Debug, Clone)]
pub struct Proof(pub Vec<(Vec<Goldilocks>, LeftOrRight)>);

/// merkle.rs:17-22, every level kept: leaves first, the root last (`ronk_merkle_level_offset`)
pub struct MerkleTree<'a> {
  hasher:         &'a Poseidon,
  pub n_leaves:   usize,
  pub digest_len: usize,
  pub tree:       Vec<u64>,
}

impl<'a> MerkleTree<'a> {
  /// `leaves`: n_leaves x leaf_len, row-major
  pub fn new(hasher: &'a Poseidon, leaves: &[Goldilocks], leaf_len: usize, digest_len: usize) -> Self {
    assert!(leaf_len > 0 && leaves.len() % leaf_len == 0 && !leaves.is_empty(), "a tree has at least one leaf");
    let n_leaves = leaves.len() / leaf_len;
    let mut tree = vec![0u64; unsafe { ffi::ronk_merkle_tree_words(n_leaves, digest_len) }];
    check(unsafe { ffi::ronk_merkle_commit(hasher.h, leaves.as_ptr() as *const u64, n_leaves, leaf_len, digest_len, tree.as_mut_ptr()) });
    MerkleTree { hasher, n_leaves, digest_len, tree }
  }

  pub fn depth(&self) -> usize {
    let mut d = 0;
    while unsafe { ffi::ronk_merkle_level_offset(self.n_leaves, self.digest_len, d + 1) } < self.tree.len() {
      d += 1;
    }
    d
  }

  pub fn root_hash(&self) -> Vec<Goldilocks> { self.tree[self.tree.len() - self.digest_len..].iter().map(|&v| Goldilocks(v)).collect() }

  /// Panics like the reference for an index out of range and for the unpaired last node of an odd level.
  pub fn get_proof(&self, leaf_index: usize) -> Proof {
    let depth = self.depth();
    let mut path = vec![0u64; (depth * self.digest_len).max(1)];
    let (idx, mut status) = (leaf_index as u64, 0 as c_int);
    check(unsafe { ffi::ronk_merkle_open(self.tree.as_ptr(), self.n_leaves, self.digest_len, &idx, 1, path.as_mut_ptr(), &mut status) });
    check(status);
    Proof(
      (0..depth)
        .map(|l| {
          let sib = path[l * self.digest_len..(l + 1) * self.digest_len].iter().map(|&v| Goldilocks(v)).collect();
          (sib, if (leaf_index >> l) & 1 == 1 { LeftOrRight::Left } else { LeftOrRight::Right })
        })
        .collect(),
    )
  }

  pub fn prove(&self, leaf: &[Goldilocks], proof: &Proof) -> bool {
    if proof.0.len() != self.depth() || proof.0.iter().any(|(s, _)| s.len() != self.digest_len) {
      return false;
    }
    let idx: u64 = proof.0.iter().enumerate().map(|(l, (_, side))| if *side == LeftOrRight::Left { 1u64 << l } else { 0 }).sum();
    let mut path: Vec<u64> = proof.0.iter().flat_map(|(s, _)| s.iter().map(|g| g.0)).collect();
    if path.is_empty() {
      path.push(0);
    }
    let root = &self.tree[self.tree.len() - self.digest_len..];
    let mut ok: c_int = 0;
    check(unsafe {
      ffi::ronk_merkle_verify(self.hasher.h, leaf.as_ptr() as *const u64, 1, leaf.len(), &idx, path.as_ptr(), self.n_leaves,
                              self.digest_len, root.as_ptr(), &mut ok)
    });
    ok == 1
  }
}
