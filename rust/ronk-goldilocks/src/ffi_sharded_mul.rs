//! `extern "C"` items of the sharded polynomial multiply (include/ronk_ntt.h, `ronk_sharded_mul_*` / `ronk_poly_mul_sharded*`).
//!
//! Kept beside `ffi.rs` rather than in it: the engine repository's header check (tests/test_cpp_host_mirror.py) maps every
//! parameter type of `ffi.rs` through a fixed table that has no entry for this plan's handle.  Same conventions: 0 or a negative
//! `RONK_ERR_*`, turned into the reference's panic by [`crate::ffi::check`].
use core::ffi::c_int;

/// `ronk_sharded_mul_plan` (opaque)
#[repr(C)]
pub struct RonkShardedMulPlan {
  _private: [u8; 0],
}
/// `RONK_SHARDED_MUL_UNFUSED`: the composed middle (forward phase 2 writes both spectra, the inverse multiplies them on load)
pub const SHARDED_MUL_UNFUSED: c_int = 1;
/// `RONK_SHARDED_MUL_FUSED`: the fused middle wherever an instantiation matches (default: only where it measured faster)
pub const SHARDED_MUL_FUSED: c_int = 2;

extern "C" {
  pub fn ronk_sharded_mul_plan_create_p(
    out: *mut *mut RonkShardedMulPlan, p: u64, g: u64, log2n: u32, devices: *const c_int, ndev: c_int, chunks: c_int,
    exchange: c_int, flags: c_int,
  ) -> c_int;
  pub fn ronk_sharded_mul_plan_create(
    out: *mut *mut RonkShardedMulPlan, log2n: u32, devices: *const c_int, ndev: c_int, chunks: c_int, exchange: c_int,
    flags: c_int,
  ) -> c_int;
  pub fn ronk_sharded_mul_plan_info(
    plan: *const RonkShardedMulPlan, rows: *mut u64, cols: *mut u64, per_rank: *mut u64, chunks: *mut c_int,
    fused_middle: *mut c_int,
  ) -> c_int;
  pub fn ronk_sharded_mul_plan_destroy(plan: *mut RonkShardedMulPlan) -> c_int;
  pub fn ronk_poly_mul_sharded_dev(
    plan: *mut RonkShardedMulPlan, d_a: *const *const u64, d_b: *const *const u64, d_out: *const *mut u64,
  ) -> c_int;
  pub fn ronk_sharded_mul_sync(plan: *mut RonkShardedMulPlan) -> c_int;
  pub fn ronk_poly_mul_sharded(
    plan: *mut RonkShardedMulPlan, a: *const u64, d: usize, b: *const u64, d2: usize, out: *mut u64,
  ) -> c_int;
}
