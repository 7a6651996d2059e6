// ext2_launch.h -- what a host-side launch of the field-policy family FriGl / FriGlW7 / FriMont (csrc/fri_kernels.h) knows, and the
// two forms that bind FF to the policy.  Shared by ronk_ext2.hip, ronk_accum.hip, ronk_plonk.hip,
// ronk_mpcs.hip (and through it ronk_pcs.hip) and ronk_fri.hip; not part of the C ABI.
#pragma once
#include "runtime.h"
#include "ext2_kernels.h"

// the policy (Montgomery, or Goldilocks arithmetic with its W = 7 form), its constants and W in register form (0: a base-field call)
struct Ext2Launch {
  bool mont = false, w7 = false;
  FriConsts k{};
  u64 w = 0;
};
// FRI chooses the policy and its constants by its own rule (fri_gl_shift_roots, fri_host_consts) ...
static inline Ext2Launch ext2_launch(bool mont, const FriConsts& k, u64 p, u64 w) {
  Ext2Launch c;
  c.mont = mont;
  c.w7 = !mont && w % p == 7;
  c.k = k;
  c.w = ext2_reg_form(mont, p, w);
  return c;
}
// ... every other caller takes the field's: Goldilocks arithmetic for Goldilocks, Montgomery for any other prime
static inline Ext2Launch ext2_launch(u64 p, u64 w) {
  const bool mont = p != RONK_GOLDILOCKS_P;
  return ext2_launch(mont, ext2_host_consts(mont, p), p, w);
}

// run the statement with FF bound to the policy of the context: the kernels that have a W = 7 body ...
#define EXT2_DISPATCH3(c, ...)                              \
  do {                                                      \
    if ((c).mont) { typedef FriMont FF; __VA_ARGS__; }      \
    else if ((c).w7) { typedef FriGlW7 FF; __VA_ARGS__; }   \
    else { typedef FriGl FF; __VA_ARGS__; }                 \
  } while (0)
// ... and those instantiated for the two base policies only (W = 7 runs the FriGl body)
#define EXT2_DISPATCH2(c, ...)                              \
  do {                                                      \
    if ((c).mont) { typedef FriMont FF; __VA_ARGS__; }      \
    else { typedef FriGl FF; __VA_ARGS__; }                 \
  } while (0)
