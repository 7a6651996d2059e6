// plonk_handle.h -- what a ronk_plonk handle owns (ronk_plonk_create, csrc/ronk_plonk.hip): shared by the quotient kernels that
// run on its domain, the PLONK quotient (ronk_plonk.hip), the logUp quotient (ronk_lookup.hip) and the constraint programs
// (ronk_air.hip).  Not part of the C ABI.
#pragma once
#include "runtime.h"
#include "ext2_launch.h"
#include "plonk_kernels.h"

struct ronk_plonk {
  u64 p = 0;
  u64 g = 0, w = 0, s = 0; // plain: the generator (mod p), W and the coset shift, for the host-side users of the domain (ronk_air.hip)
  u32 log2m = 0;
  Ext2Launch c;            // the field policy, its constants, W
  DeepDomain dm{};
  PlonkTab tab{};
  u64* d_dom = nullptr;    // lo, hi of the domain
  u64* d_vinv = nullptr;   // the B inverses of the vanishing polynomial
};
