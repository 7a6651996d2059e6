// poseidon_handle.h -- the ronk_poseidon handle and its field / width dispatch, shared by the translation units that launch
// the Poseidon bodies (ronk_hash.hip, ronk_fri.hip).  Not part of the C ABI.
#pragma once
#include "runtime.h"
#include "poseidon_kernels.h"

// ------------------------------------------------------------------------------------- handle
struct ronk_poseidon {
  u64 p;
  u32 width, W, rate, num_p, num_f;
  u64 alpha;
  u64* d_tab = nullptr;         // rc natural, mds natural, rc sponge-ordered, mds sponge-ordered (one allocation)
  PoseidonConsts nat{}, sp{};   // constants in natural order (permute) and in the sponge's layout
};

#define POS_DISPATCH_W(F, Wv, ...)                          \
  do {                                                      \
    if ((Wv) == 4) { constexpr int W = 4; typedef F FLD; __VA_ARGS__; }        \
    else if ((Wv) == 8) { constexpr int W = 8; typedef F FLD; __VA_ARGS__; }   \
    else if ((Wv) == 12) { constexpr int W = 12; typedef F FLD; __VA_ARGS__; } \
    else { constexpr int W = 16; typedef F FLD; __VA_ARGS__; }                 \
  } while (0)
// run the statement with FLD and W bound to the handle's field and register width
#define POS_DISPATCH(h, ...)                                          \
  do {                                                                \
    if ((h)->p == RONK_GOLDILOCKS_P) POS_DISPATCH_W(PosGl, (h)->W, __VA_ARGS__); \
    else POS_DISPATCH_W(PosMont, (h)->W, __VA_ARGS__);                \
  } while (0)
