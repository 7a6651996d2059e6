// roots_host.h -- the host side of the product tree shared by ronk_recover.hip (which owns it) and ronk_multipoint.hip: the
// field dispatch of the tree's kernels, the library-owned level plans with their pins, and the tree itself.
#pragma once
#include "workspace.h"
#include "roots_kernels.h"

FieldConst roots_consts(u64 p);
#define ROOTS_DISPATCH(fc, ...)                        \
  do {                                                 \
    if ((fc).p == 0) { GlField f; __VA_ARGS__; }       \
    else { MontField f(fc); __VA_ARGS__; }             \
  } while (0)

// One batched plan per level shape (2d points, count / 2 rows), owned by the library: a second call of the same shape builds
// no twiddle tables.  Every call holds g_roots_mu from its first lookup to its last launch, and pins what it uses; eviction
// (least recently used, unpinned, beyond the cache's size) waits for the entry's last work first.
struct RootsPlan {
  ronk_plan* pl = nullptr;
  u64 p, g, batch;
  u32 log2n;
  int device;
  hipEvent_t done = nullptr;
  bool used = false;
  u64 stamp = 0;
  int pins = 0;
};
extern std::mutex g_roots_mu;
// g_roots_mu held
// tiled: the plan must run on the tile kernels (the tree's fused product, TileArgs::in2); otherwise RONK_ERR_UNSUPPORTED
int roots_plan_get(u64 p, u64 g, u32 log2n, u64 batch, bool tiled, RootsPlan** out);
// the pins of one call: released (an event behind the call's work on `s`) when the call returns
struct RootsPins {
  std::vector<RootsPlan*> held;
  hipStream_t s = nullptr;
  ~RootsPins() {
    for (RootsPlan* e : held) {
      e->used = hipEventRecord(e->done, s) == hipSuccess;
      if (!e->used) (void)hipGetLastError();
      e->pins--;
    }
  }
  int get(u64 p, u64 g, u32 log2n, u64 batch, bool tiled, ronk_plan** pl) {
    RootsPlan* e = nullptr;
    RCHK(roots_plan_get(p, g, log2n, batch, tiled, &e));
    held.push_back(e);
    *pl = e->pl;
    return RONK_OK;
  }
};

// what a tree leaves behind for the walks of ronk_multipoint.hip (roots_tree)
struct RootsKeep {
  u64* leaves;       // 2M words
  u64* transforms;   // levels * 2M words
};

u32 roots_leaf();
size_t roots_padded(size_t m, u32 G);
size_t roots_ws_words(size_t m, u32 G);
int roots_field(u64 p, size_t m, u64* gtree);
int roots_tree(const FieldConst& fc, u64 p, u64 gtree, const u64* d_roots, size_t m, u64* d_out, u64* ws, RootsPins& pins,
               hipStream_t s, const RootsKeep* keep);
