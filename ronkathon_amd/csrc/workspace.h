// workspace.h -- the event-guarded workspace pool (ronk_workspace.hip) as every translation unit sees it: a lease object, the
// helper that carves one lease into consecutive spans, and the capture predicate the pool and its users share.
#pragma once
#include "runtime.h"

// is `s` capturing into a hipGraph?  A failed query clears the error and counts as "not capturing".
bool stream_capturing(hipStream_t s);

// A lease of at least `bytes`, asynchronous on the stream it was acquired on; the destructor releases it once the work that uses
// it has been queued (an event behind that work when the pool is used from more than one stream).
struct WsSlot;
struct WsLease {
  WsSlot* slot = nullptr;
  hipStream_t s = nullptr;
  ~WsLease();
  int acquire(size_t bytes, hipStream_t st);
  u64* u() const;
  u32* ctl() const;   // 64 bytes of control words, ZERO whenever the slot is not in use (fused scan kernels)
  // look-back arrays of a one-launch scan: *cur is all LB_EMPTY now, *next is cleared by the kernel for the call after
  // The parity advances only through lb_commit(), AFTER the launch was accepted: a failed launch never ran the kernel that
  // clears *next, so the same (still clean) *cur must serve the following call.
  void lb_arrays(u64** cur, u64** next);
  void lb_commit();
};

// consecutive spans of one lease: Carve c{ws.u()}; u64 *a = c.take(n_a), *b = c.take(n_b);
struct Carve {
  u64* cur;
  u64* take(size_t words) { u64* q = cur; cur += words; return q; }
};
