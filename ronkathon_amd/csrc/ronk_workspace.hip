// ronk_workspace.hip -- the event-guarded workspace pool of libronk_ntt.so (workspace.h): the temporaries of the scan, division,
// decode, product-tree and BN254 product entry points.  Host code only.
#include "workspace.h"
#include "scan_kernels.h"

bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}

// hipMalloc'd buffers, each guarded by a completion event, so a call never synchronises the device and never frees memory
// that queued work still uses.  A slot is reused when its last work has completed or was queued on the same stream (stream
// order then protects it).  (hipMallocAsync / hipFreeAsync were tried first and dropped: on ROCm 7.2 / gfx950 a kernel
// intermittently read stale data from a pool block reused across calls -- 4 of 12 test runs -- while plain allocations never
// did.)
struct WsSlot {
  void* p = nullptr;
  u32* ctl = nullptr;   // 64 bytes of control words, ZERO whenever the slot is not in use (fused scan kernels)
  u64* lb = nullptr;    // two look-back arrays of LB_WORDS entries (scan_kernels.h, one-launch forms): the one a call uses
  u32 lb_calls = 0;     // was set to LB_EMPTY by the call before it (at creation: both), parity = lb_calls & 1
  size_t bytes = 0;
  int device = -1;
  hipEvent_t done = nullptr;
  hipStream_t last = nullptr;
  bool used = false;   // ever had work queued
  bool busy = false;   // leased right now
  bool ev_valid = false;   // `done` was recorded behind the slot's last work
  bool oneoff = false;     // larger than WS_CACHE_MAX: never pooled, freed once its work has completed
};
static std::mutex g_ws_mu;
static std::vector<WsSlot*> g_ws;
// Retention bound: the pool keeps what the scans, the decode and ordinary divisions need (64 KiB .. 256 MiB per slot, a power
// of two each).  Anything larger -- the ~10 x Lp x 8 bytes of a 2^27 Newton division, 16 GiB after rounding -- is a ONE-OFF
// allocation of exactly the requested size: on release it goes to g_ws_grave with an event behind its last work and is freed
// by the next acquire / ronk_trim_workspace() that finds the event complete (never while queued work still uses it).
static constexpr size_t WS_CACHE_MAX = (size_t)256 << 20;
static std::vector<WsSlot*> g_ws_grave;
static void ws_free_slot(WsSlot* w) {
  if (w->p) (void)hipFree(w->p);
  if (w->ctl) (void)hipFree(w->ctl);
  if (w->lb) (void)hipFree(w->lb);
  if (w->done) (void)hipEventDestroy(w->done);
  delete w;
}
// g_ws_mu held.  wait = false: free what has completed; true: wait for the rest (ronk_trim_workspace).
static void ws_reap(bool wait) {
  for (size_t i = 0; i < g_ws_grave.size();) {
    WsSlot* w = g_ws_grave[i];
    bool done = !w->ev_valid || hipEventQuery(w->done) == hipSuccess;
    if (!done && wait) done = hipEventSynchronize(w->done) == hipSuccess;
    if (!done) { (void)hipGetLastError(); i++; continue; }
    ws_free_slot(w);
    g_ws_grave[i] = g_ws_grave.back();
    g_ws_grave.pop_back();
  }
}
// Completion events are recorded only once the pool has been seen from a second stream: while every call comes from ONE
// stream, stream order protects a reused slot and the hipEventRecord per call (~1.5 us of the 12.5 us an evaluate of 2^22
// coefficients takes end to end) buys nothing.  The stream that triggers the switch simply gets a fresh slot.
static bool g_ws_multi = false;

WsLease::~WsLease() {
  if (!slot) return;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (slot->oneoff) {   // never pooled: an event behind its work, freed by whoever finds it complete
    // A capturing stream: an event recorded inside a capture never completes for hipEventQuery / hipEventSynchronize, so the
    // buffer would sit in the grave for ever (through ronk_trim_workspace as well).  A captured graph may be replayed long
    // after this call returned, so its one-off workspace cannot be freed at all while the graph lives: acquire() refuses
    // one-off workspaces under capture (RONK_ERR_UNSUPPORTED); should one get here regardless, it is kept, not leaked
    // silently: the grave entry has no event and is freed by the next reap.
    if (stream_capturing(s)) {
      slot->ev_valid = false;
    } else {
      slot->ev_valid = hipEventRecord(slot->done, s) == hipSuccess;
      if (!slot->ev_valid) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); }
    }
    slot->busy = false;
    g_ws_grave.push_back(slot);
    ws_reap(false);
    return;
  }
  // (a capturing stream leaves no event: one recorded inside a capture never completes for the pool's queries; the slot stays
  //  tied to the stream it was last used on -- the captured graph's stream -- and other streams wait for the device instead)
  slot->ev_valid = !stream_capturing(s) && g_ws_multi && hipEventRecord(slot->done, s) == hipSuccess;
  slot->last = s; slot->used = true; slot->busy = false;
}

int WsLease::acquire(size_t bytes, hipStream_t st) {
  s = st;
  size_t need = 65536;
  while (need < bytes) need <<= 1;
  const bool oneoff = need > WS_CACHE_MAX;
  if (oneoff) need = (bytes + 255) & ~(size_t)255;   // exactly what was asked for, not the next power of two
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  // (see ~WsLease: a captured graph would use the buffer after it has been freed)
  if (oneoff && stream_capturing(st)) return RONK_ERR_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  ws_reap(false);
  size_t on_dev = 0;
  WsSlot* waitable = nullptr;
  for (WsSlot* w : g_ws) {
    if (oneoff) break;
    if (w->device != dev) continue;
    on_dev++;
    if (w->busy || w->bytes < need) continue;
    if (!w->used || w->last == st || (w->ev_valid && hipEventQuery(w->done) == hipSuccess)) { slot = w; break; }
    g_ws_multi = true;                        // a slot last used by ANOTHER stream: from now on every release leaves an event
    if (!waitable) waitable = w;
  }
  if (!slot && waitable && on_dev >= 32) {  // bound the pool: wait for an old slot instead of growing
    // A slot released before the pool went multi-stream has no event, and its stream handle cannot be trusted any more (a
    // destroyed hipStream_t crashes hipEventRecord / hipStreamSynchronize -- tests/test_gpu_parity.py destroys one on
    // purpose), so the one thing left to wait on is the device: the slot's device IS the current one (filter above).
    // At most once per process and device: from the switch on every release records its event.
    if (waitable->ev_valid) (void)hipEventSynchronize(waitable->done);
    else (void)hipDeviceSynchronize();
    slot = waitable;
  }
  if (!slot) {
    // A capturing stream may not be handed a FRESH slot: creating one needs hipMalloc and the look-back fills, which either
    // invalidate a global-mode capture (legacy null-stream calls) or would become nodes of the caller's graph.  The caller
    // warms the pool with one call of the same shape outside the capture (include/ronk_ntt.h); until then the captured call
    // is refused, never half-initialised.
    if (stream_capturing(st)) {
      (void)hip_fail(hipErrorStreamCaptureUnsupported, "workspace: no warm pool slot for a capturing stream (call once outside the capture first)");
      return RONK_ERR_UNSUPPORTED;
    }
    WsSlot* w = new WsSlot();
    w->oneoff = oneoff;
    hipError_t e = hipMalloc(&w->p, need);
    if (e == hipErrorOutOfMemory && !g_ws_grave.empty()) {
      // two back-to-back large divisions on one stream: the first one's one-off buffer (gigabytes) is still in the grave
      // behind its event -- wait for the grave instead of reporting out-of-memory, then try once more
      (void)hipGetLastError();
      ws_reap(true);
      e = hipMalloc(&w->p, need);
    }
    // The initial fills are ordered on the ACQUIRING stream: hipMemset runs on the null stream and returns before it has
    // executed, so a kernel launched right afterwards on a NON-BLOCKING stream could read the look-back arrays before they
    // were filled -- and take garbage for a published chunk sum (found by the four-thread fuzz sweep, round 5: one evaluate
    // in ~5 000 threaded cases, always on a caller-created stream and a fresh slot).  A later user on another stream gets
    // the slot only behind its completion event (or the device drain of the first cross-stream use), i.e. behind the fills.
    // (A capturing stream never gets here: refused above.)
    if (e == hipSuccess) e = hipMalloc((void**)&w->ctl, 64);
    if (e == hipSuccess) e = hipMemsetAsync(w->ctl, 0, 64, st);
    if (e == hipSuccess) e = hipMalloc((void**)&w->lb, (size_t)2 * LB_WORDS * 8);
    if (e == hipSuccess) e = hipMemsetAsync(w->lb, 0xFF, (size_t)2 * LB_WORDS * 8, st);   // LB_EMPTY everywhere
    if (e == hipSuccess) e = hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
    if (e != hipSuccess) { if (w->p) (void)hipFree(w->p); if (w->ctl) (void)hipFree(w->ctl); if (w->lb) (void)hipFree(w->lb); delete w; return hip_fail(e, "workspace"); }
    w->bytes = need; w->device = dev;
    if (!oneoff) g_ws.push_back(w);
    slot = w;
  }
  slot->busy = true;
  return RONK_OK;
}
u64* WsLease::u() const { return (u64*)slot->p; }
u32* WsLease::ctl() const { return slot->ctl; }
void WsLease::lb_arrays(u64** cur, u64** next) {
  const u32 par = slot->lb_calls & 1;
  *cur = slot->lb + (size_t)par * LB_WORDS;
  *next = slot->lb + (size_t)(par ^ 1) * LB_WORDS;
}
void WsLease::lb_commit() { slot->lb_calls++; }

// Releases every idle pool slot and every finished one-off buffer (include/ronk_ntt.h).  Waits for the work behind them
// (events; a slot released in single-stream mode has none: its device is synchronised).
extern "C" int ronk_trim_workspace(void) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  ws_reap(true);
  int cur = -1;
  (void)hipGetDevice(&cur);
  for (size_t i = 0; i < g_ws.size();) {
    WsSlot* w = g_ws[i];
    if (w->busy) { i++; continue; }
    (void)hipSetDevice(w->device);
    if (w->used) {   // (no event = released in single-stream mode; its stream handle may be gone: wait for the device)
      hipError_t e = w->ev_valid ? hipEventSynchronize(w->done) : hipDeviceSynchronize();
      if (e != hipSuccess) (void)hipGetLastError();
    }
    ws_free_slot(w);
    g_ws[i] = g_ws.back();
    g_ws.pop_back();
  }
  if (cur >= 0) (void)hipSetDevice(cur);
  return RONK_OK;
}
