// rnt_api.cpp -- the extern "C" boundary (include/rnsntt.h) over the HIP
// kernels.  Every entry point validates like the reference (errors.rs:4-20
// order), turns every failure into a status code, and never lets a C++
// exception or HIP error escape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rnsntt.h"
#include "rnt_hostmath.hpp"
#include "rnt_internal.hpp"
#include "rnt_ws.hpp"

namespace {

thread_local std::string g_last_error;
// the RnsNttError fields of the last failure (rnt_last_error_detail)
struct ErrDetail {
  int status;
  uint64_t a, b;
};
thread_local ErrDetail g_last_detail{0, 0, 0};

int vfail(int code, uint64_t a, uint64_t b, const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof buf, fmt, ap);
  g_last_error = buf;
  g_last_detail = {code, a, b};
  return code;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(code, 0, 0, fmt, ap);
  va_end(ap);
  return code;
}

// A failure that carries the reference variant's fields (errors.rs:4-20).
int fail_fields(int code, uint64_t a, uint64_t b, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(code, a, b, fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* where) {
  (void)hipGetLastError();  // reported here: not pending for the next call
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
    return fail(RNT_ERR_OUT_OF_MEMORY, "%s: %s", where, hipGetErrorString(e));
  return fail(RNT_ERR_DEVICE, "%s: %s", where, hipGetErrorString(e));
}

#define HIP_TRY(expr, where)                  \
  do {                                        \
    hipError_t e_ = (expr);                   \
    if (e_ != hipSuccess) return hip_fail(e_, where); \
  } while (0)

inline size_t word_bytes(const rnt::Tables* t) { return t->wide ? 8 : 4; }

// An op sequence being recorded into a hipGraph on this thread
// (rnt_capture_begin .. rnt_capture_end): workspace blocks the captured ops
// take stay with the graph, whose replays reuse those exact addresses, and
// nothing that would synchronise the stream runs while recording.
// Only blocks handed back on the recording's own device and stream go to the
// graph (a block freed on another context while recording goes back to the
// cache as usual).  Call-scoped workspace (CallWs) handed back while
// recording is idle again for the next recorded op: `idle` blocks are taken
// before the cache is asked, so N recorded key-switch ops share one
// workspace (the recorded ops are ordered on the one captured stream), and
// the graph keeps the distinct blocks only.
struct OwnedBlock {
  void* p;
  size_t bytes;
  bool idle;
};
struct Capture {
  std::vector<OwnedBlock> owned;
  hipStream_t stream = nullptr;
  int device = 0;
};
thread_local Capture* g_capture = nullptr;

const char* const kKernelNames[rnt::K_COUNT] = {
    "col_fwd", "row_fwd", "row_inv", "row_mul", "col_inv", "elementwise", "rescale",
    "automorphism", "ks_decompose", "ks_rows", "tensor_rows", "import", "export", "crt",
    "sfft", "sample", "copy", "plane_fused", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv", "whole_mul", "ks_whole", "tensor_whole", "mf_tensor", "mf_mul",
    "bsgs_mac", "hoist_digits", "hoist_mac", "modup", "moddown", "moddown_auto",
    "moddown_rescale", "lincomb", "dot_tensor", "mod_raise", "mul_monomial",
    "moddown_rescale_affine", "dh_bsgs_mac", "dh_bsgs_fold", "rotsum_mac", "rotsum_c0", "automorph_ntt", "plain_mac"};

// A profiling call failed: clear the runtime's slot, keep the first failure
// in the profiler, and stop profiling (rnt_profile_read reports it).
void prof_fail(rnt::Prof* p, hipError_t e, const char* where) {
  (void)hipGetLastError();
  if (p->err == hipSuccess) {
    p->err = e;
    p->err_where = where;
  }
  p->on = false;
}
hipEvent_t prof_event(rnt::Prof* p) {
  if (!p->pool.empty()) {
    hipEvent_t e = p->pool.back();
    p->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (const hipError_t r = hipEventCreate(&e); r != hipSuccess) {
    prof_fail(p, r, "hipEventCreate(profile)");
    return nullptr;
  }
  return e;
}

// HIP errors are never dropped.  A cleanup call whose failure cannot abort
// the call making it (a block leaving the cache, a destructor, an event
// released) goes through cleanup(): the first such failure on the thread is
// kept with the call's name, and the runtime's last-error slot is cleared.
// The library then reports it as RNT_ERR_DEVICE, naming that call: from the
// entry point that made it when that one returns a status of its own
// (rnt_buf_free, rnt_ctx_destroy, rnt_graph_destroy, rnt_pool_trim), else
// from the next launch on the thread (check_pending).  A launcher reads
// hipGetLastError() after its launch, so an error some other code left in
// the slot would otherwise be blamed on the launch: check_pending reports it
// before launching, as pending from an earlier call, instead of clearing it.
struct Deferred {
  hipError_t e = hipSuccess;
  const char* where = nullptr;
};
thread_local Deferred g_deferred;

inline void cleanup(hipError_t e, const char* where) {
  if (e == hipSuccess) return;
  (void)hipGetLastError();  // kept in g_deferred instead
  if (g_deferred.e == hipSuccess) g_deferred = {e, where};
}

// RNT_OK, or the first deferred cleanup failure of this thread as a status.
int take_deferred() {
  if (g_deferred.e == hipSuccess) return RNT_OK;
  const Deferred d = g_deferred;
  g_deferred = {};
  return fail(RNT_ERR_DEVICE, "%s failed: %s (a cleanup call, reported at the next status)", d.where,
              hipGetErrorString(d.e));
}

// A free / destroy / trim entry point reports only the failures of its own
// cleanup calls: a failure some earlier call deferred stays pending for the
// next launch (check_pending) instead of being consumed -- or blamed on the
// free -- here.  Bindings may drop a free's status (a destructor, __del__);
// an unrelated earlier failure then still reaches a status that is checked.
struct OwnCleanup {
  Deferred saved;
  OwnCleanup() : saved(g_deferred) { g_deferred = {}; }
  int finish() {
    const Deferred mine = g_deferred;
    g_deferred = saved;
    saved = {};
    if (mine.e == hipSuccess) return RNT_OK;
    return fail(RNT_ERR_DEVICE, "%s failed: %s", mine.where, hipGetErrorString(mine.e));
  }
  ~OwnCleanup() {
    if (saved.e != hipSuccess && g_deferred.e == hipSuccess) g_deferred = saved;
  }
};

// Before a launch: a deferred cleanup failure, or an error some earlier
// runtime call on this thread left unreported in the last-error slot.
int check_pending(int id) {
  if (int rc = take_deferred()) return rc;
  const hipError_t pre = hipGetLastError();
  if (pre != hipSuccess)
    return fail(RNT_ERR_DEVICE,
                "a HIP error was pending before the %s launch, left by an earlier runtime call on this "
                "thread that did not report it: %s",
                kKernelNames[id], hipGetErrorString(pre));
  return RNT_OK;
}

// Bracket one launch with events when profiling is on.
template <class F>
hipError_t prof_launch(const rnt::Tables* t, hipStream_t s, int id, F&& f) {
  rnt::Prof* p = t->prof;
  if (p == nullptr || !p->on || g_capture != nullptr) return f();
  std::lock_guard<std::mutex> g(p->mu);
  hipEvent_t a = prof_event(p), b = prof_event(p);
  bool ok = a && b;
  if (ok) {
    if (const hipError_t r = hipEventRecord(a, s); r != hipSuccess) {
      prof_fail(p, r, "hipEventRecord(profile)");
      ok = false;
    }
  }
  hipError_t e = f();
  if (ok && e == hipSuccess) {
    if (const hipError_t r = hipEventRecord(b, s); r != hipSuccess) {
      prof_fail(p, r, "hipEventRecord(profile)");
      ok = false;
    }
  }
  if (ok && e == hipSuccess) {
    p->pending.push_back({id, a, b});
  } else {
    if (a) p->pool.push_back(a);
    if (b) p->pool.push_back(b);
  }
  return e;
}

// Launch on the context's stream, or (LAUNCH_ON) on an explicit one; with
// profiling on, the launch is bracketed by events on that same stream.
#define LAUNCH(T, ID, EXPR, WHERE)                                           \
  do {                                                                       \
    if (int rc_ = check_pending(ID)) return rc_;                             \
    HIP_TRY(prof_launch((T), (T)->stream, (ID), [&]() { return (EXPR); }), WHERE); \
  } while (0)
#define LAUNCH_ON(T, S, ID, EXPR, WHERE)                                     \
  do {                                                                       \
    if (int rc_ = check_pending(ID)) return rc_;                             \
    HIP_TRY(prof_launch((T), (S), (ID), [&]() { return (EXPR); }), WHERE);   \
  } while (0)



inline rnt::Launch launch_for(const rnt_ctx* ctx, size_t n_polys) {
  rnt::Launch k;
  k.t = ctx->t.get();
  k.L = ctx->L;
  k.B = n_polys;
  k.s = k.t->stream;
  return k;
}
inline rnt::Launch launch_for(const rnt_buf* b) { return launch_for(b->ctx, b->n_polys); }

inline size_t poly_words(const rnt_buf* b) { return b->ctx->L * b->n_polys * b->ctx->t->n; }
inline uint64_t limb_stride(const rnt_buf* b) {
  return (uint64_t)(b->view_of ? b->stored_polys : b->n_polys) * b->ctx->t->n;
}

int set_device(const rnt_ctx* ctx) {
  HIP_TRY(hipSetDevice(ctx->t->device), "hipSetDevice");
  return RNT_OK;
}

// Device block cache: the data, workspace and staging blocks of freed
// buffers, kept per device for reuse.  A caller that makes fresh buffers
// every step (the limb-sharded pipeline) then reuses the same gigabytes
// instead of a hipMalloc / hipFree per call; that churn made a long ct-mul
// run fall to ~1/15 of its rate after ~30 steps at 128 ciphertexts.
// A freed block carries an event recorded on the stream of its last use.
// The next taker's stream waits on that event (hipStreamWaitEvent), so no
// free makes the host wait for the device; only a block leaving the cache
// (hipFree) waits for its event first.  Idle bytes per device are capped at
// RNT_WS_POOL_MB, by default 1/8 of the device's memory.
struct PoolBlock {
  int device;
  void* p;
  size_t bytes;
  hipEvent_t ev;     // recorded on `s` when the block was freed
  hipStream_t s;
};
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;               // oldest first
std::vector<std::pair<int, size_t>> g_pool_bytes;  // idle bytes per device
std::vector<hipEvent_t> g_free_events;       // recycled events

static size_t& pool_bytes_of(int device) {  // g_pool_mu held
  for (auto& e : g_pool_bytes)
    if (e.first == device) return e.second;
  g_pool_bytes.push_back({device, 0});
  return g_pool_bytes.back().second;
}

static size_t pool_cap(int device) {  // g_pool_mu held
  if (const char* e = getenv("RNT_WS_POOL_MB")) {  // read per call: tests set it
    const long mb = atol(e);
    return (size_t)(mb > 0 ? mb : 0) << 20;
  }
  static std::vector<std::pair<int, size_t>> caps;  // default: 1/8 of the device
  for (auto& c : caps)
    if (c.first == device) return c.second;
  size_t free_b = 0, total_b = 0;
  const size_t cap = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? total_b / 8 : ((size_t)8 << 30);
  caps.push_back({device, cap});
  return cap;
}

// A stream about to be destroyed, already synchronised: the idle blocks last
// used on it are complete, so they drop their events -- an event must not
// outlive the stream it was last recorded on (the runtime consults that stream
// when the event is waited for, as pool_take's host wait does while a graph is
// being recorded).
static void pool_forget_stream(hipStream_t s) {
  std::vector<hipEvent_t> gone;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (PoolBlock& b : g_pool)
      if (b.s == s && b.ev) {
        gone.push_back(b.ev);
        b.ev = nullptr;
      }
  }
  for (hipEvent_t e : gone) cleanup(hipEventDestroy(e), "hipEventDestroy(block of a stream being destroyed)");
}

static void pool_release(const PoolBlock& w) {  // g_pool_mu NOT held
  cleanup(hipSetDevice(w.device), "hipSetDevice(block leaving the cache)");
  if (w.ev) {
    cleanup(hipEventSynchronize(w.ev), "hipEventSynchronize(block leaving the cache)");
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_free_events.push_back(w.ev);
  }
  cleanup(hipFree(w.p), "hipFree(block leaving the cache)");
}

// Smallest idle block on `device` of at least `bytes` (and at most twice
// that, so a small request does not pin a multi-GiB block), made safe to use
// on stream `s`; nullptr if none.
static void* pool_take(int device, size_t bytes, hipStream_t s, size_t* got, bool call_scoped) {
  if (call_scoped && g_capture != nullptr && g_capture->device == device && g_capture->stream == s) {
    OwnedBlock* best = nullptr;
    for (OwnedBlock& o : g_capture->owned)
      if (o.idle && o.bytes >= bytes && o.bytes / 2 <= bytes && (!best || o.bytes < best->bytes)) best = &o;
    if (best) {
      best->idle = false;
      *got = best->bytes;
      return best->p;
    }
  }
  PoolBlock w{};
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t best = g_pool.size();
    for (size_t i = 0; i < g_pool.size(); ++i) {
      const PoolBlock& c = g_pool[i];
      if (c.device == device && c.bytes >= bytes && c.bytes / 2 <= bytes &&
          (best == g_pool.size() || c.bytes < g_pool[best].bytes))
        best = i;
    }
    if (best == g_pool.size()) return nullptr;
    w = g_pool[best];
    pool_bytes_of(device) -= w.bytes;
    g_pool.erase(g_pool.begin() + (long)best);
  }
  if (w.ev) {
    // same stream: stream order already covers the last use; while a graph
    // is being recorded the wait is a host wait (a recording stream cannot
    // wait on an event from outside the recording)
    if (w.s != s) {
      const hipError_t we = g_capture != nullptr ? hipErrorStreamCaptureUnsupported : hipStreamWaitEvent(s, w.ev, 0);
      if (we != hipSuccess) {
        if (g_capture == nullptr) (void)hipGetLastError();  // handled: a host wait instead
        cleanup(hipEventSynchronize(w.ev), "hipEventSynchronize(block from the cache)");
      }
    }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_free_events.push_back(w.ev);
  }
  *got = w.bytes;
  return w.p;
}

// Hand a block whose last use was queued on stream `s` to the cache; the
// oldest idle blocks of the device leave it while it is over its cap.
static void pool_give(int device, void* p, size_t bytes, hipStream_t s) {
  if (!p) return;
  if (g_capture != nullptr && g_capture->device == device && g_capture->stream == s) {
    // the recorded graph keeps using the block
    for (OwnedBlock& o : g_capture->owned)
      if (o.p == p) {
        o.idle = true;
        return;
      }
    g_capture->owned.push_back({p, bytes, true});
    return;
  }
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_free_events.empty()) {
      ev = g_free_events.back();
      g_free_events.pop_back();
    }
  }
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  if (!ev) (void)hipGetLastError();  // handled: drain instead
  if (ev && hipEventRecord(ev, s) != hipSuccess) {
    (void)hipGetLastError();  // handled: drain instead
    cleanup(hipStreamSynchronize(s), "hipStreamSynchronize(block handed to the cache)");
    cleanup(hipEventDestroy(ev), "hipEventDestroy(block handed to the cache)");
    ev = nullptr;
  } else if (!ev) {
    cleanup(hipStreamSynchronize(s), "hipStreamSynchronize(block handed to the cache)");
  }
  std::vector<PoolBlock> drop;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool.push_back({device, p, bytes, ev, s});
    size_t& idle = pool_bytes_of(device);
    idle += bytes;
    const size_t cap = pool_cap(device);
    for (size_t i = 0; idle > cap && i < g_pool.size();) {
      if (g_pool[i].device == device) {
        drop.push_back(g_pool[i]);
        idle -= g_pool[i].bytes;
        g_pool.erase(g_pool.begin() + (long)i);
      } else {
        ++i;
      }
    }
  }
  for (const PoolBlock& w : drop) pool_release(w);
  if (!drop.empty()) cleanup(hipSetDevice(device), "hipSetDevice(after the cache's release)");
}

// Free every idle block of `device` (-1: of every device).
static size_t pool_drain(int device) {
  std::vector<PoolBlock> drop;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size();) {
      if (device < 0 || g_pool[i].device == device) {
        drop.push_back(g_pool[i]);
        pool_bytes_of(g_pool[i].device) -= g_pool[i].bytes;
        g_pool.erase(g_pool.begin() + (long)i);
      } else {
        ++i;
      }
    }
  }
  size_t freed = 0;
  for (const PoolBlock& w : drop) {
    freed += w.bytes;
    pool_release(w);
  }
  return freed;
}

// A device block of at least `bytes` for work on stream `s`: from the cache,
// else hipMalloc (after emptying the device's cache if that fails).
static hipError_t pool_malloc(int device, size_t bytes, hipStream_t s, void** p, size_t* got,
                              bool call_scoped = false) {
  if ((*p = pool_take(device, bytes, s, got, call_scoped))) return hipSuccess;
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    if (pool_drain(device) > 0) {
      cleanup(hipSetDevice(device), "hipSetDevice(after draining the cache)");
      e = hipMalloc(p, bytes);
    }
  }
  if (e != hipSuccess) {
    *p = nullptr;
    return e;
  }
  *got = bytes;
  return hipSuccess;
}

// Grow the buffer's private workspace to at least `bytes`.
int ensure_ws(rnt_buf* b, size_t bytes) {
  if (b->ws_bytes >= bytes) return RNT_OK;
  const int dev = b->ctx->t->device;
  hipStream_t s = b->ctx->t->stream;
  if (b->ws) {
    pool_give(dev, b->ws, b->ws_bytes, s);  // the stream may still be using it
    b->ws = nullptr;
    b->ws_bytes = 0;
  }
  size_t got = 0;
  if (hipError_t e = pool_malloc(dev, bytes, s, &b->ws, &got); e != hipSuccess)
    return hip_fail(e, "hipMalloc(workspace)");
  b->ws_bytes = got;
  return RNT_OK;
}

// A call-scoped device workspace from the block cache: taken when an op
// starts and handed back when the call returns, behind an event on the op's
// stream (no host wait), so the next op -- on any buffer -- reuses the same
// block.  Key-switch scratch (gigabytes per chunk) lives here rather than
// with an output buffer: a caller that makes a fresh output per chunk (the
// limb-sharded pipeline) would otherwise hold one scratch per live output.
struct CallWs {
  int dev;
  hipStream_t s;
  void* p = nullptr;
  size_t bytes = 0;
  explicit CallWs(const rnt_ctx* ctx) : dev(ctx->t->device), s(ctx->t->stream) {}
  explicit CallWs(const rnt_buf* b) : CallWs(b->ctx) {}
  CallWs(const CallWs&) = delete;
  CallWs& operator=(const CallWs&) = delete;
  // A block of the layout's total (`floor` bytes at the least), the layout placed in it.
  int get(rnt::WsLayout& w, size_t floor = 0) {
    size_t got = 0;
    if (hipError_t e = pool_malloc(dev, w.total(floor), s, &p, &got, true); e != hipSuccess)
      return hip_fail(e, "hipMalloc(workspace)");
    bytes = got;
    w.place(p);
    return RNT_OK;
  }
  ~CallWs() {
    if (p) pool_give(dev, p, bytes, s);
  }
};

int ensure_stage(rnt_buf* b, size_t bytes) {
  if (b->stage_bytes >= bytes) return RNT_OK;
  const int dev = b->ctx->t->device;
  hipStream_t s = b->ctx->t->stream;
  if (b->stage) {
    pool_give(dev, b->stage, b->stage_bytes, s);
    b->stage = nullptr;
    b->stage_bytes = 0;
  }
  size_t got = 0;
  if (hipError_t e = pool_malloc(dev, bytes, s, &b->stage, &got); e != hipSuccess)
    return hip_fail(e, "hipMalloc(stage)");
  b->stage_bytes = got;
  return RNT_OK;
}

// Staging for uploads/downloads stays with its buffer, except very large
// ones (a 256-poly batch at N=2^16, L=16 stages 2 GiB of u64), which go back
// to the cache.
void trim_stage(rnt_buf* b) {
  if (b->stage_bytes > ((size_t)256 << 20)) {
    pool_give(b->ctx->t->device, b->stage, b->stage_bytes, b->ctx->t->stream);
    b->stage = nullptr;
    b->stage_bytes = 0;
  }
}

// A key argument of a hybrid call: a buffer or a level view of one.
int check_key_buf(const rnt_buf* b, const char* name) {
  if (b == nullptr || b->ctx == nullptr) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null buffer", name);
  return RNT_OK;
}
// Every other operand: a key level view is read-only, strided storage of
// another buffer and serves as a hybrid key alone.
int check_buf(const rnt_buf* b, const char* name) {
  if (int rc = check_key_buf(b, name)) return rc;
  if (b->view_of)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "%s: a key level view serves only as the key of a hybrid call", name);
  return RNT_OK;
}

// Same basis (Arc::ptr_eq on the basis in the reference) and batch size.
int check_same(const rnt_buf* a, const rnt_buf* b, const char* what) {
  if (a->ctx != b->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: operands belong to different bases", what);
  if (a->n_polys != b->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: batch sizes differ (%zu vs %zu)", what, a->n_polys,
                b->n_polys);
  return RNT_OK;
}

// The MFMA transforms (rnt_mfma.hip) for this context: N = 2^16 on a u32
// basis (unless RNT_PLANE=0).  Their tables are built with the context
// (rnt_ctx_create), so no op -- none recorded into a graph either -- ever
// builds them, and a context whose build failed does not exist.
bool use_mf(const rnt::Launch& k) { return rnt::mf_supported(k.t) && k.t->mf != nullptr; }

// Inverse-transform src (NTT domain) into dst (same layout): dst may equal src.
int to_coeff_into(const rnt_buf* src, void* dst) {
  rnt::Launch k = launch_for(src);
  const uint64_t ls = limb_stride(src);
  if (dst != src->data)
    HIP_TRY(hipMemcpyAsync(dst, src->data, poly_words(src) * word_bytes(k.t),
                           hipMemcpyDeviceToDevice, k.s),
            "hipMemcpyAsync");
  if (use_mf(k)) {
    LAUNCH(k.t, rnt::K_MF_NTT_INV, rnt::launch_mf_ntt(k, 1, dst, ls), "MFMA inverse transform");
    return RNT_OK;
  }
  if (rnt::whole_ok(k.t, 1)) {
    LAUNCH(k.t, rnt::K_WHOLE_INV, rnt::launch_whole(k, 1, dst, dst, nullptr, ls), "whole-plane inverse");
    return RNT_OK;
  }
  LAUNCH(k.t, rnt::K_ROW_INV, rnt::launch_row(k, 1, dst, nullptr, ls), "row inverse");
  LAUNCH(k.t, rnt::K_COL_INV, rnt::launch_col_inv(k, dst, ls, dst, ls, 0, nullptr), "column inverse");
  return RNT_OK;
}

void lincomb_forget_stream(hipStream_t s);  // (with rnt_ct_lincomb's staging slots, below)

}  // namespace

rnt::Tables::~Tables() {
  cleanup(hipSetDevice(device), "hipSetDevice(context teardown)");
  if (stream && stream != own_stream)  // a caller's stream
    cleanup(hipStreamSynchronize(stream), "hipStreamSynchronize(context teardown)");
  if (own_stream) {
    cleanup(hipStreamSynchronize(own_stream), "hipStreamSynchronize(context teardown)");
    pool_forget_stream(own_stream);
    lincomb_forget_stream(own_stream);
    cleanup(hipStreamDestroy(own_stream), "hipStreamDestroy(context teardown)");
  }
  for (auto& e : resc_ext) cleanup(hipFree(e.second), "hipFree(context tables)");
  for (auto& e : crt_cache) cleanup(hipFree(e.second.dev), "hipFree(context tables)");
  for (auto& e : hyb_cache) cleanup(hipFree(e.dev), "hipFree(context tables)");
  for (auto& e : raise_cache) cleanup(hipFree(e.dev), "hipFree(context tables)");
  for (void* p : {tw_fwd, tw_inv, sfft_tw, lconst, resc, resc_p, mf})
    cleanup(hipFree(p), "hipFree(context tables)");
  if (prof) {
    for (auto& r : prof->pending) {
      cleanup(hipEventDestroy(r.a), "hipEventDestroy(profile)");
      cleanup(hipEventDestroy(r.b), "hipEventDestroy(profile)");
    }
    for (hipEvent_t e : prof->pool) cleanup(hipEventDestroy(e), "hipEventDestroy(profile)");
    delete prof;
  }
}

static long env_long(const char* name, long dflt);

// ---------------------------------------------------------------------------
// diagnostics
// ---------------------------------------------------------------------------
extern "C" int rnt_abi_version(void) { return RNT_ABI_VERSION; }
extern "C" int rnt_last_error_detail(uint64_t fields[2]) {
  if (fields) {
    fields[0] = g_last_detail.a;
    fields[1] = g_last_detail.b;
  }
  return g_last_detail.status;
}

extern "C" const char* rnt_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* rnt_status_string(int s) {
  switch (s) {
    case RNT_OK: return "ok";
    case RNT_ERR_INVALID_DEGREE: return "InvalidDegree";
    case RNT_ERR_EMPTY_BASIS: return "EmptyBasis";
    case RNT_ERR_NON_NTT_FRIENDLY: return "NonNttFriendlyModulus";
    case RNT_ERR_INVALID_MOD_DROP: return "InvalidModDrop";
    case RNT_ERR_CHANNEL_COUNT: return "ChannelCountMismatch";
    case RNT_ERR_NON_REDUCED: return "NonReducedCoefficient";
    case RNT_ERR_DOMAIN_MISMATCH: return "DomainMismatch";
    case RNT_ERR_BASIS_MISMATCH: return "BasisMismatch";
    case RNT_ERR_DEVICE: return "DeviceError";
    case RNT_ERR_OUT_OF_MEMORY: return "OutOfMemory";
    case RNT_ERR_BAD_ARGUMENT: return "BadArgument";
    case RNT_ERR_UNSUPPORTED: return "Unsupported";
    default: return "unknown";
  }
}

// ---------------------------------------------------------------------------
// host-side number theory
// ---------------------------------------------------------------------------
extern "C" int rnt_is_ntt_friendly_prime(uint64_t p, uint64_t degree, int* out) {
  if (!out) return fail(RNT_ERR_BAD_ARGUMENT, "null out");
  if (degree == 0 || degree > UINT64_MAX / 2)
    return fail(RNT_ERR_BAD_ARGUMENT, "is_ntt_friendly_prime: degree must be in [1, 2^63)");
  *out = rnt::host::is_ntt_friendly(p, degree) ? 1 : 0;
  return RNT_OK;
}

extern "C" int rnt_generate_primes(uint32_t bit_size, size_t count, uint64_t degree,
                                   uint64_t* out) {
  if (!out && count) return fail(RNT_ERR_BAD_ARGUMENT, "null out");
  if (rnt::host::generate_primes(bit_size, count, degree, out) != 0)
    return fail(RNT_ERR_BAD_ARGUMENT,
                "Unable to find %zu NTT primes with %u-bit ceiling for degree %" PRIu64, count,
                bit_size, degree);
  return RNT_OK;
}

extern "C" int rnt_find_psi(uint64_t modulus, uint64_t degree, uint64_t* psi) {
  if (!psi) return fail(RNT_ERR_BAD_ARGUMENT, "null out");
  if (degree == 0 || (degree & (degree - 1)))
    return fail_fields(RNT_ERR_INVALID_DEGREE, degree, 0, "ring degree must be a power of two, got %" PRIu64,
                       degree);
  if (!rnt::host::is_ntt_friendly(modulus, degree))
    return fail_fields(RNT_ERR_NON_NTT_FRIENDLY, modulus, degree,
                       "modulus %" PRIu64 " is not NTT-friendly for degree %" PRIu64,
                modulus, degree);
  *psi = rnt::host::find_psi(modulus, degree);
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
namespace {

template <class W>
int build_tables(rnt::Tables* t) {
  using namespace rnt::host;
  const size_t n = t->n, L = t->L;
  const unsigned wbits = sizeof(W) * 8;
  std::vector<rnt::Tw<W>> tw(L * n), itw(L * n);
  std::vector<rnt::LimbConst<W>> lc(L);
  std::vector<W> resc(L * L, 0), rescp(L * L, 0);
  std::vector<uint64_t> pw(n), ipw(n);
  for (size_t l = 0; l < L; ++l) {
    const uint64_t q = t->moduli[l];
    const uint64_t psi = find_psi(q, n);
    if (psi == 0)
      return fail_fields(RNT_ERR_NON_NTT_FRIENDLY, q, n, "no primitive 2N-th root mod %" PRIu64, q);
    t->psi.push_back(psi);
    const uint64_t psi_inv = invmod(psi, q);
    uint64_t a = 1, b = 1;
    for (size_t j = 0; j < n; ++j) {
      pw[j] = a;
      ipw[j] = b;
      a = mulmod(a, psi, q);
      b = mulmod(b, psi_inv, q);
    }
    rnt::Tw<W>* T = tw.data() + l * n;
    rnt::Tw<W>* I = itw.data() + l * n;
    T[0] = {(W)1, (W)shoup_companion(1, q, wbits)};
    I[0] = T[0];
    for (size_t g = 1; g < n; ++g) {
      const uint64_t e = brv(g, t->log_n);
      T[g] = {(W)pw[e], (W)shoup_companion(pw[e], q, wbits)};
      I[g] = {(W)ipw[e], (W)shoup_companion(ipw[e], q, wbits)};
    }
    rnt::LimbConst<W>& c = lc[l];
    c.q = (W)q;
    c.qinv = (W)neg_free_qinv(q, wbits);
    c.one_p = (W)shoup_companion(1, q, wbits);
    const uint64_t r = (uint64_t)((((u128)1) << wbits) % q);  // 2^w mod q
    c.rmod = (W)r;
    c.rmod_p = (W)shoup_companion(r, q, wbits);
    const uint64_t ninv = invmod(n % q, q);
    const uint64_t w1 = n > 1 ? (uint64_t)I[1].w : 1;
    c.c1 = (W)ninv;
    c.c1_p = (W)shoup_companion(ninv, q, wbits);
    c.c2 = (W)mulmod(w1, ninv, q);
    c.c2_p = (W)shoup_companion(c.c2, q, wbits);
    const uint64_t ninvr = mulmod(ninv, r, q);
    c.c1r = (W)ninvr;
    c.c1r_p = (W)shoup_companion(ninvr, q, wbits);
    c.c2r = (W)mulmod(w1, ninvr, q);
    c.c2r_p = (W)shoup_companion(c.c2r, q, wbits);
    const uint64_t ninvrt = mulmod(ninvr, 4 % q, q);
    c.c1t = (W)ninvrt;
    c.c1t_p = (W)shoup_companion(ninvrt, q, wbits);
    c.c2t = (W)mulmod(w1, ninvrt, q);
    c.c2t_p = (W)shoup_companion(c.c2t, q, wbits);
    for (size_t i = 0; i < l; ++i) {
      const uint64_t qi = t->moduli[i];
      const uint64_t inv = invmod(q % qi, qi);
      if (inv == 0)
        return fail(RNT_ERR_BAD_ARGUMENT, "moduli %" PRIu64 " and %" PRIu64 " are not coprime", q, qi);
      resc[l * L + i] = (W)inv;
      rescp[l * L + i] = (W)shoup_companion(inv, qi, wbits);
    }
  }
  const size_t tb = L * n * sizeof(rnt::Tw<W>);
  HIP_TRY(hipMalloc(&t->tw_fwd, tb), "hipMalloc(tables)");
  HIP_TRY(hipMalloc(&t->tw_inv, tb), "hipMalloc(tables)");
  HIP_TRY(hipMalloc(&t->lconst, L * sizeof(rnt::LimbConst<W>)), "hipMalloc(tables)");
  HIP_TRY(hipMalloc(&t->resc, L * L * sizeof(W)), "hipMalloc(tables)");
  HIP_TRY(hipMalloc(&t->resc_p, L * L * sizeof(W)), "hipMalloc(tables)");
  HIP_TRY(hipMemcpy(t->tw_fwd, tw.data(), tb, hipMemcpyHostToDevice), "hipMemcpy");
  HIP_TRY(hipMemcpy(t->tw_inv, itw.data(), tb, hipMemcpyHostToDevice), "hipMemcpy");
  HIP_TRY(hipMemcpy(t->lconst, lc.data(), L * sizeof(rnt::LimbConst<W>), hipMemcpyHostToDevice),
          "hipMemcpy");
  HIP_TRY(hipMemcpy(t->resc, resc.data(), L * L * sizeof(W), hipMemcpyHostToDevice), "hipMemcpy");
  HIP_TRY(hipMemcpy(t->resc_p, rescp.data(), L * L * sizeof(W), hipMemcpyHostToDevice),
          "hipMemcpy");
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ctx_create(uint32_t log_n, const uint64_t* moduli, size_t count, int device,
                              rnt_ctx** out) {
  if (!out) return fail(RNT_ERR_BAD_ARGUMENT, "null out");
  *out = nullptr;
  // RnsBasis::new order (basis.rs:97-106): empty basis first, then each
  // NttTable::new (degree check, NTT-friendliness).
  if (count == 0) return fail(RNT_ERR_EMPTY_BASIS, "RNS basis must contain at least one modulus");
  if (!moduli) return fail(RNT_ERR_BAD_ARGUMENT, "null moduli");
  // log_n is the exponent of a power of two, so the reference's
  // InvalidDegree (basis.rs:22-24, "not a power of two") cannot arise here;
  // the Python/C++ mirrors raise it before calling.
  if (log_n >= 63) return fail(RNT_ERR_BAD_ARGUMENT, "log_n %u out of range", log_n);
  const uint64_t n = 1ull << log_n;
  bool wide = false, lazy30 = true, lazy62 = true;
  for (size_t i = 0; i < count; ++i) {
    if (!rnt::host::is_ntt_friendly(moduli[i], n))
      return fail_fields(RNT_ERR_NON_NTT_FRIENDLY, moduli[i], n,
                         "modulus %" PRIu64 " is not NTT-friendly for degree %" PRIu64, moduli[i], n);
    if (moduli[i] >= (1ull << 63))
      return fail(RNT_ERR_BAD_ARGUMENT,
                  "modulus %" PRIu64 " >= 2^63 (the reference's add_mod overflows)", moduli[i]);
    if (moduli[i] >= (1ull << 31)) wide = true;
    if (moduli[i] >= (1ull << 30)) lazy30 = false;
    if (moduli[i] >= (1ull << 62)) lazy62 = false;
  }
  // a valid basis the reference would accept, beyond this backend's tables
  // and grids: its own capacity status, not the reference's InvalidDegree
  if (log_n > (uint32_t)rnt::kMaxLogN)
    return fail_fields(RNT_ERR_UNSUPPORTED, n, 1ull << rnt::kMaxLogN,
                       "ring degree 2^%u exceeds this backend's maximum 2^%d (Unsupported, not "
                       "InvalidDegree: the degree is valid for the reference)",
                       log_n, rnt::kMaxLogN);
  try {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (device < 0 || device >= ndev)
      return fail(RNT_ERR_BAD_ARGUMENT, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    auto t = std::make_shared<rnt::Tables>();
    t->device = device;
    t->wide = wide ? 1 : 0;
    // RNT_LAZY30=0 keeps the canonical product path for 30-bit bases (A/B)
    t->lazy30 = !wide && lazy30 && env_long("RNT_LAZY30", 1) != 0;
    // the same Harvey-lazy product path for u64 bases of primes < 2^62 (the
    // reference's 40/61/62-bit tests); RNT_LAZY62=0 keeps the canonical one
    t->lazy62 = wide && lazy62 && env_long("RNT_LAZY62", 1) != 0;
    // the ct-mul's key-switch takes its diagonal (source limb i of target
    // limb i) from the tensor's exact d2^ instead of transforming it;
    // RNT_KS_DIAG=0 transforms every (i, j) (A/B)
    t->ks_diag = env_long("RNT_KS_DIAG", 1) != 0;
    t->rot_fuse = (int)env_long("RNT_ROT_FUSE", 1);
    {
      const long m = env_long("RNT_MODDOWN_AUTO", 1);
      t->md_auto = m == 0 || m == 2 ? (int)m : 1;
    }
    // the whole-plane product and MFMA transforms are the default where they
    // apply (N = 2^16, u32); RNT_PLANE=0 keeps the four-step kernels
    t->plane = env_long("RNT_PLANE", 1) != 0 ? 1 : 0;
    // the product on the matrix-core transforms (k_mf_mul) where they apply;
    // RNT_MF_MUL=0 keeps the VALU whole-plane product (k_plane_fused_slots)
    t->mf_mul = env_long("RNT_MF_MUL", 1) != 0 ? 1 : 0;
    {
      const long jg = env_long("RNT_DEC_JG", 0);  // A/B knob: 0 = auto, else 1..1024
      t->dec_jg = (uint32_t)(jg < 0 ? 0 : jg > 1024 ? 1024 : jg);
      // key-switch scratch cap (S = [L][L][Bc][N] words per chunk), MiB.
      // 16 GiB: 256-ct chunks at config 4 (N = 2^16, L = 16) ran the fused
      // ct-mul 2.5% faster than 64-ct ones (4 GiB), the tensor and rows
      // kernels' last-round tails amortised over 4x the grid; 32 GiB chunks
      // fell off the workspace pool (profiles/r06/ab_ks_chunk.txt)
      const long mb = env_long("RNT_KS_WS_MB", 16384);
      t->ks_ws_bytes = (size_t)(mb > 0 ? mb : 16384) << 20;
    }
    t->log_n = log_n;
    t->n = (size_t)n;
    t->L = count;
    t->moduli.assign(moduli, moduli + count);
    int rc = wide ? build_tables<uint64_t>(t.get()) : build_tables<uint32_t>(t.get());
    if (rc != RNT_OK) return rc;
    if (rnt::mf_supported(t.get())) {
      std::string err;
      if (const int m = rnt::mf_build(t.get(), &err); m != 0) {
        (void)hipGetLastError();  // reported here
        return fail(m == -3 ? RNT_ERR_OUT_OF_MEMORY : RNT_ERR_DEVICE, "%s", err.c_str());
      }
    }
    HIP_TRY(hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking), "hipStreamCreate");
    t->stream = t->own_stream;
    rnt_ctx* c = new rnt_ctx;
    c->t = std::move(t);
    c->L = count;
    *out = c;
    return RNT_OK;
  } catch (const std::bad_alloc&) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (...) {
    return fail(RNT_ERR_DEVICE, "unexpected exception in rnt_ctx_create");
  }
}

static void ctx_release(const rnt_ctx* ctx) {
  while (ctx && const_cast<rnt_ctx*>(ctx)->refs.fetch_sub(1) == 1) {
    const rnt_ctx* parent = ctx->parent;  // a level context holds its parent
    delete ctx;
    ctx = parent;
  }
}
static void ctx_retain(const rnt_ctx* ctx) { const_cast<rnt_ctx*>(ctx)->refs.fetch_add(1); }

extern "C" int rnt_ctx_destroy(rnt_ctx* ctx) {
  OwnCleanup own;
  ctx_release(ctx);  // freed once its last buffer is freed too
  return own.finish();
}

extern "C" int rnt_ctx_drop_last(const rnt_ctx* ctx, size_t drop_count, rnt_ctx** out) {
  if (!ctx || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (ctx->is_level())
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "rnt_ctx_drop_last: a level context has no prefixes");
  if (drop_count >= ctx->L)
    return fail_fields(RNT_ERR_INVALID_MOD_DROP, drop_count, ctx->L,
                       "invalid mod-drop count %zu for %zu channels", drop_count, ctx->L);
  try {
    rnt_ctx* c = new rnt_ctx;
    c->t = ctx->t;
    c->L = ctx->L - drop_count;
    *out = c;
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  return RNT_OK;
}

extern "C" int rnt_ctx_hybrid_level(const rnt_ctx* key_ctx, size_t n_special, size_t level, rnt_ctx** out) {
  if (!key_ctx || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (key_ctx->is_level())
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ctx_hybrid_level: the key context is itself a level context");
  if (n_special == 0 || n_special >= key_ctx->L)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ctx_hybrid_level: %zu special limbs of %zu", n_special, key_ctx->L);
  const size_t L = key_ctx->L - n_special;
  if (level == 0 || level > L)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ctx_hybrid_level: level %zu of %zu", level, L);
  try {
    rnt_ctx* c = new rnt_ctx;
    c->t = key_ctx->t;
    c->L = level + n_special;
    c->parent = key_ctx;
    c->level = level;
    c->gap = L - level;
    ctx_retain(key_ctx);
    *out = c;
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  return RNT_OK;
}

extern "C" int rnt_ctx_degree(const rnt_ctx* ctx, size_t* n) {
  if (!ctx || !n) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *n = ctx->t->n;
  return RNT_OK;
}
extern "C" int rnt_ctx_channel_count(const rnt_ctx* ctx, size_t* count) {
  if (!ctx || !count) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *count = ctx->L;
  return RNT_OK;
}
extern "C" int rnt_ctx_moduli(const rnt_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  for (size_t i = 0; i < ctx->L; ++i) out[i] = ctx->modulus(i);
  return RNT_OK;
}
extern "C" int rnt_ctx_total_bits(const rnt_ctx* ctx, uint32_t* bits) {
  if (!ctx || !bits) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  uint32_t s = 0;
  for (size_t i = 0; i < ctx->L; ++i) s += 63u - (uint32_t)__builtin_clzll(ctx->modulus(i));
  *bits = s;
  return RNT_OK;
}
extern "C" int rnt_ctx_psi(const rnt_ctx* ctx, size_t limb, uint64_t* psi) {
  if (!ctx || !psi) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  if (limb >= ctx->L) return fail(RNT_ERR_BAD_ARGUMENT, "limb %zu out of range", limb);
  *psi = ctx->t->psi[ctx->root_limb(limb)];
  return RNT_OK;
}
extern "C" int rnt_ctx_stream(const rnt_ctx* ctx, void** stream) {
  if (!ctx || !stream) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *stream = (void*)ctx->t->stream;
  return RNT_OK;
}
// Later ops go to `stream` (NULL: the context's own) after everything queued
// so far: the new stream waits on an event recorded on the old one.
extern "C" int rnt_ctx_set_stream(const rnt_ctx* ctx, void* stream) {
  if (!ctx) return fail(RNT_ERR_BAD_ARGUMENT, "null ctx");
  if (int rc = set_device(ctx)) return rc;
  rnt::Tables* t = ctx->t.get();
  hipStream_t next = stream ? (hipStream_t)stream : t->own_stream;
  if (next == t->stream) return RNT_OK;
  if (stream) {
    hipDevice_t dev = -1;
    HIP_TRY(hipStreamGetDevice(next, &dev), "hipStreamGetDevice");
    if (dev != t->device)
      return fail(RNT_ERR_BAD_ARGUMENT, "stream is on device %d, the context on device %d", (int)dev,
                  t->device);
  }
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
  hipError_t e = hipEventRecord(ev, t->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(next, ev, 0);
  cleanup(hipEventDestroy(ev), "hipEventDestroy(rnt_ctx_set_stream)");  // released once it completes
  if (e != hipSuccess) return hip_fail(e, "rnt_ctx_set_stream");
  t->stream = next;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// captured op sequences (hipGraph)
// ---------------------------------------------------------------------------
// A recorded graph owns the distinct workspace blocks its ops took (on
// `device`); they go back to the cache when it is destroyed, behind an event
// on `last` -- the stream the latest replay was queued on.  A replay on a
// new stream (after rnt_ctx_set_stream) is first ordered after the previous
// replays, so `last` covers every replay.
// `done`: recorded after each replay, so the next replay (on whatever
// stream the context uses by then) and the blocks' return to the cache wait
// for it -- no stream handle outlives its use here.
struct rnt_graph {
  std::shared_ptr<rnt::Tables> t;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  std::vector<OwnedBlock> owned;
  int device = 0;
  hipEvent_t done = nullptr;
  bool replayed = false;
};

extern "C" int rnt_capture_begin(const rnt_ctx* ctx) {
  if (!ctx) return fail(RNT_ERR_BAD_ARGUMENT, "null ctx");
  if (g_capture != nullptr) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_capture_begin: already recording on this thread");
  if (int rc = set_device(ctx)) return rc;
  Capture* c = nullptr;
  try {
    c = new Capture;
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  c->stream = ctx->t->stream;
  c->device = ctx->t->device;
  // relaxed: the ops' own host-side calls (none synchronising once warm)
  // are not checked against the recording
  if (hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed); e != hipSuccess) {
    delete c;
    return hip_fail(e, "hipStreamBeginCapture");
  }
  g_capture = c;
  return RNT_OK;
}

extern "C" int rnt_capture_end(const rnt_ctx* ctx, rnt_graph** out) {
  if (!ctx || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  Capture* c = g_capture;
  if (c == nullptr || c->stream != ctx->t->stream)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_capture_end: no recording on this context's stream");
  g_capture = nullptr;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(c->stream, &g);
  rnt_graph* r = nullptr;
  if (e == hipSuccess) {
    try {
      r = new rnt_graph;
    } catch (...) {
      e = hipErrorOutOfMemory;
    }
  }
  if (r != nullptr) {
    r->t = ctx->t;
    r->graph = g;
    r->owned = std::move(c->owned);
    r->device = c->device;
    e = hipEventCreateWithFlags(&r->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipGraphInstantiate(&r->exec, g, nullptr, nullptr, 0);
  }
  if (e != hipSuccess) {
    const int dev = c->device;
    const hipStream_t st = c->stream;
    std::vector<OwnedBlock> owned = r ? std::move(r->owned) : std::move(c->owned);
    if (g) cleanup(hipGraphDestroy(g), "hipGraphDestroy(failed capture)");
    if (r && r->done) cleanup(hipEventDestroy(r->done), "hipEventDestroy(failed capture)");
    delete r;
    delete c;
    for (auto& b : owned) pool_give(dev, b.p, b.bytes, st);
    return hip_fail(e, "rnt_capture_end");
  }
  delete c;
  *out = r;
  return RNT_OK;
}

extern "C" int rnt_graph_launch(rnt_graph* g) {
  if (!g) return fail(RNT_ERR_BAD_ARGUMENT, "null graph");
  if (g_capture != nullptr) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_graph_launch while recording");
  HIP_TRY(hipSetDevice(g->device), "hipSetDevice");
  hipStream_t s = g->t->stream;
  if (int rc = take_deferred()) return rc;
  // after the previous replay, wherever it was queued (same stream: free)
  if (g->replayed) HIP_TRY(hipStreamWaitEvent(s, g->done, 0), "hipStreamWaitEvent");
  HIP_TRY(hipGraphLaunch(g->exec, s), "hipGraphLaunch");
  HIP_TRY(hipEventRecord(g->done, s), "hipEventRecord");
  g->replayed = true;
  return RNT_OK;
}

extern "C" int rnt_graph_destroy(rnt_graph* g) {
  if (!g) return RNT_OK;
  OwnCleanup own;
  cleanup(hipSetDevice(g->device), "hipSetDevice(rnt_graph_destroy)");
  // a replay may still be running: the blocks go back to the cache behind
  // the context's current stream, made to wait for the last replay first
  hipStream_t s = g->t->stream;
  if (g->replayed) cleanup(hipStreamWaitEvent(s, g->done, 0), "hipStreamWaitEvent(rnt_graph_destroy)");
  for (auto& b : g->owned) pool_give(g->device, b.p, b.bytes, s);
  if (g->exec) cleanup(hipGraphExecDestroy(g->exec), "hipGraphExecDestroy");
  if (g->graph) cleanup(hipGraphDestroy(g->graph), "hipGraphDestroy");
  if (g->done) cleanup(hipEventDestroy(g->done), "hipEventDestroy(rnt_graph_destroy)");
  delete g;
  return own.finish();
}

extern "C" int rnt_graph_workspace(const rnt_graph* g, size_t* blocks, size_t* bytes) {
  if (!g || !blocks || !bytes) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *blocks = g->owned.size();
  *bytes = 0;
  for (const OwnedBlock& b : g->owned) *bytes += b.bytes;
  return RNT_OK;
}

extern "C" int rnt_sync(const rnt_ctx* ctx) {
  if (!ctx) return fail(RNT_ERR_BAD_ARGUMENT, "null ctx");
  if (int rc = set_device(ctx)) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->t->stream), "hipStreamSynchronize");
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------
static int buf_alloc(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out, bool zero);

extern "C" int rnt_buf_alloc(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out) {
  return buf_alloc(ctx, n_polys, out, true);
}

// An op's output buffer: the op overwrites every word, so the zero fill
// (a fill kernel of the whole buffer on the stream: 33 us per 16 MiB, two
// per ct-mul chunk for the tensor's d0^/d1^) is skipped.
extern "C" int rnt_buf_alloc_uninit(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out) {
  return buf_alloc(ctx, n_polys, out, false);
}

static int buf_alloc(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out, bool zero) {
  if (!ctx || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (ctx->is_level())
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "a level context holds key views alone (rnt_key_level_view)");
  if (n_polys == 0) return fail(RNT_ERR_BAD_ARGUMENT, "n_polys must be positive");
  if (int rc = set_device(ctx)) return rc;
  rnt_buf* b = nullptr;
  try {
    b = new rnt_buf;
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  b->ctx = ctx;
  const_cast<rnt_ctx*>(ctx)->refs.fetch_add(1);
  b->n_polys = n_polys;
  const size_t bytes = poly_words(b) * word_bytes(ctx->t.get());
  hipStream_t s = ctx->t->stream;
  hipError_t e = pool_malloc(ctx->t->device, bytes, s, &b->data, &b->data_bytes);
  if (e != hipSuccess) {
    ctx_release(ctx);
    delete b;
    return hip_fail(e, "hipMalloc(buffer)");
  }
  // zero (RnsPoly::zero), queued on the context stream like every op
  if (zero) e = hipMemsetAsync(b->data, 0, bytes, s);
  if (e != hipSuccess) {
    pool_give(ctx->t->device, b->data, b->data_bytes, s);
    ctx_release(ctx);
    delete b;
    return hip_fail(e, "hipMemset(buffer)");
  }
  *out = b;
  return RNT_OK;
}

// No host wait: the blocks go to the device cache with an event on the
// context stream, behind every op queued on this buffer.
extern "C" int rnt_buf_free(rnt_buf* b) {
  if (!b) return RNT_OK;
  OwnCleanup own;
  if (b->ctx) {
    const int dev = b->ctx->t->device;
    hipStream_t s = b->ctx->t->stream;
    cleanup(hipSetDevice(dev), "hipSetDevice(rnt_buf_free)");
    if (b->owns) pool_give(dev, b->data, b->data_bytes, s);
    pool_give(dev, b->ws, b->ws_bytes, s);
    pool_give(dev, b->stage, b->stage_bytes, s);
  }
  ctx_release(b->ctx);
  delete b;
  return own.finish();
}

extern "C" int rnt_debug_defer(int hip_error) {
  if (hip_error == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_debug_defer: hip_error must be nonzero");
  cleanup(static_cast<hipError_t>(hip_error), "rnt_debug_defer");
  return RNT_OK;
}

extern "C" int rnt_pool_trim(int device, size_t* freed_bytes) {
  OwnCleanup own;
  const size_t f = pool_drain(device);
  if (freed_bytes) *freed_bytes = f;
  return own.finish();
}

extern "C" int rnt_buf_wrap(const rnt_ctx* ctx, void* device_ptr, size_t n_polys, int in_ntt,
                            rnt_buf** out) {
  if (!ctx || !device_ptr || !out) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  if (ctx->is_level())
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "rnt_buf_wrap: a level context holds key views alone");
  if (n_polys == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_buf_wrap: empty batch");
  // word alignment is the whole contract (rnsntt.h): the one-word kernel
  // forms load and store W at a time, and a u64 word at % 8 == 4 is no word
  const size_t wb = word_bytes(ctx->t.get());
  if ((uintptr_t)device_ptr % wb != 0)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_buf_wrap: device_ptr is not aligned to the context's %zu-byte words", wb);
  rnt_buf* b = new (std::nothrow) rnt_buf;
  if (!b) return fail(RNT_ERR_OUT_OF_MEMORY, "rnt_buf_wrap");
  b->ctx = ctx;
  b->n_polys = n_polys;
  b->data = device_ptr;
  b->in_ntt = in_ntt ? 1 : 0;
  b->owns = false;
  ctx_retain(ctx);
  *out = b;
  return RNT_OK;
}

extern "C" int rnt_buf_device_ptr(const rnt_buf* b, void** device_ptr, size_t* word_bytes_out) {
  if (!b || !device_ptr) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = check_buf(b, "rnt_buf_device_ptr")) return rc;
  *device_ptr = b->data;
  if (word_bytes_out) *word_bytes_out = word_bytes(b->ctx->t.get());
  return RNT_OK;
}

extern "C" int rnt_key_level_view(const rnt_buf* key, const rnt_ctx* level_ctx, size_t alpha, rnt_buf** out) {
  const char* name = "rnt_key_level_view";
  if (!out || !level_ctx) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null argument", name);
  *out = nullptr;
  if (int rc = check_key_buf(key, name)) return rc;
  if (key->view_of) return fail(RNT_ERR_BAD_ARGUMENT, "%s: the key is itself a level view", name);
  if (!level_ctx->is_level()) return fail(RNT_ERR_BAD_ARGUMENT, "%s: not a level context", name);
  if (key->ctx != level_ctx->parent)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the key is not on the context the level context was made from", name);
  if (!key->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the key must be prepared (rnt_key_prepare)", name);
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  const size_t L = level_ctx->level + level_ctx->gap;
  const size_t beta = (L + alpha - 1) / alpha, beta_v = (level_ctx->level + alpha - 1) / alpha;
  if (key->n_polys % beta != 0)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, beta, key->n_polys,
                       "%s: a hybrid key for %zu limbs in digits of %zu holds a multiple of %zu polys", name, L, alpha,
                       beta);
  rnt_buf* b = new (std::nothrow) rnt_buf;
  if (!b) return fail(RNT_ERR_OUT_OF_MEMORY, "%s", name);
  b->ctx = level_ctx;
  b->n_polys = key->n_polys / beta * beta_v;
  b->data = key->data;
  b->in_ntt = 1;
  b->owns = false;
  b->view_of = key;
  b->stored_polys = key->n_polys;
  b->step_polys = beta;
  ctx_retain(level_ctx);
  *out = b;
  return RNT_OK;
}

extern "C" int rnt_buf_n_polys(const rnt_buf* b, size_t* n) {
  if (!b || !n) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *n = b->n_polys;
  return RNT_OK;
}
extern "C" int rnt_buf_is_ntt(const rnt_buf* b, int* in_ntt) {
  if (!b || !in_ntt) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  *in_ntt = b->in_ntt;
  return RNT_OK;
}

extern "C" int rnt_upload(rnt_buf* b, const uint64_t* host, size_t n_polys, size_t channels,
                          int in_ntt) {
  if (int rc = check_buf(b, "rnt_upload")) return rc;
  if (!host) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_upload: null host pointer");
  // from_channels order (poly.rs:78-93): channel count, then reducedness.
  if (channels != b->ctx->L)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, b->ctx->L, channels,
                       "channel count mismatch: expected %zu, got %zu", b->ctx->L, channels);
  if (n_polys != b->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_upload: buffer holds %zu polys, got %zu", b->n_polys,
                n_polys);
  if (int rc = set_device(b->ctx)) return rc;
  rnt::Launch k = launch_for(b);
  const size_t words = poly_words(b);
  if (int rc = ensure_stage(b, words * 8 + 64)) return rc;
  unsigned long long* err = (unsigned long long*)((char*)b->stage + words * 8);
  HIP_TRY(hipMemcpyAsync(b->stage, host, words * 8, hipMemcpyHostToDevice, k.s), "hipMemcpy H2D");
  HIP_TRY(hipMemsetAsync(err, 0xff, 8, k.s), "hipMemset");
  LAUNCH(k.t, rnt::K_IMPORT, rnt::launch_import(k, b->data, (const uint64_t*)b->stage, in_ntt ? 1 : 0, err), "import");
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, err, 8, hipMemcpyDeviceToHost, k.s), "hipMemcpy D2H");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  if (bad != ~0ull) {
    const size_t n = b->ctx->t->n;
    const size_t ch = (size_t)((bad / n) % b->ctx->L);
    // device data is now partially written; the reference returns Err and
    // builds no polynomial, so zero the buffer to keep it well-defined.
    cleanup(hipMemsetAsync(b->data, 0, words * word_bytes(k.t), k.s), "hipMemsetAsync(rejected upload)");
    cleanup(hipStreamSynchronize(k.s), "hipStreamSynchronize(rejected upload)");
    b->in_ntt = 0;
    return fail_fields(RNT_ERR_NON_REDUCED, host[bad], b->ctx->t->moduli[ch],
                       "coefficient %" PRIu64 " is not reduced modulo %" PRIu64, host[bad],
                       b->ctx->t->moduli[ch]);
  }
  b->in_ntt = in_ntt ? 1 : 0;
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_upload_coeffs(rnt_buf* b, const int64_t* coeffs, size_t n_polys) {
  if (int rc = check_buf(b, "rnt_upload_coeffs")) return rc;
  if (!coeffs) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_upload_coeffs: null pointer");
  if (n_polys != b->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_upload_coeffs: buffer holds %zu polys, got %zu",
                b->n_polys, n_polys);
  if (int rc = set_device(b->ctx)) return rc;
  rnt::Launch k = launch_for(b);
  const size_t words = n_polys * b->ctx->t->n;
  if (int rc = ensure_stage(b, words * 8)) return rc;
  HIP_TRY(hipMemcpyAsync(b->stage, coeffs, words * 8, hipMemcpyHostToDevice, k.s), "hipMemcpy H2D");
  LAUNCH(k.t, rnt::K_IMPORT, rnt::launch_import_coeffs(k, b->data, (const int64_t*)b->stage), "import_coeffs");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  b->in_ntt = 0;
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_download(const rnt_buf* cb, uint64_t* host, size_t n_polys) {
  rnt_buf* b = const_cast<rnt_buf*>(cb);  // staging only; contents unchanged
  if (int rc = check_buf(b, "rnt_download")) return rc;
  if (!host) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_download: null host pointer");
  if (n_polys != b->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_download: buffer holds %zu polys, got %zu", b->n_polys,
                n_polys);
  if (int rc = set_device(b->ctx)) return rc;
  rnt::Launch k = launch_for(b);
  const size_t words = poly_words(b);
  if (int rc = ensure_stage(b, words * 8)) return rc;
  LAUNCH(k.t, rnt::K_EXPORT, rnt::launch_export(k, (uint64_t*)b->stage, b->data, b->in_ntt), "export");
  HIP_TRY(hipMemcpyAsync(host, b->stage, words * 8, hipMemcpyDeviceToHost, k.s), "hipMemcpy D2H");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_download_polys(const rnt_buf* cb, uint64_t* host, size_t first, size_t count) {
  rnt_buf* b = const_cast<rnt_buf*>(cb);  // staging only; contents unchanged
  if (int rc = check_buf(b, "rnt_download_polys")) return rc;
  if (!host) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_download_polys: null host pointer");
  if (first > b->n_polys || count > b->n_polys - first)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_download_polys: polys [%zu, %zu) outside a batch of %zu",
                first, first + count, b->n_polys);
  if (count == 0) return RNT_OK;
  if (int rc = set_device(b->ctx)) return rc;
  rnt::Launch k = launch_for(b);
  k.B = count;
  const size_t n = k.t->n, words = count * b->ctx->L * n;
  if (int rc = ensure_stage(b, words * 8)) return rc;
  const char* src = (const char*)b->data + first * n * word_bytes(k.t);
  LAUNCH(k.t, rnt::K_EXPORT, rnt::launch_export(k, (uint64_t*)b->stage, src, b->in_ntt, limb_stride(b)),
         "export");
  HIP_TRY(hipMemcpyAsync(host, b->stage, words * 8, hipMemcpyDeviceToHost, k.s), "hipMemcpy D2H");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_copy(rnt_buf* dst, const rnt_buf* src) {
  if (int rc = check_buf(dst, "rnt_copy")) return rc;
  if (int rc = check_buf(src, "rnt_copy")) return rc;
  if (int rc = check_same(dst, src, "rnt_copy")) return rc;
  if (dst == src) return RNT_OK;
  if (int rc = set_device(dst->ctx)) return rc;
  rnt::Launch k = launch_for(dst);
  const uint64_t bytes = poly_words(src) * word_bytes(k.t);
  if (bytes % 16 == 0 && ((uintptr_t)dst->data | (uintptr_t)src->data) % 16 == 0) {
    // a 16-byte-per-lane copy kernel: 6.0+ TB/s against hipMemcpyAsync's
    // 4.6 (bench.py's stream_copy_GBs times this)
    LAUNCH(k.t, rnt::K_COPY, rnt::launch_copy(k.s, dst->data, src->data, bytes), "copy");
  } else {
    HIP_TRY(hipMemcpyAsync(dst->data, src->data, bytes, hipMemcpyDeviceToDevice, k.s),
            "hipMemcpyAsync");
  }
  dst->in_ntt = src->in_ntt;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// ring ops
// ---------------------------------------------------------------------------
extern "C" int rnt_ntt_fwd(rnt_buf* b) {
  if (int rc = check_buf(b, "rnt_ntt_fwd")) return rc;
  if (b->in_ntt) return RNT_OK;  // poly.rs:137-139
  if (int rc = set_device(b->ctx)) return rc;
  rnt::Launch k = launch_for(b);
  const uint64_t ls = limb_stride(b);
  if (use_mf(k)) {
    // N = 2^16, u32 bases: the whole-plane MFMA transform (rnt_mfma.hip)
    LAUNCH(k.t, rnt::K_MF_NTT_FWD, rnt::launch_mf_ntt(k, 0, b->data, ls), "MFMA forward transform");
  } else if (rnt::whole_ok(k.t, 0)) {
    // 2^10 <= N <= 2^14: the whole transform in one row launch
    LAUNCH(k.t, rnt::K_WHOLE_FWD, rnt::launch_whole(k, 0, b->data, b->data, nullptr, ls), "whole-plane forward");
  } else {
    LAUNCH(k.t, rnt::K_COL_FWD, rnt::launch_col_fwd(k, b->data, b->data, nullptr, nullptr, ls, ls),
           "column forward");
    LAUNCH(k.t, rnt::K_ROW_FWD, rnt::launch_row(k, 0, b->data, nullptr, ls), "row forward");
  }
  b->in_ntt = 1;
  return RNT_OK;
}

extern "C" int rnt_ntt_inv(rnt_buf* b) {
  if (int rc = check_buf(b, "rnt_ntt_inv")) return rc;
  if (!b->in_ntt) return RNT_OK;  // poly.rs:155-157
  if (int rc = set_device(b->ctx)) return rc;
  if (int rc = to_coeff_into(b, b->data)) return rc;
  b->in_ntt = 0;
  return RNT_OK;
}

static long env_long(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}

extern "C" int rnt_mul(rnt_buf* out, const rnt_buf* a, const rnt_buf* b) {
  if (int rc = check_buf(out, "rnt_mul")) return rc;
  if (int rc = check_buf(a, "rnt_mul")) return rc;
  if (int rc = check_buf(b, "rnt_mul")) return rc;
  if (int rc = check_same(a, b, "rnt_mul")) return rc;
  if (int rc = check_same(out, a, "rnt_mul")) return rc;
  if (a->in_ntt != b->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "mul_assign: domain mismatch (both must be in the same domain)");
  if (int rc = set_device(out->ctx)) return rc;
  rnt::Launch k = launch_for(out);
  if (a->in_ntt) {  // poly.rs:297-306
    LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(k, 3, out->data, a->data, b->data), "pointwise mul");
    out->in_ntt = 1;
    return RNT_OK;
  }
  // poly.rs:307-329: fwd(a), fwd(b), pointwise, inv -- three fused launches
  // over the whole batch: column passes of both operands (b's into the
  // workspace), the row kernel (both forward row passes, Montgomery
  // pointwise product, inverse rows), the inverse column pass.
  const uint64_t ls = limb_stride(out);
  if (rnt::whole_ok(k.t, 2)) {
    // 2^10 <= N <= 2^14: both transforms, the product and the inverse in
    // one row launch, 3 planes per (poly, limb)
    LAUNCH(k.t, rnt::K_WHOLE_MUL, rnt::launch_whole(k, 2, out->data, a->data, b->data, ls), "whole-plane product");
    out->in_ntt = 0;
    return RNT_OK;
  }
  if (rnt::plane_ok(k.t)) {
    const uint64_t planes = rnt::plane_scratch_planes((uint64_t)k.B * k.L);
    if (int rc = ensure_ws(out, planes * k.t->n * 4)) return rc;
    if (k.t->mf_mul && use_mf(k))
      LAUNCH(k.t, rnt::K_MF_MUL, rnt::launch_mf_mul(k, out->data, a->data, b->data, ls, out->ws),
             "matrix-core product");
    else
      LAUNCH(k.t, rnt::K_PLANE_FUSED, rnt::launch_plane_fused(k, out->data, a->data, b->data, out->ws, ls),
             "plane fused product");
    out->in_ntt = 0;
    return RNT_OK;
  }
  if (int rc = ensure_ws(out, poly_words(out) * word_bytes(k.t))) return rc;
  // lazy: the Harvey variant when every q < 2^30 (u32, Tables::lazy30) or
  // every q < 2^62 (u64, Tables::lazy62)
  LAUNCH(k.t, rnt::K_COL_FWD, rnt::launch_col_fwd(k, out->data, a->data, out->ws, b->data, ls, ls, true),
         "column forward");
  LAUNCH(k.t, rnt::K_ROW_MUL, rnt::launch_row(k, 2, out->data, out->ws, ls, true), "row mul");
  LAUNCH(k.t, rnt::K_COL_INV,
         rnt::launch_col_inv(k, out->data, ls, out->data, ls, rnt::mul_truncated(k.t) ? 2 : 1, nullptr, true),
         "column inverse");
  out->in_ntt = 0;
  return RNT_OK;
}

static int binary_elementwise(rnt_buf* out, const rnt_buf* a, const rnt_buf* b, int op,
                              const char* name) {
  if (int rc = check_buf(out, name)) return rc;
  if (int rc = check_buf(a, name)) return rc;
  if (int rc = check_buf(b, name)) return rc;
  if (int rc = check_same(a, b, name)) return rc;
  if (int rc = check_same(out, a, name)) return rc;
  if (a->in_ntt != b->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: domain mismatch", name);
  if (int rc = set_device(out->ctx)) return rc;
  rnt::Launch k = launch_for(out);
  LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(k, op, out->data, a->data, b->data), name);
  out->in_ntt = a->in_ntt;
  return RNT_OK;
}

extern "C" int rnt_add(rnt_buf* out, const rnt_buf* a, const rnt_buf* b) {
  return binary_elementwise(out, a, b, 0, "add_assign");
}
extern "C" int rnt_sub(rnt_buf* out, const rnt_buf* a, const rnt_buf* b) {
  return binary_elementwise(out, a, b, 1, "sub");
}
extern "C" int rnt_neg(rnt_buf* out, const rnt_buf* a) {
  if (int rc = check_buf(out, "rnt_neg")) return rc;
  if (int rc = check_buf(a, "rnt_neg")) return rc;
  if (int rc = check_same(out, a, "rnt_neg")) return rc;
  if (int rc = set_device(out->ctx)) return rc;
  rnt::Launch k = launch_for(out);
  LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(k, 2, out->data, a->data, nullptr), "neg");
  out->in_ntt = a->in_ntt;
  return RNT_OK;
}

extern "C" int rnt_rescale(rnt_buf* out, const rnt_buf* in) {
  if (int rc = check_buf(out, "rnt_rescale")) return rc;
  if (int rc = check_buf(in, "rnt_rescale")) return rc;
  const size_t L = in->ctx->L;
  if (L < 2)  // poly.rs:191-197
    return fail_fields(RNT_ERR_INVALID_MOD_DROP, 1, L, "invalid mod-drop count 1 for %zu channels", L);
  if (out->ctx->t != in->ctx->t || out->ctx->L != L - 1)
    return fail(RNT_ERR_BASIS_MISMATCH, "rescale: output basis is not drop_last(1) of the input's");
  if (out->n_polys != in->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "rescale: batch sizes differ");
  if (int rc = set_device(in->ctx)) return rc;
  rnt::Launch k = launch_for(in);
  const void* src = in->data;
  if (in->in_ntt) {  // poly.rs:199-210: clone + to_coeff_domain
    if (int rc = ensure_ws(out, poly_words(in) * word_bytes(k.t))) return rc;
    if (int rc = to_coeff_into(in, out->ws)) return rc;
    src = out->ws;
  }
  LAUNCH(k.t, rnt::K_RESCALE, rnt::launch_rescale(k, out->data, src), "rescale");
  out->in_ntt = 0;
  return RNT_OK;
}

// Device constants {inv[L], invp[L]} for rescaling by an external modulus.
static int resc_ext_table(const rnt_ctx* ctx, uint64_t q_last, const void** inv, const void** invp) {
  rnt::Tables* t = ctx->t.get();
  const size_t Lr = t->L;  // table covers every limb of the root basis
  std::lock_guard<std::mutex> g(t->resc_mu);
  for (auto& e : t->resc_ext)
    if (e.first == q_last) {
      *inv = e.second;
      *invp = (const char*)e.second + Lr * word_bytes(t);
      return RNT_OK;
    }
  const unsigned wbits = t->wide ? 64 : 32;
  std::vector<uint64_t> h(2 * Lr);
  for (size_t l = 0; l < Lr; ++l) {
    const uint64_t ql = t->moduli[l];
    if (ql == q_last) {  // the limb being dropped: never read
      h[l] = h[Lr + l] = 0;
      continue;
    }
    const uint64_t v = rnt::host::invmod(q_last % ql, ql);
    if (v == 0)
      return fail(RNT_ERR_BAD_ARGUMENT, "rescale: modulus %" PRIu64 " is not coprime to %" PRIu64, q_last, ql);
    h[l] = v;
    h[Lr + l] = rnt::host::shoup_companion(v, ql, wbits);
  }
  void* d = nullptr;
  const size_t wb = word_bytes(t);
  HIP_TRY(hipMalloc(&d, 2 * Lr * wb), "hipMalloc(rescale constants)");
  if (wb == 4) {
    std::vector<uint32_t> h32(h.begin(), h.end());
    HIP_TRY(hipMemcpy(d, h32.data(), 2 * Lr * 4, hipMemcpyHostToDevice), "hipMemcpy");
  } else {
    HIP_TRY(hipMemcpy(d, h.data(), 2 * Lr * 8, hipMemcpyHostToDevice), "hipMemcpy");
  }
  t->resc_ext.push_back({q_last, d});
  *inv = d;
  *invp = (const char*)d + Lr * wb;
  return RNT_OK;
}

extern "C" int rnt_rescale_ext(rnt_buf* out, const rnt_buf* in, const void* last_limb,
                               uint64_t q_last) {
  if (int rc = check_buf(out, "rnt_rescale_ext")) return rc;
  if (int rc = check_buf(in, "rnt_rescale_ext")) return rc;
  if (!last_limb) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_rescale_ext: null last limb");
  if (in->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_rescale_ext: input must be in coefficient domain");
  const size_t L = in->ctx->L;
  const rnt::Tables* t = in->ctx->t.get();
  // the owner of q_last drops it; every other shard keeps all its limbs
  const size_t keep = (L > 0 && t->moduli[L - 1] == q_last) ? L - 1 : L;
  if (keep == 0)
    return fail_fields(RNT_ERR_INVALID_MOD_DROP, 1, L, "rescale: nothing left after dropping the last limb");
  if (out->ctx->t != in->ctx->t || out->ctx->L != keep)
    return fail(RNT_ERR_BASIS_MISMATCH, "rnt_rescale_ext: output basis must keep %zu limbs of the input's", keep);
  if (out->n_polys != in->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_rescale_ext: batch sizes differ");
  if (int rc = set_device(in->ctx)) return rc;
  const void* inv = nullptr;
  const void* invp = nullptr;
  if (int rc = resc_ext_table(in->ctx, q_last, &inv, &invp)) return rc;
  rnt::Launch k = launch_for(in);
  k.L = keep;
  LAUNCH(k.t, rnt::K_RESCALE, rnt::launch_rescale_ext(k, out->data, in->data, last_limb, inv, invp),
         "rescale_ext");
  out->in_ntt = 0;
  return RNT_OK;
}

// ---- decode-side CRT (basis.rs:158-180, poly.rs:404-427) ----------------

namespace {

// Little-endian 32-bit-word big integers for the host-side constants.
using Big = std::vector<uint32_t>;
void big_mul_small(Big& a, uint64_t m) {
  // a *= m (m < 2^64), growing a
  const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
  Big r(a.size() + 2, 0);
  for (int half = 0; half < 2; ++half) {
    const uint64_t f = half ? mhi : mlo;
    if (!f) continue;
    uint64_t carry = 0;
    for (size_t w = 0; w < a.size(); ++w) {
      const uint64_t t = (uint64_t)a[w] * f + r[w + half] + carry;
      r[w + half] = (uint32_t)t;
      carry = t >> 32;
    }
    for (size_t w = a.size() + half; carry && w < r.size(); ++w) {
      const uint64_t t = (uint64_t)r[w] + carry;
      r[w] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  while (r.size() > 1 && r.back() == 0) r.pop_back();
  a.swap(r);
}

}  // namespace

// Constants of the centred CRT for the first L limbs of a basis, cached per
// (tables, L): device block {qi_words[L][MW], q[MW], qh[MW], inv[L],
// inv_p[L], rq[L]} and the CrtConsts pointing into it.
static int crt_tables(const rnt_ctx* ctx, const void** consts, uint32_t* mw_out) {
  rnt::Tables* t = ctx->t.get();
  const size_t L = ctx->L;
  std::lock_guard<std::mutex> g(t->resc_mu);
  for (auto& e : t->crt_cache)
    if (e.first == L) {
      *consts = &e.second.cc;
      *mw_out = e.second.mw;
      return RNT_OK;
    }
  Big Q{1};
  for (size_t l = 0; l < L; ++l) big_mul_small(Q, t->moduli[l]);
  uint32_t mw = 4;
  while (mw < Q.size()) mw *= 2;
  if (mw > 128) return fail(RNT_ERR_BAD_ARGUMENT, "CRT: Q has %zu 32-bit words (max 128)", Q.size());
  std::vector<uint32_t> qi(L * mw, 0), qw(mw, 0), qh(mw, 0);
  std::vector<uint64_t> inv(L), invp(L);
  std::vector<double> rq(L);
  const unsigned wbits = t->wide ? 64 : 32;
  for (size_t l = 0; l < L; ++l) {
    Big Ql{1};
    uint64_t ql_mod = 1;  // (Q/q_l) mod q_l
    for (size_t m = 0; m < L; ++m) {
      if (m == l) continue;
      big_mul_small(Ql, t->moduli[m]);
      ql_mod = rnt::host::mulmod(ql_mod, t->moduli[m] % t->moduli[l], t->moduli[l]);
    }
    for (size_t w = 0; w < Ql.size() && w < mw; ++w) qi[l * mw + w] = Ql[w];
    inv[l] = rnt::host::invmod(ql_mod, t->moduli[l]);
    if (inv[l] == 0 && L > 1)
      return fail(RNT_ERR_BAD_ARGUMENT, "CRT: moduli are not pairwise coprime");
    if (L == 1) inv[l] = 1;
    invp[l] = rnt::host::shoup_companion(inv[l], t->moduli[l], wbits);
    rq[l] = 1.0 / (double)t->moduli[l];
  }
  for (size_t w = 0; w < Q.size(); ++w) qw[w] = Q[w];
  for (size_t w = 0; w < mw; ++w) qh[w] = (qw[w] >> 1) | (w + 1 < mw ? qw[w + 1] << 31 : 0);
  const size_t bytes = (L * mw + 2 * mw) * 4 + L * 8 * 2 + L * 8;
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes), "hipMalloc(CRT constants)");
  std::vector<unsigned char> h(bytes);
  size_t off = 0;
  auto put = [&](const void* src, size_t n) {
    memcpy(h.data() + off, src, n);
    off += n;
  };
  rnt::CrtDev cd;
  cd.dev = d;
  cd.mw = mw;
  cd.cc.qi_words = (const uint32_t*)((char*)d + off);
  put(qi.data(), qi.size() * 4);
  cd.cc.q_words = (const uint32_t*)((char*)d + off);
  put(qw.data(), mw * 4);
  cd.cc.qh_words = (const uint32_t*)((char*)d + off);
  put(qh.data(), mw * 4);
  cd.cc.inv = (const uint64_t*)((char*)d + off);
  put(inv.data(), L * 8);
  cd.cc.inv_p = (const uint64_t*)((char*)d + off);
  put(invp.data(), L * 8);
  cd.cc.rq = (const double*)((char*)d + off);
  put(rq.data(), L * 8);
  HIP_TRY(hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy(CRT constants)");
  t->crt_cache.push_back({L, cd});
  *consts = &t->crt_cache.back().second.cc;
  *mw_out = mw;
  return RNT_OK;
}

static int crt_download(const rnt_buf* cb, uint64_t* host, size_t n_polys, size_t out_words,
                        const char* name) {
  rnt_buf* b = const_cast<rnt_buf*>(cb);  // workspace / staging only
  if (int rc = check_buf(b, name)) return rc;
  if (!host) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null host pointer", name);
  if (n_polys != b->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: buffer holds %zu polys, got %zu", name, b->n_polys, n_polys);
  if (out_words == 0 || out_words > 64) return fail(RNT_ERR_BAD_ARGUMENT, "%s: 1..64 words", name);
  if (int rc = set_device(b->ctx)) return rc;
  const void* consts = nullptr;
  uint32_t mw = 0;
  if (int rc = crt_tables(b->ctx, &consts, &mw)) return rc;
  rnt::Launch k = launch_for(b);
  const void* src = b->data;
  if (b->in_ntt) {  // poly.rs:408-417: a coefficient-domain clone
    if (int rc = ensure_ws(b, poly_words(b) * word_bytes(k.t))) return rc;
    if (int rc = to_coeff_into(b, b->ws)) return rc;
    src = b->ws;
  }
  const size_t coeffs = b->n_polys * k.t->n;
  if (int rc = ensure_stage(b, coeffs * out_words * 8)) return rc;
  LAUNCH(k.t, rnt::K_CRT, rnt::launch_crt(k, (uint64_t*)b->stage, src, consts, mw, (uint32_t)out_words),
         "crt");
  HIP_TRY(hipMemcpyAsync(host, b->stage, coeffs * out_words * 8, hipMemcpyDeviceToHost, k.s),
          "hipMemcpy D2H");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_to_coeffs(const rnt_buf* buf, int64_t* host, size_t n_polys) {
  return crt_download(buf, (uint64_t*)host, n_polys, 1, "rnt_to_coeffs");
}

extern "C" int rnt_crt_centered(const rnt_buf* buf, uint64_t* host, size_t n_polys, size_t words) {
  return crt_download(buf, host, n_polys, words, "rnt_crt_centered");
}

// ---------------------------------------------------------------------------
// samplers (PolySampler, traits.rs:74-127; rnt_sample.hip)
// ---------------------------------------------------------------------------
static int sample_into(rnt_buf* out, int kind, double sigma, size_t h, uint64_t seed,
                       uint64_t stream, const char* name) {
  if (int rc = set_device(out->ctx)) return rc;
  rnt::Launch k = launch_for(out);
  rnt::SampleKey s;
  s.k0 = (uint32_t)seed;
  s.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(stream >> 32);
  s.stream = (uint32_t)stream;
  LAUNCH(k.t, rnt::K_SAMPLE, rnt::launch_sample(k, kind, out->data, s, sigma, (uint32_t)h), name);
  out->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_sample_uniform(rnt_buf* out, uint64_t seed, uint64_t stream) {
  if (int rc = check_buf(out, "rnt_sample_uniform")) return rc;
  return sample_into(out, 0, 0.0, 0, seed, stream, "sample_uniform");
}

extern "C" int rnt_sample_gaussian(rnt_buf* out, double std_dev, uint64_t seed, uint64_t stream) {
  if (int rc = check_buf(out, "rnt_sample_gaussian")) return rc;
  // poly.rs:452-453 / sampling.rs:31-45 panic on these
  if (!(std_dev > 0.0) || !std::isfinite(std_dev))
    return fail(RNT_ERR_BAD_ARGUMENT, "sample_gaussian: std_dev must be finite and positive");
  return sample_into(out, 1, std_dev, 0, seed, stream, "sample_gaussian");
}

extern "C" int rnt_sample_ternary(rnt_buf* out, size_t hamming_weight, uint64_t seed,
                                  uint64_t stream) {
  if (int rc = check_buf(out, "rnt_sample_ternary")) return rc;
  // sampling.rs:71-80 panics on an oversized Hamming weight
  if (hamming_weight > out->ctx->t->n)
    return fail(RNT_ERR_BAD_ARGUMENT, "sample_tribits: hamming weight %zu exceeds degree %zu",
                hamming_weight, out->ctx->t->n);
  return sample_into(out, 2, 0.0, hamming_weight, seed, stream, "sample_tribits");
}

// ---------------------------------------------------------------------------
// CKKS encoder / decoder (ckks_encoder.rs:85-156, special_fft.rs; the
// special FFT in rnt_encode.hip)
// ---------------------------------------------------------------------------
static int sfft_table(const rnt_ctx* ctx, const void** tab) {
  rnt::Tables* t = ctx->t.get();
  std::lock_guard<std::mutex> g(t->sfft_mu);
  if (!t->sfft_tw) {
    const std::vector<double> h = rnt::sfft_twiddles(t->log_n);
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, h.size() * sizeof(double)), "hipMalloc(sfft twiddles)");
    const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      cleanup(hipFree(d), "hipFree(sfft twiddles)");
      return hip_fail(e, "hipMemcpy(sfft twiddles)");
    }
    t->sfft_tw = d;
  }
  *tab = t->sfft_tw;
  return RNT_OK;
}

static int sfft_check(const rnt_buf* b, const double* values, size_t n_values,
                      uint32_t scale_bits, const char* name) {
  if (int rc = check_buf(b, name)) return rc;
  const size_t n = b->ctx->t->n;
  if (!rnt::sfft_supported(b->ctx->t->log_n))
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: degree %zu has no slots", name, n);
  // ckks_encoder.rs:70-75 (a panic in the reference)
  if (n_values > n / 2)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: %zu values exceed max slots %zu", name, n_values, n / 2);
  if (n_values && b->n_polys && !values) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null values", name);
  // ckks_encoder.rs:43 asserts scale_bits > 0; 2^scale_bits must be a finite f64
  if (scale_bits == 0 || scale_bits > 1000)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: scale_bits must be in [1, 1000], got %u", name, scale_bits);
  return RNT_OK;
}

extern "C" int rnt_encode(rnt_buf* out, const double* values, size_t n_values, uint32_t scale_bits) {
  if (int rc = sfft_check(out, values, n_values, scale_bits, "rnt_encode")) return rc;
  if (int rc = set_device(out->ctx)) return rc;
  const void* tw = nullptr;
  if (int rc = sfft_table(out->ctx, &tw)) return rc;
  rnt::Launch k = launch_for(out);
  const size_t B = out->n_polys, n = k.t->n;
  if (B == 0) {
    out->in_ntt = 0;
    return RNT_OK;
  }
  // stage: the slot values in, then the rounded i64 coefficients;
  // ws: [B][N/2] complex working planes
  if (int rc = ensure_stage(out, B * n * 8)) return rc;
  if (int rc = ensure_ws(out, B * n * 8)) return rc;
  if (n_values)
    HIP_TRY(hipMemcpyAsync(out->stage, values, B * n_values * 16, hipMemcpyHostToDevice, k.s),
            "hipMemcpy H2D");
  LAUNCH(k.t, rnt::K_SFFT,
         rnt::launch_sfft_encode(k, (int64_t*)out->stage, out->ws, out->stage, (uint32_t)n_values,
                                 scale_bits, tw),
         "special fft (encode)");
  LAUNCH(k.t, rnt::K_IMPORT, rnt::launch_import_coeffs(k, out->data, (const int64_t*)out->stage),
         "import_coeffs");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  out->in_ntt = 0;
  trim_stage(out);
  return RNT_OK;
}

extern "C" int rnt_decode(const rnt_buf* cb, double* values, size_t n_values, uint32_t scale_bits) {
  rnt_buf* b = const_cast<rnt_buf*>(cb);  // workspace / staging only
  if (int rc = sfft_check(b, values, n_values, scale_bits, "rnt_decode")) return rc;
  if (int rc = set_device(b->ctx)) return rc;
  const void* tw = nullptr;
  if (int rc = sfft_table(b->ctx, &tw)) return rc;
  const void* consts = nullptr;
  uint32_t mw = 0;
  if (int rc = crt_tables(b->ctx, &consts, &mw)) return rc;
  rnt::Launch k = launch_for(b);
  const size_t B = b->n_polys, n = k.t->n;
  if (B == 0 || n_values == 0) return RNT_OK;
  // ws holds the coefficient-domain clone of an NTT-domain input, then the
  // complex planes; stage the centred i64 coefficients (to_coeffs)
  if (int rc = ensure_ws(b, std::max(poly_words(b) * word_bytes(k.t), B * n * 8))) return rc;
  if (int rc = ensure_stage(b, B * n * 8)) return rc;
  const void* src = b->data;
  if (b->in_ntt) {  // poly.rs:408-417: a coefficient-domain clone
    if (int rc = to_coeff_into(b, b->ws)) return rc;
    src = b->ws;
  }
  LAUNCH(k.t, rnt::K_CRT, rnt::launch_crt(k, (uint64_t*)b->stage, src, consts, mw, 1), "crt");
  LAUNCH(k.t, rnt::K_SFFT,
         rnt::launch_sfft_decode(k, b->ws, (const int64_t*)b->stage, scale_bits, tw),
         "special fft (decode)");
  HIP_TRY(hipMemcpy2DAsync(values, n_values * 16, b->ws, (n / 2) * 16, n_values * 16, B,
                           hipMemcpyDeviceToHost, k.s),
          "hipMemcpy2D D2H");
  HIP_TRY(hipStreamSynchronize(k.s), "hipStreamSynchronize");
  trim_stage(b);
  return RNT_OK;
}

extern "C" int rnt_mod_drop_last(rnt_buf* out, const rnt_buf* in) {
  if (int rc = check_buf(out, "rnt_mod_drop_last")) return rc;
  if (int rc = check_buf(in, "rnt_mod_drop_last")) return rc;
  if (out->ctx->t != in->ctx->t || out->ctx->L > in->ctx->L)
    return fail(RNT_ERR_BASIS_MISMATCH, "mod_drop_last: output basis is not a prefix of the input's");
  if (out->n_polys != in->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "mod_drop_last: batch sizes differ");
  if (int rc = set_device(in->ctx)) return rc;
  rnt::Launch k = launch_for(out);
  // [L][B][N]: the kept channels are a contiguous prefix
  if (out != in)
    HIP_TRY(hipMemcpyAsync(out->data, in->data, poly_words(out) * word_bytes(k.t),
                           hipMemcpyDeviceToDevice, k.s),
            "hipMemcpyAsync");
  out->in_ntt = in->in_ntt;
  return RNT_OK;
}

extern "C" int rnt_automorphism(rnt_buf* out, const rnt_buf* in, uint64_t g) {
  if (int rc = check_buf(out, "rnt_automorphism")) return rc;
  if (int rc = check_buf(in, "rnt_automorphism")) return rc;
  if (int rc = check_same(out, in, "rnt_automorphism")) return rc;
  if (int rc = set_device(in->ctx)) return rc;
  rnt::Launch k = launch_for(in);
  const uint64_t two_n = 2 * (uint64_t)k.t->n;
  if (g % two_n == 0) return rnt_copy(out, in);  // poly.rs:508-511: self.clone()
  const void* src = in->data;
  if (in->in_ntt || out == in) {
    if (int rc = ensure_ws(out, poly_words(in) * word_bytes(k.t))) return rc;
    if (in->in_ntt) {
      if (int rc = to_coeff_into(in, out->ws)) return rc;
    } else {
      HIP_TRY(hipMemcpyAsync(out->ws, in->data, poly_words(in) * word_bytes(k.t),
                             hipMemcpyDeviceToDevice, k.s),
              "hipMemcpyAsync");
    }
    src = out->ws;
  }
  LAUNCH(k.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(k, out->data, src, g), "automorphism");
  out->in_ntt = 0;
  return RNT_OK;
}

static uint64_t rotation_exponent(int32_t k, uint64_t two_n) {
  // poly.rs:546-569: 5^|k| mod 2N, and for k < 0 the composition with
  // X -> X^(2N-1): both are odd, so the two automorphisms compose exactly
  // into one with exponent 5^|k| * (2N-1) mod 2N.
  const uint64_t r = k >= 0 ? (uint64_t)k : (uint64_t)(-(int64_t)k);
  uint64_t e = rnt::host::powmod(5, r, two_n);
  if (k < 0) e = rnt::host::mulmod(e, two_n - 1, two_n);
  return e;
}

extern "C" int rnt_rotate_slots(rnt_buf* out, const rnt_buf* in, int32_t k) {
  if (int rc = check_buf(in, "rnt_rotate_slots")) return rc;
  return rnt_automorphism(out, in, rotation_exponent(k, 2 * (uint64_t)in->ctx->t->n));
}

extern "C" int rnt_automorphism_ntt(rnt_buf* out, const rnt_buf* in, uint64_t g) {
  const char* name = "rnt_automorphism_ntt";
  if (int rc = check_buf(out, name)) return rc;
  if (int rc = check_buf(in, name)) return rc;
  if (int rc = check_same(out, in, name)) return rc;
  if (!in->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the input must be in the NTT domain", name);
  if ((g & 1) == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: the exponent must be odd, got %" PRIu64, name, g);
  if (out == in || out->data == in->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out aliases in", name);
  if (int rc = set_device(in->ctx)) return rc;
  rnt::Launch k = launch_for(in);
  LAUNCH(k.t, rnt::K_AUTOMORPH_NTT, rnt::launch_automorphism_ntt(k, out->data, in->data, g),
         "automorphism in the NTT domain");
  out->in_ntt = 1;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// ModRaise and the monomial product (rnt_raise.hip)
// ---------------------------------------------------------------------------
// a / m for a little-endian a of 32-bit words, in place; returns a mod m.
static uint64_t big_divmod_small(Big& a, uint64_t m) {
  rnt::host::u128 rem = 0;
  for (size_t w = a.size(); w-- > 0;) {
    rem = (rem << 32) | a[w];
    a[w] = (uint32_t)(rem / m);  // rem < m before the shift: the quotient fits a word
    rem %= m;
  }
  return (uint64_t)rem;
}

// The constants of a raise from the first l0 limbs of `t` onto all of it,
// cached on the tables per l0 (they depend on nothing else: the input basis
// has those l0 moduli by value).  The first use allocates and copies, so it
// cannot be recorded into a graph (one un-recorded run first).
static int raise_tables(rnt::Tables* t, size_t l0, rnt::RaiseConsts* out) {
  std::lock_guard<std::mutex> g(t->resc_mu);
  for (auto& e : t->raise_cache)
    if (e.l0 == l0) {
      *out = e.rc;
      return RNT_OK;
    }
  const size_t L = t->L, M = rnt::kRaiseMax;
  const unsigned wbits = t->wide ? 64 : 32;
  const std::vector<uint64_t>& q = t->moduli;
  std::vector<uint64_t> h(L * (2 * M + 1), 0);  // rad[L][M], radp[L][M], q0m[L]
  for (size_t j = 0; j < L; ++j) {
    uint64_t r = 1 % q[j];
    for (size_t i = 0; i < l0; ++i) {
      h[j * M + i] = r;
      h[L * M + j * M + i] = rnt::host::shoup_companion(r, q[j], wbits);
      r = rnt::host::mulmod(r, q[i] % q[j], q[j]);
    }
    h[2 * L * M + j] = r;
  }
  rnt::RaiseDev rd;
  rd.l0 = l0;
  for (size_t i = 1; i < l0; ++i) {
    for (size_t k = 0; k < i; ++k) {
      rd.rc.g.pre[i][k] = h[i * M + k];
      rd.rc.g.prep[i][k] = h[L * M + i * M + k];
    }
    rd.rc.g.ginv[i] = rnt::host::invmod(h[i * M + i], q[i]);
    if (rd.rc.g.ginv[i] == 0) return fail(RNT_ERR_BAD_ARGUMENT, "mod_raise: the moduli are not pairwise coprime");
    rd.rc.g.ginvp[i] = rnt::host::shoup_companion(rd.rc.g.ginv[i], q[i], wbits);
  }
  Big half{1};
  for (size_t i = 0; i < l0; ++i) big_mul_small(half, q[i]);
  for (size_t w = 0; w < half.size(); ++w)  // floor(Q0 / 2)
    half[w] = (half[w] >> 1) | (w + 1 < half.size() ? half[w + 1] << 31 : 0);
  for (size_t i = 0; i < l0; ++i) rd.rc.g.half[i] = big_divmod_small(half, q[i]);
  const size_t wb = word_bytes(t);
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, h.size() * wb), "hipMalloc(mod_raise constants)");
  hipError_t e;
  if (wb == 4) {
    std::vector<uint32_t> h32(h.begin(), h.end());
    e = hipMemcpy(d, h32.data(), h.size() * 4, hipMemcpyHostToDevice);
  } else {
    e = hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    cleanup(hipFree(d), "hipFree(mod_raise constants)");
    return hip_fail(e, "hipMemcpy(mod_raise constants)");
  }
  rd.dev = d;
  rd.rc.rad = d;
  rd.rc.radp = (const char*)d + L * M * wb;
  rd.rc.q0m = (const char*)d + 2 * L * M * wb;
  t->raise_cache.push_back(rd);
  *out = rd.rc;
  return RNT_OK;
}

extern "C" int rnt_mod_raise(rnt_buf* out, const rnt_buf* in) {
  if (int rc = check_buf(out, "rnt_mod_raise")) return rc;
  if (int rc = check_buf(in, "rnt_mod_raise")) return rc;
  rnt::Tables* tc = out->ctx->t.get();
  const rnt::Tables* t0 = in->ctx->t.get();
  const size_t l0 = in->ctx->L, L = out->ctx->L;
  if (t0->log_n != tc->log_n || t0->device != tc->device)
    return fail(RNT_ERR_BASIS_MISMATCH, "mod_raise: the two bases differ in degree or device");
  if (l0 >= L)
    return fail(RNT_ERR_BAD_ARGUMENT, "mod_raise: the input has %zu limbs, the output %zu (nothing to raise onto)", l0,
                L);
  for (size_t l = 0; l < l0; ++l)
    if (t0->moduli[l] != tc->moduli[l])
      return fail(RNT_ERR_BASIS_MISMATCH, "mod_raise: limb %zu of the input basis is %" PRIu64 ", the output's %" PRIu64,
                  l, t0->moduli[l], tc->moduli[l]);
  if (t0->wide != tc->wide)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "mod_raise: the two bases have different device word widths");
  if (l0 > rnt::kRaiseMax)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "mod_raise: %zu input limbs (at most %zu)", l0, rnt::kRaiseMax);
  if (out->n_polys != in->n_polys)
    return fail(RNT_ERR_BAD_ARGUMENT, "mod_raise: batch sizes differ (%zu vs %zu)", out->n_polys, in->n_polys);
  if (in->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "mod_raise: the input must be in the coefficient domain");
  if (int rc = set_device(out->ctx)) return rc;
  rnt::RaiseConsts rc;
  if (int r = raise_tables(tc, l0, &rc)) return r;
  if (t0 != tc && t0->stream != tc->stream && g_capture == nullptr) {
    // the input may still be in the making on its own basis' stream
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(mod_raise order)");
    hipError_t e = hipEventRecord(ev, t0->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(tc->stream, ev, 0);
    cleanup(hipEventDestroy(ev), "hipEventDestroy(mod_raise order)");
    HIP_TRY(e, "hipStreamWaitEvent(mod_raise order)");
  }
  rnt::Launch k = launch_for(out);
  LAUNCH(k.t, rnt::K_MOD_RAISE, rnt::launch_mod_raise(k, out->data, in->data, l0, rc), "mod_raise");
  out->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_mul_monomial(rnt_buf* out, const rnt_buf* in, int64_t k) {
  if (int rc = check_buf(out, "rnt_mul_monomial")) return rc;
  if (int rc = check_buf(in, "rnt_mul_monomial")) return rc;
  if (out == in) return fail(RNT_ERR_BAD_ARGUMENT, "mul_monomial: out and in are one buffer");
  if (int rc = check_same(out, in, "rnt_mul_monomial")) return rc;
  if (in->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "mul_monomial: the input must be in the coefficient domain");
  if (int rc = set_device(in->ctx)) return rc;
  rnt::Launch l = launch_for(in);
  const int64_t two_n = 2 * (int64_t)l.t->n;
  const uint64_t shift = (uint64_t)(((k % two_n) + two_n) % two_n);
  LAUNCH(l.t, rnt::K_MUL_MONOMIAL, rnt::launch_mul_monomial(l, out->data, in->data, shift), "mul_monomial");
  out->in_ntt = 0;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// key-switching
// ---------------------------------------------------------------------------
extern "C" int rnt_key_prepare(rnt_buf* key_a, rnt_buf* key_b) {
  if (int rc = check_buf(key_a, "rnt_key_prepare")) return rc;
  if (int rc = check_buf(key_b, "rnt_key_prepare")) return rc;
  if (int rc = check_same(key_a, key_b, "rnt_key_prepare")) return rc;
  // one poly per SOURCE limb: the basis' own channel count for rnt_keyswitch,
  // the global count for a limb shard's rnt_keyswitch_ext (checked there)
  if (key_a->n_polys != key_b->n_polys)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, key_a->n_polys, key_b->n_polys,
                       "gadget key halves differ: %zu vs %zu polys", key_a->n_polys, key_b->n_polys);
  if (int rc = rnt_ntt_fwd(key_a)) return rc;
  return rnt_ntt_fwd(key_b);
}

namespace {

// The key check of every gadget call: both halves are buffers of the basis
// `ctx`, hold `polys` polys each and are NTT-resident.  stage: "", or "baby " /
// "giant " of a two-stage call.
int check_key_set(const char* name, const char* stage, const rnt_ctx* ctx, const rnt_buf* keys_a,
                  const rnt_buf* keys_b, size_t polys) {
  if (int rc = check_buf(keys_a, name)) return rc;
  if (int rc = check_buf(keys_b, name)) return rc;
  if (keys_a->ctx != ctx || keys_b->ctx != ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the %skeys and the ciphertext belong to different bases", name, stage);
  if (keys_a->n_polys != polys || keys_b->n_polys != polys)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, polys, keys_a->n_polys != polys ? keys_a->n_polys : keys_b->n_polys,
                       "%s: the %skeys must hold one poly per step and source limb (%zu)", name, stage, polys);
  if (!keys_a->in_ntt || !keys_b->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH,
                "%s: the %skeys must be prepared (rnt_key_prepare; rnt_key_prepare_hoisted for a hoisted call)", name,
                stage);
  return RNT_OK;
}

// One gadget key as the kernels read it: the first plane of either half and
// the limb stride (words) of the buffers they stand in.  A key pair, or step t
// of a packed key set ([L][n_steps L][N]: the set's stride, t L planes in).
struct GadgetKey {
  const void *a, *b;
  uint64_t ls;
  GadgetKey(const rnt_buf* keys_a, const rnt_buf* keys_b, size_t t = 0) : ls(limb_stride(keys_a)) {
    const rnt::Tables* tb = keys_a->ctx->t.get();
    const size_t off = t * keys_a->ctx->L * tb->n * word_bytes(tb);
    a = (const char*)keys_a->data + off;
    b = (const char*)keys_b->data + off;
  }
};

// Polys per chunk of a batch of B within the key-switch workspace cap
// (RNT_KS_WS_MB), at `planes` planes of N words per poly; one poly is the floor.
// The key rows are read once per chunk from HBM (the batch hits them in cache,
// see row_pos_pfast), so bigger chunks cut key traffic per ciphertext; the
// default 4 GiB is a small slice of the 288 GB.
size_t chunk_polys(const rnt::Tables* t, size_t planes, size_t B) {
  return std::min(B, std::max<size_t>(t->ks_ws_bytes / (planes * t->n * word_bytes(t)), 1));
}
// The chunk of the calls whose whole layout is to fit the cap (the hybrid family, the plain MAC), set on the layout.
size_t fit_chunk(const rnt::Tables* t, rnt::WsLayout& w, size_t B) { return w.chunk(chunk_polys(t, w.planes, B)).bc; }

// The chunk of the calls that bound S ([L][L][Bc][N]) alone.  (The whole-plane
// key-switch has no S: its chunk is bounded by the ct-mul's seven chunk-local
// planes per limb instead.)
size_t ks_chunk(const rnt::Tables* t, size_t L, size_t B) {
  return chunk_polys(t, rnt::ks_whole_ok(t) ? 7 * L : L * L, B);
}

// A layout over the words of t's basis; its gadget scratch (rnt::gadget_ws), Lt target limbs over Ls.
rnt::WsLayout ws_layout(const rnt::Tables* t) { return rnt::WsLayout(t->n, word_bytes(t)); }
rnt::WsLayout gadget_ws(const rnt::Tables* t, size_t Lt, size_t Ls) {
  return rnt::gadget_ws(t->n, word_bytes(t), Lt, Ls, rnt::ks_whole_ok(t));
}
// The gadget scratch of a chunk of kc.B polys, carved at ws (limb stride ls).
struct GadgetWs {
  char *S, *U0, *U1;
  uint64_t ls;
  GadgetWs(const rnt::Launch& kc, void* ws) : ls((uint64_t)kc.B * kc.t->n) {
    const rnt::WsLayout w = gadget_ws(kc.t, kc.L, kc.src_limbs()).chunk(kc.B).place(ws);
    S = w.at(rnt::WS_S), U0 = w.at(rnt::WS_U0), U1 = w.at(rnt::WS_U1);
  }
};

// The stages of every gadget call, for the kc.B polys of a chunk.
//
// Rows: the decomposition of src (coefficient domain, kc.src_limbs() limbs at
// limb stride src_ls) into S, then the key-switch rows into U0/U1, seeded with
// init0 / init1 (NTT rows, Montgomery-scaled, may be null); with `lin` the LIN
// rows of one term of a linear combination (launch_ks_rows_lin).
// (Running them per group of target limbs, so each S slice could stay in the
// Infinity Cache between the two kernels, was slower: profiles/r02_ab_ks_groups.txt.)
int gadget_rows(const rnt::Launch& kc, const GadgetWs& ws, const void* src, uint64_t src_ls, const GadgetKey& key,
                const void* init0, const void* init1, uint64_t init_ls, const rnt::KsLin* lin = nullptr) {
  LAUNCH(kc.t, rnt::K_KS_DECOMPOSE, rnt::launch_ks_decompose(kc, ws.S, src, src_ls), "ks decompose");
  if (lin) {
    LAUNCH(kc.t, rnt::K_KS_ROWS,
           rnt::launch_ks_rows_lin(kc, ws.U0, ws.U1, ws.ls, ws.S, key.a, key.b, key.ls, init0, init1, init_ls, *lin),
           "ks rows");
  } else {
    LAUNCH(kc.t, rnt::K_KS_ROWS,
           rnt::launch_ks_rows(kc, ws.U0, ws.U1, ws.ls, ws.S, key.a, key.b, key.ls, init0, init1, init_ls),
           "ks rows");
  }
  return RNT_OK;
}

// Lower: the two inverse column passes, out0 = INV(U0) (+ add0), out1 =
// INV(U1), at limb stride out_ls.
int gadget_lower(const rnt::Launch& kc, const GadgetWs& ws, void* out0, void* out1, uint64_t out_ls,
                 const void* add0) {
  LAUNCH(kc.t, rnt::K_COL_INV, rnt::launch_col_inv(kc, out0, out_ls, ws.U0, ws.ls, 1, add0), "ks inverse");
  LAUNCH(kc.t, rnt::K_COL_INV, rnt::launch_col_inv(kc, out1, out_ls, ws.U1, ws.ls, 1, nullptr), "ks inverse");
  return RNT_OK;
}

// Lower with the rescale as the inverse's epilogue (engine.rs:263-282 after
// :530-531), kc.L - 1 output limbs: per output the dropped limb's inverse runs
// first, into the chunk plane LAST0 / LAST1 that the kept limbs' inverse reads.
int gadget_lower_rescale(const rnt::Launch& kc, const GadgetWs& ws, char* LAST0, char* LAST1, void* out0, void* out1,
                         uint64_t out_ls) {
  const size_t L = kc.L;
  rnt::Launch kl = kc;  // the dropped limb: its coefficient plane only
  kl.L = 1;
  rnt::ColRescArgs la;
  la.limb0 = (uint32_t)(L - 1);
  rnt::Launch kr = kc;  // the kept limbs, rescaled by it
  kr.L = L - 1;
  char* U[2] = {ws.U0, ws.U1};
  char* LAST[2] = {LAST0, LAST1};
  void* out[2] = {out0, out1};
  for (int o = 0; o < 2; ++o) {
    LAUNCH(kl.t, rnt::K_COL_INV,
           rnt::launch_col_inv(kl, LAST[o], ws.ls, U[o] + (L - 1) * ws.ls * word_bytes(kc.t), ws.ls, 1, nullptr, false,
                               la),
           "ks inverse (dropped limb)");
    rnt::ColRescArgs ra;
    ra.last = LAST[o];
    ra.inv = rnt::resc_inv_row(kc.t, L - 1, 0);
    ra.invp = rnt::resc_inv_row(kc.t, L - 1, 1);
    LAUNCH(kr.t, rnt::K_COL_INV, rnt::launch_col_inv(kr, out[o], out_ls, U[o], ws.ls, 1, nullptr, false, ra),
           "ks inverse + rescale");
  }
  return RNT_OK;
}

// The gadget sum of one chunk: out0 = INV(sum_i NTT(alpha_i(src)) key_b[i] +
// init0) (+ add0), out1 with key_a and init1 -- the whole-plane key-switch in
// one launch (2^10 <= N <= 2^14: no S, ws unused), or rows and lower.
int gadget_chunk_run(const rnt::Launch& kc, void* ws, const void* src, uint64_t src_ls, const GadgetKey& key,
                     void* out0, void* out1, uint64_t out_ls, const void* init0, const void* init1,
                     uint64_t init_ls, const void* add0) {
  if (rnt::ks_whole_ok(kc.t)) {
    LAUNCH(kc.t, rnt::K_KS_WHOLE,
           rnt::launch_ks_whole(kc, out0, out1, out_ls, src, src_ls, key.a, key.b, key.ls, init0, init1, init_ls,
                                add0),
           "whole-plane key-switch");
    return RNT_OK;
  }
  const GadgetWs g(kc, ws);
  if (int rc = gadget_rows(kc, g, src, src_ls, key, init0, init1, init_ls)) return rc;
  return gadget_lower(kc, g, out0, out1, out_ls, add0);
}

}  // namespace

extern "C" int rnt_keyswitch(rnt_buf* acc0, rnt_buf* acc1, const rnt_buf* d, const rnt_buf* key_a,
                             const rnt_buf* key_b) {
  if (int rc = check_buf(acc0, "rnt_keyswitch")) return rc;
  if (int rc = check_buf(acc1, "rnt_keyswitch")) return rc;
  if (int rc = check_buf(d, "rnt_keyswitch")) return rc;
  if (int rc = check_same(acc0, d, "rnt_keyswitch")) return rc;
  if (int rc = check_same(acc1, d, "rnt_keyswitch")) return rc;
  if (int rc = check_key_set("rnt_keyswitch", "", d->ctx, key_a, key_b, d->ctx->L)) return rc;
  if (d->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "key-switch input must be in coefficient domain");
  if (acc0 == acc1 || acc0 == d || acc1 == d)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_keyswitch: outputs must not alias each other or d");
  if (int rc = set_device(d->ctx)) return rc;
  const rnt::Launch k = launch_for(d);
  const size_t L = k.L, wb = word_bytes(k.t);
  const size_t bc = ks_chunk(k.t, L, d->n_polys);
  const uint64_t ls = limb_stride(d);
  rnt::WsLayout w = ws_layout(k.t).sub(gadget_ws(k.t, L, L)).chunk(bc);
  CallWs ws(acc0);
  if (int rc = ws.get(w, 16)) return rc;
  for (size_t p0 = 0; p0 < d->n_polys; p0 += bc) {
    rnt::Launch kc = k;
    kc.B = std::min(bc, d->n_polys - p0);
    const size_t off = p0 * k.t->n * wb;
    if (int rc = gadget_chunk_run(kc, w.at(0), (const char*)d->data + off, ls, GadgetKey(key_a, key_b),
                                  (char*)acc0->data + off, (char*)acc1->data + off, ls, nullptr, nullptr, 0, nullptr))
      return rc;
  }
  acc0->in_ntt = acc1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_keyswitch_ext(rnt_buf* acc0, rnt_buf* acc1, const void* src, size_t src_limbs,
                                 const rnt_buf* key_a, const rnt_buf* key_b, const rnt_buf* init0,
                                 const rnt_buf* init1) {
  if (int rc = check_buf(acc0, "rnt_keyswitch_ext")) return rc;
  if (int rc = check_buf(acc1, "rnt_keyswitch_ext")) return rc;
  if (int rc = check_same(acc0, acc1, "rnt_keyswitch_ext")) return rc;
  if (!src || src_limbs == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_keyswitch_ext: empty source");
  if (int rc = check_key_set("rnt_keyswitch_ext", "", acc0->ctx, key_a, key_b, src_limbs)) return rc;
  const rnt_buf* seeds[2] = {init0, init1};
  for (const rnt_buf* sd : seeds) {
    if (!sd) continue;
    if (int rc = check_same(acc0, sd, "rnt_keyswitch_ext")) return rc;
    if (!sd->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "key-switch seeds must be in the NTT domain");
    if (sd->n_polys != acc0->n_polys) return fail(RNT_ERR_BAD_ARGUMENT, "key-switch seed batch differs");
  }
  if (acc0 == acc1) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_keyswitch_ext: outputs alias");
  if (int rc = set_device(acc0->ctx)) return rc;
  rnt::Launch k = launch_for(acc0);
  k.Ls = src_limbs;
  const size_t Lt = k.L, Ls = src_limbs, n = k.t->n, wb = word_bytes(k.t), B = acc0->n_polys;
  const uint64_t src_ls = (uint64_t)B * n, full_ls = limb_stride(acc0);
  // polys per chunk: S is [Lt][Ls][Bc][N]; the whole-plane key-switch (2^10 <=
  // N <= 2^14) has no S and takes the whole batch in one launch
  const bool whole = rnt::ks_whole_ok(k.t);
  const size_t bc = whole ? B : chunk_polys(k.t, Lt * Ls, B);  // (S alone, not the layout's total)
  rnt::WsLayout w = ws_layout(k.t).sub(gadget_ws(k.t, Lt, Ls)).chunk(bc);
  CallWs ws(acc0);
  if (!whole)
    if (int rc = ws.get(w)) return rc;
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    rnt::Launch kc = k;
    kc.B = std::min(bc, B - p0);
    const size_t off = p0 * n * wb;
    const char* i0 = init0 ? (const char*)init0->data + off : nullptr;
    const char* i1 = init1 ? (const char*)init1->data + off : nullptr;
    if (int rc = gadget_chunk_run(kc, w.at(0), (const char*)src + off, src_ls, GadgetKey(key_a, key_b),
                                  (char*)acc0->data + off, (char*)acc1->data + off, full_ls, i0, i1, full_ls, nullptr))
      return rc;
  }
  acc0->in_ntt = acc1->in_ntt = 0;
  return RNT_OK;
}

namespace {

// Scratch blocks (of the outputs' size) the tensor needs: none on the
// whole-plane rings, one for the matrix-core tensor (N = 2^16, u32; it uses
// plane_scratch_planes(L B) <= L B planes of it), the four-step path's four
// column outputs.
size_t tensor_blocks(const rnt::Launch& k) { return rnt::tensor_whole_ok(k.t) ? 0 : use_mf(k) ? 1 : 4; }

// The tensor of every multiply for kc.B polys (inputs in the coefficient
// domain at limb stride in_ls, read in place): d0^, d1^ (NTT domain, scaled by
// 2^-w as the key-switch seeds are, engine.rs:486-493) and the
// coefficient-domain d2, each at limb stride ls.  T: tensor_blocks(kc) scratch
// blocks.  The gadget key-switch's diagonal (kc.d2hat) travels in kc.
int tensor(const rnt::Launch& kc, char* const* T, void* D0, void* D1, void* D2, uint64_t ls, const void* c0,
           const void* c1, const void* c0p, const void* c1p, uint64_t in_ls) {
  switch (tensor_blocks(kc)) {
    case 0:
      LAUNCH(kc.t, rnt::K_TENSOR_WHOLE, rnt::launch_tensor_whole(kc, D0, D1, D2, ls, c0, c1, c0p, c1p, in_ls),
             "tensor whole");
      break;
    case 1:
      LAUNCH(kc.t, rnt::K_MF_TENSOR, rnt::launch_mf_tensor(kc, D0, D1, D2, ls, c0, c1, c0p, c1p, in_ls, T[0]),
             "MFMA tensor");
      break;
    default:
      LAUNCH(kc.t, rnt::K_COL_FWD, rnt::launch_col_fwd(kc, T[0], c0, T[1], c1, in_ls, ls), "tensor column");
      LAUNCH(kc.t, rnt::K_COL_FWD, rnt::launch_col_fwd(kc, T[2], c0p, T[3], c1p, in_ls, ls), "tensor column");
      LAUNCH(kc.t, rnt::K_TENSOR_ROWS, rnt::launch_tensor_rows(kc, D0, D1, D2, T[0], T[1], T[2], T[3], ls),
             "tensor rows");
      // d2 -> coefficient domain (engine.rs:493), in place
      LAUNCH(kc.t, rnt::K_COL_INV, rnt::launch_col_inv(kc, D2, ls, D2, ls, 1, nullptr), "d2 inverse");
  }
  return RNT_OK;
}

// The output rules of a call that ends in a rescale: both outputs on one
// drop_last(1) context of the input's, n_polys polys each.
int rescaled_outputs_check(const char* name, const rnt_buf* out0, const rnt_buf* out1, const rnt_buf* in,
                           size_t n_polys) {
  const size_t L = in->ctx->L;
  if (L < 2)  // poly.rs:191-197
    return fail_fields(RNT_ERR_INVALID_MOD_DROP, 1, L, "invalid mod-drop count 1 for %zu channels", L);
  for (const rnt_buf* o : {out0, out1}) {
    if (o->ctx->t != in->ctx->t || o->ctx->L != L - 1)
      return fail(RNT_ERR_BASIS_MISMATCH, "%s: an output's basis is not drop_last(1) of the inputs'", name);
    if (o->n_polys != n_polys)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output of %zu polys for a batch of %zu", name, o->n_polys, n_polys);
  }
  if (out0->ctx != out1->ctx)  // engine.rs:272-274: one shared new basis
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: outputs must share one basis", name);
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_tensor(rnt_buf* d0, rnt_buf* d1, rnt_buf* d2, const rnt_buf* c0,
                             const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p) {
  const rnt_buf* all[7] = {d0, d1, d2, c0, c1, c0p, c1p};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, "rnt_ct_tensor")) return rc;
  for (int i = 1; i < 7; ++i)
    if (int rc = check_same(all[0], all[i], "rnt_ct_tensor")) return rc;
  if (c0->in_ntt || c1->in_ntt || c0p->in_ntt || c1p->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_tensor: inputs must be in coefficient domain");
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 7; ++j)
      if (i != j && all[i] == all[j])
        return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_tensor: outputs must not alias other operands");
  if (int rc = set_device(c0->ctx)) return rc;
  rnt::Launch k = launch_for(c0);
  const uint64_t ls = limb_stride(c0);
  const size_t nt = tensor_blocks(k);
  // (the matrix-core tensor's scratch at its own size, not a whole block)
  rnt::WsLayout w = ws_layout(k.t).chunk(c0->n_polys);
  if (nt == 1) w.bytes(rnt::plane_scratch_planes((uint64_t)k.L * c0->n_polys) * k.t->n * word_bytes(k.t));
  else w.blocks(k.L, nt);
  CallWs ws(d0);
  if (nt)
    if (int rc = ws.get(w)) return rc;
  char* T[4] = {};
  for (size_t i = 0; i < nt; ++i) T[i] = w.at(0, i);
  if (int rc = tensor(k, T, d0->data, d1->data, d2->data, ls, c0->data, c1->data, c0p->data, c1p->data, ls)) return rc;
  d0->in_ntt = d1->in_ntt = 1;
  d2->in_ntt = 0;
  return RNT_OK;
}

// The ct-mul body; with `resc` the outputs are on drop_last(1) and each
// chunk's key-switch inverse applies the rescale as its epilogue
// (rnt_ct_mul_relin_rescale: the dropped limb's inverse runs first, into a
// chunk plane the other limbs' inverse reads), so the un-rescaled product
// never goes through HBM.
static int ct_mul_relin_body(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                             const rnt_buf* c0p, const rnt_buf* c1p, const rnt_buf* key_a,
                             const rnt_buf* key_b, bool resc) {
  if (int rc = set_device(c0->ctx)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys;
  const size_t bc = ks_chunk(k.t, L, B);  // (S alone, not the layout's total)
  const size_t nt = tensor_blocks(k);
  // the key-switch's diagonal from the tensor's d2^ (one more chunk plane
  // set, D2H): the four-step key-switch on tiled grids, whose tensor writes it
  const bool diag = k.t->ks_diag && nt != 0 && !rnt::ks_whole_ok(k.t) && rnt::col_resc_ok(k.t);
  rnt::WsLayout w = rnt::mul_relin_ws(n, wb, L, nt, rnt::ks_whole_ok(k.t), resc, diag).chunk(bc);
  CallWs cws(out0);
  if (int rc = cws.get(w)) return rc;
  char* T[4] = {};
  for (size_t i = 0; i < nt; ++i) T[i] = w.at(rnt::MR_T, i);
  char *D0 = w.at(rnt::MR_D, 0), *D1 = w.at(rnt::MR_D, 1), *D2 = w.at(rnt::MR_D, 2);
  char *KS = w.at(rnt::MR_KS), *LAST0 = w.at(rnt::MR_LAST, 0), *LAST1 = w.at(rnt::MR_LAST, 1), *D2H = w.at(rnt::MR_D2H);
  const uint64_t full_ls = limb_stride(c0);
  const GadgetKey key(key_a, key_b);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    if (diag) {
      kc.d2hat = D2H;  // written by the tensor, read by the key-switch rows
      kc.d2hat_ls = cls;
    }
    auto off = [&](const rnt_buf* b) { return (char*)b->data + p0 * n * wb; };
    // the ciphertexts read in place (full limb stride) into the chunk's D0..D2
    if (int rc = tensor(kc, T, D0, D1, D2, cls, off(c0), off(c1), off(c0p), off(c1p), full_ls)) return rc;
    // gadget sum with d0hat / d1hat as accumulator seeds (engine.rs:530-531)
    if (!resc) {
      if (int rc = gadget_chunk_run(kc, KS, D2, cls, key, off(out0), off(out1), full_ls, D0, D1, cls, nullptr))
        return rc;
      continue;
    }
    // into the chunk's NTT-row accumulators, then the inverse with the rescale fused
    const GadgetWs g(kc, KS);
    if (int rc = gadget_rows(kc, g, D2, cls, key, D0, D1, cls)) return rc;
    if (int rc = gadget_lower_rescale(kc, g, LAST0, LAST1, off(out0), off(out1), limb_stride(out0))) return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

static int ct_mul_check(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                        const rnt_buf* c0p, const rnt_buf* c1p, const rnt_buf* key_a, const rnt_buf* key_b,
                        const char* name) {
  const rnt_buf* all[6] = {out0, out1, c0, c1, c0p, c1p};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  for (int i = 3; i < 6; ++i)
    if (int rc = check_same(c0, all[i], name)) return rc;
  if (int rc = check_key_set(name, "", c0->ctx, key_a, key_b, c0->ctx->L)) return rc;
  if (c0->in_ntt || c1->in_ntt || c0p->in_ntt || c1p->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "mul_ciphertexts_gadget: inputs must be in coefficient domain");
  if (out0 == out1) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  return RNT_OK;
}

extern "C" int rnt_ct_mul_relin(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                                const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p,
                                const rnt_buf* key_a, const rnt_buf* key_b) {
  if (int rc = ct_mul_check(out0, out1, c0, c1, c0p, c1p, key_a, key_b, "rnt_ct_mul_relin")) return rc;
  if (int rc = check_same(out0, c0, "rnt_ct_mul_relin")) return rc;
  if (int rc = check_same(out1, c0, "rnt_ct_mul_relin")) return rc;
  return ct_mul_relin_body(out0, out1, c0, c1, c0p, c1p, key_a, key_b, false);
}

extern "C" int rnt_ct_mul_relin_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                                        const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p,
                                        const rnt_buf* key_a, const rnt_buf* key_b) {
  if (int rc = ct_mul_check(out0, out1, c0, c1, c0p, c1p, key_a, key_b, "rnt_ct_mul_relin_rescale")) return rc;
  if (int rc = rescaled_outputs_check("rnt_ct_mul_relin_rescale", out0, out1, c0, c0->n_polys)) return rc;
  if (rnt::col_resc_ok(c0->ctx->t.get()) && !rnt::ks_whole_ok(c0->ctx->t.get()))
    return ct_mul_relin_body(out0, out1, c0, c1, c0p, c1p, key_a, key_b, true);
  // small rings (the whole-plane key-switch, no column inverse): the product,
  // then the rescale, through two call-scoped temporaries
  rnt_buf* t0 = nullptr;
  rnt_buf* t1 = nullptr;
  int rc = rnt_buf_alloc_uninit(c0->ctx, c0->n_polys, &t0);
  if (rc == RNT_OK) rc = rnt_buf_alloc_uninit(c0->ctx, c0->n_polys, &t1);
  if (rc == RNT_OK) rc = ct_mul_relin_body(t0, t1, c0, c1, c0p, c1p, key_a, key_b, false);
  if (rc == RNT_OK) rc = rnt_ct_rescale(out0, out1, t0, t1);
  rnt_buf_free(t0);
  rnt_buf_free(t1);
  return rc;
}

namespace {
// The rotation's body on raw [L][B][N] blocks of the basis `ctx` (defined with
// the linear transforms, which run it per term on the whole-plane rings).
int ct_rotate_body(const rnt_ctx* ctx, size_t B, void* out0, void* out1, const void* c0, bool c0_ntt, const void* c1,
                   bool c1_ntt, int32_t kk, const GadgetKey& key);
}  // namespace

extern "C" int rnt_ct_rotate(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                             int32_t kk, const rnt_buf* key_a, const rnt_buf* key_b) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, "rnt_ct_rotate")) return rc;
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(all[0], all[i], "rnt_ct_rotate")) return rc;
  if (int rc = check_key_set("rnt_ct_rotate", "", c0->ctx, key_a, key_b, c0->ctx->L)) return rc;
  if (out0 == out1) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate: out0 aliases out1");
  if (int rc = ct_rotate_body(c0->ctx, c0->n_polys, out0->data, out1->data, c0->data, c0->in_ntt, c1->data,
                              c1->in_ntt, kk, GadgetKey(key_a, key_b)))
    return rc;
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// linear transform: out = sum_t diag_t * rotate_ciphertext(ct, steps[t])
// ---------------------------------------------------------------------------
namespace {

// `rows` runs of `run_words` contiguous words, dst row r at dst + r dst_ls,
// src row r at src + r src_ls (strides in words): the polys [first, first +
// count) of every limb of a [L][B][N] buffer are one such run per limb.
int copy_rows(const rnt::Launch& k, void* dst, uint64_t dst_ls, const void* src, uint64_t src_ls,
              uint64_t run_words, size_t rows) {
  const size_t wb = word_bytes(k.t);
  if (dst_ls == run_words && src_ls == run_words) {  // contiguous on both sides: one copy
    run_words *= rows;
    rows = 1;
  }
  for (size_t r = 0; r < rows; ++r)
    HIP_TRY(hipMemcpyAsync((char*)dst + r * dst_ls * wb, (const char*)src + r * src_ls * wb, run_words * wb,
                           hipMemcpyDeviceToDevice, k.s),
            "hipMemcpyAsync");
  return RNT_OK;
}

// Forward / inverse transform in place of a raw [k.L][k.B][N] block at limb
// stride ls: the launches of rnt_ntt_fwd / rnt_ntt_inv, on k.s.  pt: the
// tables whose profile counts them (nullptr: k.t, whose stream k.s then is) --
// the hybrid key-switch transforms over the key basis' tables on the
// ciphertext context's stream.
// Over a level view with a gap (k.map_gap, the hybrid calls' launches alone)
// the working limbs are two contiguous runs of root limbs -- [0, level) and
// [level + gap, ..) -- and the same launches run once per run, the second with
// its table-limb base (Launch::tab0) on the block's limb `level`.
bool raw_split(const rnt::Launch& k, rnt::Launch* lo, rnt::Launch* hi) {
  if (k.map_gap == 0 || k.L <= k.map_level) return false;
  *lo = *hi = k;
  lo->map_level = hi->map_level = UINT32_MAX;
  lo->map_gap = hi->map_gap = 0;
  lo->L = k.map_level;
  hi->L = k.L - k.map_level;
  hi->tab0 = k.map_level + k.map_gap;
  return true;
}
int fwd_raw(const rnt::Launch& k, void* p, uint64_t ls, const rnt::Tables* pt = nullptr) {
  if (!pt) pt = k.t;
  rnt::Launch lo, hi;
  if (raw_split(k, &lo, &hi)) {
    if (int rc = fwd_raw(lo, p, ls, pt)) return rc;
    return fwd_raw(hi, (char*)p + (size_t)k.map_level * ls * word_bytes(k.t), ls, pt);
  }
  if (use_mf(k)) {
    LAUNCH_ON(pt, k.s, rnt::K_MF_NTT_FWD, rnt::launch_mf_ntt(k, 0, p, ls), "MFMA forward transform");
  } else if (rnt::whole_ok(k.t, 0)) {
    LAUNCH_ON(pt, k.s, rnt::K_WHOLE_FWD, rnt::launch_whole(k, 0, p, p, nullptr, ls), "whole-plane forward");
  } else {
    LAUNCH_ON(pt, k.s, rnt::K_COL_FWD, rnt::launch_col_fwd(k, p, p, nullptr, nullptr, ls, ls), "column forward");
    LAUNCH_ON(pt, k.s, rnt::K_ROW_FWD, rnt::launch_row(k, 0, p, nullptr, ls), "row forward");
  }
  return RNT_OK;
}
int inv_raw(const rnt::Launch& k, void* p, uint64_t ls, const rnt::Tables* pt = nullptr) {
  if (!pt) pt = k.t;
  rnt::Launch lo, hi;
  if (raw_split(k, &lo, &hi)) {
    if (int rc = inv_raw(lo, p, ls, pt)) return rc;
    return inv_raw(hi, (char*)p + (size_t)k.map_level * ls * word_bytes(k.t), ls, pt);
  }
  if (use_mf(k)) {
    LAUNCH_ON(pt, k.s, rnt::K_MF_NTT_INV, rnt::launch_mf_ntt(k, 1, p, ls), "MFMA inverse transform");
  } else if (rnt::whole_ok(k.t, 1)) {
    LAUNCH_ON(pt, k.s, rnt::K_WHOLE_INV, rnt::launch_whole(k, 1, p, p, nullptr, ls), "whole-plane inverse");
  } else {
    LAUNCH_ON(pt, k.s, rnt::K_ROW_INV, rnt::launch_row(k, 1, p, nullptr, ls), "row inverse");
    LAUNCH_ON(pt, k.s, rnt::K_COL_INV, rnt::launch_col_inv(k, p, ls, p, ls, 0, nullptr), "column inverse");
  }
  return RNT_OK;
}

// z (+)= x^ (.) m_t for one term: x^ a [k.L][k.B][N] NTT-domain block, m_t
// plane t of the Montgomery-form plaintexts dm ([L][n_terms][N]).
int lin_mac(const rnt::Launch& k, void* z, const void* x, const char* dm, size_t t, size_t n_terms, bool accum) {
  const size_t n = k.t->n, wb = word_bytes(k.t);
  LAUNCH(k.t, rnt::K_ELEMENTWISE,
         rnt::launch_bcast_mul(k, 0, z, x, dm + t * n * wb, (uint64_t)n_terms * n, accum), "plaintext product");
  return RNT_OK;
}

// g^-1 mod 2N (g odd): Newton's iteration mod 2^64, then the mask.
uint64_t exponent_inverse(uint64_t g, uint64_t two_n) {
  uint64_t x = g;
  for (int it = 0; it < 6; ++it) x *= 2 - g * x;
  return x & (two_n - 1);
}

// inv_raw, then + addend (coefficient domain, a contiguous block in p's
// layout): the four-step inverse column pass adds it as it stores, the
// one-launch transforms take an add_assign after them.
int inv_add_raw(const rnt::Launch& k, void* p, uint64_t ls, const void* addend) {
  if (use_mf(k) || rnt::whole_ok(k.t, 1)) {
    if (int rc = inv_raw(k, p, ls)) return rc;
    LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(k, 0, p, p, addend), "add_assign");
    return RNT_OK;
  }
  LAUNCH(k.t, rnt::K_ROW_INV, rnt::launch_row(k, 1, p, nullptr, ls), "row inverse");
  LAUNCH(k.t, rnt::K_COL_INV, rnt::launch_col_inv(k, p, ls, p, ls, 0, addend), "column inverse");
  return RNT_OK;
}

// The rotation's body (arguments checked by the caller): out = the key-switch
// of sigma(c1) + sigma(c0), on contiguous [L][B][N] blocks of the basis `ctx`;
// an input flagged NTT-domain is converted first.
int ct_rotate_body(const rnt_ctx* ctx, size_t B, void* out0, void* out1, const void* c0, bool c0_ntt, const void* c1,
                   bool c1_ntt, int32_t kk, const GadgetKey& key) {
  if (int rc = set_device(ctx)) return rc;
  const rnt::Launch k = launch_for(ctx, B);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t);
  const size_t words = L * B * n;
  const uint64_t ls = (uint64_t)B * n, two_n = 2 * (uint64_t)n;
  const uint64_t g = rotation_exponent(kk, two_n);
  const size_t bc = ks_chunk(k.t, L, B);  // (S alone, not the layout's total)
  // sigma(c0) needs no launch of its own on the tiled four-step key-switch:
  // its inverse column pass gathers it from c0 as it adds it (k_colt_inv's
  // addend with g^-1 mod 2N).  Only for one ciphertext by default
  // (RNT_ROT_FUSE=1; 2: any batch, 0: never): the scattered 4-byte gather
  // costs the inverse about what the automorphism launch costs, which at one
  // ciphertext is mostly launch and tail (config 5: +2.0% at one ciphertext,
  // -0.5% at eight, profiles/r06/ab_rot_fuse.txt).  Not in place on out0: a
  // workgroup's gather would race the stores of the others on the same plane
  const bool fuse0 = (k.t->rot_fuse == 2 || (k.t->rot_fuse == 1 && B == 1)) && (g & 1) && !c0_ntt &&
                     !rnt::ks_whole_ok(k.t) && rnt::col_resc_ok(k.t) && out0 != c0;
  // sigma(c0) | sigma(c1) (the batch) | a block for an NTT-domain input | the chunk's gadget scratch
  rnt::WsLayout w = ws_layout(k.t).bytes(words * wb).bytes(words * wb).bytes(c0_ntt || c1_ntt ? words * wb : 0)
                        .sub(gadget_ws(k.t, L, L)).chunk(bc);
  CallWs ws(ctx);
  if (int rc = ws.get(w)) return rc;
  char *sig0 = w.at(0), *sig1 = w.at(1), *tmp = w.at(2), *KS = w.at(3);
  // sigma(c0), sigma(c1) in coefficient domain (engine.rs:417-419; poly.rs:494-504
  // converts an NTT-domain input first)
  for (int i = fuse0 ? 1 : 0; i < 2; ++i) {
    const void* s = i ? c1 : c0;
    if (i ? c1_ntt : c0_ntt) {
      if (int rc = copy_rows(k, tmp, ls, s, ls, ls, L)) return rc;
      if (int rc = inv_raw(k, tmp, ls)) return rc;
      s = tmp;
    }
    LAUNCH(k.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(k, i ? sig1 : sig0, s, g), "automorphism");
  }
  rnt::Launch kr = k;
  if (fuse0) kr.add_ginv = (uint32_t)exponent_inverse(g, two_n);
  const char* add0 = fuse0 ? (const char*)c0 : sig0;
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    kr.B = std::min(bc, B - p0);
    const size_t off = p0 * n * wb;
    if (int rc = gadget_chunk_run(kr, KS, sig1 + off, ls, key, (char*)out0 + off, (char*)out1 + off, ls, nullptr,
                                  nullptr, 0, add0 + off))
      return rc;
  }
  return RNT_OK;
}

// The hoisted gadget sums of one chunk (kc.B polys of c1 at limb stride
// c1_ls): the digits once -- D ([L][L kc.B][N]) <- NTT_j(c1_i 2^w mod q_j), a
// buffer of L limbs and L kc.B polys through the ordinary forward transform,
// so in the device order of rnt_key_prepare's output -- then one k_hoist_mac
// launch per group of kHoistT nonzero steps into ACC (2 kHoistT blocks of
// [L][kc.B][N]) and finish(t, acc0, acc1) for every step t of the group, the
// accumulators canonical and in the NTT domain: INV(acc0) = sum_i D_i
// sigma^-1(key_b[t][i]).
template <class Finish>
int hoist_chunk(const rnt::Launch& kc, char* D, char* ACC, const void* c1, uint64_t c1_ls, const int32_t* steps,
                size_t n_steps, const rnt_buf* keys_a, const rnt_buf* keys_b, Finish&& finish) {
  const size_t L = kc.L, n = kc.t->n, wb = word_bytes(kc.t);
  const size_t pw = L * kc.B * n * wb;
  bool any_rot = false;
  for (size_t t = 0; t < n_steps; ++t) any_rot = any_rot || steps[t] != 0;
  if (!any_rot) return RNT_OK;
  LAUNCH(kc.t, rnt::K_HOIST_DIGITS, rnt::launch_hoist_digits(kc, D, c1, c1_ls), "hoisted digits");
  rnt::Launch kd = kc;
  kd.B = L * kc.B;
  if (int rc = fwd_raw(kd, D, (uint64_t)kd.B * n)) return rc;
  for (size_t t = 0; t < n_steps;) {
    size_t idx[rnt::kHoistT];
    void* a0[rnt::kHoistT] = {};
    void* a1[rnt::kHoistT] = {};
    const void* ka[rnt::kHoistT] = {};
    const void* kb[rnt::kHoistT] = {};
    uint32_t nt = 0;
    for (; t < n_steps && nt < rnt::kHoistT; ++t) {
      if (steps[t] == 0) continue;
      idx[nt] = t;
      a0[nt] = ACC + 2 * nt * pw;
      a1[nt] = ACC + (2 * nt + 1) * pw;
      const GadgetKey key(keys_a, keys_b, t);
      ka[nt] = key.a;
      kb[nt] = key.b;
      ++nt;
    }
    if (nt == 0) break;
    LAUNCH(kc.t, rnt::K_HOIST_MAC, rnt::launch_hoist_mac(kc, a0, a1, nt, D, ka, kb, limb_stride(keys_a)),
           "hoisted gadget sums");
    for (uint32_t u = 0; u < nt; ++u)
      if (int rc = finish(idx[u], (char*)a0[u], (char*)a1[u])) return rc;
  }
  return RNT_OK;
}

// The polys of a chunk stay where they are in the full batch (*x, limb stride
// full_ls) or, with more than one chunk (X non-null), are gathered into X at
// the chunk's own limb stride.
int chunk_gather(const rnt::Launch& kc, char* X, const char** x, uint64_t full_ls) {
  if (!X) return RNT_OK;
  const uint64_t cls = (uint64_t)kc.B * kc.t->n;
  if (int rc = copy_rows(kc, X, cls, *x, full_ls, cls, kc.L)) return rc;
  *x = X;
  return RNT_OK;
}

// One rotated term of a sum of rotations, into the chunk's accumulators:
// sigma_g(x1) -> decomposition -> LIN rows with the seed NTT(sigma_g(x0)) 2^-w,
// the Montgomery-form multiplier plane `mul` (limb stride mul_ls) and, with
// `accum`, accumulation into U0/U1.  x0, x1 at the chunk's limb stride; SIG1,
// SEED: chunk blocks.
int lin_term(const rnt::Launch& kc, const GadgetWs& ws, char* SIG1, char* SEED, const void* x0, const void* x1,
             uint64_t g, const GadgetKey& key, const void* mul, uint64_t mul_ls, bool accum) {
  LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SIG1, x1, g), "automorphism");
  LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SEED, x0, g), "automorphism");
  if (int rc = fwd_raw(kc, SEED, ws.ls)) return rc;
  LAUNCH(kc.t, rnt::K_ELEMENTWISE, rnt::launch_bcast_mul(kc, 0, SEED, SEED, nullptr, 0, false), "seed scale");
  rnt::KsLin lin;
  lin.mul = mul;
  lin.mul_ls = mul_ls;
  lin.accum = accum ? 1u : 0u;
  return gadget_rows(kc, ws, SIG1, ws.ls, key, SEED, nullptr, ws.ls, &lin);
}

// The epilogue of a chunk of such terms, per output o: without any rotated
// term the unrotated sum Z[o] is the result; one chunk inverts U straight into
// the output (limb stride full_ls), adding Z[o] (may be null); more chunks
// invert into tmp[o] -- the addend shares the output's limb stride: a
// chunk-local output -- and copy the rows out.
int lin_finish(const rnt::Launch& kc, const GadgetWs& ws, bool any_rot, bool multi, char* const dst[2],
               uint64_t full_ls, char* const Z[2], char* const tmp[2]) {
  char* const U[2] = {ws.U0, ws.U1};
  for (int o = 0; o < 2; ++o) {
    if (!any_rot) {
      if (int rc = copy_rows(kc, dst[o], full_ls, Z[o], ws.ls, ws.ls, kc.L)) return rc;
    } else if (!multi) {
      LAUNCH(kc.t, rnt::K_COL_INV, rnt::launch_col_inv(kc, dst[o], full_ls, U[o], ws.ls, 1, Z[o]), "ks inverse");
    } else {
      LAUNCH(kc.t, rnt::K_COL_INV, rnt::launch_col_inv(kc, tmp[o], ws.ls, U[o], ws.ls, 1, Z[o]), "ks inverse");
      if (int rc = copy_rows(kc, dst[o], full_ls, tmp[o], ws.ls, ws.ls, kc.L)) return rc;
    }
  }
  return RNT_OK;
}

// hoist_chunk's finish for a baby step of the BSGS bodies: the accumulators
// back to coefficients (+ x0 on the first), sigma_g, and forward again into the
// step's pair of baby blocks R, R + pw.
int hoisted_baby_finish(const rnt::Launch& k, uint64_t ls, char* A0, char* A1, const void* x0, uint64_t g, char* R,
                        size_t pw) {
  if (int rc = inv_add_raw(k, A0, ls, x0)) return rc;
  if (int rc = inv_raw(k, A1, ls)) return rc;
  char* A[2] = {A0, A1};
  for (int o = 0; o < 2; ++o) {
    LAUNCH(k.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(k, R + o * pw, A[o], g), "automorphism");
    if (int rc = fwd_raw(k, R + o * pw, ls)) return rc;
  }
  return RNT_OK;
}

// The whole-plane rings (ks_whole_ok: no U0/U1 for the terms to share): the
// composition itself -- every term's rotation through the whole-plane
// key-switch, its product with the plaintext taken in the NTT domain and
// summed there, one inverse of each sum.  w: dm | Z0 Z1 | R0 R1 over the batch.
int ct_linear_composed(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                       const int32_t* steps, size_t n_terms, const rnt_buf* keys_a, const rnt_buf* keys_b,
                       const rnt::WsLayout& w) {
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, B = c0->n_polys;
  const uint64_t ls = limb_stride(c0);
  const char* dm = w.at(0);
  char *Z[2] = {w.at(1, 0), w.at(1, 1)}, *R[2] = {w.at(2, 0), w.at(2, 1)};
  const rnt_buf* src[2] = {c0, c1};
  for (size_t t = 0; t < n_terms; ++t) {
    if (steps[t] != 0) {
      if (int rc = ct_rotate_body(c0->ctx, B, R[0], R[1], c0->data, false, c1->data, false, steps[t],
                                  GadgetKey(keys_a, keys_b, t)))
        return rc;
    } else {
      for (int o = 0; o < 2; ++o)
        if (int rc = copy_rows(k, R[o], ls, src[o]->data, ls, ls, L)) return rc;
    }
    for (int o = 0; o < 2; ++o) {
      if (int rc = fwd_raw(k, R[o], ls)) return rc;
      if (int rc = lin_mac(k, Z[o], R[o], dm, t, n_terms, t != 0)) return rc;
    }
  }
  rnt_buf* out[2] = {out0, out1};
  for (int o = 0; o < 2; ++o) {
    if (int rc = inv_raw(k, Z[o], ls)) return rc;
    if (int rc = copy_rows(k, out[o]->data, ls, Z[o], ls, ls, L)) return rc;
  }
  return RNT_OK;
}

// The four-step key-switch: chunks outside, terms inside, on rnt::lin_fused_ws.
// Every nonzero term is a lin_term with the plaintext row; the step-0 terms'
// products are summed in the NTT domain, inverted and added by the chunk's two
// inverse column passes (lin_finish).
int ct_linear_fused(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                    const int32_t* steps, size_t n_terms, const rnt_buf* keys_a, const rnt_buf* keys_b,
                    const rnt::WsLayout& w, bool any_zero, bool any_rot) {
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys, bc = w.bc;
  const uint64_t full_ls = limb_stride(c0), two_n = 2 * (uint64_t)n;
  const bool multi = bc < B;
  const char* dm = w.at(rnt::LF_DM);
  char* X[2] = {w.at(rnt::LF_X, 0), w.at(rnt::LF_X, 1)};
  char *SIG1 = w.at(rnt::LF_SIG1), *SEED = w.at(rnt::LF_SEED), *KS = w.at(rnt::LF_KS);
  char* NT[2] = {w.at(rnt::LF_RA, 0), w.at(rnt::LF_RA, 1)};
  char* Z[2] = {w.at(rnt::LF_RB, 0), w.at(rnt::LF_RB, 1)};
  char* const tmp[2] = {SEED, SIG1};
  const rnt_buf* src[2] = {c0, c1};
  rnt_buf* out[2] = {out0, out1};
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    rnt::Launch kc = k;
    kc.B = std::min(bc, B - p0);
    const GadgetWs g(kc, KS);
    const uint64_t cls = g.ls;
    const char* x[2];
    char* dst[2];
    for (int o = 0; o < 2; ++o) {
      x[o] = (const char*)src[o]->data + p0 * n * wb;
      dst[o] = (char*)out[o]->data + p0 * n * wb;
      if (int rc = chunk_gather(kc, X[o], &x[o], full_ls)) return rc;
    }
    if (any_zero) {
      bool first = true;
      for (int o = 0; o < 2; ++o) {
        if (int rc = copy_rows(kc, NT[o], cls, x[o], multi ? cls : full_ls, cls, L)) return rc;
        if (int rc = fwd_raw(kc, NT[o], cls)) return rc;
      }
      for (size_t t = 0; t < n_terms; ++t) {
        if (steps[t] != 0) continue;
        for (int o = 0; o < 2; ++o)
          if (int rc = lin_mac(kc, Z[o], NT[o], dm, t, n_terms, !first)) return rc;
        first = false;
      }
      for (int o = 0; o < 2; ++o)
        if (int rc = inv_raw(kc, Z[o], cls)) return rc;
    }
    bool first = true;
    for (size_t t = 0; t < n_terms; ++t) {
      if (steps[t] == 0) continue;
      if (int rc = lin_term(kc, g, SIG1, SEED, x[0], x[1], rotation_exponent(steps[t], two_n),
                            GadgetKey(keys_a, keys_b, t), dm + t * n * wb, (uint64_t)n_terms * n, !first))
        return rc;
      first = false;
    }
    if (int rc = lin_finish(kc, g, any_rot, multi, dst, full_ls, Z, tmp)) return rc;
  }
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_linear(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                             const int32_t* steps, size_t n_terms, const rnt_buf* diag,
                             const rnt_buf* keys_a, const rnt_buf* keys_b) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, "rnt_ct_linear")) return rc;
  if (int rc = check_buf(diag, "rnt_ct_linear")) return rc;
  if (n_terms == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear: no terms");
  if (!steps) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear: null steps");
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(all[0], all[i], "rnt_ct_linear")) return rc;
  if (diag->ctx != c0->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "rnt_ct_linear: the plaintexts belong to a different basis");
  if (diag->n_polys != n_terms)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear: %zu plaintexts for %zu terms", diag->n_polys, n_terms);
  bool any_rot = false, any_zero = false;
  for (size_t t = 0; t < n_terms; ++t) (steps[t] == 0 ? any_zero : any_rot) = true;
  const size_t L = c0->ctx->L;
  if (any_rot || keys_a || keys_b) {
    if (int rc = check_key_set("rnt_ct_linear", "", c0->ctx, keys_a, keys_b, n_terms * L)) return rc;
  }
  if (!diag->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_linear: the plaintexts must be in the NTT domain");
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_linear: the ciphertext must be in coefficient domain");
  const rnt_buf* ins[5] = {c0, c1, diag, keys_a, keys_b};
  if (out0 == out1) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear: out0 aliases out1");
  for (int i = 0; i < 5; ++i) {
    if ((out0 == ins[i] && i != 0) || (out1 == ins[i] && i != 1))
      return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear: an output aliases an input other than its own component");
  }
  if (int rc = set_device(c0->ctx)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys, dm_bytes = L * n_terms * n * wb;
  const bool composed = rnt::ks_whole_ok(k.t);
  const size_t bc = composed ? B : ks_chunk(k.t, L, B);  // (S alone, not the layout's total)
  rnt::WsLayout w = composed ? ws_layout(k.t).bytes(dm_bytes).blocks(L, 2).blocks(L, 2)
                             : rnt::lin_fused_ws(n, wb, L, dm_bytes, false, bc < B, any_zero, any_zero, 0);
  CallWs ws(out0);
  if (int rc = ws.get(w.chunk(bc), 16)) return rc;
  // the plaintexts in Montgomery form (m^ 2^w mod q), once per call: a
  // Montgomery product with them is then the canonical product, and the
  // key-switch sums keep their single factor 2^-w for the inverse to fold
  rnt::Launch kd = k;
  kd.B = n_terms;
  LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_bcast_mul(kd, 1, w.at(0), diag->data, nullptr, 0, false),  // dm leads
         "plaintexts to Montgomery form");
  int rc;
  if (composed)
    rc = ct_linear_composed(out0, out1, c0, c1, steps, n_terms, keys_a, keys_b, w);
  else
    rc = ct_linear_fused(out0, out1, c0, c1, steps, n_terms, keys_a, keys_b, w, any_zero, any_rot);
  if (rc) return rc;
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// hoisted rotations: out_t = sigma_t(c0 + sum_i D_i sigma_t^-1(key_b[t][i])),
//                            sigma_t(     sum_i D_i sigma_t^-1(key_a[t][i]))
// with D_i = alpha_i(c1) decomposed and transformed once for every step
// ---------------------------------------------------------------------------
extern "C" int rnt_key_prepare_hoisted(rnt_buf* key_a, rnt_buf* key_b, int32_t k) {
  if (int rc = check_buf(key_a, "rnt_key_prepare_hoisted")) return rc;
  if (int rc = check_buf(key_b, "rnt_key_prepare_hoisted")) return rc;
  if (int rc = check_same(key_a, key_b, "rnt_key_prepare_hoisted")) return rc;
  if (k == 0) return rnt_key_prepare(key_a, key_b);
  const uint64_t two_n = 2 * (uint64_t)key_a->ctx->t->n;
  const uint64_t ginv = exponent_inverse(rotation_exponent(k, two_n), two_n);
  // (rnt_automorphism converts an NTT-domain key first and runs in place
  // through the buffer's workspace)
  for (rnt_buf* key : {key_a, key_b}) {
    if (int rc = rnt_automorphism(key, key, ginv)) return rc;
    if (int rc = rnt_ntt_fwd(key)) return rc;
  }
  return RNT_OK;
}

extern "C" int rnt_ct_rotate_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                     const int32_t* steps, size_t n_steps, const rnt_buf* keys_a,
                                     const rnt_buf* keys_b) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, "rnt_ct_rotate_hoisted")) return rc;
  if (n_steps == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate_hoisted: no steps");
  if (!steps) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate_hoisted: null steps");
  if (int rc = check_same(c0, c1, "rnt_ct_rotate_hoisted")) return rc;
  if (out0->ctx != c0->ctx || out1->ctx != c0->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "rnt_ct_rotate_hoisted: operands belong to different bases");
  const size_t L = c0->ctx->L, B = c0->n_polys;
  if (n_steps > SIZE_MAX / std::max<size_t>(B, 1) || out0->n_polys != n_steps * B || out1->n_polys != n_steps * B)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate_hoisted: outputs of %zu and %zu polys for %zu steps of %zu",
                out0->n_polys, out1->n_polys, n_steps, B);
  size_t nz = 0;
  for (size_t t = 0; t < n_steps; ++t) nz += steps[t] != 0;
  if (nz || keys_a || keys_b) {
    if (int rc = check_key_set("rnt_ct_rotate_hoisted", "", c0->ctx, keys_a, keys_b, n_steps * L)) return rc;
  }
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_rotate_hoisted: the ciphertext must be in coefficient domain");
  if (out0 == out1) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate_hoisted: out0 aliases out1");
  for (const rnt_buf* in : {c0, c1, keys_a, keys_b})
    if (in && (out0 == in || out1 == in || out0->data == in->data || out1->data == in->data))
      return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_rotate_hoisted: an output aliases an input");
  if (int rc = set_device(c0->ctx)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t n = k.t->n, wb = word_bytes(k.t);
  const uint64_t full_ls = limb_stride(c0), out_ls = limb_stride(out0), two_n = 2 * (uint64_t)n;
  const rnt_buf* src[2] = {c0, c1};
  rnt_buf* out[2] = {out0, out1};
  // the digits D | one k_hoist_mac group's accumulator pairs ACC | the automorphism's staging TMP | the gathered
  // c0 (more than one chunk only; the chunk counts it regardless: not the layout's total where one holds the batch)
  const size_t tg = std::min<size_t>(nz, rnt::kHoistT);
  auto lay = [&](bool multi) { return ws_layout(k.t).blocks(L, L).blocks(L, 2 * tg).blocks(L).blocks(L, multi); };
  const size_t bc = nz ? chunk_polys(k.t, lay(true).planes, B) : B;
  const bool multi = bc < B;
  rnt::WsLayout w = lay(multi).chunk(bc);
  CallWs ws(out0);
  if (nz)
    if (int rc = ws.get(w)) return rc;
  char *D = nullptr, *ACC = nullptr, *TMP = nullptr, *X0 = nullptr;
  if (nz) D = w.at(0), ACC = w.at(1), TMP = w.at(2), X0 = w.at(3);
  for (size_t t = 0; t < n_steps; ++t) {
    if (steps[t] != 0) continue;
    for (int o = 0; o < 2; ++o)
      LAUNCH(k.t, rnt::K_COPY,
             rnt::launch_copy_rows(k.s, (char*)out[o]->data + t * B * n * wb, out_ls * wb, src[o]->data,
                                   full_ls * wb, full_ls * wb, L),
             "step-0 copy");
  }
  for (size_t p0 = 0; nz && p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    const char* x0 = (const char*)c0->data + p0 * n * wb;
    if (multi) {
      LAUNCH(kc.t, rnt::K_COPY, rnt::launch_copy_rows(kc.s, X0, cls * wb, x0, full_ls * wb, cls * wb, L),
             "chunk gather");
      x0 = X0;
    }
    auto finish = [&](size_t t, char* A0, char* A1) -> int {
      const uint64_t g = rotation_exponent(steps[t], two_n);
      if (int rc = inv_add_raw(kc, A0, cls, x0)) return rc;
      if (int rc = inv_raw(kc, A1, cls)) return rc;
      char* A[2] = {A0, A1};
      for (int o = 0; o < 2; ++o) {
        char* dst = (char*)out[o]->data + (t * B + p0) * n * wb;
        if (out_ls == cls) {  // one step, one chunk
          LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, dst, A[o], g), "automorphism");
        } else {  // (the automorphism launch takes no limb stride)
          LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, TMP, A[o], g), "automorphism");
          LAUNCH(kc.t, rnt::K_COPY, rnt::launch_copy_rows(kc.s, dst, out_ls * wb, TMP, cls * wb, cls * wb, L),
                 "rotation into its output polys");
        }
      }
      return RNT_OK;
    };
    if (int rc = hoist_chunk(kc, D, ACC, (const char*)c1->data + p0 * n * wb, full_ls, steps, n_steps, keys_a,
                             keys_b, finish))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// ---------------------------------------------------------------------------
// hybrid key-switching: digits of alpha limbs raised to Q u P (ModUp), one
// multiply-accumulate against a key over Q u P, division by P (ModDown)
// ---------------------------------------------------------------------------
namespace {

struct HybridPlan {
  const rnt_ctx* C = nullptr;  // the ciphertext's context (Lv limbs)
  const rnt_ctx* E = nullptr;  // the key's context (Lv + K limbs)
  size_t Lv = 0, K = 0, LE = 0, alpha = 0, beta = 0;
  // the key context's limb map (a level context with a gap; else the identity)
  size_t level = UINT32_MAX, gap = 0;
  rnt::HybridConsts hc{};
  // its hybrid scratch (rnt::hybrid_ws) with `pairs` accumulator pairs
  rnt::WsLayout ws(size_t pairs = 1) const { return rnt::hybrid_ws(C->t->n, C->t->wide ? 8 : 4, LE, beta, pairs); }
};

// The polys between two steps of a key set: a view keeps the full key's beta.
size_t key_step_polys(const rnt_buf* keys, const HybridPlan& pl) { return keys->view_of ? keys->step_polys : pl.beta; }

// The argument rules the three hybrid calls share (no device work).
int hybrid_check(const char* name, const rnt_ctx* C, const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha,
                 HybridPlan* pl) {
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  if (int rc = check_key_buf(key_a, name)) return rc;
  if (int rc = check_key_buf(key_b, name)) return rc;
  if (key_a->ctx != key_b->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the key halves belong to different bases", name);
  const rnt_ctx* E = key_a->ctx;
  const rnt::Tables* tc = C->t.get();
  const rnt::Tables* te = E->t.get();
  if (te->log_n != tc->log_n || te->device != tc->device)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: key and ciphertext bases differ in degree or device", name);
  const size_t Lv = C->L;
  if (E->L <= Lv)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the key basis (%zu limbs) has no special limb above the ciphertext's %zu",
                name, E->L, Lv);
  for (size_t l = 0; l < Lv; ++l)
    if (E->modulus(l) != tc->moduli[l])
      return fail(RNT_ERR_BASIS_MISMATCH, "%s: limb %zu of the key basis is %" PRIu64 ", the ciphertext's %" PRIu64,
                  name, l, E->modulus(l), tc->moduli[l]);
  if (te->wide != tc->wide)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "%s: key and ciphertext bases have different device word widths",
                       name);
  const size_t beta = (Lv + alpha - 1) / alpha;
  if (key_a->n_polys != beta || key_b->n_polys != beta)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, beta, key_a->n_polys != beta ? key_a->n_polys : key_b->n_polys,
                       "a hybrid key for %zu limbs in digits of %zu holds %zu polys", Lv, alpha, beta);
  if (!key_a->in_ntt || !key_b->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: keys must be prepared (rnt_key_prepare)", name);
  pl->C = C;
  pl->E = E;
  pl->Lv = Lv;
  pl->LE = E->L;
  pl->K = E->L - Lv;
  pl->alpha = std::min(alpha, Lv);  // (one digit holds every limb from alpha = Lv on)
  pl->beta = beta;
  if (E->is_level() && E->gap != 0) {
    pl->level = E->level;
    pl->gap = E->gap;
  }
  return RNT_OK;
}

// The device constants of (key limbs, ciphertext limbs, alpha, limb map),
// cached on the key basis' tables -- the map is part of the key: a level view
// and a drop_last prefix of one root can agree in the first three and differ
// in their special primes; the first use allocates and copies, so it cannot be
// recorded into a graph (one un-recorded run first).  Also orders the call
// after the work queued on the key basis' stream where that is another stream
// than the ciphertext's (its keys may still be in preparation there).
int hybrid_prepare(HybridPlan* pl) {
  rnt::Tables* te = pl->E->t.get();
  const rnt::Tables* tc = pl->C->t.get();
  if (te != tc && te->stream != tc->stream && g_capture == nullptr) {
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(hybrid key order)");
    hipError_t e = hipEventRecord(ev, te->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(tc->stream, ev, 0);
    cleanup(hipEventDestroy(ev), "hipEventDestroy(hybrid key order)");
    HIP_TRY(e, "hipStreamWaitEvent(hybrid key order)");
  }
  std::lock_guard<std::mutex> g(te->resc_mu);
  for (auto& e : te->hyb_cache)
    if (e.LE == pl->LE && e.Lv == pl->Lv && e.alpha == pl->alpha && e.level == pl->level && e.gap == pl->gap) {
      pl->hc = e.hc;
      return RNT_OK;
    }
  const rnt::host::HybridLayout lay(pl->Lv, pl->K, pl->alpha);
  std::vector<uint64_t> h(lay.total);
  std::vector<uint64_t> mod(pl->LE);  // the key basis' moduli through the limb map
  for (size_t t = 0; t < pl->LE; ++t) mod[t] = pl->E->modulus(t);
  if (!rnt::host::hybrid_constants(mod.data(), lay, te->wide ? 64 : 32, h.data()))
    return fail(RNT_ERR_BAD_ARGUMENT, "hybrid key-switch: the moduli of the key basis are not pairwise coprime");
  const size_t wb = word_bytes(te);
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, lay.total * wb), "hipMalloc(hybrid constants)");
  hipError_t e;
  if (wb == 4) {
    std::vector<uint32_t> h32(h.begin(), h.end());
    e = hipMemcpy(d, h32.data(), lay.total * 4, hipMemcpyHostToDevice);
  } else {
    e = hipMemcpy(d, h.data(), lay.total * 8, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    cleanup(hipFree(d), "hipFree(hybrid constants)");
    return hip_fail(e, "hipMemcpy(hybrid constants)");
  }
  rnt::HybridDev hd;
  hd.LE = pl->LE;
  hd.Lv = pl->Lv;
  hd.alpha = pl->alpha;
  hd.level = pl->level;
  hd.gap = pl->gap;
  hd.dev = d;
  auto at = [&](size_t o) { return (const void*)((const char*)d + o * wb); };
  hd.hc.yinv = at(lay.yinv), hd.hc.yinvp = at(lay.yinvp);
  hd.hc.conv = at(lay.conv), hd.hc.convp = at(lay.convp);
  hd.hc.pinv = at(lay.pinv), hd.hc.pinvp = at(lay.pinvp);
  hd.hc.pq = at(lay.pq), hd.hc.pqp = at(lay.pqp);
  hd.hc.Pinv = at(lay.Pinv), hd.hc.Pinvp = at(lay.Pinvp);
  hd.hc.Pw = at(lay.Pw), hd.hc.Pwp = at(lay.Pwp);
  hd.hc.Lv = (uint32_t)pl->Lv, hd.hc.K = (uint32_t)pl->K;
  hd.hc.alpha = (uint32_t)pl->alpha, hd.hc.beta = (uint32_t)pl->beta;
  te->hyb_cache.push_back(hd);
  pl->hc = hd.hc;
  return RNT_OK;
}

// A launch of c polys over the key basis: its tables and limb map, on the
// ciphertext context's stream.
rnt::Launch hybrid_launch(const HybridPlan& pl, size_t c) {
  rnt::Launch k;
  k.t = pl.E->t.get();
  k.L = pl.LE;
  k.B = c;
  k.s = pl.C->t->stream;
  k.map_level = (uint32_t)pl.level;
  k.map_gap = (uint32_t)pl.gap;
  return k;
}

// The hybrid scratch carved at ws for c polys: D | A0 | A1 (of the first pair).
struct HybridWs {
  char *D = nullptr, *A0 = nullptr, *A1 = nullptr;
  HybridWs() = default;
  HybridWs(const HybridPlan& pl, size_t c, void* ws, size_t pairs = 1) {
    const rnt::WsLayout w = pl.ws(pairs).chunk(c).place(ws);
    D = w.at(rnt::WS_D), A0 = w.at(rnt::WS_ACC, 0), A1 = w.at(rnt::WS_ACC, 1);
  }
};

// The stages of every hybrid call, for c polys.  Every launch runs on the
// ciphertext context's stream and counts in its profile; the transforms, the
// limb map and the constants are the key basis'.
//
// Raise: D = the forward transforms of ModUp_d(x), x in the coefficient domain
// at limb stride x_ls over the ciphertext's limbs.
int hybrid_raise(const HybridPlan& pl, size_t c, char* D, const void* x, uint64_t x_ls) {
  const rnt::Tables* tc = pl.C->t.get();
  const rnt::Launch k = hybrid_launch(pl, c);
  LAUNCH_ON(tc, k.s, rnt::K_MODUP, rnt::launch_modup(k, D, x, x_ls, pl.hc), "ModUp");
  rnt::Launch kd = k;
  kd.B = pl.beta * c;
  return fwd_raw(kd, D, (uint64_t)kd.B * tc->n, tc);
}

// Products: A0 = sum_d D_d key_b[d], A1 with key_a (one key: beta polys at
// limb stride key_ls) -- stored, added to what A0 / A1 hold, or started from
// the seeds d0^ 2^-w, d1^ 2^-w that stand in the accumulators' first Lv limbs
// (k_hoist_mac_seed: A = sum + P d, so ModDown(A) = ModDown(sum) + d).
enum class HybridMac { set, accumulate, seeded };
int hybrid_products(const HybridPlan& pl, size_t c, const char* D, char* A0, char* A1, const void* key_a,
                    const void* key_b, uint64_t key_ls, HybridMac mode) {
  const rnt::Tables* tc = pl.C->t.get();
  rnt::Launch km = hybrid_launch(pl, c);
  km.Ls = pl.beta;
  void* a0[1] = {A0};
  void* a1[1] = {A1};
  const void* ka[1] = {key_a};
  const void* kb[1] = {key_b};
  switch (mode) {
    case HybridMac::set:
      LAUNCH_ON(tc, km.s, rnt::K_HOIST_MAC, rnt::launch_hoist_mac(km, a0, a1, 1, D, ka, kb, key_ls),
                "hybrid key products");
      break;
    case HybridMac::accumulate:
      LAUNCH_ON(tc, km.s, rnt::K_HOIST_MAC, rnt::launch_hoist_mac_acc(km, a0, a1, 1, D, ka, kb, key_ls),
                "hybrid key products (accumulating)");
      break;
    case HybridMac::seeded:
      LAUNCH_ON(tc, km.s, rnt::K_HOIST_MAC,
                rnt::launch_hoist_mac_seed(km, A0, A1, D, key_a, key_b, key_ls, A1, A0, (uint64_t)c * tc->n, pl.hc),
                "hybrid key products (seeded)");
  }
  return RNT_OK;
}

// Lower: both accumulators back to the coefficient domain, then out0 =
// ModDown(A0) (+ add0), out1 = ModDown(A1) (+ add1) at limb stride out_ls, the
// optional coefficient-domain addends at add_ls; with `rescale` the results
// are rescaled by their last limb on the way out (k_moddown_rescale, Lv - 1
// output limbs).  `af` (rescale alone): the affine epilogue of that kernel,
// out = w r + u z (+ bias on component 0) with r the rescaled result and z0 /
// z1 the chunk's addends at limb stride z_ls (both or neither; z may be out).
struct HybridAffine {
  bool on = false;
  int64_t w = 1, u = 0, bias = 0;
  const void *z0 = nullptr, *z1 = nullptr;
  uint64_t z_ls = 0;
};
int hybrid_lower(const HybridPlan& pl, size_t c, char* A0, char* A1, void* out0, void* out1, uint64_t out_ls,
                 const void* add0, const void* add1, uint64_t add_ls, bool rescale,
                 const HybridAffine& af = HybridAffine{}) {
  const rnt::Tables* tc = pl.C->t.get();
  const rnt::Launch k = hybrid_launch(pl, c);
  const uint64_t cls = (uint64_t)c * tc->n;
  if (int rc = inv_raw(k, A0, cls, tc)) return rc;
  if (int rc = inv_raw(k, A1, cls, tc)) return rc;
  const char* A[2] = {A0, A1};
  void* out[2] = {out0, out1};
  const void* add[2] = {add0, add1};
  for (int o = 0; o < 2; ++o) {
    if (rescale && af.on) {
      rnt::MdAffine ma;
      ma.on = true;
      ma.w = af.w, ma.u = af.u, ma.bias = o == 0 ? af.bias : 0;  // the bias is component 0's
      ma.z = o == 0 ? af.z0 : af.z1, ma.z_ls = af.z_ls;
      LAUNCH_ON(tc, k.s, rnt::K_MODDOWN_RESCALE_AFFINE,
                rnt::launch_moddown_rescale(k, out[o], out_ls, A[o], cls, add[o], add_ls,
                                            rnt::resc_inv_row(tc, pl.Lv - 1, 0), rnt::resc_inv_row(tc, pl.Lv - 1, 1),
                                            pl.hc, ma),
                "ModDown, rescale and affine step");
    } else if (rescale) {
      LAUNCH_ON(tc, k.s, rnt::K_MODDOWN_RESCALE,
                rnt::launch_moddown_rescale(k, out[o], out_ls, A[o], cls, add[o], add_ls,
                                            rnt::resc_inv_row(tc, pl.Lv - 1, 0), rnt::resc_inv_row(tc, pl.Lv - 1, 1),
                                            pl.hc),
                "ModDown and rescale");
    } else {
      LAUNCH_ON(tc, k.s, rnt::K_MODDOWN, rnt::launch_moddown(k, out[o], out_ls, A[o], cls, add[o], add_ls, pl.hc),
                "ModDown");
    }
  }
  return RNT_OK;
}

// One chunk of c polys through the three stages with one key: raise x, the
// products (seeded: from the seeds the caller's tensor left in ws.A0 / ws.A1),
// lower into out0 / out1.
int hybrid_chunk_run(const HybridPlan& pl, size_t c, const HybridWs& ws, const void* x, uint64_t x_ls,
                     const rnt_buf* key_a, const rnt_buf* key_b, void* out0, void* out1, uint64_t out_ls,
                     const void* add0, const void* add1, uint64_t add_ls, bool rescale = false,
                     bool seeded = false, const HybridAffine& af = HybridAffine{}) {
  if (int rc = hybrid_raise(pl, c, ws.D, x, x_ls)) return rc;
  if (int rc = hybrid_products(pl, c, ws.D, ws.A0, ws.A1, key_a->data, key_b->data, limb_stride(key_a),
                               seeded ? HybridMac::seeded : HybridMac::set))
    return rc;
  return hybrid_lower(pl, c, ws.A0, ws.A1, out0, out1, out_ls, add0, add1, add_ls, rescale, af);
}

// INV(d^ 2^-w) 2^w = d, canonical: a tensor output (kc.B polys at limb stride
// ls) back to the coefficient domain, in place.
int seeds_to_coeff(const rnt::Launch& kc, char* Dx, uint64_t ls) {
  if (int rc = inv_raw(kc, Dx, ls)) return rc;
  LAUNCH(kc.t, rnt::K_ELEMENTWISE, rnt::launch_bcast_mul(kc, 1, Dx, Dx, nullptr, 0, false), "seed unscale");
  return RNT_OK;
}

// The relinearisation of a chunk of kc.B ciphertexts whose tensor stands ready
// at limb stride kc.B N: d2 (coefficient domain) through the stages.  seeded:
// D0 == ws.A0 and D1 == ws.A1 hold d0^ 2^-w, d1^ 2^-w and seed the products;
// else D0, D1 go back to the coefficient domain and are ModDown's addends.
int hybrid_relin_chunk(const HybridPlan& pl, const rnt::Launch& kc, const HybridWs& ws, bool rescale, bool seeded,
                       char* D0, char* D1, const char* D2, const rnt_buf* key_a, const rnt_buf* key_b, void* out0,
                       void* out1, uint64_t out_ls, const HybridAffine& af = HybridAffine{}) {
  const uint64_t cls = (uint64_t)kc.B * kc.t->n;
  if (!seeded)
    for (char* Dx : {D0, D1})
      if (int rc = seeds_to_coeff(kc, Dx, cls)) return rc;
  return hybrid_chunk_run(pl, kc.B, ws, D2, cls, key_a, key_b, out0, out1, out_ls, seeded ? nullptr : D0,
                          seeded ? nullptr : D1, cls, rescale, seeded, af);
}

// Whether an NTT-domain plane of the ciphertext context's transforms is, on a
// limb both bases hold, a plane of the key basis': limb j is the same modulus
// and degree (hybrid_check), so the same psi (find_psi is a function of (q, N))
// and the same twiddles; the word width is the same (hybrid_check); and
// fwd_raw / inv_raw choose their kernels from (plane, wide, log_n) alone -- mf
// is set exactly where mf_supported() holds.  What is left is `plane`, read
// from the environment when a root context is created.
bool hybrid_same_transforms(const HybridPlan& pl) { return pl.C->t->plane == pl.E->t->plane; }

// The shared body of rnt_ct_dot_relin_hybrid and its rescaling form.  Per
// chunk of ciphertexts and group of up to kDotT terms: the group's planes are
// gathered into call-scoped workspace (the inputs are const) and transformed
// there, k_dot_tensor sums d0^, d1^, d2^ (2^-w scaled; groups after the first
// accumulate); then one inverse and unscale of d2 and the tail of the hybrid
// multiply -- for the rescaling call with the seeds in the accumulators'
// first Lv limbs where hybrid_same_transforms holds.
int ct_dot_hybrid_body(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0,
                       const rnt_buf* x1, const rnt_buf* y0, const rnt_buf* y1, size_t n_terms, const rnt_buf* key_a,
                       const rnt_buf* key_b, size_t alpha) {
  const rnt_buf* in[4] = {x0, x1, y0, y1};
  for (const rnt_buf* b : {(const rnt_buf*)out0, (const rnt_buf*)out1, x0, x1, y0, y1})
    if (int rc = check_buf(b, name)) return rc;
  if (n_terms == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: n_terms must be at least 1", name);
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (const rnt_buf* b : in)
    if (out0 == b || out1 == b || out0->data == b->data || out1->data == b->data)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input", name);
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(x0, in[i], name)) return rc;
  if (x0->n_polys % n_terms != 0)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: inputs of %zu polys are no %zu terms of a batch", name, x0->n_polys,
                n_terms);
  const size_t B = x0->n_polys / n_terms;
  HybridPlan pl;
  if (int rc = hybrid_check(name, x0->ctx, key_a, key_b, alpha, &pl)) return rc;
  for (const rnt_buf* b : in)
    if (b->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: inputs must be in coefficient domain", name);
  const size_t L = x0->ctx->L;
  if (rescale) {
    if (int rc = rescaled_outputs_check(name, out0, out1, x0, B)) return rc;
  } else {
    for (const rnt_buf* o : {out0, out1}) {
      if (o->ctx != x0->ctx) return fail(RNT_ERR_BASIS_MISMATCH, "%s: an output's basis is not the inputs'", name);
      if (o->n_polys != B)
        return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output of %zu polys for a batch of %zu", name, o->n_polys, B);
    }
  }
  if (int rc = set_device(x0->ctx)) return rc;
  if (int rc = hybrid_prepare(&pl)) return rc;
  rnt::Launch k = launch_for(x0);
  const size_t n = k.t->n, wb = word_bytes(k.t);
  const bool sq = y0->data == x0->data && y1->data == x1->data;  // a sum of squares: each plane transformed once
  const size_t nx = sq ? 2 : 4;
  const size_t gmax = std::min<size_t>(n_terms, rnt::kDotT);
  const bool seeded = rescale && hybrid_same_transforms(pl);
  const size_t nd = seeded ? 1 : 3;  // d2 (and, un-seeded, d0 and d1) over the ciphertext limbs
  // X0 | X1 | [Y0 | Y1] (gmax terms each) | D2 | [D0 | D1] | the hybrid scratch
  enum { WX, WD, WH };
  rnt::WsLayout w = ws_layout(k.t).blocks(gmax * L, nx).blocks(L, nd).sub(pl.ws());
  const size_t bc = fit_chunk(pl.C->t.get(), w, B);
  CallWs cws(out0);
  if (int rc = cws.get(w, 16)) return rc;
  char* X[4];
  for (size_t j = 0; j < 4; ++j) X[j] = w.at(WX, j % nx);
  char *D2 = w.at(WD, 0), *HW = w.at(WH);
  const uint64_t full_ls = limb_stride(x0), out_ls = limb_stride(out0);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    const size_t po = p0 * n * wb;
    const HybridWs hw(pl, c, HW);
    char* D0 = seeded ? hw.A0 : w.at(WD, 1);
    char* D1 = seeded ? hw.A1 : w.at(WD, 2);
    for (size_t t0 = 0; t0 < n_terms; t0 += gmax) {
      const size_t g = std::min(gmax, n_terms - t0);
      rnt::Launch kg = k;
      kg.B = g * c;
      const uint64_t gls = (uint64_t)g * cls;
      for (size_t j = 0; j < nx; ++j) {
        // term t of the chunk: polys [t B + p0, t B + p0 + c) of every limb; one run a limb where the chunk is the batch
        const size_t runs = c == B ? 1 : g;
        for (size_t i = 0; i < runs; ++i)
          LAUNCH(kc.t, rnt::K_COPY,
                 rnt::launch_copy_rows(kc.s, X[j] + i * cls * wb, gls * wb,
                                       (const char*)in[j]->data + ((t0 + i) * B + p0) * n * wb, full_ls * wb,
                                       (c == B ? gls : cls) * wb, L),
                 "term gather");
        if (int rc = fwd_raw(kg, X[j], gls)) return rc;
      }
      LAUNCH(kc.t, rnt::K_DOT_TENSOR,
             rnt::launch_dot_tensor(kc, D0, D1, D2, cls, X[0], X[1], X[2], X[3], gls, cls, g, t0 != 0), "dot tensor");
    }
    if (int rc = seeds_to_coeff(kc, D2, cls)) return rc;  // for ModUp
    if (int rc = hybrid_relin_chunk(pl, kc, hw, rescale, seeded, D0, D1, D2, key_a, key_b, (char*)out0->data + po,
                                    (char*)out1->data + po, out_ls))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_dot_relin_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                                       const rnt_buf* y0, const rnt_buf* y1, size_t n_terms, const rnt_buf* key_a,
                                       const rnt_buf* key_b, size_t alpha) {
  return ct_dot_hybrid_body("rnt_ct_dot_relin_hybrid", false, out0, out1, x0, x1, y0, y1, n_terms, key_a, key_b,
                            alpha);
}

extern "C" int rnt_ct_dot_relin_rescale_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                                               const rnt_buf* y0, const rnt_buf* y1, size_t n_terms,
                                               const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha) {
  return ct_dot_hybrid_body("rnt_ct_dot_relin_rescale_hybrid", true, out0, out1, x0, x1, y0, y1, n_terms, key_a,
                            key_b, alpha);
}

extern "C" int rnt_keyswitch_hybrid(rnt_buf* acc0, rnt_buf* acc1, const rnt_buf* d, const rnt_buf* key_a,
                                    const rnt_buf* key_b, size_t alpha) {
  const char* name = "rnt_keyswitch_hybrid";
  for (const rnt_buf* b : {(const rnt_buf*)acc0, (const rnt_buf*)acc1, d})
    if (int rc = check_buf(b, name)) return rc;
  if (acc0 == acc1 || acc0 == d || acc1 == d || acc0->data == acc1->data || acc0->data == d->data ||
      acc1->data == d->data)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: outputs must not alias each other or d", name);
  if (int rc = check_same(acc0, d, name)) return rc;
  if (int rc = check_same(acc1, d, name)) return rc;
  HybridPlan pl;
  if (int rc = hybrid_check(name, d->ctx, key_a, key_b, alpha, &pl)) return rc;
  if (d->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: d must be in coefficient domain", name);
  if (int rc = set_device(d->ctx)) return rc;
  if (int rc = hybrid_prepare(&pl)) return rc;
  const size_t n = d->ctx->t->n, wb = word_bytes(d->ctx->t.get()), B = d->n_polys;
  rnt::WsLayout w = ws_layout(d->ctx->t.get()).sub(pl.ws());
  const size_t bc = fit_chunk(pl.C->t.get(), w, B);
  CallWs ws(acc0);
  if (int rc = ws.get(w, 16)) return rc;
  const uint64_t ls = limb_stride(d);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    const size_t off = p0 * n * wb;
    if (int rc = hybrid_chunk_run(pl, c, HybridWs(pl, c, w.at(0)), (const char*)d->data + off, ls, key_a, key_b,
                                  (char*)acc0->data + off, (char*)acc1->data + off, ls, nullptr, nullptr, 0))
      return rc;
  }
  acc0->in_ntt = acc1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_ct_rotate_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1, int32_t kk,
                                    const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha) {
  const char* name = "rnt_ct_rotate_hybrid";
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(all[0], all[i], name)) return rc;
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertext must be in coefficient domain", name);
  if (kk == 0) {  // the identity: no key-switch, the key is not read
    if (out0 == c1 && out1 == c0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: the outputs swap the inputs", name);
    if (out0 == c1) {
      if (int rc = rnt_copy(out1, c1)) return rc;
      return rnt_copy(out0, c0);
    }
    if (int rc = rnt_copy(out0, c0)) return rc;
    return rnt_copy(out1, c1);
  }
  HybridPlan pl;
  if (int rc = hybrid_check(name, c0->ctx, key_a, key_b, alpha, &pl)) return rc;
  if (int rc = set_device(c0->ctx)) return rc;
  if (int rc = hybrid_prepare(&pl)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys;
  const size_t words = pl.Lv * B * n;
  const uint64_t g = rotation_exponent(kk, 2 * (uint64_t)n);
  // sigma(c0) | sigma(c1) (the batch, so the outputs may be the inputs) | the hybrid scratch
  rnt::WsLayout w = ws_layout(k.t).bytes(words * wb).bytes(words * wb).sub(pl.ws());
  const size_t bc = fit_chunk(pl.C->t.get(), w, B);
  CallWs ws(out0);
  if (int rc = ws.get(w, 16)) return rc;
  char *sig0 = w.at(0), *sig1 = w.at(1), *HW = w.at(2);
  LAUNCH(k.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(k, sig0, c0->data, g), "automorphism");
  LAUNCH(k.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(k, sig1, c1->data, g), "automorphism");
  const uint64_t ls = limb_stride(c0);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    const size_t off = p0 * n * wb;
    if (int rc = hybrid_chunk_run(pl, c, HybridWs(pl, c, HW), sig1 + off, ls, key_a, key_b, (char*)out0->data + off,
                                  (char*)out1->data + off, ls, sig0 + off, nullptr, ls))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// The shared body of rnt_ct_mul_relin_hybrid and its rescaling form, which is
// that call followed by rnt_ct_rescale, word for word.  Per chunk: the tensor
// of rnt_ct_mul_relin (d0^, d1^ in the NTT domain, scaled by 2^-w, and d2),
// then d2 through the three stages.  The plain call takes d0, d1 back to the
// coefficient domain as ModDown's addends.  The rescaling call has the tensor
// write d0^ 2^-w, d1^ 2^-w into the first Lv limbs of the accumulators A0, A1
// themselves and seeds the products with them: no seed inverse, no unscale
// pass, no addend, no level-Lv product in memory.  Where the two contexts'
// transforms may differ (hybrid_same_transforms) its seeds take the plain
// call's way and only the ModDown is fused with the rescale.
//
// The two calls validate in their own orders: the plain one compares all six
// operands with out0 before it looks at the key; the rescaling one compares
// the inputs with c0, then checks the key and the domain, and its outputs last.
//
// CtAffine (the rescaling call alone, rnt_ct_mul_relin_rescale_affine_hybrid):
// out0 = w r0 + u z0 + bias X^0, out1 = w r1 + u z1 in the epilogue of the two
// closing k_moddown_rescale launches.  Its rules are checked after the
// multiply's own, before any device work.
struct CtAffine {
  int64_t w, u, bias;
  const rnt_buf *z0, *z1;
};
static int ct_affine_check(const char* name, const CtAffine& a, const rnt_buf* out0, const rnt_buf* out1,
                           const rnt_buf* const (&in)[4]) {
  constexpr int64_t kW = (int64_t)1 << 31, kB = (int64_t)1 << 62;
  if (a.w <= -kW || a.w >= kW) return fail(RNT_ERR_BAD_ARGUMENT, "%s: |w| must be below 2^31", name);
  if (a.bias <= -kB || a.bias >= kB) return fail(RNT_ERR_BAD_ARGUMENT, "%s: |bias| must be below 2^62", name);
  for (const rnt_buf* b : in)
    if (out0 == b || out1 == b || out0->data == b->data || out1->data == b->data)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input", name);
  if ((a.z0 == nullptr) != (a.z1 == nullptr))
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: z0 and z1 are both given or both null", name);
  if (a.z0 == nullptr) return RNT_OK;
  if (a.u <= -kW || a.u >= kW) return fail(RNT_ERR_BAD_ARGUMENT, "%s: |u| must be below 2^31", name);
  for (const rnt_buf* z : {a.z0, a.z1}) {
    if (int rc = check_buf(z, name)) return rc;
    if (z->ctx != out0->ctx) return fail(RNT_ERR_BASIS_MISMATCH, "%s: an addend's basis is not the outputs'", name);
    if (z->n_polys != out0->n_polys)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an addend of %zu polys for a batch of %zu", name, z->n_polys,
                  out0->n_polys);
    if (z->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: addends must be in coefficient domain", name);
  }
  // in place: z0 is out0 together with z1 is out1; every other overlap of an addend and an output is refused
  const bool same0 = a.z0 == out0 || a.z0->data == out0->data, same1 = a.z1 == out1 || a.z1->data == out1->data;
  if (same0 != same1 || a.z0 == out1 || a.z0->data == out1->data || a.z1 == out0 || a.z1->data == out0->data)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: an addend aliases an output (only z0 == out0 with z1 == out1 is allowed)",
                name);
  return RNT_OK;
}

static int ct_mul_hybrid_body(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                              const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p, const rnt_buf* key_a,
                              const rnt_buf* key_b, size_t alpha, const CtAffine* aff = nullptr) {
  const rnt_buf* all[6] = {out0, out1, c0, c1, c0p, c1p};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (int i = rescale ? 3 : 1; i < 6; ++i)
    if (int rc = check_same(rescale ? c0 : out0, all[i], name)) return rc;
  HybridPlan pl;
  if (int rc = hybrid_check(name, c0->ctx, key_a, key_b, alpha, &pl)) return rc;
  if (c0->in_ntt || c1->in_ntt || c0p->in_ntt || c1p->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: inputs must be in coefficient domain", name);
  if (rescale)
    if (int rc = rescaled_outputs_check(name, out0, out1, c0, c0->n_polys)) return rc;
  if (aff) {
    const rnt_buf* const in[4] = {c0, c1, c0p, c1p};
    if (int rc = ct_affine_check(name, *aff, out0, out1, in)) return rc;
  }
  if (int rc = set_device(c0->ctx)) return rc;
  if (int rc = hybrid_prepare(&pl)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys;
  const bool seeded = rescale && hybrid_same_transforms(pl);
  const size_t nt = tensor_blocks(k);
  const size_t nd = seeded ? 1 : 3;  // d2 (and, un-seeded, d0 and d1) over the ciphertext limbs
  // [T0..T3] | D2 | [D0 | D1] | the hybrid scratch
  enum { WT, WD, WH };
  rnt::WsLayout w = ws_layout(k.t).blocks(L, nt).blocks(L, nd).sub(pl.ws());
  const size_t bc = fit_chunk(pl.C->t.get(), w, B);
  CallWs cws(out0);
  if (int rc = cws.get(w, 16)) return rc;
  char* T[4] = {};
  for (size_t i = 0; i < nt; ++i) T[i] = w.at(WT, i);
  char *D2 = w.at(WD, 0), *HW = w.at(WH);
  const uint64_t full_ls = limb_stride(c0), out_ls = limb_stride(out0);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    const size_t po = p0 * n * wb;
    auto off = [&](const rnt_buf* b) { return (const char*)b->data + po; };
    const HybridWs hw(pl, c, HW);
    char* D0 = seeded ? hw.A0 : w.at(WD, 1);
    char* D1 = seeded ? hw.A1 : w.at(WD, 2);
    if (int rc = tensor(kc, T, D0, D1, D2, cls, off(c0), off(c1), off(c0p), off(c1p), full_ls)) return rc;
    HybridAffine ha;
    if (aff) {
      ha.on = true;
      ha.w = aff->w, ha.bias = aff->bias;
      if (aff->z0) {  // the chunk's polys of the addends
        ha.u = aff->u;
        ha.z0 = off(aff->z0), ha.z1 = off(aff->z1);
        ha.z_ls = limb_stride(aff->z0);
      }
    }
    if (int rc = hybrid_relin_chunk(pl, kc, hw, rescale, seeded, D0, D1, D2, key_a, key_b, (char*)out0->data + po,
                                    (char*)out1->data + po, out_ls, ha))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_ct_mul_relin_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                       const rnt_buf* c0p, const rnt_buf* c1p, const rnt_buf* key_a,
                                       const rnt_buf* key_b, size_t alpha) {
  return ct_mul_hybrid_body("rnt_ct_mul_relin_hybrid", false, out0, out1, c0, c1, c0p, c1p, key_a, key_b, alpha);
}

extern "C" int rnt_ct_mul_relin_rescale_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                               const rnt_buf* c0p, const rnt_buf* c1p, const rnt_buf* key_a,
                                               const rnt_buf* key_b, size_t alpha) {
  return ct_mul_hybrid_body("rnt_ct_mul_relin_rescale_hybrid", true, out0, out1, c0, c1, c0p, c1p, key_a, key_b,
                            alpha);
}

extern "C" int rnt_ct_mul_relin_rescale_affine_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                                                      const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p,
                                                      const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha,
                                                      int64_t w, const rnt_buf* z0, const rnt_buf* z1, int64_t u,
                                                      int64_t bias) {
  const CtAffine aff{w, u, bias, z0, z1};
  return ct_mul_hybrid_body("rnt_ct_mul_relin_rescale_affine_hybrid", true, out0, out1, c0, c1, c0p, c1p, key_a,
                            key_b, alpha, &aff);
}

// ---------------------------------------------------------------------------
// baby-step giant-step linear transform:
//   R_i = rotate(ct, baby[i]),  V_j = sum_i P[j][i] R_i,  out = sum_j rotate(V_j, giant[j])
// ---------------------------------------------------------------------------
namespace {

// Where the inner sums go and how k_bsgs_mac's launches group them.  Every
// nonzero giant step owns a pair of blocks; the step-0 giants share one (their
// V_j are only ever added), the first storing and the others accumulating, so
// a launch -- a run of consecutive giants, kBsgsJt at the most -- holds at most
// one of them.
struct BsgsPlan {
  struct Group {
    size_t j0;
    uint32_t nj, accum_mask;
  };
  std::vector<size_t> slot;  // giant j's pair of blocks
  std::vector<Group> groups;
  size_t nv = 0;             // pairs of blocks
  size_t zslot = 0;          // the step-0 giants' pair (any_zero)
  bool any_zero = false, any_rot = false;
};

BsgsPlan bsgs_plan(const int32_t* giant, size_t n2) {
  BsgsPlan p;
  p.slot.resize(n2);
  bool zero_in_group = false;
  for (size_t j = 0; j < n2; ++j) {
    const bool zero = giant[j] == 0;
    bool accum = false;
    if (zero) {
      accum = p.any_zero;
      if (!p.any_zero) p.zslot = p.nv++;
      p.any_zero = true;
      p.slot[j] = p.zslot;
    } else {
      p.any_rot = true;
      p.slot[j] = p.nv++;
    }
    if (p.groups.empty() || p.groups.back().nj == rnt::kBsgsJt || (zero && zero_in_group)) {
      p.groups.push_back({j, 0, 0});
      zero_in_group = false;
    }
    BsgsPlan::Group& g = p.groups.back();
    if (accum) g.accum_mask |= 1u << g.nj;
    ++g.nj;
    zero_in_group = zero_in_group || zero;
  }
  return p;
}

// V^ = sum_i R^_i (.) P_ji for every giant j: RB holds the 2 n1 baby blocks
// (block 2 i + component), VB the plan's 2 nv output blocks, each of blk bytes.
int bsgs_inner_sums(const rnt::Launch& k, const BsgsPlan& plan, char* VB, const char* RB, size_t blk,
                    const char* dm, size_t n1, size_t n2) {
  const size_t n = k.t->n, wb = word_bytes(k.t);
  for (const BsgsPlan::Group& g : plan.groups) {
    void* outs[rnt::kBsgsJt] = {};
    for (uint32_t jj = 0; jj < g.nj; ++jj) outs[jj] = VB + 2 * plan.slot[g.j0 + jj] * blk;
    LAUNCH(k.t, rnt::K_BSGS_MAC,
           rnt::launch_bsgs_mac(k, outs, g.nj, g.accum_mask, RB, blk / wb, dm + g.j0 * n1 * n * wb,
                                (uint64_t)n1 * n2 * n, (uint32_t)n1),
           "bsgs inner sums");
  }
  return RNT_OK;
}

// The whole-plane rings: the composition itself on the whole batch -- every
// baby rotation through the whole-plane key-switch and a forward transform,
// the inner sums, one inverse per sum, every giant rotation, adds.
// w, over the batch: dm | RB | VB | T0 T1 | hoisted: the digits | the accumulator blocks (ct_linear_bsgs_body).
int ct_bsgs_composed(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                     const int32_t* baby, size_t n1, const int32_t* giant, size_t n2, const BsgsPlan& plan,
                     const rnt_buf* bka, const rnt_buf* bkb, const rnt_buf* gka, const rnt_buf* gkb,
                     const rnt::WsLayout& w, bool hoisted) {
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, B = c0->n_polys, pw = w.pitch(1);
  const uint64_t ls = limb_stride(c0);
  const char* dm = w.at(0);
  char *RB = w.at(1), *VB = w.at(2), *T = w.at(3), *HD = w.at(4), *HACC = w.at(5);
  const rnt_buf* src[2] = {c0, c1};
  for (size_t i = 0; i < n1; ++i) {
    char* R[2] = {RB + 2 * i * pw, RB + (2 * i + 1) * pw};
    if (baby[i] == 0) {
      for (int o = 0; o < 2; ++o)
        if (int rc = copy_rows(k, R[o], ls, src[o]->data, ls, ls, L)) return rc;
    } else if (hoisted) {
      continue;  // below: one decomposition for all of them
    } else {
      if (int rc = ct_rotate_body(c0->ctx, B, R[0], R[1], c0->data, false, c1->data, false, baby[i],
                                  GadgetKey(bka, bkb, i)))
        return rc;
    }
    for (int o = 0; o < 2; ++o)
      if (int rc = fwd_raw(k, R[o], ls)) return rc;
  }
  if (hoisted) {
    auto finish = [&](size_t i, char* A0, char* A1) -> int {
      return hoisted_baby_finish(k, ls, A0, A1, c0->data, rotation_exponent(baby[i], 2 * (uint64_t)n),
                                 RB + 2 * i * pw, pw);
    };
    if (int rc = hoist_chunk(k, HD, HACC, c1->data, ls, baby, n1, bka, bkb, finish)) return rc;
  }
  if (int rc = bsgs_inner_sums(k, plan, VB, RB, pw, dm, n1, n2)) return rc;
  for (size_t v = 0; v < 2 * plan.nv; ++v)
    if (int rc = inv_raw(k, VB + v * pw, ls)) return rc;
  // (the inputs are consumed: out may be c)
  rnt_buf* out[2] = {out0, out1};
  bool have = false;
  if (plan.any_zero) {
    for (int o = 0; o < 2; ++o)
      if (int rc = copy_rows(k, out[o]->data, ls, VB + (2 * plan.zslot + o) * pw, ls, ls, L)) return rc;
    have = true;
  }
  for (size_t j = 0; j < n2; ++j) {
    if (giant[j] == 0) continue;
    char* V0 = VB + 2 * plan.slot[j] * pw;
    char* r[2] = {have ? T : (char*)out0->data, have ? T + pw : (char*)out1->data};
    if (int rc = ct_rotate_body(c0->ctx, B, r[0], r[1], V0, false, V0 + pw, false, giant[j], GadgetKey(gka, gkb, j)))
      return rc;
    if (have) {
      for (int o = 0; o < 2; ++o)
        LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(k, 0, out[o]->data, out[o]->data, r[o]),
               "add_assign");
    }
    have = true;
  }
  return RNT_OK;
}

// The four-step key-switch: chunks outside as in ct_linear_fused, on
// rnt::lin_fused_ws.
// Baby stage: every nonzero step runs the whole key-switch (sigma(c1) -> rows
// -> lower, sigma(c0) as the addend) into its pair of RB blocks, a step-0 baby
// is a copy; each block is then transformed forward.  Inner sums: k_bsgs_mac,
// one inverse per block.  Giant stage: every nonzero step is a lin_term on
// (V0_j, V1_j) with the Montgomery-one plane `one`; the step-0 giants' sum is
// the addend of the chunk's two inverse column passes (lin_finish).
int ct_bsgs_fused(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1, const int32_t* baby,
                  size_t n1, const int32_t* giant, size_t n2, const BsgsPlan& plan, const rnt_buf* bka,
                  const rnt_buf* bkb, const rnt_buf* gka, const rnt_buf* gkb, const rnt::WsLayout& w, bool hoisted) {
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys, bc = w.bc, pw = w.pitch(rnt::LF_RA);
  const uint64_t full_ls = limb_stride(c0), two_n = 2 * (uint64_t)n;
  const bool multi = bc < B;
  const char *dm = w.at(rnt::LF_DM), *one = w.at(rnt::LF_ONE);
  char* X[2] = {w.at(rnt::LF_X, 0), w.at(rnt::LF_X, 1)};
  char *SIG1 = w.at(rnt::LF_SIG1), *SEED = w.at(rnt::LF_SEED), *RB = w.at(rnt::LF_RA), *VB = w.at(rnt::LF_RB);
  char *HACC = w.at(rnt::LF_HACC), *KS = w.at(rnt::LF_KS);  // (a hoisted call's digits take S)
  char* const tmp[2] = {SEED, SIG1};
  char* Z[2] = {nullptr, nullptr};  // the step-0 giants' sum
  if (plan.any_zero)
    for (int o = 0; o < 2; ++o) Z[o] = VB + (2 * plan.zslot + o) * pw;
  const rnt_buf* src[2] = {c0, c1};
  rnt_buf* out[2] = {out0, out1};
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    rnt::Launch kc = k;
    kc.B = std::min(bc, B - p0);
    const GadgetWs g(kc, KS);
    const uint64_t cls = g.ls;
    const char* x[2];
    char* dst[2];
    for (int o = 0; o < 2; ++o) {
      x[o] = (const char*)src[o]->data + p0 * n * wb;
      dst[o] = (char*)out[o]->data + p0 * n * wb;
      if (int rc = chunk_gather(kc, X[o], &x[o], full_ls)) return rc;
    }
    // baby stage
    const char* zero_done = nullptr;
    for (size_t i = 0; i < n1; ++i) {
      char* R[2] = {RB + 2 * i * pw, RB + (2 * i + 1) * pw};
      if (baby[i] == 0) {
        if (zero_done) {  // NTT(c) is there already
          for (int o = 0; o < 2; ++o)
            if (int rc = copy_rows(kc, R[o], cls, zero_done + o * pw, cls, cls, L)) return rc;
          continue;
        }
        for (int o = 0; o < 2; ++o)
          if (int rc = copy_rows(kc, R[o], cls, x[o], multi ? cls : full_ls, cls, L)) return rc;
        zero_done = R[0];
      } else if (hoisted) {
        continue;  // below: one decomposition for all of them
      } else {
        const uint64_t ge = rotation_exponent(baby[i], two_n);
        LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SIG1, x[1], ge), "automorphism");
        LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SEED, x[0], ge), "automorphism");
        if (int rc = gadget_rows(kc, g, SIG1, cls, GadgetKey(bka, bkb, i), nullptr, nullptr, 0)) return rc;
        if (int rc = gadget_lower(kc, g, R[0], R[1], cls, SEED)) return rc;
      }
      for (int o = 0; o < 2; ++o)
        if (int rc = fwd_raw(kc, R[o], cls)) return rc;
    }
    if (hoisted) {
      auto finish = [&](size_t i, char* A0, char* A1) -> int {
        return hoisted_baby_finish(kc, cls, A0, A1, x[0], rotation_exponent(baby[i], two_n), RB + 2 * i * pw, pw);
      };
      if (int rc = hoist_chunk(kc, g.S, HACC, x[1], cls, baby, n1, bka, bkb, finish)) return rc;
    }
    // inner sums, back to coefficients for the giant decomposition
    if (int rc = bsgs_inner_sums(kc, plan, VB, RB, pw, dm, n1, n2)) return rc;
    for (size_t v = 0; v < 2 * plan.nv; ++v)
      if (int rc = inv_raw(kc, VB + v * pw, cls)) return rc;
    // giant stage
    bool first = true;
    for (size_t j = 0; j < n2; ++j) {
      if (giant[j] == 0) continue;
      const char* V0 = VB + 2 * plan.slot[j] * pw;
      if (int rc = lin_term(kc, g, SIG1, SEED, V0, V0 + pw, rotation_exponent(giant[j], two_n),
                            GadgetKey(gka, gkb, j), one, (uint64_t)n, !first))
        return rc;
      first = false;
    }
    if (int rc = lin_finish(kc, g, plan.any_rot, multi, dst, full_ls, Z, tmp)) return rc;
  }
  return RNT_OK;
}

int check_stage_keys(const rnt_buf* c0, const int32_t* steps, size_t count, const rnt_buf* keys_a,
                     const rnt_buf* keys_b, const char* stage) {
  bool any_rot = false;
  for (size_t t = 0; t < count; ++t) any_rot = any_rot || steps[t] != 0;
  if (!(any_rot || keys_a || keys_b)) return RNT_OK;
  return check_key_set("rnt_ct_linear_bsgs", stage, c0->ctx, keys_a, keys_b, count * c0->ctx->L);
}

}  // namespace

static int ct_linear_bsgs_body(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                               const int32_t* baby_steps, size_t n_baby, const int32_t* giant_steps,
                               size_t n_giant, const rnt_buf* diag, const rnt_buf* baby_keys_a,
                               const rnt_buf* baby_keys_b, const rnt_buf* giant_keys_a,
                               const rnt_buf* giant_keys_b, bool hoisted) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, "rnt_ct_linear_bsgs")) return rc;
  if (int rc = check_buf(diag, "rnt_ct_linear_bsgs")) return rc;
  if (n_baby == 0 || n_giant == 0) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear_bsgs: no steps");
  if (!baby_steps || !giant_steps) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear_bsgs: null steps");
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(all[0], all[i], "rnt_ct_linear_bsgs")) return rc;
  if (diag->ctx != c0->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "rnt_ct_linear_bsgs: the plaintexts belong to a different basis");
  if (n_baby > SIZE_MAX / n_giant || diag->n_polys != n_baby * n_giant)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear_bsgs: %zu plaintexts for %zu x %zu steps", diag->n_polys,
                n_giant, n_baby);
  if (int rc = check_stage_keys(c0, baby_steps, n_baby, baby_keys_a, baby_keys_b, "baby ")) return rc;
  if (int rc = check_stage_keys(c0, giant_steps, n_giant, giant_keys_a, giant_keys_b, "giant ")) return rc;
  if (!diag->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_linear_bsgs: the plaintexts must be in the NTT domain");
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_ct_linear_bsgs: the ciphertext must be in coefficient domain");
  const rnt_buf* ins[7] = {c0, c1, diag, baby_keys_a, baby_keys_b, giant_keys_a, giant_keys_b};
  if (out0 == out1) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_ct_linear_bsgs: out0 aliases out1");
  for (int i = 0; i < 7; ++i) {
    if ((out0 == ins[i] && i != 0) || (out1 == ins[i] && i != 1))
      return fail(RNT_ERR_BAD_ARGUMENT,
                  "rnt_ct_linear_bsgs: an output aliases an input other than its own component");
  }
  if (int rc = set_device(c0->ctx)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t L = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys;
  const size_t n_terms = n_baby * n_giant;
  BsgsPlan plan;
  try {
    plan = bsgs_plan(giant_steps, n_giant);
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  const bool composed = rnt::ks_whole_ok(k.t);
  // the whole-plane rings take the batch; else the chunk is what fits the key-switch workspace cap, counted
  // with the two gather blocks even where one chunk holds the batch (then it is not the layout's total)
  const size_t dm_bytes = L * n_terms * n * wb, acc = hoisted ? rnt::kHoistT : 0;
  auto fused = [&](bool multi) { return rnt::lin_fused_ws(n, wb, L, dm_bytes, true, multi, n_baby, plan.nv, acc); };
  const size_t bc = composed ? B : chunk_polys(k.t, fused(true).planes, B);
  rnt::WsLayout w = fused(bc < B);
  if (composed)  // dm | RB | VB | T0 T1 | hoisted: the digits | the accumulator blocks
    w = ws_layout(k.t).bytes(dm_bytes).blocks(L, 2 * n_baby).blocks(L, 2 * plan.nv).blocks(L, 2).blocks(L, acc ? L : 0)
            .blocks(L, 2 * acc);
  CallWs ws(out0);
  if (int rc = ws.get(w.chunk(bc), 16)) return rc;
  // the plaintexts in Montgomery form (m^ 2^w mod q), once per call: the inner
  // sums' Montgomery products are then the canonical products
  rnt::Launch kd = k;
  kd.B = n_terms;
  LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_bcast_mul(kd, 1, w.at(0), diag->data, nullptr, 0, false),  // dm leads
         "plaintexts to Montgomery form");
  int rc;
  if (composed) {
    rc = ct_bsgs_composed(out0, out1, c0, c1, baby_steps, n_baby, giant_steps, n_giant, plan, baby_keys_a,
                          baby_keys_b, giant_keys_a, giant_keys_b, w, hoisted);
  } else {
    if (plan.any_rot)
      LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_mont_one(k, w.at(rnt::LF_ONE)), "Montgomery one");
    rc = ct_bsgs_fused(out0, out1, c0, c1, baby_steps, n_baby, giant_steps, n_giant, plan, baby_keys_a,
                       baby_keys_b, giant_keys_a, giant_keys_b, w, hoisted);
  }
  if (rc) return rc;
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_ct_linear_bsgs(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                  const int32_t* baby_steps, size_t n_baby, const int32_t* giant_steps,
                                  size_t n_giant, const rnt_buf* diag, const rnt_buf* baby_keys_a,
                                  const rnt_buf* baby_keys_b, const rnt_buf* giant_keys_a,
                                  const rnt_buf* giant_keys_b) {
  return ct_linear_bsgs_body(out0, out1, c0, c1, baby_steps, n_baby, giant_steps, n_giant, diag, baby_keys_a,
                             baby_keys_b, giant_keys_a, giant_keys_b, false);
}

extern "C" int rnt_ct_linear_bsgs_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                          const int32_t* baby_steps, size_t n_baby, const int32_t* giant_steps,
                                          size_t n_giant, const rnt_buf* diag, const rnt_buf* baby_keys_a,
                                          const rnt_buf* baby_keys_b, const rnt_buf* giant_keys_a,
                                          const rnt_buf* giant_keys_b) {
  return ct_linear_bsgs_body(out0, out1, c0, c1, baby_steps, n_baby, giant_steps, n_giant, diag, baby_keys_a,
                             baby_keys_b, giant_keys_a, giant_keys_b, true);
}

// ---------------------------------------------------------------------------
// hoisted rotations and the baby-step giant-step transform on hybrid keys:
//   out_t = sigma_t(c0 + ModDown(sum_d D_d sigma_t^-1(key_b[t][d]))),
//           sigma_t(     ModDown(sum_d D_d sigma_t^-1(key_a[t][d])))
// with D_d = ModUp_d(c1) raised and transformed once for every step
// ---------------------------------------------------------------------------
namespace {

// The argument rules of one stage's hybrid key set (n steps, n beta polys over
// E): hybrid_check's on a one-key view, then the key-count rule of
// rnt_ct_rotate_hoisted.  *nz: the steps that rotate.  *have: the stage has
// keys (else nothing is checked: every step is 0 and both buffers are NULL).
int hybrid_set_check(const char* name, const rnt_ctx* C, const int32_t* steps, size_t n_steps,
                     const rnt_buf* keys_a, const rnt_buf* keys_b, size_t alpha, HybridPlan* pl, size_t* nz,
                     bool* have) {
  *nz = 0;
  for (size_t t = 0; t < n_steps; ++t) *nz += steps[t] != 0;
  *have = *nz || keys_a || keys_b;
  if (!*have) return RNT_OK;
  if (int rc = check_key_buf(keys_a, name)) return rc;
  if (int rc = check_key_buf(keys_b, name)) return rc;
  const size_t beta = alpha >= C->L ? 1 : (C->L + alpha - 1) / alpha;
  rnt_buf va, vb;  // step 0's slot: a key of beta polys for hybrid_check
  auto view = [&](rnt_buf& v, const rnt_buf* kbuf) {
    v.ctx = kbuf->ctx;
    v.n_polys = beta;
    v.data = kbuf->data;
    v.in_ntt = kbuf->in_ntt;
    v.owns = false;
    v.view_of = kbuf->view_of;
    v.stored_polys = kbuf->stored_polys;
    v.step_polys = kbuf->step_polys;
  };
  view(va, keys_a);
  view(vb, keys_b);
  if (int rc = hybrid_check(name, C, &va, &vb, alpha, pl)) return rc;
  const size_t want = n_steps * beta;
  if (n_steps > SIZE_MAX / beta || keys_a->n_polys != want || keys_b->n_polys != want)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, want, keys_a->n_polys != want ? keys_a->n_polys : keys_b->n_polys,
                       "%s: the key set must hold one poly per step and digit (%zu)", name, want);
  return RNT_OK;
}

// Whether the tail of a chunk of bc ciphertexts is k_moddown_auto.  Its result
// planes leave as single words.  Measured (profiles/
// rotate_hybrid_hoisted_bench.jsonl): with 4 MiB a
// component (one ciphertext, 2^16 x 16) the fused kernel is the faster tail,
// 1.03-1.08x; with 16 MiB (2^17 x 32) and with 256 MiB (64 ciphertexts) the
// three un-fused launches win on eight steps, 1.04x and 1.10x.  Nothing was
// measured between 4 and 16 MiB: the crossover is put at the smallest size at
// which the un-fused tail was seen to win, which is a guess, as is the reading
// that the partial lines stop meeting in the L2s there.
constexpr size_t kMdAutoBytes = (size_t)16 << 20;
bool tail_fused(const rnt::Tables* tc, size_t Lv, size_t bc) {
  if (tc->md_auto != 1) return tc->md_auto == 2;
  return Lv * bc * tc->n * word_bytes(tc) < kMdAutoBytes;
}

// The layout of a hoisted call, chunked to fit the cap.  lay(tmp) declares it with `tmp` staging blocks for the tail.
// The tail is chosen for the chunk that fits without staging; an un-fused tail then shrinks the chunk to make room.
template <class Lay>
rnt::WsLayout hoist_layout(const HybridPlan& pl, size_t B, Lay&& lay, bool* fused) {
  const rnt::Tables* tc = pl.C->t.get();
  rnt::WsLayout w = lay(0);
  *fused = tail_fused(tc, pl.Lv, fit_chunk(tc, w, B));
  if (!*fused) fit_chunk(tc, w = lay(2), B);
  return w;
}

// The per-step tail: dst = sigma_g(ModDown(A) (+ add)) at limb stride dst_ls,
// A the coefficient-domain accumulator of c polys over E.  fused: one
// k_moddown_auto; else k_moddown into TMP, the automorphism launch into TMP +
// one block and a strided copy (TMP: two blocks of Lv c N words).
int hybrid_tail(const HybridPlan& pl, size_t c, char* dst, uint64_t dst_ls, const char* A, const void* add,
                uint64_t add_ls, uint64_t g, char* TMP, bool fused) {
  const rnt::Tables* tc = pl.C->t.get();
  const rnt::Launch k = hybrid_launch(pl, c);
  const uint64_t cls = (uint64_t)c * tc->n;
  if (fused) {
    LAUNCH_ON(tc, k.s, rnt::K_MODDOWN_AUTO, rnt::launch_moddown_auto(k, dst, dst_ls, A, cls, add, add_ls, g, pl.hc),
              "ModDown with automorphism");
    return RNT_OK;
  }
  const size_t wb = word_bytes(tc);
  char* T2 = TMP + pl.Lv * cls * wb;
  LAUNCH_ON(tc, k.s, rnt::K_MODDOWN, rnt::launch_moddown(k, TMP, cls, A, cls, add, add_ls, pl.hc), "ModDown");
  rnt::Launch kc;
  kc.t = tc;
  kc.L = pl.Lv;
  kc.B = c;
  kc.s = tc->stream;
  LAUNCH(tc, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, T2, TMP, g), "automorphism");
  LAUNCH(tc, rnt::K_COPY, rnt::launch_copy_rows(kc.s, dst, dst_ls * wb, T2, cls * wb, cls * wb, pl.Lv),
         "rotation into its output polys");
  return RNT_OK;
}

// The hoisted hybrid sums of one chunk (c polys of c1 at limb stride x1_ls):
// one ModUp and one forward transform of D ([LE][beta c][N]) on E's tables,
// then one k_hoist_mac launch per group of kHoistT nonzero steps into ACC
// (ws.A0 on: 2 kHoistT blocks of [LE][c][N]), both accumulators taken back to the
// coefficient domain, and finish(t, A0, A1) for every step t of the group:
// A0 = sum_d D_d sigma_t^-1(key_b[t][d]) over E.  The caller has seen a step
// that rotates.
template <class Finish>
int hybrid_hoist_chunk(const HybridPlan& pl, size_t c, const HybridWs& ws, const void* x1, uint64_t x1_ls,
                       const int32_t* steps, size_t n_steps, const rnt_buf* keys_a, const rnt_buf* keys_b,
                       Finish&& finish) {
  const rnt::Tables* tc = pl.C->t.get();
  const size_t n = tc->n, wb = word_bytes(tc);
  const rnt::Launch k = hybrid_launch(pl, c);
  const size_t pe = pl.LE * c * n * wb;  // (the chunk's own pitch: a last chunk packs its pairs closer)
  const uint64_t cls = (uint64_t)c * n;
  if (int rc = hybrid_raise(pl, c, ws.D, x1, x1_ls)) return rc;
  rnt::Launch km = k;
  km.Ls = pl.beta;
  for (size_t t = 0; t < n_steps;) {
    size_t idx[rnt::kHoistT];
    void* a0[rnt::kHoistT] = {};
    void* a1[rnt::kHoistT] = {};
    const void* ka[rnt::kHoistT] = {};
    const void* kb[rnt::kHoistT] = {};
    uint32_t nt = 0;
    for (; t < n_steps && nt < rnt::kHoistT; ++t) {
      if (steps[t] == 0) continue;
      idx[nt] = t;
      a0[nt] = ws.A0 + 2 * nt * pe;
      a1[nt] = ws.A0 + (2 * nt + 1) * pe;
      ka[nt] = (const char*)keys_a->data + t * key_step_polys(keys_a, pl) * n * wb;
      kb[nt] = (const char*)keys_b->data + t * key_step_polys(keys_b, pl) * n * wb;
      ++nt;
    }
    if (nt == 0) break;
    LAUNCH_ON(tc, k.s, rnt::K_HOIST_MAC, rnt::launch_hoist_mac(km, a0, a1, nt, ws.D, ka, kb, limb_stride(keys_a)),
              "hoisted hybrid key products");
    for (uint32_t u = 0; u < nt; ++u) {
      if (int rc = inv_raw(k, a0[u], cls, tc)) return rc;
      if (int rc = inv_raw(k, a1[u], cls, tc)) return rc;
      if (int rc = finish(idx[u], (char*)a0[u], (char*)a1[u])) return rc;
    }
  }
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_rotate_hybrid_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                            const int32_t* steps, size_t n_steps, const rnt_buf* keys_a,
                                            const rnt_buf* keys_b, size_t alpha) {
  const char* name = "rnt_ct_rotate_hybrid_hoisted";
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (n_steps == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: no steps", name);
  if (!steps) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null steps", name);
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  if (int rc = check_same(c0, c1, name)) return rc;
  if (out0->ctx != c0->ctx || out1->ctx != c0->ctx)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: operands belong to different bases", name);
  const size_t B = c0->n_polys;
  if (n_steps > SIZE_MAX / std::max<size_t>(B, 1) || out0->n_polys != n_steps * B || out1->n_polys != n_steps * B)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: outputs of %zu and %zu polys for %zu steps of %zu", name, out0->n_polys,
                out1->n_polys, n_steps, B);
  HybridPlan pl;
  size_t nz = 0;
  bool have = false;
  if (int rc = hybrid_set_check(name, c0->ctx, steps, n_steps, keys_a, keys_b, alpha, &pl, &nz, &have)) return rc;
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertext must be in coefficient domain", name);
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (const rnt_buf* in : {c0, c1, keys_a, keys_b})
    if (in && (out0 == in || out1 == in || out0->data == in->data || out1->data == in->data))
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input", name);
  if (int rc = set_device(c0->ctx)) return rc;
  if (nz)
    if (int rc = hybrid_prepare(&pl)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t n = k.t->n, wb = word_bytes(k.t), Lv = k.L;
  const uint64_t full_ls = limb_stride(c0), out_ls = limb_stride(out0), two_n = 2 * (uint64_t)n;
  const rnt_buf* src[2] = {c0, c1};
  rnt_buf* out[2] = {out0, out1};
  // the hybrid scratch with a k_hoist_mac group's accumulator pairs | the tail's staging, where a step rotates
  bool fused = true;
  size_t bc = B;
  HybridWs hw;
  char* TMP = nullptr;
  CallWs ws(out0);
  if (nz) {
    const size_t tg = std::min<size_t>(nz, rnt::kHoistT);
    auto lay = [&](size_t tmp) { return ws_layout(k.t).sub(pl.ws(tg)).blocks(Lv, tmp); };
    rnt::WsLayout w = hoist_layout(pl, B, lay, &fused);
    bc = w.bc;
    if (int rc = ws.get(w)) return rc;
    hw = HybridWs(pl, bc, w.at(0), tg);
    TMP = w.at(1);
  }
  for (size_t t = 0; t < n_steps; ++t) {
    if (steps[t] != 0) continue;
    for (int o = 0; o < 2; ++o)
      LAUNCH(k.t, rnt::K_COPY,
             rnt::launch_copy_rows(k.s, (char*)out[o]->data + t * B * n * wb, out_ls * wb, src[o]->data,
                                   full_ls * wb, full_ls * wb, Lv),
             "step-0 copy");
  }
  for (size_t p0 = 0; nz && p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    const char* x0 = (const char*)c0->data + p0 * n * wb;
    auto finish = [&](size_t t, char* A0, char* A1) -> int {
      const uint64_t g = rotation_exponent(steps[t], two_n);
      const size_t off = (t * B + p0) * n * wb;
      if (int rc = hybrid_tail(pl, c, (char*)out0->data + off, out_ls, A0, x0, full_ls, g, TMP, fused)) return rc;
      return hybrid_tail(pl, c, (char*)out1->data + off, out_ls, A1, nullptr, 0, g, TMP, fused);
    };
    if (int rc = hybrid_hoist_chunk(pl, c, hw, (const char*)c1->data + p0 * n * wb, full_ls, steps, n_steps,
                                    keys_a, keys_b, finish))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// Rotate-and-sum on hybrid keys: with NZ the steps that rotate, z the others,
//   A0   = sum_{t in NZ} sum_d sigma_t(D_d) key_b[t][d] over E,  A1 with key_a
//   out0 = z c0 + sum_{t in NZ} sigma_t(c0) + ModDown(A0),  out1 = z c1 + ModDown(A1)
// with D_d = ModUp_d(c1) raised and transformed ONCE: sigma_t acts on the
// transformed digits as a gather (k_rotsum_mac).  Per chunk: hybrid_raise, one
// k_rotsum_mac launch per group of kRotsumT rotating steps into one A0 / A1,
// one k_rotsum_c0 launch per group of kRotsumT steps into S (and, where z != 0,
// one for z c1 into S1), hybrid_lower with S / S1 as ModDown's addends.
extern "C" int rnt_ct_rotsum_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                    const int32_t* steps, size_t n_steps, const rnt_buf* keys_a,
                                    const rnt_buf* keys_b, size_t alpha) {
  const char* name = "rnt_ct_rotsum_hybrid";
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (n_steps == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: no steps", name);
  if (!steps) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null steps", name);
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  for (int i = 1; i < 4; ++i)
    if (int rc = check_same(all[0], all[i], name)) return rc;
  HybridPlan pl;
  size_t nz = 0;
  bool have = false;
  if (int rc = hybrid_set_check(name, c0->ctx, steps, n_steps, keys_a, keys_b, alpha, &pl, &nz, &have)) return rc;
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertext must be in coefficient domain", name);
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  const rnt_buf* ins[4] = {c0, c1, keys_a, keys_b};
  for (int i = 0; i < 4; ++i) {
    if (!ins[i]) continue;
    if ((i != 0 && (out0 == ins[i] || out0->data == ins[i]->data)) ||
        (i != 1 && (out1 == ins[i] || out1->data == ins[i]->data)))
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input other than its own component", name);
  }
  if (int rc = set_device(c0->ctx)) return rc;
  if (nz)
    if (int rc = hybrid_prepare(&pl)) return rc;
  const rnt::Launch k = launch_for(c0);
  const rnt::Tables* tc = k.t;
  const size_t n = tc->n, wb = word_bytes(tc), Lv = k.L, B = c0->n_polys;
  const size_t z = n_steps - nz;
  const uint64_t full_ls = limb_stride(c0), two_n = 2 * (uint64_t)n;
  // the hybrid scratch (where a step rotates) | S over C (the c0 sum) | S1 over C (z c1, where a step is 0)
  rnt::WsLayout w = ws_layout(tc).sub(nz ? pl.ws() : ws_layout(tc)).blocks(Lv).blocks(Lv, z ? 1 : 0);
  const size_t bc = fit_chunk(tc, w, B);
  CallWs ws(out0);
  if (int rc = ws.get(w)) return rc;
  char *S = w.at(1), *S1 = w.at(2);
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    const uint64_t cls = (uint64_t)c * n;
    const char* x0 = (const char*)c0->data + p0 * n * wb;
    const char* x1 = (const char*)c1->data + p0 * n * wb;
    char* dst0 = (char*)out0->data + p0 * n * wb;
    char* dst1 = (char*)out1->data + p0 * n * wb;
    rnt::Launch kc = k;
    kc.B = c;
    // S = z c0 + sum sigma_t(c0), kRotsumT steps a launch; S1 = z c1
    for (size_t t = 0; t < n_steps;) {
      uint64_t g[rnt::kRotsumT];
      uint32_t nt = 0, zg = 0;
      const bool first = t == 0;
      for (size_t e = std::min(n_steps, t + rnt::kRotsumT); t < e; ++t) {
        if (steps[t] == 0) ++zg;
        else g[nt++] = rotation_exponent(steps[t], two_n);
      }
      LAUNCH(tc, rnt::K_ROTSUM_C0, rnt::launch_rotsum_c0(kc, S, x0, full_ls, nt, g, zg, !first),
             "rotate-and-sum of c0");
    }
    if (z)
      LAUNCH(tc, rnt::K_ROTSUM_C0, rnt::launch_rotsum_c0(kc, S1, x1, full_ls, 0, nullptr, (uint32_t)z, false),
             "z c1");
    if (!nz) {
      LAUNCH(tc, rnt::K_COPY, rnt::launch_copy_rows(k.s, dst0, full_ls * wb, S, cls * wb, cls * wb, Lv), "z c0");
      LAUNCH(tc, rnt::K_COPY, rnt::launch_copy_rows(k.s, dst1, full_ls * wb, S1, cls * wb, cls * wb, Lv), "z c1");
      continue;
    }
    const HybridWs hw(pl, bc, w.at(0));  // (at the call's pitch in every chunk)
    if (int rc = hybrid_raise(pl, c, hw.D, x1, full_ls)) return rc;
    rnt::Launch km = hybrid_launch(pl, c);
    km.Ls = pl.beta;
    bool first = true;
    for (size_t t = 0; t < n_steps;) {
      uint64_t g[rnt::kRotsumT];
      const void* ka[rnt::kRotsumT] = {};
      const void* kb[rnt::kRotsumT] = {};
      uint32_t nt = 0;
      for (; t < n_steps && nt < rnt::kRotsumT; ++t) {
        if (steps[t] == 0) continue;
        g[nt] = rotation_exponent(steps[t], two_n);
        ka[nt] = (const char*)keys_a->data + t * key_step_polys(keys_a, pl) * n * wb;
        kb[nt] = (const char*)keys_b->data + t * key_step_polys(keys_b, pl) * n * wb;
        ++nt;
      }
      if (nt == 0) break;
      LAUNCH_ON(tc, km.s, rnt::K_ROTSUM_MAC,
                rnt::launch_rotsum_mac(km, hw.A0, hw.A1, nt, g, hw.D, ka, kb, limb_stride(keys_a), !first),
                "rotate-and-sum key products");
      first = false;
    }
    if (int rc = hybrid_lower(pl, c, hw.A0, hw.A1, dst0, dst1, full_ls, S, S1, cls, false)) return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

// rnt_ct_linear_bsgs_hybrid (rescale false) and rnt_ct_linear_bsgs_hybrid_rescale
// (true): the same stages; with `rescale` the outputs are on drop_last(1) of
// the ciphertext's context and the tail is the rescaling one -- with a nonzero
// giant step the two final ModDowns are k_moddown_rescale with the same
// addends, without one k_rescale reads the sums (no fusion there).
static int ct_linear_bsgs_hybrid_body(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1,
                                      const rnt_buf* c0, const rnt_buf* c1, const int32_t* baby_steps, size_t n_baby,
                                      const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                                      const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                      const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (int rc = check_buf(diag, name)) return rc;
  if (n_baby == 0 || n_giant == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: no steps", name);
  if (!baby_steps || !giant_steps) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null steps", name);
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  if (rescale) {
    if (int rc = check_same(c0, c1, name)) return rc;
  } else {
    for (int i = 1; i < 4; ++i)
      if (int rc = check_same(all[0], all[i], name)) return rc;
  }
  if (diag->ctx != c0->ctx) return fail(RNT_ERR_BASIS_MISMATCH, "%s: the plaintexts belong to a different basis", name);
  if (n_baby > SIZE_MAX / n_giant || diag->n_polys != n_baby * n_giant)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: %zu plaintexts for %zu x %zu steps", name, diag->n_polys, n_giant, n_baby);
  HybridPlan plb, plg;
  size_t nzb = 0, nzg = 0;
  bool have_b = false, have_g = false;
  if (int rc = hybrid_set_check(name, c0->ctx, baby_steps, n_baby, baby_keys_a, baby_keys_b, alpha, &plb, &nzb,
                                &have_b))
    return rc;
  if (int rc = hybrid_set_check(name, c0->ctx, giant_steps, n_giant, giant_keys_a, giant_keys_b, alpha, &plg, &nzg,
                                &have_g))
    return rc;
  if (have_b && have_g && plb.E != plg.E)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the baby and giant keys belong to different key bases", name);
  if (!diag->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the plaintexts must be in the NTT domain", name);
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertext must be in coefficient domain", name);
  if (rescale)
    if (int rc = rescaled_outputs_check(name, out0, out1, c0, c0->n_polys)) return rc;
  const rnt_buf* ins[7] = {c0, c1, diag, baby_keys_a, baby_keys_b, giant_keys_a, giant_keys_b};
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (int i = 0; i < 7; ++i) {
    if ((out0 == ins[i] && i != 0) || (out1 == ins[i] && i != 1))
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input other than its own component", name);
  }
  BsgsPlan plan;
  try {
    plan = bsgs_plan(giant_steps, n_giant);
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  const bool hyb = nzb != 0 || nzg != 0;
  HybridPlan pl = have_b ? plb : plg;
  if (int rc = set_device(c0->ctx)) return rc;
  if (hyb)
    if (int rc = hybrid_prepare(&pl)) return rc;
  rnt::Launch k = launch_for(c0);
  const size_t Lv = k.L, n = k.t->n, wb = word_bytes(k.t), B = c0->n_polys;
  const size_t n_terms = n_baby * n_giant;
  const uint64_t full_ls = limb_stride(c0), two_n = 2 * (uint64_t)n;
  // dm, then chunk blocks over C: the baby blocks | the inner sums | SIG1 | SIG0 | S0 | the tail's staging; over E
  // the hybrid scratch: its pairs the baby stage's k_hoist_mac group, then the giant stage's one A0 / A1 there
  const size_t tg = std::max<size_t>(std::min<size_t>(nzb, rnt::kHoistT), 1);
  enum { WDM, WRB, WVB, WSIG1, WSIG0, WS0X, WTMP, WH };
  auto lay = [&](size_t tmp) {
    return ws_layout(k.t).bytes(Lv * n_terms * n * wb).blocks(Lv, 2 * n_baby).blocks(Lv, 2 * plan.nv).blocks(Lv)
        .blocks(Lv).blocks(Lv).blocks(Lv, tmp).sub(hyb ? pl.ws(tg) : ws_layout(k.t));
  };
  bool fused = true;
  rnt::WsLayout w = hyb ? hoist_layout(pl, B, lay, &fused) : lay(0);
  if (!hyb) fit_chunk(k.t, w, B);
  const size_t bc = w.bc, pw = w.pitch(WRB);
  CallWs ws(out0);
  if (int rc = ws.get(w)) return rc;
  // the plaintexts in Montgomery form (m^ 2^w mod q), once per call: the inner
  // sums' Montgomery products are then the canonical products
  char *dm = w.at(WDM), *TMP = w.at(WTMP);
  rnt::Launch kdm = k;
  kdm.B = n_terms;
  LAUNCH(k.t, rnt::K_ELEMENTWISE, rnt::launch_bcast_mul(kdm, 1, dm, diag->data, nullptr, 0, false),
         "plaintexts to Montgomery form");
  char *RB = w.at(WRB), *VB = w.at(WVB), *SIG1 = w.at(WSIG1), *SIG0 = w.at(WSIG0), *S0X = w.at(WS0X);
  const HybridWs hw = hyb ? HybridWs(pl, bc, w.at(WH), tg) : HybridWs();
  rnt_buf* out[2] = {out0, out1};
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    const char* x[2] = {(const char*)c0->data + p0 * n * wb, (const char*)c1->data + p0 * n * wb};
    // baby stage: R_i into RB (block 2 i + component, chunk pitch), NTT domain
    for (size_t i = 0; i < n_baby; ++i) {
      if (baby_steps[i] != 0) continue;
      for (int o = 0; o < 2; ++o) {
        char* R = RB + (2 * i + o) * pw;
        if (int rc = copy_rows(kc, R, cls, x[o], full_ls, cls, Lv)) return rc;
        if (int rc = fwd_raw(kc, R, cls)) return rc;
      }
    }
    if (nzb) {
      auto finish = [&](size_t i, char* A0, char* A1) -> int {
        const uint64_t g = rotation_exponent(baby_steps[i], two_n);
        char* R0 = RB + 2 * i * pw;
        if (int rc = hybrid_tail(pl, c, R0, cls, A0, x[0], full_ls, g, TMP, fused)) return rc;
        if (int rc = hybrid_tail(pl, c, R0 + pw, cls, A1, nullptr, 0, g, TMP, fused)) return rc;
        if (int rc = fwd_raw(kc, R0, cls)) return rc;
        return fwd_raw(kc, R0 + pw, cls);
      };
      if (int rc = hybrid_hoist_chunk(pl, c, hw, x[1], full_ls, baby_steps, n_baby, baby_keys_a, baby_keys_b,
                                      finish))
        return rc;
    }
    // inner sums, back to coefficients
    if (int rc = bsgs_inner_sums(kc, plan, VB, RB, pw, dm, n_baby, n_giant)) return rc;
    for (size_t v = 0; v < 2 * plan.nv; ++v)
      if (int rc = inv_raw(kc, VB + v * pw, cls)) return rc;
    // giant stage: sigma(V1_j) -> ModUp -> forward -> products summed into ONE
    // A0, A1 over E; sigma(V0_j) summed over C into S0, ModDown's addend
    char* S0 = plan.any_zero ? VB + 2 * plan.zslot * pw : S0X;
    char *A0 = hw.A0, *A1 = hw.A1;
    bool first = true;
    for (size_t j = 0; j < n_giant; ++j) {
      if (giant_steps[j] == 0) continue;
      const char* V0 = VB + 2 * plan.slot[j] * pw;
      const uint64_t g = rotation_exponent(giant_steps[j], two_n);
      LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SIG1, V0 + pw, g), "automorphism");
      if (first && !plan.any_zero) {
        LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, S0, V0, g), "automorphism");
      } else {
        LAUNCH(kc.t, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SIG0, V0, g), "automorphism");
        LAUNCH(kc.t, rnt::K_ELEMENTWISE, rnt::launch_elementwise(kc, 0, S0, S0, SIG0), "add_assign");
      }
      if (int rc = hybrid_raise(pl, c, hw.D, SIG1, cls)) return rc;
      if (int rc = hybrid_products(pl, c, hw.D, A0, A1,
                                   (const char*)giant_keys_a->data + j * key_step_polys(giant_keys_a, pl) * n * wb,
                                   (const char*)giant_keys_b->data + j * key_step_polys(giant_keys_b, pl) * n * wb,
                                   limb_stride(giant_keys_a), first ? HybridMac::set : HybridMac::accumulate))
        return rc;
      first = false;
    }
    char* dst[2] = {(char*)out[0]->data + p0 * n * wb, (char*)out[1]->data + p0 * n * wb};
    if (!plan.any_rot) {
      for (int o = 0; o < 2; ++o) {
        const char* V = VB + (2 * plan.zslot + o) * pw;
        if (rescale) {
          LAUNCH(kc.t, rnt::K_RESCALE, rnt::launch_rescale_strided(kc, dst[o], limb_stride(out[o]), V, cls), "rescale");
        } else if (int rc = copy_rows(kc, dst[o], full_ls, V, cls, cls, Lv)) {
          return rc;
        }
      }
    } else {
      // (both outputs have the batch's polys, on the ciphertext's limbs or on one fewer: one limb stride)
      const char* Z1 = plan.any_zero ? VB + (2 * plan.zslot + 1) * pw : nullptr;
      if (int rc = hybrid_lower(pl, c, A0, A1, dst[0], dst[1], limb_stride(out0), S0, Z1, cls, rescale)) return rc;
    }
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_ct_linear_bsgs_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                         const int32_t* baby_steps, size_t n_baby, const int32_t* giant_steps,
                                         size_t n_giant, const rnt_buf* diag, const rnt_buf* baby_keys_a,
                                         const rnt_buf* baby_keys_b, const rnt_buf* giant_keys_a,
                                         const rnt_buf* giant_keys_b, size_t alpha) {
  return ct_linear_bsgs_hybrid_body("rnt_ct_linear_bsgs_hybrid", false, out0, out1, c0, c1, baby_steps, n_baby,
                                    giant_steps, n_giant, diag, baby_keys_a, baby_keys_b, giant_keys_a, giant_keys_b,
                                    alpha);
}

extern "C" int rnt_ct_linear_bsgs_hybrid_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                                 const int32_t* baby_steps, size_t n_baby,
                                                 const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                                                 const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                                 const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b,
                                                 size_t alpha) {
  return ct_linear_bsgs_hybrid_body("rnt_ct_linear_bsgs_hybrid_rescale", true, out0, out1, c0, c1, baby_steps, n_baby,
                                    giant_steps, n_giant, diag, baby_keys_a, baby_keys_b, giant_keys_a, giant_keys_b,
                                    alpha);
}

// rnt_ct_linear_bsgs_hybrid_dh (rescale false) and its _rescale form: the
// double-hoisted transform.  The baby key products T_i stay over E in the NTT
// domain; k_dh_bsgs_mac reads them through sigma_{b_i}'s permutation, adds the
// P c0 seed and forms the inner sums Vt_j over E against the plaintexts over
// E; k_dh_bsgs_fold starts A0 / A1 from the first components; each rotating
// giant takes ModDown(Vt1_j) through the automorphism, ModUp and its key into
// the same A0 / A1; two ModDowns (with the rescale in them where asked) close
// the call.  No special case: with every step 0 the accumulators hold P x on
// the q-limbs and 0 on the special ones, and ModDown returns x.
static int ct_linear_bsgs_hybrid_dh_body(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1,
                                         const rnt_buf* c0, const rnt_buf* c1, const int32_t* baby_steps,
                                         size_t n_baby, const int32_t* giant_steps, size_t n_giant,
                                         const rnt_buf* diagE, const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                         const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha) {
  const rnt_buf* all[4] = {out0, out1, c0, c1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (int rc = check_buf(diagE, name)) return rc;
  if (n_baby == 0 || n_giant == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: no steps", name);
  if (!baby_steps || !giant_steps) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null steps", name);
  if (alpha == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: alpha must be at least 1", name);
  if (rescale) {
    if (int rc = check_same(c0, c1, name)) return rc;
  } else {
    for (int i = 1; i < 4; ++i)
      if (int rc = check_same(all[0], all[i], name)) return rc;
  }
  HybridPlan plb, plg;
  size_t nzb = 0, nzg = 0;
  bool have_b = false, have_g = false;
  if (int rc = hybrid_set_check(name, c0->ctx, baby_steps, n_baby, baby_keys_a, baby_keys_b, alpha, &plb, &nzb,
                                &have_b))
    return rc;
  if (int rc = hybrid_set_check(name, c0->ctx, giant_steps, n_giant, giant_keys_a, giant_keys_b, alpha, &plg, &nzg,
                                &have_g))
    return rc;
  if (have_b && have_g && plb.E != plg.E)
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: the baby and giant keys belong to different key bases", name);
  // E: the keys' basis; without any key the plaintexts' own (every step is 0, and P is still E's)
  const rnt_ctx* C = c0->ctx;
  const rnt_ctx* D = diagE->ctx;
  const size_t Lv = C->L;
  HybridPlan pl = have_b ? plb : plg;
  if (!have_b && !have_g) {
    pl.C = C, pl.E = D, pl.Lv = Lv, pl.LE = D->L;
    pl.K = D->L > Lv ? D->L - Lv : 0;
    pl.alpha = std::min(alpha, Lv);
    pl.beta = (Lv + alpha - 1) / alpha;
  }
  bool same = D->L == pl.LE && D->L > Lv && D->t->log_n == C->t->log_n && D->t->device == C->t->device;
  for (size_t t = 0; same && t < pl.LE; ++t)
    same = D->modulus(t) == (t < Lv ? C->modulus(t) : pl.E->modulus(t));
  if (!same)
    return fail(RNT_ERR_BASIS_MISMATCH,
                "%s: the plaintexts' basis does not hold the ciphertext's moduli followed by the special primes", name);
  if (D->t->wide != C->t->wide)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "%s: plaintext and ciphertext bases have different device word widths",
                       name);
  const size_t n_terms = n_baby * n_giant;
  if (n_baby > SIZE_MAX / n_giant || diagE->n_polys != n_terms)
    return fail_fields(RNT_ERR_CHANNEL_COUNT, n_terms, diagE->n_polys, "%s: %zu plaintexts for %zu x %zu steps", name,
                       diagE->n_polys, n_giant, n_baby);
  if (!diagE->in_ntt) return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the plaintexts must be in the NTT domain", name);
  if (c0->in_ntt || c1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertext must be in coefficient domain", name);
  if (rescale)
    if (int rc = rescaled_outputs_check(name, out0, out1, c0, c0->n_polys)) return rc;
  const rnt_buf* ins[7] = {c0, c1, diagE, baby_keys_a, baby_keys_b, giant_keys_a, giant_keys_b};
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (int i = 0; i < 7; ++i) {
    if (!ins[i]) continue;
    if ((i != 0 && (out0 == ins[i] || out0->data == ins[i]->data)) ||
        (i != 1 && (out1 == ins[i] || out1->data == ins[i]->data)))
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input other than its own component", name);
  }
  if (int rc = set_device(C)) return rc;
  if (int rc = hybrid_prepare(&pl)) return rc;
  const rnt::Launch k = launch_for(c0);
  const rnt::Tables* tc = k.t;
  if (D->t.get() != tc && D->t->stream != tc->stream && g_capture == nullptr) {
    // the plaintexts may still be in the making (an upload, their transform) on their own basis' stream
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(plaintext order)");
    hipError_t e = hipEventRecord(ev, D->t->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(tc->stream, ev, 0);
    cleanup(hipEventDestroy(ev), "hipEventDestroy(plaintext order)");
    HIP_TRY(e, "hipStreamWaitEvent(plaintext order)");
  }
  const size_t n = tc->n, wb = word_bytes(tc), B = c0->n_polys, LE = pl.LE;
  const uint64_t full_ls = limb_stride(c0), two_n = 2 * (uint64_t)n;
  // chunk blocks: c0^ c1^ over C | W = ModDown(Vt1_j) | its automorphism | over E the baby products T0_i T1_i | the
  // inner sums of one giant group Vt0_j Vt1_j | the hybrid scratch (the digits, A0 A1)
  const size_t jg = std::min<size_t>(n_giant, rnt::kDhJt);
  enum { WCH, WW, WSIG, WT, WV, WH };
  rnt::WsLayout w = ws_layout(tc).blocks(Lv, 2).blocks(Lv, nzg ? 1 : 0).blocks(Lv, nzg ? 1 : 0).blocks(LE, 2 * nzb)
                        .blocks(LE, 2 * jg).sub(pl.ws());
  const size_t bc = fit_chunk(tc, w, B);
  CallWs ws(out0);
  if (int rc = ws.get(w)) return rc;
  char *CH0 = w.at(WCH, 0), *CH1 = w.at(WCH, 1), *Wd = w.at(WW), *SIG = w.at(WSIG);
  const HybridWs hw(pl, bc, w.at(WH));  // (at the call's pitch in every chunk)
  std::vector<const void*> t0, t1;
  std::vector<uint64_t> gb;
  try {
    t0.assign(n_baby, nullptr), t1.assign(n_baby, nullptr), gb.assign(n_baby, 1);
  } catch (...) {
    return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  for (size_t i = 0, ti = 0; i < n_baby; ++i) {
    if (baby_steps[i] == 0) continue;
    t0[i] = w.at(WT, 2 * ti), t1[i] = w.at(WT, 2 * ti + 1);
    gb[i] = rotation_exponent(baby_steps[i], two_n);
    ++ti;
  }
  const uint64_t m_ls = limb_stride(diagE), m_row = (uint64_t)n_baby * n;
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const rnt::Launch ke = hybrid_launch(pl, c);
    rnt::Launch kq = ke;  // the ciphertext's limbs on the key basis' transforms
    kq.L = Lv;
    const uint64_t cls = (uint64_t)c * n;
    const char* x[2] = {(const char*)c0->data + p0 * n * wb, (const char*)c1->data + p0 * n * wb};
    char* CH[2] = {CH0, CH1};
    for (int o = 0; o < 2; ++o) {
      if (int rc = copy_rows(kc, CH[o], cls, x[o], full_ls, cls, Lv)) return rc;
      if (int rc = fwd_raw(kq, CH[o], cls, tc)) return rc;
    }
    // baby stage: T_i = sum_d D_d sigma_i^-1(key[i][d]) over E, kHoistT steps a launch; nothing comes down
    if (nzb) {
      if (int rc = hybrid_raise(pl, c, hw.D, x[1], full_ls)) return rc;
      rnt::Launch km = ke;
      km.Ls = pl.beta;
      for (size_t i = 0; i < n_baby;) {
        void* a0[rnt::kHoistT] = {};
        void* a1[rnt::kHoistT] = {};
        const void* ka[rnt::kHoistT] = {};
        const void* kb[rnt::kHoistT] = {};
        uint32_t nt = 0;
        for (; i < n_baby && nt < rnt::kHoistT; ++i) {
          if (baby_steps[i] == 0) continue;
          a0[nt] = const_cast<void*>(t0[i]);
          a1[nt] = const_cast<void*>(t1[i]);
          ka[nt] = (const char*)baby_keys_a->data + i * key_step_polys(baby_keys_a, pl) * n * wb;
          kb[nt] = (const char*)baby_keys_b->data + i * key_step_polys(baby_keys_b, pl) * n * wb;
          ++nt;
        }
        if (nt == 0) break;
        LAUNCH_ON(tc, ke.s, rnt::K_HOIST_MAC,
                  rnt::launch_hoist_mac(km, a0, a1, nt, hw.D, ka, kb, limb_stride(baby_keys_a)),
                  "hoisted hybrid key products");
      }
    }
    // giant groups: inner sums over E, the fold into A0 / A1, then each rotating giant's key products
    for (size_t j0 = 0; j0 < n_giant; j0 += jg) {
      const uint32_t nj = (uint32_t)std::min(jg, n_giant - j0);
      void* v0[rnt::kDhJt] = {};
      void* v1[rnt::kDhJt] = {};
      uint64_t gf[rnt::kDhJt] = {};
      for (uint32_t jj = 0; jj < nj; ++jj) {
        v0[jj] = w.at(WV, 2 * jj), v1[jj] = w.at(WV, 2 * jj + 1);
        gf[jj] = giant_steps[j0 + jj] == 0 ? 0 : rotation_exponent(giant_steps[j0 + jj], two_n);
      }
      for (size_t b0 = 0; b0 < n_baby; b0 += rnt::kDhBt) {
        const uint32_t nb = (uint32_t)std::min<size_t>(rnt::kDhBt, n_baby - b0);
        const char* m = (const char*)diagE->data + (j0 * n_baby + b0) * n * wb;
        LAUNCH_ON(tc, ke.s, rnt::K_DH_BSGS_MAC,
                  rnt::launch_dh_bsgs_mac(ke, v0, v1, nj, t0.data() + b0, t1.data() + b0, gb.data() + b0, nb, CH0, CH1,
                                          m, m_ls, m_row, b0 != 0, pl.hc),
                  "double-hoisted inner sums");
      }
      LAUNCH_ON(tc, ke.s, rnt::K_DH_BSGS_FOLD, rnt::launch_dh_bsgs_fold(ke, hw.A0, hw.A1, v0, v1, gf, nj, j0 != 0),
                "double-hoisted fold");
      for (uint32_t jj = 0; jj < nj; ++jj) {
        if (gf[jj] == 0) continue;
        const size_t j = j0 + jj;
        if (int rc = inv_raw(ke, v1[jj], cls, tc)) return rc;
        LAUNCH_ON(tc, ke.s, rnt::K_MODDOWN, rnt::launch_moddown(ke, Wd, cls, v1[jj], cls, nullptr, 0, pl.hc),
                  "ModDown");
        LAUNCH(tc, rnt::K_AUTOMORPHISM, rnt::launch_automorphism(kc, SIG, Wd, gf[jj]), "automorphism");
        if (int rc = hybrid_raise(pl, c, hw.D, SIG, cls)) return rc;
        if (int rc = hybrid_products(pl, c, hw.D, hw.A0, hw.A1,
                                     (const char*)giant_keys_a->data + j * key_step_polys(giant_keys_a, pl) * n * wb,
                                     (const char*)giant_keys_b->data + j * key_step_polys(giant_keys_b, pl) * n * wb,
                                     limb_stride(giant_keys_a), HybridMac::accumulate))
          return rc;
      }
    }
    if (int rc = hybrid_lower(pl, c, hw.A0, hw.A1, (char*)out0->data + p0 * n * wb, (char*)out1->data + p0 * n * wb,
                              limb_stride(out0), nullptr, nullptr, 0, rescale))
      return rc;
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

extern "C" int rnt_ct_linear_bsgs_hybrid_dh(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                            const int32_t* baby_steps, size_t n_baby, const int32_t* giant_steps,
                                            size_t n_giant, const rnt_buf* diagE, const rnt_buf* baby_keys_a,
                                            const rnt_buf* baby_keys_b, const rnt_buf* giant_keys_a,
                                            const rnt_buf* giant_keys_b, size_t alpha) {
  return ct_linear_bsgs_hybrid_dh_body("rnt_ct_linear_bsgs_hybrid_dh", false, out0, out1, c0, c1, baby_steps, n_baby,
                                       giant_steps, n_giant, diagE, baby_keys_a, baby_keys_b, giant_keys_a,
                                       giant_keys_b, alpha);
}

extern "C" int rnt_ct_linear_bsgs_hybrid_dh_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                                    const int32_t* baby_steps, size_t n_baby,
                                                    const int32_t* giant_steps, size_t n_giant, const rnt_buf* diagE,
                                                    const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                                    const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b,
                                                    size_t alpha) {
  return ct_linear_bsgs_hybrid_dh_body("rnt_ct_linear_bsgs_hybrid_dh_rescale", true, out0, out1, c0, c1, baby_steps,
                                       n_baby, giant_steps, n_giant, diagE, baby_keys_a, baby_keys_b, giant_keys_a,
                                       giant_keys_b, alpha);
}

extern "C" int rnt_copy_polys(rnt_buf* dst, size_t dst_first, const rnt_buf* src, size_t src_first,
                              size_t count) {
  if (int rc = check_buf(dst, "rnt_copy_polys")) return rc;
  if (int rc = check_buf(src, "rnt_copy_polys")) return rc;
  if (dst->ctx != src->ctx) return fail(RNT_ERR_BASIS_MISMATCH, "rnt_copy_polys: operands belong to different bases");
  if (dst == src) return fail(RNT_ERR_BAD_ARGUMENT, "rnt_copy_polys: dst aliases src");
  if (count == 0 || dst_first > dst->n_polys || count > dst->n_polys - dst_first || src_first > src->n_polys ||
      count > src->n_polys - src_first)
    return fail(RNT_ERR_BAD_ARGUMENT, "rnt_copy_polys: range outside the batch (%zu+%zu of %zu -> %zu+%zu of %zu)",
                src_first, count, src->n_polys, dst_first, count, dst->n_polys);
  const bool whole = count == dst->n_polys;
  if (!whole && dst->in_ntt != src->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "rnt_copy_polys: domain mismatch on a partial copy");
  if (int rc = set_device(dst->ctx)) return rc;
  rnt::Launch k = launch_for(dst);
  const size_t n = k.t->n, wb = word_bytes(k.t);
  if (int rc = copy_rows(k, (char*)dst->data + dst_first * n * wb, limb_stride(dst),
                         (const char*)src->data + src_first * n * wb, limb_stride(src), (uint64_t)count * n, k.L))
    return rc;
  dst->in_ntt = src->in_ntt;
  return RNT_OK;
}

extern "C" int rnt_ct_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1) {
  if (int rc = check_buf(out0, "rnt_ct_rescale")) return rc;
  if (int rc = check_buf(out1, "rnt_ct_rescale")) return rc;
  if (out0->ctx != out1->ctx)  // engine.rs:272-274: one shared new basis
    return fail(RNT_ERR_BASIS_MISMATCH, "rescale_ciphertext: outputs must share one basis");
  if (int rc = rnt_rescale(out0, c0)) return rc;
  return rnt_rescale(out1, c1);
}

// ---------------------------------------------------------------------------
// ciphertext x plaintext multiply-accumulate (k_plain_mac)
// ---------------------------------------------------------------------------
namespace {

// The shared body of rnt_ct_plain_mac and its rescaling form.  Per chunk of
// ciphertexts and group of up to kPlainT terms: the group's planes of x0 and x1
// go, forward-transformed, into one call-scoped block X ([L][2 g c][N]: x0's g
// terms, then x1's, on every limb) -- by the four-step column pass straight
// from the inputs (launch_col_fwd reads one place and writes another) and one
// row pass over the block, or, where the transform is one in-place launch (the
// whole-plane and matrix-core paths), by a gather and that launch over the
// block; k_plain_mac then sums the group against the plaintexts where they lie
// (groups after the first accumulate, the last adds the bias).  Un-rescaled the
// sums are written to the outputs and inverse-transformed there; rescaling they
// go to one block S ([L][2 c][N]: s0 | s1 on every limb), one inverse runs over
// both and launch_rescale_strided writes each output.
int ct_plain_mac_body(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0,
                      const rnt_buf* x1, const rnt_buf* m, const rnt_buf* bias, size_t n_terms) {
  const rnt_buf* in[4] = {x0, x1, m, bias};
  for (const rnt_buf* b : {(const rnt_buf*)out0, (const rnt_buf*)out1, x0, x1, m})
    if (int rc = check_buf(b, name)) return rc;
  if (bias)
    if (int rc = check_buf(bias, name)) return rc;
  if (n_terms == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: n_terms must be at least 1", name);
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (const rnt_buf* b : in)
    if (b && (out0 == b || out1 == b || out0->data == b->data || out1->data == b->data))
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input", name);
  if (int rc = check_same(x0, x1, name)) return rc;
  if (m->ctx != x0->ctx || (bias && bias->ctx != x0->ctx))
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: operands belong to different bases", name);
  if (x0->n_polys % n_terms != 0)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: inputs of %zu polys are no %zu terms of a batch", name, x0->n_polys,
                n_terms);
  const size_t B = x0->n_polys / n_terms;
  const bool m_shared = m->n_polys == n_terms;  // (one ciphertext: the two forms are one)
  if (!m_shared && m->n_polys != n_terms * B)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: %zu plaintexts for %zu terms of a batch of %zu", name, m->n_polys, n_terms,
                B);
  const bool b_shared = bias && bias->n_polys == 1;
  if (bias && !b_shared && bias->n_polys != B)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: a bias of %zu polys for a batch of %zu", name, bias->n_polys, B);
  if (x0->in_ntt || x1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the ciphertexts must be in coefficient domain", name);
  if (!m->in_ntt || (bias && !bias->in_ntt))
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: the plaintexts and the bias must be in NTT domain", name);
  const size_t L = x0->ctx->L;
  if (rescale) {
    if (int rc = rescaled_outputs_check(name, out0, out1, x0, B)) return rc;
  } else {
    for (const rnt_buf* o : {out0, out1}) {
      if (o->ctx != x0->ctx) return fail(RNT_ERR_BASIS_MISMATCH, "%s: an output's basis is not the inputs'", name);
      if (o->n_polys != B)
        return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output of %zu polys for a batch of %zu", name, o->n_polys, B);
    }
  }
  if (int rc = set_device(x0->ctx)) return rc;
  rnt::Launch k = launch_for(x0);
  const size_t n = k.t->n, wb = word_bytes(k.t);
  const size_t gmax = std::min<size_t>(n_terms, rnt::kPlainT);
  const size_t ns = rescale ? 2 : 0;  // s0, s1 in workspace
  // X (x0's and x1's gmax terms) | S (s0 | s1, the rescaling call alone)
  rnt::WsLayout w = ws_layout(k.t).blocks(2 * gmax * L).blocks(ns * L, ns ? 1 : 0);
  const size_t bc = fit_chunk(k.t, w, B);
  CallWs cws(out0);
  if (int rc = cws.get(w, 16)) return rc;
  char *X = w.at(0), *S = w.at(1);
  const bool four_step = !use_mf(k) && !rnt::whole_ok(k.t, 0);
  const uint64_t full_ls = limb_stride(x0), out_ls = limb_stride(out0), m_ls = limb_stride(m);
  const uint64_t b_ls = bias ? limb_stride(bias) : 0;
  for (size_t p0 = 0; p0 < B; p0 += bc) {
    const size_t c = std::min(bc, B - p0);
    rnt::Launch kc = k;
    kc.B = c;
    const uint64_t cls = (uint64_t)c * n;
    const size_t po = p0 * n * wb;
    char* D0 = rescale ? S : (char*)out0->data + po;
    char* D1 = rescale ? S + cls * wb : (char*)out1->data + po;
    const uint64_t d_ls = rescale ? 2 * cls : out_ls;
    for (size_t t0 = 0; t0 < n_terms; t0 += gmax) {
      const size_t g = std::min(gmax, n_terms - t0);
      const uint64_t gls = (uint64_t)g * cls, xls = 2 * gls;
      rnt::Launch kx = k;
      kx.B = 2 * g * c;
      // term t of the chunk: polys [t B + p0, t B + p0 + c) of every limb; one run a limb where the chunk is the batch
      const size_t runs = c == B ? 1 : g;
      rnt::Launch kr = k;
      kr.B = c == B ? g * c : c;
      for (size_t i = 0; i < runs; ++i) {
        const size_t src = ((t0 + i) * B + p0) * n * wb;
        char* dst = X + i * cls * wb;
        if (four_step) {
          LAUNCH(k.t, rnt::K_COL_FWD,
                 rnt::launch_col_fwd(kr, dst, (const char*)x0->data + src, dst + gls * wb,
                                     (const char*)x1->data + src, full_ls, xls),
                 "column forward");
        } else {
          for (size_t j = 0; j < 2; ++j)
            LAUNCH(k.t, rnt::K_COPY,
                   rnt::launch_copy_rows(k.s, dst + j * gls * wb, xls * wb, (const char*)in[j]->data + src,
                                         full_ls * wb, (c == B ? gls : cls) * wb, L),
                   "term gather");
        }
      }
      if (four_step) {
        LAUNCH(k.t, rnt::K_ROW_FWD, rnt::launch_row(kx, 0, X, nullptr, xls), "row forward");
      } else {
        if (int rc = fwd_raw(kx, X, xls)) return rc;
      }
      const bool last = t0 + g >= n_terms;
      const char* mp = (const char*)m->data + (m_shared ? t0 : t0 * B + p0) * n * wb;
      const char* bp = bias && last ? (const char*)bias->data + (b_shared ? 0 : po) : nullptr;
      LAUNCH(k.t, rnt::K_PLAIN_MAC,
             rnt::launch_plain_mac(kc, D0, D1, d_ls, X, X + gls * wb, xls, cls, mp, m_ls, m_shared ? n : B * n,
                                   m_shared, bp, b_ls, b_shared, g, t0 != 0),
             "plaintext multiply-accumulate");
    }
    if (rescale) {
      rnt::Launch ks = k;
      ks.B = 2 * c;
      if (int rc = inv_raw(ks, S, d_ls)) return rc;
      LAUNCH(k.t, rnt::K_RESCALE, rnt::launch_rescale_strided(kc, (char*)out0->data + po, out_ls, D0, d_ls),
             "rescale");
      LAUNCH(k.t, rnt::K_RESCALE, rnt::launch_rescale_strided(kc, (char*)out1->data + po, out_ls, D1, d_ls),
             "rescale");
    } else {
      if (int rc = inv_raw(kc, D0, d_ls)) return rc;
      if (int rc = inv_raw(kc, D1, d_ls)) return rc;
    }
  }
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_plain_mac(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1, const rnt_buf* m,
                                const rnt_buf* bias, size_t n_terms) {
  return ct_plain_mac_body("rnt_ct_plain_mac", false, out0, out1, x0, x1, m, bias, n_terms);
}

extern "C" int rnt_ct_plain_mac_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                                        const rnt_buf* m, const rnt_buf* bias, size_t n_terms) {
  return ct_plain_mac_body("rnt_ct_plain_mac_rescale", true, out0, out1, x0, x1, m, bias, n_terms);
}

// ---------------------------------------------------------------------------
// scalar linear combinations of ciphertexts (k_lincomb)
// ---------------------------------------------------------------------------
namespace {

// Pinned host staging for the weights of rnt_ct_lincomb: the caller's arrays
// are packed here during the call and copied up on the op's stream, so the
// call neither waits for the device nor leaves a pointer to caller memory
// behind.  A ring of slots per thread, each behind an event on the stream of
// its last copy: the host waits only when kLcSlots later calls find the copy of
// this one still queued.  The slots live as long as the thread.
constexpr unsigned kLcSlots = 4;
struct LcSlot {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;  // of the copy the event was last recorded behind
  int device = -1;
  bool busy = false;
};
thread_local LcSlot g_lc_slots[kLcSlots];
thread_local unsigned g_lc_next = 0;

// A stream about to be destroyed, already synchronised (pool_forget_stream's
// rule: an event must not outlive the stream it was last recorded on -- the
// runtime consults that stream when the event is waited for): the copies this
// thread's slots queued on it are complete, so the slots drop their events.
void lincomb_forget_stream(hipStream_t s) {
  for (LcSlot& slot : g_lc_slots)
    if (slot.ev && slot.stream == s) {
      cleanup(hipEventDestroy(slot.ev), "hipEventDestroy(lincomb weights of a stream being destroyed)");
      slot.ev = nullptr;
      slot.stream = nullptr;
      slot.busy = false;
    }
}

int lincomb_stage(int device, size_t bytes, LcSlot** out) {
  LcSlot& s = g_lc_slots[g_lc_next++ % kLcSlots];
  if (s.busy) {
    HIP_TRY(hipEventSynchronize(s.ev), "hipEventSynchronize(lincomb weights)");
    s.busy = false;
  }
  if (s.ev && s.device != device) {  // an event records on its own device's streams
    HIP_TRY(hipEventDestroy(s.ev), "hipEventDestroy(lincomb weights)");
    s.ev = nullptr;
  }
  if (!s.ev) {
    HIP_TRY(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming), "hipEventCreate(lincomb weights)");
    s.device = device;
  }
  if (s.bytes < bytes) {
    if (s.p) {
      HIP_TRY(hipHostFree(s.p), "hipHostFree(lincomb weights)");
      s.p = nullptr;
      s.bytes = 0;
    }
    const size_t cap = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipHostMalloc(&s.p, cap, hipHostMallocPortable), "hipHostMalloc(lincomb weights)");
    s.bytes = cap;
  }
  *out = &s;
  return RNT_OK;
}

template <class W>
void lincomb_pack(W* dst, const rnt_ctx* ctx, size_t n_in, size_t n_out, const uint64_t* weights,
                  const uint64_t* bias) {
  const size_t Lv = ctx->L, nw = Lv * n_out * n_in;
  const unsigned wbits = sizeof(W) * 8;
  for (size_t t = 0; t < Lv; ++t) {
    const uint64_t q = ctx->modulus(t);
    for (size_t j = 0; j < n_out; ++j) {
      for (size_t i = 0; i < n_in; ++i) {
        const uint64_t v = weights[(j * n_in + i) * Lv + t];
        dst[(t * n_out + j) * n_in + i] = (W)v;
        dst[nw + (t * n_out + j) * n_in + i] = (W)rnt::host::shoup_companion(v, q, wbits);
      }
      if (bias) dst[2 * nw + t * n_out + j] = (W)bias[j * Lv + t];
    }
  }
}

int lincomb_impl(const char* name, bool rescale, rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                 size_t n_in, size_t n_out, const uint64_t* weights, const uint64_t* bias) {
  const rnt_buf* all[4] = {out0, out1, x0, x1};
  for (const rnt_buf* b : all)
    if (int rc = check_buf(b, name)) return rc;
  if (n_in == 0 || n_out == 0) return fail(RNT_ERR_BAD_ARGUMENT, "%s: n_in and n_out must be at least 1", name);
  if (n_in > rnt::kLincombMax || n_out > rnt::kLincombMax)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0, "%s: %zu inputs and %zu outputs (at most %zu of either)", name, n_in,
                       n_out, rnt::kLincombMax);
  if (!weights) return fail(RNT_ERR_BAD_ARGUMENT, "%s: null weights", name);
  if (g_capture != nullptr)
    return fail_fields(RNT_ERR_UNSUPPORTED, 0, 0,
                       "%s cannot be recorded: its weights go up by a host copy that a graph does not own", name);
  if (int rc = check_same(x0, x1, name)) return rc;
  if (x0->n_polys % n_in != 0)
    return fail(RNT_ERR_BAD_ARGUMENT, "%s: inputs of %zu polys are no %zu terms of a batch", name, x0->n_polys, n_in);
  const size_t B = x0->n_polys / n_in, Lv = x0->ctx->L;
  if (x0->in_ntt || x1->in_ntt)
    return fail(RNT_ERR_DOMAIN_MISMATCH, "%s: inputs must be in coefficient domain", name);
  for (size_t t = 0; t < Lv; ++t) {
    const uint64_t q = x0->ctx->modulus(t);
    for (size_t e = 0; e < n_out * n_in; ++e)
      if (weights[e * Lv + t] >= q)
        return fail_fields(RNT_ERR_NON_REDUCED, weights[e * Lv + t], q,
                           "%s: weight %" PRIu64 " is not reduced mod %" PRIu64, name, weights[e * Lv + t], q);
    for (size_t j = 0; bias && j < n_out; ++j)
      if (bias[j * Lv + t] >= q)
        return fail_fields(RNT_ERR_NON_REDUCED, bias[j * Lv + t], q,
                           "%s: bias %" PRIu64 " is not reduced mod %" PRIu64, name, bias[j * Lv + t], q);
  }
  if (rescale && Lv < 2)  // poly.rs:191-197
    return fail_fields(RNT_ERR_INVALID_MOD_DROP, 1, Lv, "invalid mod-drop count 1 for %zu channels", Lv);
  for (const rnt_buf* o : {out0, out1}) {
    if (rescale ? (o->ctx->t != x0->ctx->t || o->ctx->L != Lv - 1) : o->ctx != x0->ctx)
      return fail(RNT_ERR_BASIS_MISMATCH, "%s: an output's basis is not %s the inputs'", name,
                  rescale ? "drop_last(1) of" : "");
    if (o->n_polys != n_out * B)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output of %zu polys for %zu outputs of %zu", name, o->n_polys, n_out, B);
  }
  if (out0->ctx != out1->ctx)  // engine.rs:272-274: one shared new basis
    return fail(RNT_ERR_BASIS_MISMATCH, "%s: outputs must share one basis", name);
  if (out0 == out1 || out0->data == out1->data) return fail(RNT_ERR_BAD_ARGUMENT, "%s: out0 aliases out1", name);
  for (const rnt_buf* in : {x0, x1})
    if (out0 == in || out1 == in || out0->data == in->data || out1->data == in->data)
      return fail(RNT_ERR_BAD_ARGUMENT, "%s: an output aliases an input", name);
  if (int rc = set_device(x0->ctx)) return rc;
  rnt::Launch k = launch_for(x0);
  k.B = B;
  const size_t wb = word_bytes(k.t);
  const size_t words = Lv * n_out * (2 * n_in + (bias ? 1 : 0));
  LcSlot* slot = nullptr;
  if (int rc = lincomb_stage(k.t->device, words * wb, &slot)) return rc;
  if (wb == 4) lincomb_pack<uint32_t>((uint32_t*)slot->p, x0->ctx, n_in, n_out, weights, bias);
  else lincomb_pack<uint64_t>((uint64_t*)slot->p, x0->ctx, n_in, n_out, weights, bias);
  // the weights | their Shoup companions | the bias, as packed
  const size_t nw = Lv * n_out * n_in * wb;
  rnt::WsLayout w = ws_layout(k.t).bytes(nw).bytes(nw).bytes(bias ? Lv * n_out * wb : 0);
  CallWs cws(out0);
  if (int rc = cws.get(w, 16)) return rc;
  HIP_TRY(hipMemcpyAsync(w.at(0), slot->p, words * wb, hipMemcpyHostToDevice, k.s), "hipMemcpyAsync(lincomb weights)");
  HIP_TRY(hipEventRecord(slot->ev, k.s), "hipEventRecord(lincomb weights)");
  slot->stream = k.s;
  slot->busy = true;
  LAUNCH(k.t, rnt::K_LINCOMB,
         rnt::launch_lincomb(k, out0->data, out1->data, limb_stride(out0), x0->data, x1->data, limb_stride(x0), n_in,
                             n_out, w.at(0), w.at(1), w.at(2), rescale),
         "lincomb");
  out0->in_ntt = out1->in_ntt = 0;
  return RNT_OK;
}

}  // namespace

extern "C" int rnt_ct_lincomb(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1, size_t n_in,
                              size_t n_out, const uint64_t* weights, const uint64_t* bias) {
  return lincomb_impl("rnt_ct_lincomb", false, out0, out1, x0, x1, n_in, n_out, weights, bias);
}

extern "C" int rnt_ct_lincomb_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1, size_t n_in,
                                      size_t n_out, const uint64_t* weights, const uint64_t* bias) {
  return lincomb_impl("rnt_ct_lincomb_rescale", true, out0, out1, x0, x1, n_in, n_out, weights, bias);
}

// ---------------------------------------------------------------------------
// device count / profiling
// ---------------------------------------------------------------------------
extern "C" int rnt_device_count(int* n) {
  if (!n) return fail(RNT_ERR_BAD_ARGUMENT, "null out");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return RNT_OK;
}

extern "C" int rnt_profile_enable(const rnt_ctx* ctx, int enable) {
  if (!ctx) return fail(RNT_ERR_BAD_ARGUMENT, "null ctx");
  rnt::Tables* t = ctx->t.get();
  if (int rc = set_device(ctx)) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream), "hipStreamSynchronize");
  if (t->prof == nullptr) {
    try {
      t->prof = new rnt::Prof;
    } catch (...) {
      return fail(RNT_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
  }
  std::lock_guard<std::mutex> g(t->prof->mu);
  for (auto& r : t->prof->pending) {
    t->prof->pool.push_back(r.a);
    t->prof->pool.push_back(r.b);
  }
  t->prof->pending.clear();
  for (int i = 0; i < rnt::K_COUNT; ++i) {
    t->prof->launches[i] = 0;
    t->prof->ms[i] = 0;
  }
  t->prof->on = enable != 0;
  return RNT_OK;
}

extern "C" int rnt_profile_read(const rnt_ctx* ctx, const char* kernel, uint64_t* launches,
                                double* total_ms) {
  if (!ctx || !kernel || !launches || !total_ms) return fail(RNT_ERR_BAD_ARGUMENT, "null argument");
  rnt::Tables* t = ctx->t.get();
  int id = -1;
  for (int i = 0; i < rnt::K_COUNT; ++i)
    if (std::strcmp(kKernelNames[i], kernel) == 0) id = i;
  if (id < 0) return fail(RNT_ERR_BAD_ARGUMENT, "unknown kernel name '%s'", kernel);
  *launches = 0;
  *total_ms = 0;
  if (t->prof == nullptr) return RNT_OK;
  if (int rc = set_device(ctx)) return rc;
  HIP_TRY(hipStreamSynchronize(t->stream), "hipStreamSynchronize");
  std::lock_guard<std::mutex> g(t->prof->mu);
  for (auto& r : t->prof->pending) {
    float ms = 0;
    if (const hipError_t e = hipEventElapsedTime(&ms, r.a, r.b); e == hipSuccess) {
      t->prof->launches[r.id] += 1;
      t->prof->ms[r.id] += ms;
    } else {
      prof_fail(t->prof, e, "hipEventElapsedTime(profile)");
    }
    t->prof->pool.push_back(r.a);
    t->prof->pool.push_back(r.b);
  }
  t->prof->pending.clear();
  *launches = t->prof->launches[id];
  *total_ms = t->prof->ms[id];
  if (t->prof->err != hipSuccess) {
    const hipError_t e = t->prof->err;
    const char* where = t->prof->err_where;
    t->prof->err = hipSuccess;
    return fail(RNT_ERR_DEVICE, "%s failed: %s (profiling was turned off; the launches ran)", where,
                hipGetErrorString(e));
  }
  return RNT_OK;
}
