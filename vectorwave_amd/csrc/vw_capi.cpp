// vw_capi.cpp -- C ABI of the MI355X MODWT/SWT engine (include/vectorwave_amd.h).
//
// Contexts, streams, graphs, pipelines, staging, argument checks and status mapping; the transforms
// execute the plans of vw_plan.cpp (which kernels, launch shapes, LDS layouts, buffers, reservations):
// one fused HIP launch per transform, or the per-level steps for signals longer than LDS holds.
#include "../../include/vectorwave_amd.h"
#include "vw_internal.h"
#include "vw_deep.h"
#include "vw_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

using namespace vw;

// ------------------------------------------------------------------------------------------------
// Errors (thread-local, like the reference's exceptions are per call site)
static thread_local std::string t_err;
static thread_local int64_t t_err_index = -1;
static thread_local int64_t t_signal_base = 0;  // run_sharded: global row of this block's first signal

static vw_status fail(vw_status code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  t_err = buf;
  if (code != VW_ERR_NONFINITE) t_err_index = -1;
  return code;
}

static vw_status ok() {
  t_err.clear();
  t_err_index = -1;
  return VW_OK;
}

#define VW_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return fail(VW_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define VW_TRY(expr)                      \
  do {                                    \
    vw_status s_ = (expr);                \
    if (s_ != VW_OK) return s_;           \
  } while (0)

// ------------------------------------------------------------------------------------------------
struct TimedLaunch {
  std::string family;
  hipEvent_t start, stop;
  bool graph_owned = false;  // recorded inside a captured graph: its events live as long as the graph
};

struct vw_graph;
struct vw_ctx;
static void kill_pipelines_of(vw_ctx* c);

// A forward recorded during the current capture that the NEXT call may turn into a round trip (try_pair_fuse):
// its kernel node, and the call as it was launched.  No pointer of the caller's that may die is kept: the taps
// are in `args`.
struct PairPending {
  bool valid = false;
  hipGraphNode_t node = nullptr;
  FwdCall<double> call;
  FwdPlan<double> plan;
  FwdArgs<double> args;
};

struct vw_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool capturing = false;      // between vw_capture_begin / vw_capture_end
  unsigned ws_gen = 0;         // bumped when ws / ws2 move: graphs recorded before are stale
  Tuning tune;
  int cus = 256;               // compute units of the device (small-batch policies)
  std::recursive_mutex mu;
  void* ws = nullptr;          // tiled-path ping-pong buffers
  size_t ws_bytes = 0;
  void* ws2 = nullptr;         // denoise coefficients / thresholds
  size_t ws2_bytes = 0;
  unsigned long long* bad = nullptr;   // device word for the fused non-finite check
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<TimedLaunch> captured;   // timed launches recorded during the current capture
  std::vector<hipEvent_t> event_pool;
  std::map<std::string, std::pair<double, int64_t>> totals;
  std::set<vw_graph*> graphs;          // live graphs recorded on this context (invalidated at destroy)
  std::vector<std::pair<void*, size_t>> stage;  // host-memory staging pool (Staging), kept across calls
  void* med = nullptr;         // vw_median_f64 deviations of long rows (not ws: growing ws invalidates graphs)
  size_t med_bytes = 0;
  int* nf = nullptr;           // VW_FLAG_REF_NONFINITE row flags [nf_rows], zero between calls (vw_ref.hip)
  int64_t nf_rows = 0;
  PairPending pair;            // VW_PAIR_FUSE: the forward the next call may fuse with (capture only)
  int fused_pairs = 0;         // round trips recorded by the current capture
  void* cwt_dev = nullptr;     // vw_cwt_*: the scale descriptors and tap tables of the last call, on the device
  size_t cwt_dev_bytes = 0;
  std::vector<unsigned char> cwt_img;  // ... and the host image they were copied from (a call with the same one uploads nothing)
};

struct vw_graph {
  vw_ctx* ctx = nullptr;          // nullptr once the context is destroyed (the graph is then dead)
  int device = 0;
  unsigned ws_gen = 0;
  std::vector<TimedLaunch> timed;  // event-record nodes (timing enabled at capture)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int fused_pairs = 0;             // forward -> inverse pairs recorded as one k_roundtrip node
};

// Frees the HIP objects of a graph (its context's device must be current).
static void release_graph(vw_graph* gr) {
  for (auto& t : gr->timed) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
  gr->timed.clear();
  if (gr->exec) hipGraphExecDestroy(gr->exec);
  if (gr->graph) hipGraphDestroy(gr->graph);
  gr->exec = nullptr;
  gr->graph = nullptr;
}

struct vw_stream {
  vw_ctx* ctx = nullptr;
  std::vector<double> lo, hi;
  int L = 0;
  int boundary = 0;
  int levels = 0;
  int64_t last_batch = -1;
  bool hist_init = false;
  std::vector<double*> hist;        // device [B][hist_len_j]
  std::vector<double*> snap;        // VW_FLAG_REF_NONFINITE: the histories a block read (same shapes)
  std::vector<int> hist_len;
};

static hipEvent_t pool_event(vw_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// An event-record node appended to the graph being captured on `st` (after the current capture
// dependencies, which it then replaces): the graph-API form of recording a timing event inside a
// captured sequence.  Falls back to hipEventRecordWithFlags(..., hipEventRecordExternal).  A failed
// attempt's error is cleared so it does not surface at the next launch's hipGetLastError.
static bool capture_event(hipStream_t st, hipEvent_t ev) {
  hipStreamCaptureStatus status;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  if (hipStreamGetCaptureInfo_v2(st, &status, &id, &g, &deps, &ndeps) == hipSuccess &&
      status == hipStreamCaptureStatusActive && g) {
    hipGraphNode_t node = nullptr;
    if (hipGraphAddEventRecordNode(&node, g, deps, ndeps, ev) == hipSuccess &&
        hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies) == hipSuccess)
      return true;
  }
  (void)hipGetLastError();
  if (hipEventRecordWithFlags(ev, st, hipEventRecordExternal) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}

// Brackets a kernel launch with HIP events on the context stream when timing is enabled.  While
// capturing, the events become event-record nodes of the graph (hipEventRecordExternal), owned by
// the graph: every replay re-records them, so the launch is timed inside the replayed graph.
struct LaunchTimer {
  vw_ctx* c;
  TimedLaunch tl;
  bool on;
  LaunchTimer(vw_ctx* ctx, const char* family) : c(ctx), on(ctx->timing) {
    c->pair.valid = false;  // whatever launches next, the remembered forward is no longer the previous call
    if (!on) return;
    tl.family = family;
    if (c->capturing) {
      tl.graph_owned = true;
      tl.start = tl.stop = nullptr;
      if (hipEventCreate(&tl.start) != hipSuccess || hipEventCreate(&tl.stop) != hipSuccess ||
          !capture_event(c->stream, tl.start)) {
        if (tl.start) hipEventDestroy(tl.start);
        if (tl.stop) hipEventDestroy(tl.stop);
        on = false;
      }
      return;
    }
    tl.start = pool_event(c);
    tl.stop = pool_event(c);
    if (!tl.start || !tl.stop) { on = false; return; }
    hipEventRecord(tl.start, c->stream);
  }
  ~LaunchTimer() {
    if (!on) return;
    if (tl.graph_owned) {
      if (capture_event(c->stream, tl.stop)) {
        c->captured.push_back(tl);
      } else {
        hipEventDestroy(tl.start);
        hipEventDestroy(tl.stop);
      }
      return;
    }
    hipEventRecord(tl.stop, c->stream);
    c->pending.push_back(tl);
  }
};

static void collect_timing(vw_ctx* c) {
  for (auto& tl : c->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(tl.stop) == hipSuccess && hipEventElapsedTime(&ms, tl.start, tl.stop) == hipSuccess) {
      auto& t = c->totals[tl.family];
      t.first += ms;
      t.second += 1;
    }
    if (!tl.graph_owned) {
      c->event_pool.push_back(tl.start);
      c->event_pool.push_back(tl.stop);
    }
  }
  c->pending.clear();
}

static vw_status ensure_ws(vw_ctx* c, size_t bytes) {
  if (bytes <= c->ws_bytes) return VW_OK;
  if (c->capturing) return fail(VW_ERR_STATE, "workspace growth during capture: run the call once before capturing it");
  if (c->ws) {
    // the workspace may have been used on streams the context was bound to before: drain the device
    hipDeviceSynchronize();
    ++c->ws_gen;
    hipFree(c->ws);
    c->ws = nullptr;
    c->ws_bytes = 0;
  }
  size_t want = std::max(bytes, (size_t)1 << 20);
  VW_HIP(hipMalloc(&c->ws, want));
  c->ws_bytes = want;
  return VW_OK;
}

// the REF_NONFINITE row flags: zeroed once at allocation, kept zero by the kernels that consume them
static vw_status ensure_nf(vw_ctx* c, int64_t B) {
  if (B <= c->nf_rows) return VW_OK;
  if (c->capturing) return fail(VW_ERR_STATE, "row-flag growth during capture: run the call once before capturing it");
  if (c->nf) {
    hipDeviceSynchronize();
    ++c->ws_gen;
    hipFree(c->nf);
    c->nf = nullptr;
    c->nf_rows = 0;
  }
  const int64_t rows = std::max<int64_t>(B, 4096);
  VW_HIP(hipMalloc(&c->nf, (size_t)rows * sizeof(int)));
  VW_HIP(hipMemset(c->nf, 0, (size_t)rows * sizeof(int)));
  VW_HIP(hipDeviceSynchronize());
  c->nf_rows = rows;
  return VW_OK;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------
// Bookkeeping restated from the reference (vw_plan.cpp).
extern "C" int vw_max_levels(int64_t N, int L) { return max_levels(N, L); }
extern "C" int64_t vw_upsampled_length(int L, int level) { return upsampled_length(L, level); }

// ------------------------------------------------------------------------------------------------
// Context
extern "C" vw_status vw_ctx_create(int device, vw_ctx** out) {
  if (!out) return fail(VW_ERR_NULL, "out is null");
  int n = 0;
  VW_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(VW_ERR_ARG, "device %d out of range (%d devices)", device, n);
  VW_HIP(hipSetDevice(device));
  vw_ctx* c = new vw_ctx();
  c->device = device;
  c->tune = read_tuning();
  { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->cus = n; }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(VW_ERR_DEVICE, "hipStreamCreate failed");
  }
  c->own_stream = true;
  if (hipMalloc(&c->bad, sizeof(unsigned long long)) != hipSuccess) {
    hipStreamDestroy(c->stream);
    delete c;
    return fail(VW_ERR_DEVICE, "hipMalloc failed");
  }
  *out = c;
  return ok();
}

extern "C" vw_status vw_ctx_destroy(vw_ctx* c) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  hipSetDevice(c->device);
  if (c->capturing) {  // an unfinished capture: end it and drop what it recorded
    hipGraph_t gph = nullptr;
    if (hipStreamEndCapture(c->stream, &gph) == hipSuccess && gph) hipGraphDestroy(gph);
    (void)hipGetLastError();
    for (auto& t : c->captured) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
    c->captured.clear();
    c->capturing = false;
  }
  hipStreamSynchronize(c->stream);
  kill_pipelines_of(c);
  hipSetDevice(c->device);
  collect_timing(c);
  // graphs outliving their context: free their HIP objects now; the handles stay valid for
  // vw_graph_destroy, and vw_graph_launch on them fails with VW_ERR_STATE
  for (vw_graph* gr : c->graphs) {
    release_graph(gr);
    gr->ctx = nullptr;
  }
  c->graphs.clear();
  for (auto e : c->event_pool) hipEventDestroy(e);
  if (c->ws) hipFree(c->ws);
  if (c->ws2) hipFree(c->ws2);
  if (c->med) hipFree(c->med);
  if (c->nf) hipFree(c->nf);
  if (c->cwt_dev) hipFree(c->cwt_dev);
  for (auto& b : c->stage) hipFree(b.first);
  if (c->bad) hipFree(c->bad);
  if (c->own_stream) hipStreamDestroy(c->stream);
  delete c;
  return ok();
}

// The device's null (legacy default) stream -- what torch uses when no stream is set: its handle is
// 0, which vw_ctx_set_stream reads as "own stream".
// Rebinding the context: work already enqueued on the old stream (it may still use the shared
// workspaces ws / ws2) is ordered before anything the new stream runs -- an event on the old stream
// that the new one waits for.  An owned stream is drained and destroyed instead.
static vw_status rebind_stream(vw_ctx* c, hipStream_t next, bool own_next) {
  if (c->capturing) return fail(VW_ERR_STATE, "stream change during capture");
  hipStream_t prev = c->stream;
  if (c->own_stream) {
    VW_HIP(hipStreamSynchronize(prev));
    VW_HIP(hipStreamDestroy(prev));
    c->own_stream = false;
  } else if (prev != next) {
    hipEvent_t ev = nullptr;
    VW_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, prev);
    if (e == hipSuccess && next) e = hipStreamWaitEvent(next, ev, 0);
    if (e == hipSuccess && !next) e = hipEventSynchronize(ev);  // the legacy null stream: drain
    hipEventDestroy(ev);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "stream ordering failed: %s", hipGetErrorString(e));
  }
  c->stream = next;
  c->own_stream = own_next;
  return VW_OK;
}

extern "C" vw_status vw_ctx_use_null_stream(vw_ctx* c) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(rebind_stream(c, nullptr, false));
  return ok();
}

extern "C" vw_status vw_ctx_set_stream(vw_ctx* c, void* s) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (s) {
    VW_TRY(rebind_stream(c, (hipStream_t)s, false));
  } else {
    hipStream_t ns = nullptr;
    VW_HIP(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
    VW_TRY(rebind_stream(c, ns, true));
  }
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Captured steps: the calls made between vw_capture_begin and vw_capture_end are recorded (stream
// capture of the context stream) into one executable HIP graph, replayed by vw_graph_launch with
// one host call -- the host-side planning, argument packing and per-kernel launch cost of the
// transforms are paid once at capture.  Calls that must synchronize (validation, host memory,
// SYNC, workspace growth) are rejected while capturing.

extern "C" vw_status vw_capture_begin(vw_ctx* c) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (c->capturing) return fail(VW_ERR_STATE, "already capturing");
  if (!c->stream) return fail(VW_ERR_STATE, "the null stream cannot be captured; bind a stream first");
  hipSetDevice(c->device);
  VW_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  c->capturing = true;
  c->captured.clear();
  c->pair.valid = false;
  c->fused_pairs = 0;
  return ok();
}

extern "C" vw_status vw_capture_end(vw_ctx* c, vw_graph** out) {
  if (!c || !out) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!c->capturing) return fail(VW_ERR_STATE, "not capturing");
  hipSetDevice(c->device);
  c->capturing = false;
  c->pair.valid = false;
  std::vector<TimedLaunch> timed;
  timed.swap(c->captured);
  auto drop = [&] { for (auto& t : timed) { hipEventDestroy(t.start); hipEventDestroy(t.stop); } };
  hipGraph_t graph = nullptr;
  hipError_t ec = hipStreamEndCapture(c->stream, &graph);
  if (ec != hipSuccess) {
    drop();
    return fail(VW_ERR_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(ec));
  }
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    hipGraphDestroy(graph);
    drop();
    return fail(VW_ERR_DEVICE, "graph instantiate failed: %s", hipGetErrorString(e));
  }
  vw_graph* gr = new vw_graph();
  gr->timed.swap(timed);
  gr->ctx = c;
  gr->device = c->device;
  gr->ws_gen = c->ws_gen;
  gr->graph = graph;
  gr->exec = exec;
  gr->fused_pairs = c->fused_pairs;
  c->graphs.insert(gr);
  *out = gr;
  return ok();
}


extern "C" vw_status vw_graph_launch(vw_graph* gr, int64_t count) {
  if (!gr) return fail(VW_ERR_NULL, "graph is null");
  vw_ctx* c = gr->ctx;
  if (!c) return fail(VW_ERR_STATE, "the context of this graph was destroyed");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (gr->ws_gen != c->ws_gen)
    return fail(VW_ERR_STATE, "the context workspace moved since this graph was recorded; record it again");
  hipSetDevice(c->device);
  for (int64_t i = 0; i < count; ++i) VW_HIP(hipGraphLaunch(gr->exec, c->stream));
  // Timed launches recorded inside the graph: their events hold the LAST replay only, so a graph's
  // entries are pending at most once (a second launch before a collect replaces, not duplicates, them).
  if (c->timing && count > 0 && !gr->timed.empty()) {
    std::set<hipEvent_t> mine;
    for (const auto& t : gr->timed) mine.insert(t.start);
    c->pending.erase(std::remove_if(c->pending.begin(), c->pending.end(),
                                    [&](const TimedLaunch& t) { return t.graph_owned && mine.count(t.start); }),
                     c->pending.end());
    for (const auto& t : gr->timed) c->pending.push_back(t);
  }
  return ok();
}

extern "C" vw_status vw_graph_stats(vw_graph* gr, int* kernel_nodes, int* fused_pairs) {
  if (!gr) return fail(VW_ERR_NULL, "graph is null");
  vw_ctx* c = gr->ctx;
  if (!c) return fail(VW_ERR_STATE, "the context of this graph was destroyed");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (kernel_nodes) {
    size_t n = 0;
    VW_HIP(hipGraphGetNodes(gr->graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) VW_HIP(hipGraphGetNodes(gr->graph, nodes.data(), &n));
    int kernels = 0;
    for (size_t i = 0; i < n; ++i) {
      hipGraphNodeType ty;
      VW_HIP(hipGraphNodeGetType(nodes[i], &ty));
      if (ty == hipGraphNodeTypeKernel) ++kernels;
    }
    *kernel_nodes = kernels;
  }
  if (fused_pairs) *fused_pairs = gr->fused_pairs;
  return ok();
}

extern "C" vw_status vw_graph_destroy(vw_graph* gr) {
  if (!gr) return fail(VW_ERR_NULL, "graph is null");
  vw_ctx* c = gr->ctx;
  if (!c) {  // context already destroyed: it released the HIP objects
    delete gr;
    return ok();
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  collect_timing(c);  // pending entries may reference this graph's events
  release_graph(gr);
  c->graphs.erase(gr);
  delete gr;
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Pipelined round trips (include/vectorwave_amd.h "pipelined round trips").  Step i runs the forward
// of buffer set i mod R on the forward context's stream and then, after an event, its inverse on the
// inverse context's stream; step i's forward waits for step i - R's inverse (the set it overwrites).
// So step i + 1's forward runs beside step i's inverse while every step still does its whole forward
// and inverse.  The loop is issued here, in C++, so a small shard (the 8-GPU headline: 512 rows,
// ~50 us of GPU work per step) is not limited by a Python caller's per-call overhead.
struct vw_pipeline {
  vw_ctx* cf = nullptr;
  vw_ctx* ci = nullptr;
  int device = 0;
  int esz = 8;
  int R = 0;
  std::vector<void*> x, det, app, y;
  int64_t B = 0, N = 0;
  std::vector<double> lo, hi;
  int L = 0, wavelet_id = 0, boundary = 0, J = 0;
  unsigned flags = 0;
  std::vector<hipEvent_t> ev_f, ev_i;
  std::vector<char> live;
  hipEvent_t join_ev = nullptr;
  int64_t next = 0;       // index of the next step (selects its buffer set)
  bool dead = false;      // a context was destroyed under it
  std::mutex mu;          // run / join / kill: a kill waits until an in-flight run has issued its steps
};

static std::mutex g_pipe_mu;
static std::set<vw_pipeline*> g_pipes;

static void release_pipeline(vw_pipeline* p) {
  for (auto e : p->ev_f) if (e) hipEventDestroy(e);
  for (auto e : p->ev_i) if (e) hipEventDestroy(e);
  if (p->join_ev) hipEventDestroy(p->join_ev);
  p->ev_f.clear();
  p->ev_i.clear();
  p->join_ev = nullptr;
}

// vw_ctx_destroy: pipelines that use the context die with it (their events are freed, the handles
// stay valid for vw_pipeline_destroy, vw_pipeline_run fails with VW_ERR_STATE)
static void kill_pipelines_of(vw_ctx* c) {
  std::lock_guard<std::mutex> g(g_pipe_mu);
  for (vw_pipeline* p : g_pipes)
    if (!p->dead && (p->cf == c || p->ci == c)) {
      std::lock_guard<std::mutex> pg(p->mu);
      hipSetDevice(p->device);
      hipStreamSynchronize(p->cf->stream);
      hipStreamSynchronize(p->ci->stream);
      release_pipeline(p);
      p->dead = true;
    }
}

extern "C" vw_status vw_pipeline_create(vw_ctx* cf, vw_ctx* ci, int elem_bytes, int sets, void* const* x,
                                        void* const* details, void* const* approx, void* const* y, int64_t B,
                                        int64_t N, const double* lo, const double* hi, int L, int wavelet_id,
                                        int boundary, int J, unsigned flags, vw_pipeline** out) {
  if (!cf || !ci || !x || !details || !approx || !y || !lo || !hi || !out) return fail(VW_ERR_NULL, "null argument");
  if (elem_bytes != 8 && elem_bytes != 4) return fail(VW_ERR_ARG, "elem_bytes must be 8 (f64) or 4 (f32)");
  if (sets < 1 || sets > 1024) return fail(VW_ERR_ARG, "sets must be in [1, 1024]");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "Signals cannot be null or empty");
  if (L <= 0 || L > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d out of range", L);
  if (J < 1) return fail(VW_ERR_ARG, "levels must be >= 1");
  if (cf->device != ci->device) return fail(VW_ERR_ARG, "both contexts must be on one device");
  // calls that synchronize or stage host memory have no place in an asynchronous pipeline
  if (flags & (VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC | VW_FLAG_VALIDATE))
    return fail(VW_ERR_ARG, "pipeline steps take device buffers, no SYNC / VALIDATE / HOST_MEMORY");
  for (int r = 0; r < sets; ++r)
    if (!x[r] || !details[r] || !approx[r] || !y[r]) return fail(VW_ERR_NULL, "buffer set %d has a null pointer", r);
  if (cf->capturing || ci->capturing) return fail(VW_ERR_STATE, "a context is capturing");
  vw_pipeline* p = new vw_pipeline();
  p->cf = cf;
  p->ci = ci;
  p->device = cf->device;
  p->esz = elem_bytes;
  p->R = sets;
  p->x.assign(x, x + sets);
  p->det.assign(details, details + sets);
  p->app.assign(approx, approx + sets);
  p->y.assign(y, y + sets);
  p->B = B;
  p->N = N;
  p->lo.assign(lo, lo + L);
  p->hi.assign(hi, hi + L);
  p->L = L;
  p->wavelet_id = wavelet_id;
  p->boundary = boundary;
  p->J = J;
  p->flags = flags;
  hipSetDevice(p->device);
  p->ev_f.assign(sets, nullptr);
  p->ev_i.assign(sets, nullptr);
  p->live.assign(sets, 0);
  hipError_t e = hipEventCreateWithFlags(&p->join_ev, hipEventDisableTiming);
  for (int r = 0; r < sets && e == hipSuccess; ++r) {
    e = hipEventCreateWithFlags(&p->ev_f[r], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_i[r], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    release_pipeline(p);
    delete p;
    return fail(VW_ERR_DEVICE, "event creation failed: %s", hipGetErrorString(e));
  }
  {
    std::lock_guard<std::mutex> g(g_pipe_mu);
    g_pipes.insert(p);
  }
  *out = p;
  return ok();
}

extern "C" vw_status vw_pipeline_run(vw_pipeline* p, int64_t steps) {
  if (!p) return fail(VW_ERR_NULL, "pipeline is null");
  std::lock_guard<std::mutex> pg(p->mu);
  if (p->dead) return fail(VW_ERR_STATE, "a context of this pipeline was destroyed");
  if (steps < 0) return fail(VW_ERR_ARG, "steps must be >= 0");
  // a capture on either context would record one stream's half of each step and wait on events of the
  // other, uncaptured stream: an invalid graph
  if (p->cf->capturing || p->ci->capturing) return fail(VW_ERR_STATE, "a context of this pipeline is capturing");
  hipSetDevice(p->device);
  const bool f32 = p->esz == 4;
  for (int64_t k = 0; k < steps; ++k) {
    const int r = (int)(p->next % p->R);
    hipStream_t sf = p->cf->stream, si = p->ci->stream;
    if (p->live[r]) VW_HIP(hipStreamWaitEvent(sf, p->ev_i[r], 0));
    vw_status st = f32 ? vw_modwt_forward_f32(p->cf, (const float*)p->x[r], p->B, p->N, p->N, p->lo.data(),
                                              p->hi.data(), p->L, p->wavelet_id, p->boundary, p->J, p->flags,
                                              (float*)p->det[r], (float*)p->app[r])
                       : vw_modwt_forward_f64(p->cf, (const double*)p->x[r], p->B, p->N, p->N, p->lo.data(),
                                              p->hi.data(), p->L, p->wavelet_id, p->boundary, p->J, p->flags,
                                              (double*)p->det[r], (double*)p->app[r]);
    if (st != VW_OK) return st;
    VW_HIP(hipEventRecord(p->ev_f[r], sf));
    VW_HIP(hipStreamWaitEvent(si, p->ev_f[r], 0));
    st = f32 ? vw_modwt_inverse_f32(p->ci, (const float*)p->det[r], (const float*)p->app[r], p->B, p->N,
                                    p->lo.data(), p->hi.data(), p->L, p->wavelet_id, p->boundary, p->J, 0xFFFFFFFFu,
                                    0, p->flags, (float*)p->y[r])
             : vw_modwt_inverse_f64(p->ci, (const double*)p->det[r], (const double*)p->app[r], p->B, p->N,
                                    p->lo.data(), p->hi.data(), p->L, p->wavelet_id, p->boundary, p->J, 0xFFFFFFFFu,
                                    0, p->flags, (double*)p->y[r]);
    if (st != VW_OK) return st;
    VW_HIP(hipEventRecord(p->ev_i[r], si));
    p->live[r] = 1;
    ++p->next;
  }
  return ok();
}

extern "C" vw_status vw_pipeline_join(vw_pipeline* p) {
  if (!p) return fail(VW_ERR_NULL, "pipeline is null");
  std::lock_guard<std::mutex> pg(p->mu);
  if (p->dead) return fail(VW_ERR_STATE, "a context of this pipeline was destroyed");
  if (p->cf->capturing || p->ci->capturing) return fail(VW_ERR_STATE, "a context of this pipeline is capturing");
  hipSetDevice(p->device);
  VW_HIP(hipEventRecord(p->join_ev, p->ci->stream));
  VW_HIP(hipStreamWaitEvent(p->cf->stream, p->join_ev, 0));
  std::fill(p->live.begin(), p->live.end(), 0);
  return ok();
}

extern "C" int64_t vw_pipeline_last_set(vw_pipeline* p) {
  if (!p || p->next == 0) return -1;
  return (p->next - 1) % p->R;
}

extern "C" vw_status vw_pipeline_destroy(vw_pipeline* p) {
  if (!p) return fail(VW_ERR_NULL, "pipeline is null");
  {
    std::lock_guard<std::mutex> g(g_pipe_mu);
    g_pipes.erase(p);
  }
  if (!p->dead) {
    hipSetDevice(p->device);
    hipStreamSynchronize(p->cf->stream);
    hipStreamSynchronize(p->ci->stream);
    release_pipeline(p);
  }
  delete p;
  return ok();
}

extern "C" vw_status vw_ctx_set_option(vw_ctx* c, const char* key, int value) {
  if (!c || !key) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!set_tuning(c->tune, key, value)) return fail(VW_ERR_ARG, "unknown option %s", key);
  return ok();
}

extern "C" void* vw_ctx_get_stream(vw_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int vw_ctx_device(vw_ctx* c) { return c ? c->device : -1; }

extern "C" vw_status vw_ctx_synchronize(vw_ctx* c) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  hipSetDevice(c->device);
  VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" const char* vw_last_error(void) { return t_err.c_str(); }
extern "C" int64_t vw_last_error_index(void) { return t_err_index; }
extern "C" const char* vw_version(void) { return "vectorwave_amd 0.1.0 (gfx950)"; }
extern "C" void vw_set_signal_base(int64_t base) { t_signal_base = base; }

extern "C" vw_status vw_ctx_enable_timing(vw_ctx* c, int enable) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->timing = enable != 0;
  return ok();
}

extern "C" vw_status vw_ctx_reset_timing(vw_ctx* c) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  collect_timing(c);
  c->totals.clear();
  return ok();
}

// Start / end of the not-yet-collected timed launches of `family` (the last replay of each graph, or
// the direct launches since the last collect), in ms after `ref_event` (a hipEvent_t recorded before
// them, on any stream of the device) -- for callers that run several contexts concurrently and need
// the wall window of a kernel family across them.  Call before vw_ctx_kernel_time, which consumes the
// launches.  *count receives the number found (at most max are written).
extern "C" vw_status vw_ctx_kernel_spans(vw_ctx* c, const char* family, void* ref_event, int64_t max,
                                         double* start_ms, double* end_ms, int64_t* count) {
  if (!c || !family || !ref_event || !count) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  int64_t n = 0;
  for (const auto& tl : c->pending) {
    if (tl.family != family) continue;
    float a = 0.f, b = 0.f;
    VW_HIP(hipEventSynchronize(tl.stop));
    VW_HIP(hipEventElapsedTime(&a, (hipEvent_t)ref_event, tl.start));
    VW_HIP(hipEventElapsedTime(&b, (hipEvent_t)ref_event, tl.stop));
    if (n < max) {
      if (start_ms) start_ms[n] = a;
      if (end_ms) end_ms[n] = b;
    }
    ++n;
  }
  *count = n;
  return ok();
}

extern "C" vw_status vw_ctx_kernel_time(vw_ctx* c, const char* family, double* total_ms, int64_t* launches) {
  if (!c || !family) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  collect_timing(c);
  auto it = c->totals.find(family);
  if (total_ms) *total_ms = it == c->totals.end() ? 0.0 : it->second.first;
  if (launches) *launches = it == c->totals.end() ? 0 : it->second.second;
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Common argument checks (MultiLevelMODWTTransform.decompose :209-239, BatchMODWT.validateAoS :201-212)
static vw_status check_common(vw_ctx* c, const void* a, const void* b, const double* lo, const double* hi,
                              int64_t B, int64_t N, int L, int boundary) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!a || !b || !lo || !hi) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING)
    return fail(VW_ERR_BOUNDARY, "MODWT only supports PERIODIC, ZERO_PADDING, and SYMMETRIC boundary modes");
  if (L < 1 || L > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", L, kMaxTaps);
  return VW_OK;
}

static vw_status check_levels(int64_t N, int L, int J, unsigned flags) {
  if (flags & VW_FLAG_CORE_LEVELS) {
    const int maxl = vw_max_levels(N, L);
    if (J < 1 || J > maxl)
      return fail(VW_ERR_LEVEL, "Invalid number of decomposition levels: %d (valid 1..%d for N=%lld, L=%d)", J, maxl,
                  (long long)N, L);
  } else {
    if (J < 1) return fail(VW_ERR_LEVEL, "levels must be >= 1");
    if (J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels %d exceeds engine limit %d", J, kMaxLevels);
    if (vw_upsampled_length(L, J) > (int64_t)1 << 30) return fail(VW_ERR_TOO_LARGE, "upsampled filter too long");
  }
  return VW_OK;
}

// The _bi_ entry points (two filter lengths; Lhi == 0: an equal-length entry point, nothing to check).  L has
// passed check_common / check_levels, which for CORE_LEVELS is the reference's cap on the low-pass length alone
// (calculateMaxLevels :455-501); its guards then want both upsampled filters within the signal (:717-729,
// :561-574).  Without CORE_LEVELS the longer filter meets the equal-length call's checks.
static vw_status check_bank(int64_t N, int L, int Lhi, int J, unsigned flags, bool forward) {
  if (Lhi == 0) return VW_OK;
  if (Lhi < 1 || Lhi > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", Lhi, kMaxTaps);
  if (flags & VW_FLAG_CORE_LEVELS) {
    if (vw_upsampled_length(std::max(L, Lhi), J) > N)
      return fail(VW_ERR_TOO_LARGE, "Upsampled %s filter length exceeds signal length", forward ? "analysis" : "reconstruction");
  } else if (forward && Lhi > L) {
    if (vw_upsampled_length(Lhi, J) > (int64_t)1 << 30) return fail(VW_ERR_TOO_LARGE, "upsampled filter too long");
  }
  return VW_OK;
}

template <typename T>
static void copy_taps(T* dst, const double* src, int L) {
  // base taps * (1.0 / Math.sqrt(2.0)) in double, then rounded to T  (ScalarOps.java:911-914)
  const double s = 1.0 / std::sqrt(2.0);
  for (int i = 0; i < L; ++i) dst[i] = (T)(src[i] * s);
  for (int i = L; i < kMaxTaps; ++i) dst[i] = T(0);
}

// Both filters of a call for a kernel of `taps` taps (the plan's, vw_plan.h): a bank of two lengths has its shorter
// filter zero-extended, and on the pairwise inverses (taps = k.L) a longer high-pass truncated.
template <typename T, typename Call>
static void copy_bank(T* lo, T* hi, const Call& k, int taps, int taps_hi = 0) {
  copy_taps(lo, k.lo, std::min(k.L, taps));
  copy_taps(hi, k.hi, std::min(k.Lhi > 0 ? k.Lhi : k.L, taps_hi > 0 ? taps_hi : taps));
}

// Calls that synchronize cannot be recorded into a graph (vw_capture_begin).
static vw_status capture_guard(vw_ctx* c, unsigned flags) {
  if (c->capturing && (flags & (VW_FLAG_VALIDATE | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC)))
    return fail(VW_ERR_STATE, "validation, host memory and SYNC cannot be captured");
  return VW_OK;
}

static vw_status read_bad(vw_ctx* c, unsigned long long* out) {
  VW_HIP(hipMemcpyAsync(out, c->bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

static vw_status report_bad(unsigned long long bad, int64_t N) {
  if (bad == ~0ull) return VW_OK;
  const bool out = (bad >> 62) & 1ull;
  const unsigned long long flat = bad & ((1ull << 62) - 1);
  t_err_index = (int64_t)(flat % (unsigned long long)N);
  return fail(VW_ERR_NONFINITE, "%s contains non-finite value at index %lld (signal %lld)",
              out ? "coefficients" : "signal", (long long)(flat % (unsigned long long)N),
              (long long)(flat / (unsigned long long)N) + (long long)t_signal_base);
}

// ------------------------------------------------------------------------------------------------
// VW_FLAG_REF_NONFINITE (vw_ref.hip): after the fast kernels, flag the rows holding a non-finite value
// in any of `planes` (the call's inputs and outputs: an overflow to Inf inside the cascade shows in an
// output), then recompute those rows with the reference's full-tap loops.  Stream-ordered, capturable
// once the workspace has grown.  Row flags and scratch (`grid` workgroups) are the plan's reservation,
// made before the launches.
template <typename T>
struct ScanPlane {
  const T* p;
  int64_t ld;
  int len;  // 0: the call's N
};

template <typename T>
static vw_status ref_nonfinite(vw_ctx* c, const std::vector<ScanPlane<T>>& planes, RefArgs<T>& r,
                               bool inverse, bool flagged, int grid) {
  const int64_t B = r.B, N = r.N;
  if ((int)planes.size() > kRefPlanes) return fail(VW_ERR_ARG, "too many planes for the non-finite scan");
  // timing families: "ref_nonfinite" (the cascade over rows the fast kernel flagged), "ref_nonfinite_scan"
  // (scan + cascade)
  LaunchTimer lt(c, flagged ? "ref_nonfinite" : "ref_nonfinite_scan");
  hipError_t e;
  if (!flagged) {  // the fast kernel did not probe its rows: scan the call's planes
    RefScan<T> s;
    memset(&s, 0, sizeof(s));
    for (const auto& p : planes) {
      s.p[s.np] = p.p;
      s.ld[s.np] = p.ld;
      s.len[s.np] = p.len;
      ++s.np;
    }
    s.B = B; s.N = (int)N; s.chunks = ref_scan_chunks((int)N); s.flag = c->nf;
    e = launch_flag_nonfinite<T>(s, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "non-finite scan launch failed: %s", hipGetErrorString(e));
  }
  r.flag = c->nf;
  r.scratch = reinterpret_cast<T*>(c->ws);
  e = launch_ref_cascade<T>(r, (int)grid, inverse, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "reference-arithmetic launch failed: %s", hipGetErrorString(e));
  return VW_OK;
}

// the matrix-core kernels are fp32 only (vw_mfma.hip); the double overloads are never reached
static hipError_t mfma_forward(const FwdArgs<float>& a, int lds, hipStream_t st) { return launch_forward_mfma(a, lds, st); }
static hipError_t mfma_forward(const FwdArgs<double>&, int, hipStream_t) { return hipErrorNotSupported; }
static hipError_t mfma_inverse(const InvArgs<float>& a, int lds, hipStream_t st) { return launch_inverse_mfma(a, lds, st); }
static hipError_t mfma_inverse(const InvArgs<double>&, int, hipStream_t) { return hipErrorNotSupported; }

// ------------------------------------------------------------------------------------------------
// Executors.  Selection is vw_plan.cpp's: plan_forward / plan_inverse return which kernels run with what
// launch shape and layout, which buffers they read and write, and what must be reserved.  The code below
// adds the pointers and issues the launches; it decides nothing.

// Everything a plan lists, before the first launch: a failure leaves nothing queued (no row flags set by a
// probing kernel whose fix-up then cannot run).
static vw_status reserve(vw_ctx* c, const PlanReserve& r) {
  if (r.ws_bytes) VW_TRY(ensure_ws(c, r.ws_bytes));
  if (r.nf_rows) VW_TRY(ensure_nf(c, r.nf_rows));
  return VW_OK;
}

static const char* const kStepNames[] = {"deep", "multi-level", "level-group", "level", "level"};
static vw_status step_failed(const char* dir, int kind, hipError_t e) {
  return fail(VW_ERR_DEVICE, "%s %s launch failed: %s", dir, kStepNames[kind - kStepDeep], hipGetErrorString(e));
}

// Per-level forward: the plan's steps, ping-ponging the running approximation through the workspace.
template <typename T>
static vw_status forward_steps(vw_ctx* c, const FwdCall<T>& k, const FwdPlan<T>& p) {
  const size_t plane = (size_t)k.B * (size_t)k.N;
  T* const ws[2] = {reinterpret_cast<T*>(c->ws), reinterpret_cast<T*>(c->ws) + plane};
  for (const PlanStep<T>& s : p.steps) {
    const T* const src = s.src == kBufIn ? k.x : ws[s.src - kBufWs0];
    T* const dst = s.dst == kBufOut ? k.approx : ws[s.dst - kBufWs0];
    T* const det = k.details + (size_t)(s.jlo - 1) * plane;  // d of the step's first level
    hipError_t e;
    if (s.kind == kStepDeep) {
      DeepArgs<T> d = s.deep;
      d.src = src; d.out = dst;
      d.nf_flag = s.probe ? c->nf : nullptr;
      for (int g = 0; g < d.g; ++g) d.out_d[g] = det + (size_t)g * plane;
      copy_bank(d.lo, d.hi, k, d.taps);
      LaunchTimer lt(c, "forward_level");
      e = launch_deep<T>(d, s.lds, p.fma, false, c->stream);
    } else if (s.kind == kStepMulti) {
      MultiArgs<T> m = s.multi;
      m.src_a = src; m.out_a = dst;
      for (int g = 0; g < m.nlev; ++g) m.out_d[g] = det + (size_t)g * plane;
      copy_bank(m.lo, m.hi, k, m.taps);
      LaunchTimer lt(c, "forward_level");
      e = launch_forward_multi<T>(m, s.lds, p.fma, c->stream);
    } else {
      LevelArgs<T> a = s.lvl;
      a.src_a = src; a.out_a = dst; a.out_d = det;
      a.hist = k.hist ? k.hist[s.jlo - 1] : nullptr;
      a.bad = c->bad;
      copy_bank(a.lo, a.hi, k, a.taps);
      LaunchTimer lt(c, "forward_level");
      e = s.kind == kStepSweep ? launch_forward_sweep<T>(a, p.fma, c->stream)
                               : launch_forward_level<T>(a, s.lds, p.fma, c->stream);
    }
    if (e != hipSuccess) return step_failed("forward", s.kind, e);
    if (s.hist_update) {
      e = launch_history_update<T>(src, s.lvl.lda, k.hist[s.jlo - 1], k.hist[s.jlo - 1], k.B, (int)k.N,
                                   s.lvl.lv.hist_len, c->stream);
      if (e != hipSuccess) return fail(VW_ERR_DEVICE, "history update failed: %s", hipGetErrorString(e));
    }
  }
  return VW_OK;
}

// ------------------------------------------------------------------------------------------------
// Forward -> inverse pairs as one k_roundtrip launch (vw_pair.hip; vw_plan.h pair_fusable; VW_PAIR_FUSE).
// While capturing with timing off, an eligible forward is launched as ever and its kernel node remembered; if
// the very next call is the inverse of its coefficients, that node's parameters are replaced by the round trip's
// and no inverse node is added.  Nothing is held back: work a caller captures on the stream between the two calls
// keeps its place, and ends the pairing (the stream's capture dependencies are then no longer that node alone).

// The one node the next operation captured on `st` would depend on (false: not capturing, or not exactly one).
static bool capture_tail(hipStream_t st, hipGraphNode_t* node) {
  hipStreamCaptureStatus status;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  if (hipStreamGetCaptureInfo_v2(st, &status, &id, &g, &deps, &ndeps) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (status != hipStreamCaptureStatusActive || ndeps != 1 || !deps) return false;
  *node = deps[0];
  return true;
}

// what a forward plan must be for its launch to become a round trip (pair_fusable decides on the pair)
static bool pair_forward_shape(const FwdPlan<double>& p) {
  return p.fused && p.kernel == kFwdPersist && p.args.level_ct && p.nv == 4 && p.args.taps <= kPairMaxTaps;
}

// After an eligible forward's launch.  Uncaptured: the round trip's LDS limit and occupancy, which a capture
// cannot query.  Captured: remember the node.
static void pair_after_forward(vw_ctx* c, const FwdCall<double>& k, const FwdPlan<double>& p, const FwdArgs<double>& a) {
  c->pair.valid = false;
  if (!c->tune.pair_fuse || !pair_forward_shape(p)) return;
  if (!c->capturing) {
    if (pair_prepare(a.taps, p.fma, p.threads, p.lds, c->tune.pair_keep, nullptr, nullptr) != hipSuccess) (void)hipGetLastError();
    return;
  }
  if (c->timing || p.ref_nf || p.validate) return;
  hipGraphNode_t node = nullptr;
  hipGraphNodeType ty;
  if (!capture_tail(c->stream, &node)) return;
  if (hipGraphNodeGetType(node, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) {
    (void)hipGetLastError();
    return;
  }
  c->pair.node = node;
  c->pair.call = k;
  c->pair.call.lo = c->pair.call.hi = nullptr;  // the caller's arrays: a.lo / a.hi hold their values
  c->pair.plan = p;
  c->pair.args = a;
  c->pair.valid = true;
}
static void pair_after_forward(vw_ctx* c, const FwdCall<float>&, const FwdPlan<float>&, const FwdArgs<float>&) {
  c->pair.valid = false;
}

// The round trip's arguments: the forward's as launched, the inverse's taps, output and right halos.
static void pair_args(const FwdArgs<double>& f, const InvCall<double>& k, const InvPlan<double>& p, PairArgs<double>* a) {
  a->f = f;
  a->y = k.y;
  double lo[kMaxTaps], hi[kMaxTaps];
  copy_bank(lo, hi, k, p.args.taps, p.args.taps_hi);
  for (int i = 0; i < kPairMaxTaps; ++i) { a->ilo[i] = lo[i]; a->ihi[i] = hi[i]; }
  for (int j = 0; j < kMaxLevels; ++j) { a->hr[j] = p.args.lv[j].hr; a->own[j] = p.args.lv[j].own; }
}

// At an inverse call: true when the remembered forward's node now runs the round trip (no inverse launch needed).
static bool try_pair_fuse(vw_ctx* c, const InvCall<double>& k, const InvPlan<double>& p) {
  const bool pending = c->pair.valid;
  c->pair.valid = false;
  if (!pending || !c->capturing || c->timing || !c->tune.pair_fuse) return false;
  hipGraphNode_t tail = nullptr;
  if (!capture_tail(c->stream, &tail) || tail != c->pair.node) return false;  // something was captured in between
  if (!pair_fusable(c->pair.call, c->pair.plan, k, p)) return false;
  const FwdPlan<double>& fp = c->pair.plan;
  PairLaunch l;
  if (!pair_launch_shape(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, k.B, c->cus, &l)) return false;  // never run uncaptured
  PairArgs<double> a;
  pair_args(c->pair.args, k, p, &a);
  void* params[] = {&a};
  hipKernelNodeParams np;
  memset(&np, 0, sizeof(np));
  np.func = const_cast<void*>(l.func);
  np.gridDim = dim3(l.grid);
  np.blockDim = dim3(l.threads);
  np.sharedMemBytes = l.lds;
  np.kernelParams = params;
  if (hipGraphKernelNodeSetParams(c->pair.node, &np) != hipSuccess) {
    (void)hipGetLastError();  // this runtime keeps the node as it is: the inverse is launched as ever
    return false;
  }
  ++c->fused_pairs;
  return true;
}
static bool try_pair_fuse(vw_ctx* c, const InvCall<float>&, const InvPlan<float>&) {
  c->pair.valid = false;
  return false;
}

// Forward (multi-level and single-level share this path).
template <typename T>
static vw_status forward_impl(vw_ctx* c, FwdCall<T> k) {
  VW_TRY(capture_guard(c, k.flags));
  k.cus = c->cus;
  FwdPlan<T> p;
  plan_forward(c->tune, k, &p);
  if (p.error != VW_OK) return fail((vw_status)p.error, "%s", p.msg);
  VW_TRY(reserve(c, p.res));
  const LevelDesc* const lv = p.args.lv;
  if (p.snapshot)
    for (int j = 0; j < k.J; ++j)
      if (lv[j].hist_len > 0)
        VW_HIP(hipMemcpyAsync(k.hist_snap[j], k.hist[j], (size_t)k.B * lv[j].hist_len * sizeof(T),
                              hipMemcpyDeviceToDevice, c->stream));
  if (p.validate) VW_HIP(hipMemsetAsync(c->bad, 0xFF, sizeof(unsigned long long), c->stream));
  if (p.fused) {
    FwdArgs<T> a = p.args;
    a.x = k.x; a.details = k.details; a.approx = k.approx;
    a.bad = c->bad;
    a.nf_flag = p.nf_probed ? c->nf : nullptr;
    for (int j = 0; j < k.J; ++j) a.hist[j] = k.hist ? k.hist[j] : nullptr;
    copy_bank(a.lo, a.hi, k, a.taps, a.taps_hi);
    {
      LaunchTimer lt(c, "forward");
      hipError_t e = p.kernel == kFwdMfma    ? mfma_forward(a, p.lds, c->stream)
                   : p.kernel == kFwdBlk     ? launch_forward_blk<T>(a, p.threads, p.lds, p.fma, p.nv, c->stream)
                   : p.kernel == kFwdPersist ? launch_forward_persist<T>(a, p.threads, p.lds, p.fma, p.nv, c->stream)
                                             : launch_forward_fused<T>(a, p.threads, p.lds, p.fma, p.nv, c->stream);
      if (e != hipSuccess) return fail(VW_ERR_DEVICE, "forward launch failed: %s", hipGetErrorString(e));
    }
    pair_after_forward(c, k, p, a);  // VW_PAIR_FUSE: the next call may be this forward's inverse
  } else {
    VW_TRY(forward_steps(c, k, p));
  }
  if (p.ref_nf) {
    // a_J alone: every non-finite level input (x, a_1 .. a_{J-1}, a history) reaches it (vw_ref.hip)
    std::vector<ScanPlane<T>> planes{{k.approx, k.N, 0}};
    RefArgs<T> r;
    memset(&r, 0, sizeof(r));
    r.x = k.x; r.ldx = k.ldx; r.details = k.details; r.approx = k.approx;
    r.B = k.B; r.N = (int)k.N; r.J = k.J; r.L = k.L; r.mode = ref_mode(k.boundary);
    if (k.hist) {  // BatchStreamingMODWT block / flush: the histories the block read, and the ones it leaves
      r.hist_mode = 1;
      r.hist_first = k.hist_first ? 1 : 0;
      for (int j = 0; j < k.J; ++j) {
        r.hist_len[j] = lv[j].hist_len;
        r.hist_old[j] = k.hist_first ? nullptr : (k.hist_update ? k.hist_snap[j] : k.hist[j]);
        r.hist_new[j] = k.hist_update ? k.hist[j] : nullptr;
      }
    }
    r.Lhi = k.Lhi;
    copy_bank(r.lo, r.hi, k, p.args.taps, p.args.taps_hi);
    VW_TRY(ref_nonfinite<T>(c, planes, r, false, p.nf_probed, p.res.ref_grid));
  }
  if (p.validate) {
    unsigned long long bad = 0;
    VW_TRY(read_bad(c, &bad));
    VW_TRY(report_bad(bad, k.N));
  }
  if (k.flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

// Per-level inverse: the plan's steps from level J down.
template <typename T>
static vw_status inverse_steps(vw_ctx* c, const InvCall<T>& k, const InvPlan<T>& p) {
  const size_t plane = (size_t)k.B * (size_t)k.N;
  T* const ws[2] = {reinterpret_cast<T*>(c->ws), reinterpret_cast<T*>(c->ws) + plane};
  auto det = [&](int j, int use_d) { return use_d ? k.details + (size_t)(j - 1) * plane : nullptr; };
  auto thr = [&](int j) { return k.thr ? k.thr + (size_t)(j - 1) * (size_t)k.thr_ld : nullptr; };
  for (const PlanStep<T>& s : p.steps) {
    const T* const src = s.src == kBufNone ? nullptr : s.src == kBufIn ? k.approx : ws[s.src - kBufWs0];
    T* const dst = s.dst == kBufOut ? k.y : ws[s.dst - kBufWs0];
    hipError_t e;
    if (s.kind == kStepDeep) {
      DeepArgs<T> d = s.deep;
      d.src = src; d.out = dst;
      for (int g = 0; g < d.g; ++g) {
        d.src_d[g] = det(s.jlo + g, p.args.lv[s.jlo - 1 + g].use_d);
        d.thr[g] = thr(s.jlo + g);
      }
      copy_bank(d.lo, d.hi, k, d.taps);
      LaunchTimer lt(c, "inverse_level");
      e = launch_deep<T>(d, s.lds, p.fma, true, c->stream);
    } else if (s.kind == kStepMulti) {
      MultiArgs<T> m = s.multi;
      m.src_a = src; m.out_a = dst;
      m.nf_flag = s.probe ? c->nf : nullptr;
      for (int g = 0; g < m.nlev; ++g) {
        m.src_d[g] = det(s.jlo + g, p.args.lv[s.jlo - 1 + g].use_d);
        m.thr[g] = thr(s.jlo + g);
      }
      copy_bank(m.lo, m.hi, k, m.taps);
      LaunchTimer lt(c, "inverse_level");
      e = launch_inverse_multi<T>(m, s.lds, p.fma, c->stream);
    } else {
      LevelArgs<T> a = s.lvl;
      a.src_a = src; a.out_a = dst;
      a.src_d = det(s.jhi, a.use_d);
      a.thr = thr(s.jhi);
      if (s.kind == kStepSweepG) {  // the chained sweeps read the details of the levels below the top too
        a.src_d2 = det(s.jhi - 1, a.use_d2);
        a.thr2 = thr(s.jhi - 1);
        if (s.jhi - s.jlo == 2) {
          a.src_d3 = det(s.jhi - 2, a.use_d3);
          a.thr3 = thr(s.jhi - 2);
        }
      }
      copy_bank(a.lo, a.hi, k, a.taps);
      LaunchTimer lt(c, "inverse_level");
      e = s.kind == kStepSweepG ? launch_inverse_sweepg<T>(a, s.G, s.ka, s.R, p.fma, c->stream)
        : s.kind == kStepSweep  ? launch_inverse_sweep<T>(a, p.fma, c->stream)
                                : launch_inverse_level<T>(a, s.lds, p.fma, c->stream);
    }
    if (e != hipSuccess) return step_failed("inverse", s.kind, e);
  }
  return VW_OK;
}

// Inverse
template <typename T>
static vw_status inverse_impl(vw_ctx* c, InvCall<T> k) {
  VW_TRY(capture_guard(c, k.flags));
  k.cus = c->cus;
  InvPlan<T> p;
  plan_inverse(c->tune, k, &p);
  if (p.error != VW_OK) return fail((vw_status)p.error, "%s", p.msg);
  VW_TRY(reserve(c, p.res));
  if (try_pair_fuse(c, k, p)) return VW_OK;  // the captured forward before this call now runs both (VW_PAIR_FUSE)
  if (p.fused) {
    InvArgs<T> a = p.args;
    a.details = k.details; a.approx = k.approx; a.y = k.y; a.thr = k.thr;
    a.nf_flag = p.nf_probed ? c->nf : nullptr;
    copy_bank(a.lo, a.hi, k, a.taps, a.taps_hi);
    LaunchTimer lt(c, "inverse");
    hipError_t e = p.kernel == kInvMfma ? mfma_inverse(a, p.lds, c->stream)
                                        : launch_inverse_fused<T>(a, p.threads, p.lds, p.fma, p.nv, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "inverse launch failed: %s", hipGetErrorString(e));
  } else {
    VW_TRY(inverse_steps(c, k, p));
  }
  if (p.ref_nf) {
    // y alone: every non-finite level input (a_J, a kept d_j, an intermediate approximation) reaches it
    std::vector<ScanPlane<T>> planes{{k.y, k.N, 0}};
    RefArgs<T> r;
    memset(&r, 0, sizeof(r));
    r.x = k.approx_zero ? nullptr : k.approx; r.det_in = k.details; r.y = k.y;
    r.thr = k.thr; r.thr_ld = k.thr_ld; r.soft = k.soft;
    r.B = k.B; r.N = (int)k.N; r.J = k.J; r.L = k.L; r.mode = ref_mode(k.boundary);
    r.Lhi = k.Lhi;
    copy_bank(r.lo, r.hi, k, p.args.taps, p.args.taps_hi);
    for (int j = 0; j < k.J; ++j) r.lv[j] = p.args.lv[j];
    VW_TRY(ref_nonfinite<T>(c, planes, r, true, p.nf_probed, p.res.ref_grid));
  }
  if (k.flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

// ------------------------------------------------------------------------------------------------
// Host-memory staging (the JNI / FFM path): copy in, run on device, copy out, synchronize.  Device
// buffers are carved from the context's staging pool (blocks kept across calls, never hipMalloc /
// hipFree per call: a JNI caller's per-batch loop pays only the copies and the kernels).  A call
// carves from offset 0 of the pool; its destructor synchronizes the stream, so the next call may
// reuse the same bytes.  Calls on one context are serialized by its mutex.
struct Staging {
  vw_ctx* c;
  size_t used_block = 0, used_off = 0;
  explicit Staging(vw_ctx* ctx) : c(ctx) {}
  // After the call's copies and kernels: keep only the largest block (the next call of the same
  // shape allocates at most one block >= its whole need, and frees this one here), so the pool holds
  // one block of about the largest call's size instead of every block it ever grew through.
  ~Staging() {
    hipStreamSynchronize(c->stream);
    if (c->stage.size() > 1) {
      auto big = std::max_element(c->stage.begin(), c->stage.end(),
                                  [](const std::pair<void*, size_t>& a, const std::pair<void*, size_t>& b) {
                                    return a.second < b.second;
                                  });
      const auto keep = *big;
      for (auto& blk : c->stage)
        if (blk.first != keep.first) hipFree(blk.first);
      c->stage.assign(1, keep);
    }
  }
  vw_status carve(size_t bytes, void** out) {
    bytes = align_up(std::max<size_t>(bytes, 16), 256);
    for (; used_block < c->stage.size(); ++used_block, used_off = 0) {
      auto& blk = c->stage[used_block];
      if (used_off + bytes <= blk.second) {
        *out = static_cast<char*>(blk.first) + used_off;
        used_off += bytes;
        return VW_OK;
      }
    }
    // a new block covers everything this call has carved so far plus this request, so the pool
    // converges to one block per call shape (see the destructor)
    size_t carved = bytes;
    for (size_t k = 0; k < used_block && k < c->stage.size(); ++k) carved += c->stage[k].second;
    if (used_block < c->stage.size()) carved += used_off;
    const size_t want = std::max({carved, (size_t)4 << 20});
    void* p = nullptr;
    VW_HIP(hipMalloc(&p, want));
    c->stage.push_back({p, want});
    used_block = c->stage.size() - 1;
    used_off = bytes;
    *out = p;
    return VW_OK;
  }
  template <typename T>
  vw_status in(const T* host, size_t count, T** dev) {
    void* p = nullptr;
    VW_TRY(carve(count * sizeof(T), &p));
    if (host && count) VW_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dev = reinterpret_cast<T*>(p);
    return VW_OK;
  }
  // `planes` blocks of `count` elements, the host blocks `host_stride` elements apart (a row block of a
  // [planes][B][N] host array), packed on the device
  template <typename T>
  vw_status in_planes(const T* host, size_t planes, size_t count, size_t host_stride, T** dev) {
    void* p = nullptr;
    VW_TRY(carve(planes * count * sizeof(T), &p));
    if (host && count && planes)
      VW_HIP(hipMemcpy2DAsync(p, count * sizeof(T), host, host_stride * sizeof(T), count * sizeof(T), planes,
                              hipMemcpyHostToDevice, c->stream));
    *dev = reinterpret_cast<T*>(p);
    return VW_OK;
  }
  template <typename T>
  vw_status out(T* host, const T* dev, size_t count) {
    if (host && count) VW_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return VW_OK;
  }
  template <typename T>
  vw_status out_planes(T* host, const T* dev, size_t planes, size_t count, size_t host_stride) {
    if (host && count && planes)
      VW_HIP(hipMemcpy2DAsync(host, host_stride * sizeof(T), dev, count * sizeof(T), count * sizeof(T), planes,
                              hipMemcpyDeviceToHost, c->stream));
    return VW_OK;
  }
};


// Host-memory forward of B rows: x[B][ldx] in, details as J host planes `det_stride` elements apart
// (B * N for a whole batch; the global B * N for a row block of a sharded batch), approx [B][N].
// Caller holds c->mu.  Synchronous.
template <typename T>
static vw_status forward_host(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                              const double* hi, int L, int boundary, int J, unsigned flags, T* details,
                              int64_t det_stride, T* approx, int Lhi = 0) {
  if (c->capturing) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
  Staging s(c);
  T *dx, *dd, *da;
  VW_TRY(s.in(x, (size_t)(B - 1) * ldx + N, &dx));  // (the last row's padding need not exist)
  VW_TRY(s.in<T>(nullptr, (size_t)J * B * N, &dd));
  VW_TRY(s.in<T>(nullptr, (size_t)B * N, &da));
  FwdCall<T> fk;
  fk.x = dx; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
  fk.flags = flags & ~(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY); fk.details = dd; fk.approx = da; fk.Lhi = Lhi;
  VW_TRY(forward_impl<T>(c, fk));
  VW_TRY(s.out_planes(details, dd, (size_t)J, (size_t)(B * N), (size_t)det_stride));
  VW_TRY(s.out(approx, da, (size_t)B * N));
  VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

template <typename T>
static vw_status inverse_host(vw_ctx* c, const T* details, int64_t det_stride, const T* approx, int64_t B, int64_t N,
                              const double* lo, const double* hi, int L, int wid, int boundary, int J,
                              unsigned detail_mask, int approx_zero, unsigned flags, T* y, int Lhi = 0) {
  if (c->capturing) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
  Staging s(c);
  T *dd = nullptr, *da = nullptr, *dy;
  if (detail_mask) VW_TRY(s.in_planes(details, (size_t)J, (size_t)(B * N), (size_t)det_stride, &dd));
  if (!approx_zero) VW_TRY(s.in(approx, (size_t)B * N, &da));
  VW_TRY(s.in<T>(nullptr, (size_t)B * N, &dy));
  InvCall<T> ik;
  ik.details = dd; ik.approx = da; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.wid = wid;
  ik.boundary = boundary; ik.J = J; ik.detail_mask = detail_mask; ik.approx_zero = approx_zero;
  ik.flags = flags & ~(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY); ik.y = dy; ik.Lhi = Lhi;
  VW_TRY(inverse_impl<T>(c, ik));
  VW_TRY(s.out(y, dy, (size_t)B * N));
  VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

template <typename T>
static vw_status modwt_forward(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                               const double* hi, int L, int wid, int boundary, int J, unsigned flags, T* details,
                               T* approx, int Lhi = 0) {
  (void)wid;
  VW_TRY(check_common(c, x, details, lo, hi, B, N, L, boundary));
  if (!approx) return fail(VW_ERR_NULL, "approx is null");
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  VW_TRY(check_levels(N, L, J, flags));
  VW_TRY(check_bank(N, L, Lhi, J, flags, true));
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    VW_TRY(forward_host<T>(c, x, B, N, ldx, lo, hi, L, boundary, J, flags, details, B * N, approx, Lhi));
    return ok();
  }
  FwdCall<T> fk;
  fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
  fk.flags = flags; fk.details = details; fk.approx = approx; fk.Lhi = Lhi;
  VW_TRY(forward_impl<T>(c, fk));
  return ok();
}

// The argument checks of vw_modwt_inverse_* (shared with the multiresolution calls, which make them too).
static vw_status check_inverse(vw_ctx* c, const void* details, const void* approx, const void* y, const double* lo,
                               const double* hi, int64_t B, int64_t N, int L, int boundary, int J, unsigned detail_mask,
                               int approx_zero, unsigned flags) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!y || !lo || !hi) return fail(VW_ERR_NULL, "null argument");
  if (!details && detail_mask) return fail(VW_ERR_NULL, "details is null");
  if (!approx && !approx_zero) return fail(VW_ERR_NULL, "approx is null");
  VW_TRY(check_common(c, y, y, lo, hi, B, N, L, boundary));
  if (J < 1 || J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels must be in 1..%d", kMaxLevels);
  // applyScaledInverseMODWT guard :561-574 (reconstruct has no level cap, only L_j <= N); the SWT
  // periodic inverse (VectorWaveSwtAdapter.reconstructPeriodic :444-474) wraps instead.
  if ((flags & VW_FLAG_CORE_LEVELS) && vw_upsampled_length(L, J) > N)
    return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  return VW_OK;
}

template <typename T>
static vw_status modwt_inverse(vw_ctx* c, const T* details, const T* approx, int64_t B, int64_t N, const double* lo,
                               const double* hi, int L, int wid, int boundary, int J, unsigned detail_mask,
                               int approx_zero, unsigned flags, T* y, int Lhi = 0) {
  VW_TRY(check_inverse(c, details, approx, y, lo, hi, B, N, L, boundary, J, detail_mask, approx_zero, flags));
  VW_TRY(check_bank(N, L, Lhi, J, flags, false));
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    VW_TRY(inverse_host<T>(c, details, B * N, approx, B, N, lo, hi, L, wid, boundary, J, detail_mask, approx_zero,
                           flags, y, Lhi));
    return ok();
  }
  InvCall<T> ik;
  ik.details = details; ik.approx = approx; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.wid = wid;
  ik.boundary = boundary; ik.J = J; ik.detail_mask = detail_mask; ik.approx_zero = approx_zero; ik.flags = flags;
  ik.y = y; ik.Lhi = Lhi;
  VW_TRY(inverse_impl<T>(c, ik));
  return ok();
}

extern "C" vw_status vw_modwt_forward_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                          const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                          unsigned flags, double* details, double* approx) {
  return modwt_forward<double>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, details, approx);
}
extern "C" vw_status vw_modwt_forward_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx,
                                          const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                          unsigned flags, float* details, float* approx) {
  return modwt_forward<float>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, details, approx);
}
extern "C" vw_status vw_modwt_inverse_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                          int64_t N, const double* lo, const double* hi, int L, int wid, int boundary,
                                          int J, unsigned detail_mask, int approx_zero, unsigned flags, double* y) {
  return modwt_inverse<double>(c, details, approx, B, N, lo, hi, L, wid, boundary, J, detail_mask, approx_zero,
                               flags, y);
}
extern "C" vw_status vw_modwt_inverse_f32(vw_ctx* c, const float* details, const float* approx, int64_t B,
                                          int64_t N, const double* lo, const double* hi, int L, int wid, int boundary,
                                          int J, unsigned detail_mask, int approx_zero, unsigned flags, float* y) {
  return modwt_inverse<float>(c, details, approx, B, N, lo, hi, L, wid, boundary, J, detail_mask, approx_zero, flags,
                              y);
}

// Forward, then inverse of its coefficients (include/vectorwave_amd.h): one k_roundtrip launch where the pair is
// eligible (pair_fusable) and the launch shape is, or can be made, ready; the two calls otherwise.
extern "C" vw_status vw_modwt_roundtrip_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                            const double* lo, const double* hi, const double* rlo, const double* rhi,
                                            int L, int wid, int boundary, int J, unsigned flags, double* details,
                                            double* approx, double* y) {
  if (c && x && details && approx && y && lo && hi && rlo && rhi && !(flags & VW_FLAG_HOST_MEMORY) && B > 0 && N > 0 &&
      ldx >= N && L >= 1 && L <= kPairMaxTaps && J >= 1 && J <= kMaxLevels && boundary == VW_PERIODIC) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    hipSetDevice(c->device);
    FwdCall<double> fk;
    fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
    fk.flags = flags; fk.details = details; fk.approx = approx; fk.cus = c->cus;
    InvCall<double> ik;
    ik.details = details; ik.approx = approx; ik.B = B; ik.N = N; ik.lo = rlo; ik.hi = rhi; ik.L = L; ik.wid = wid;
    ik.boundary = boundary; ik.J = J; ik.flags = flags; ik.y = y; ik.cus = c->cus;
    FwdPlan<double> fp;
    InvPlan<double> ip;
    if (c->tune.pair_fuse && check_levels(N, L, J, flags) == VW_OK && capture_guard(c, flags) == VW_OK) {
      plan_forward(c->tune, fk, &fp);
      plan_inverse(c->tune, ik, &ip);
      PairLaunch l;
      if (pair_fusable(fk, fp, ik, ip) &&
          (c->capturing ||
           pair_prepare(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, nullptr, nullptr) == hipSuccess) &&
          pair_launch_shape(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, B, c->cus, &l)) {
        FwdArgs<double> f = fp.args;
        f.x = x; f.details = details; f.approx = approx;
        f.bad = c->bad;
        copy_bank(f.lo, f.hi, fk, f.taps, f.taps_hi);
        PairArgs<double> a;
        pair_args(f, ik, ip, &a);
        {
          LaunchTimer lt(c, "roundtrip");
          hipError_t e = launch_roundtrip(a, l, c->stream);
          if (e != hipSuccess) return fail(VW_ERR_DEVICE, "round-trip launch failed: %s", hipGetErrorString(e));
        }
        if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
        return ok();
      }
      (void)hipGetLastError();
    }
  }
  // the two calls, with their own argument checks
  VW_TRY(modwt_forward<double>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, details, approx));
  return modwt_inverse<double>(c, details, approx, B, N, rlo, rhi, L, wid, boundary, J, ~0u, 0, flags, y);
}

// The round-trip launch for rows of N samples on this context: the variant VW_PAIR_KEEP and the occupancies choose
// (kept detail planes) and its resident workgroups per CU; both 0 where the shape is not eligible.
static vw_status roundtrip_variant(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* keep, int* per_cu) {
  *keep = *per_cu = 0;
  if (N <= 0 || N > (1LL << 30) || L < 1 || L > kPairMaxTaps || J < 1 || J > kMaxLevels) return ok();
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (c->capturing) return fail(VW_ERR_STATE, "occupancy queries cannot be captured");
  hipSetDevice(c->device);
  // the planner reads a pointer's alignment and nothing behind it
  double* const aligned = reinterpret_cast<double*>(uintptr_t(4096));
  static const double taps[kPairMaxTaps] = {0};
  FwdCall<double> fk;
  fk.x = aligned; fk.details = aligned; fk.approx = aligned;
  fk.B = 4LL * c->cus; fk.N = N; fk.ldx = N; fk.lo = taps; fk.hi = taps; fk.L = L; fk.J = J;
  fk.flags = flags & VW_FLAG_FMA; fk.cus = c->cus;
  FwdPlan<double> fp;
  plan_forward(c->tune, fk, &fp);
  if (fp.error != VW_OK || !pair_forward_shape(fp)) return ok();
  if (pair_prepare(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, per_cu, keep) != hipSuccess) {
    (void)hipGetLastError();
    *keep = *per_cu = 0;
  }
  return ok();
}

extern "C" vw_status vw_roundtrip_occupancy(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* per_cu) {
  if (!c || !per_cu) return fail(VW_ERR_NULL, "null argument");
  int keep;
  return roundtrip_variant(c, N, L, J, flags, &keep, per_cu);
}

extern "C" vw_status vw_roundtrip_variant(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* keep, int* per_cu) {
  if (!c || !keep || !per_cu) return fail(VW_ERR_NULL, "null argument");
  return roundtrip_variant(c, N, L, J, flags, keep, per_cu);
}

// Biorthogonal banks (BiorthogonalSpline / ReverseBiorthogonalSpline): lo has Llo taps, hi has Lhi.  Equal
// lengths are the calls above, argument for argument.
static int bank_hi(int Llo, int Lhi) { return Lhi == Llo ? 0 : Lhi; }
static vw_status bank_arg(int Lhi) {
  if (Lhi < 1 || Lhi > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", Lhi, kMaxTaps);
  return VW_OK;
}
extern "C" vw_status vw_modwt_forward_bi_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                             const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned flags, double* details, double* approx) {
  VW_TRY(bank_arg(Lhi));
  return modwt_forward<double>(c, x, B, N, ldx, lo, hi, Llo, wid, boundary, J, flags, details, approx, bank_hi(Llo, Lhi));
}
extern "C" vw_status vw_modwt_forward_bi_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx,
                                             const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned flags, float* details, float* approx) {
  VW_TRY(bank_arg(Lhi));
  return modwt_forward<float>(c, x, B, N, ldx, lo, hi, Llo, wid, boundary, J, flags, details, approx, bank_hi(Llo, Lhi));
}
extern "C" vw_status vw_modwt_inverse_bi_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                             int64_t N, const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned detail_mask, int approx_zero,
                                             unsigned flags, double* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt_inverse<double>(c, details, approx, B, N, lo, hi, Llo, wid, boundary, J, detail_mask, approx_zero,
                               flags, y, bank_hi(Llo, Lhi));
}
extern "C" vw_status vw_modwt_inverse_bi_f32(vw_ctx* c, const float* details, const float* approx, int64_t B,
                                             int64_t N, const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned detail_mask, int approx_zero,
                                             unsigned flags, float* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt_inverse<float>(c, details, approx, B, N, lo, hi, Llo, wid, boundary, J, detail_mask, approx_zero,
                              flags, y, bank_hi(Llo, Lhi));
}

// ------------------------------------------------------------------------------------------------
// One batch over several contexts, one host thread per context ("each device has its
// own context, stream, input generator and output buffers; one host thread per device").  The
// reference parallelises one call in-process too (VectorWaveSwtAdapter.java:210-267 executor,
// BatchMODWT.multiLevelAoS :90-111 over a batch); here the batch is split into contiguous row
// blocks (vectorwave_amd/shard.py shard_rows: the first B % n blocks get one extra row) and block k
// runs on ctxs[k] from its own std::thread -- no exchange between devices.  Host memory only (the
// JNI / FFM caller's arrays): each thread stages its block through its context.
static void shard_block(int64_t B, int n, int k, int64_t* start, int64_t* rows) {
  const int64_t base = B / n, extra = B % n;
  *start = k * base + std::min<int64_t>(k, extra);
  *rows = base + (k < extra ? 1 : 0);
}

// fn(k) on context k, one host thread per context (k = 0 on the calling thread); the first failing
// context's status, its message prefixed with `what` k.
template <typename F>
static vw_status run_per_ctx(vw_ctx* const* ctxs, int nctx, const char* what, F&& fn) {
  if (!ctxs) return fail(VW_ERR_NULL, "ctxs is null");
  if (nctx < 1) return fail(VW_ERR_ARG, "need at least one context (got %d)", nctx);
  for (int k = 0; k < nctx; ++k)
    if (!ctxs[k]) return fail(VW_ERR_NULL, "ctxs[%d] is null", k);
  struct Res { vw_status st = VW_OK; std::string msg; int64_t idx = -1; };
  std::vector<Res> res(nctx);
  auto work = [&](int k) {
    const vw_status st = fn(k);
    res[k].st = st;
    if (st != VW_OK) { res[k].msg = t_err; res[k].idx = t_err_index; }
  };
  std::vector<std::thread> th;
  th.reserve(nctx);
  for (int k = 1; k < nctx; ++k) th.emplace_back(work, k);
  work(0);
  for (auto& t : th) t.join();
  for (int k = 0; k < nctx; ++k)
    if (res[k].st != VW_OK) {
      t_err = std::string(what) + " " + std::to_string(k) + ": " + res[k].msg;
      t_err_index = res[k].idx;
      return res[k].st;
    }
  return ok();
}

template <typename F>
static vw_status run_sharded(vw_ctx* const* ctxs, int nctx, int64_t B, F&& fn) {
  if (!ctxs) return fail(VW_ERR_NULL, "ctxs is null");
  if (nctx < 1) return fail(VW_ERR_ARG, "need at least one context (got %d)", nctx);
  for (int k = 0; k < nctx; ++k)
    if (!ctxs[k]) return fail(VW_ERR_NULL, "ctxs[%d] is null", k);
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  const int used = (int)std::min<int64_t>(nctx, B);
  struct Res { vw_status st = VW_OK; std::string msg; int64_t idx = -1; };
  std::vector<Res> res(used);
  auto work = [&](int k) {
    int64_t start, rows;
    shard_block(B, used, k, &start, &rows);
    t_signal_base = start;  // signal numbers in this thread's error messages count from row 0 of the batch
    const vw_status st = fn(ctxs[k], start, rows);
    t_signal_base = 0;
    res[k].st = st;
    if (st != VW_OK) { res[k].msg = t_err; res[k].idx = t_err_index; }
  };
  std::vector<std::thread> th;
  th.reserve(used);
  for (int k = 1; k < used; ++k) th.emplace_back(work, k);
  work(0);
  for (auto& t : th) t.join();
  for (int k = 0; k < used; ++k)
    if (res[k].st != VW_OK) {
      int64_t start, rows;
      shard_block(B, used, k, &start, &rows);
      t_err = "block " + std::to_string(k) + " (rows " + std::to_string(start) + ".." +
              std::to_string(start + rows - 1) + "): " + res[k].msg;
      t_err_index = res[k].idx;
      return res[k].st;
    }
  return ok();
}

extern "C" vw_status vw_modwt_forward_multi_f64(vw_ctx* const* ctxs, int nctx, const double* x, int64_t B, int64_t N,
                                                int64_t ldx, const double* lo, const double* hi, int L, int wid,
                                                int boundary, int J, unsigned flags, double* details,
                                                double* approx) {
  if (!(flags & VW_FLAG_HOST_MEMORY)) return fail(VW_ERR_ARG, "multi-context calls take host memory (VW_FLAG_HOST_MEMORY)");
  if (!x || !details || !approx || !lo || !hi) return fail(VW_ERR_NULL, "null array argument");
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  return run_sharded(ctxs, nctx, B, [&](vw_ctx* c, int64_t start, int64_t rows) -> vw_status {
    (void)wid;
    VW_TRY(check_common(c, x, details, lo, hi, rows, N, L, boundary));
    VW_TRY(check_levels(N, L, J, flags));
    std::lock_guard<std::recursive_mutex> g(c->mu);
    hipSetDevice(c->device);
    return forward_host<double>(c, x + start * ldx, rows, N, ldx, lo, hi, L, boundary, J, flags,
                                details + start * N, B * N, approx + start * N);
  });
}

extern "C" vw_status vw_modwt_inverse_multi_f64(vw_ctx* const* ctxs, int nctx, const double* details,
                                                const double* approx, int64_t B, int64_t N, const double* lo,
                                                const double* hi, int L, int wid, int boundary, int J,
                                                unsigned detail_mask, int approx_zero, unsigned flags, double* y) {
  if (!(flags & VW_FLAG_HOST_MEMORY)) return fail(VW_ERR_ARG, "multi-context calls take host memory (VW_FLAG_HOST_MEMORY)");
  if (!y || !lo || !hi) return fail(VW_ERR_NULL, "null argument");
  if (!details && detail_mask) return fail(VW_ERR_NULL, "details is null");
  if (!approx && !approx_zero) return fail(VW_ERR_NULL, "approx is null");
  if (J < 1 || J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels must be in 1..%d", kMaxLevels);
  if ((flags & VW_FLAG_CORE_LEVELS) && vw_upsampled_length(L, J) > N)
    return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  return run_sharded(ctxs, nctx, B, [&](vw_ctx* c, int64_t start, int64_t rows) -> vw_status {
    VW_TRY(check_common(c, y, y, lo, hi, rows, N, L, boundary));
    std::lock_guard<std::recursive_mutex> g(c->mu);
    hipSetDevice(c->device);
    return inverse_host<double>(c, details ? details + start * N : nullptr, B * N,
                                approx ? approx + start * N : nullptr, rows, N, lo, hi, L, wid, boundary, J,
                                detail_mask, approx_zero, flags, y + start * N);
  });
}

extern "C" vw_status vw_modwt_forward_multi_dev_f64(vw_ctx* const* ctxs, int nctx, const double* const* x,
                                                    const int64_t* rows, int64_t N, int64_t ldx, const double* lo,
                                                    const double* hi, int L, int wid, int boundary, int J,
                                                    unsigned flags, double* const* details,
                                                    double* const* approx) {
  if (flags & VW_FLAG_HOST_MEMORY)
    return fail(VW_ERR_ARG, "device-resident multi-context calls take device memory (no VW_FLAG_HOST_MEMORY)");
  if (!x || !rows || !details || !approx) return fail(VW_ERR_NULL, "null array argument");
  return run_per_ctx(ctxs, nctx, "context", [&](int k) -> vw_status {
    if (rows[k] == 0) return VW_OK;
    return modwt_forward<double>(ctxs[k], x[k], rows[k], N, ldx, lo, hi, L, wid, boundary, J, flags, details[k],
                                 approx[k]);
  });
}

extern "C" vw_status vw_modwt_inverse_multi_dev_f64(vw_ctx* const* ctxs, int nctx, const double* const* details,
                                                    const double* const* approx, const int64_t* rows, int64_t N,
                                                    const double* lo, const double* hi, int L, int wid,
                                                    int boundary, int J, unsigned detail_mask, int approx_zero,
                                                    unsigned flags, double* const* y) {
  if (flags & VW_FLAG_HOST_MEMORY)
    return fail(VW_ERR_ARG, "device-resident multi-context calls take device memory (no VW_FLAG_HOST_MEMORY)");
  if (!rows || !y || (!details && detail_mask) || (!approx && !approx_zero))
    return fail(VW_ERR_NULL, "null array argument");
  return run_per_ctx(ctxs, nctx, "context", [&](int k) -> vw_status {
    if (rows[k] == 0) return VW_OK;
    return modwt_inverse<double>(ctxs[k], details ? details[k] : nullptr, approx ? approx[k] : nullptr, rows[k], N,
                                 lo, hi, L, wid, boundary, J, detail_mask, approx_zero, flags, y[k]);
  });
}

// ------------------------------------------------------------------------------------------------
// Single level (MODWTTransform): any N >= 1 (no L <= N guard), pairwise inverse sums.
// Lhi: the high-pass length of a two-length bank (0 = L)
static vw_status modwt1_forward(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                const double* hi, int L, int Lhi, int boundary, unsigned flags, double* approx,
                                double* detail) {
  VW_TRY(check_common(c, x, detail, lo, hi, B, N, L, boundary));
  if (!approx) return fail(VW_ERR_NULL, "approx is null");
  if (ldx < N) return fail(VW_ERR_ARG, "ldx < N");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const bool haar_quirk = (flags & VW_FLAG_BATCH_HAAR) && L == 2 && Lhi == 0 && boundary == VW_PERIODIC;
  auto run = [&](const double* dx, double* da, double* dd, unsigned fl) -> vw_status {
    if (haar_quirk) {
      LaunchTimer lt(c, "forward1");
      hipError_t e = launch_single_haar_batch<double>(dx, ldx, B, (int)N, da, dd, c->stream);
      if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
      return VW_OK;
    }
    FwdCall<double> fk;
    fk.x = dx; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = 1;
    fk.flags = fl & ~VW_FLAG_FFT_SWITCH; fk.details = dd; fk.approx = da; fk.single_level = true; fk.Lhi = Lhi;
    return forward_impl<double>(c, fk);
  };
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dx, *da, *dd;
    VW_TRY(s.in(x, (size_t)B * ldx, &dx));
    VW_TRY(s.in<double>(nullptr, (size_t)B * N, &da));
    VW_TRY(s.in<double>(nullptr, (size_t)B * N, &dd));
    VW_TRY(run(dx, da, dd, flags & ~VW_FLAG_SYNC));
    VW_TRY(s.out(approx, da, (size_t)B * N));
    VW_TRY(s.out(detail, dd, (size_t)B * N));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(run(x, approx, detail, flags));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" vw_status vw_modwt1_forward_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                           const double* lo, const double* hi, int L, int boundary, unsigned flags,
                                           double* approx, double* detail) {
  return modwt1_forward(c, x, B, N, ldx, lo, hi, L, 0, boundary, flags, approx, detail);
}
extern "C" vw_status vw_modwt1_forward_bi_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                              const double* lo, int Llo, const double* hi, int Lhi, int boundary,
                                              unsigned flags, double* approx, double* detail) {
  VW_TRY(bank_arg(Lhi));
  return modwt1_forward(c, x, B, N, ldx, lo, hi, Llo, bank_hi(Llo, Lhi), boundary, flags, approx, detail);
}

static vw_status modwt1_inverse(vw_ctx* c, const double* approx, const double* detail, int64_t B, int64_t N,
                                const double* lo, const double* hi, int L, int Lhi, int boundary, unsigned flags,
                                double* y) {
  VW_TRY(check_common(c, approx, detail, lo, hi, B, N, L, boundary));
  if (!y) return fail(VW_ERR_NULL, "y is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *da, *dd, *dy;
    VW_TRY(s.in(approx, (size_t)B * N, &da));
    VW_TRY(s.in(detail, (size_t)B * N, &dd));
    VW_TRY(s.in<double>(nullptr, (size_t)B * N, &dy));
    InvCall<double> ik;
    ik.details = dd; ik.approx = da; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.boundary = boundary;
    ik.J = 1; ik.detail_mask = 1u; ik.flags = flags & ~VW_FLAG_SYNC; ik.y = dy; ik.single_level = true; ik.Lhi = Lhi;
    VW_TRY(inverse_impl<double>(c, ik));
    VW_TRY(s.out(y, dy, (size_t)B * N));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  InvCall<double> ik;
  ik.details = detail; ik.approx = approx; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L;
  ik.boundary = boundary; ik.J = 1; ik.detail_mask = 1u; ik.flags = flags; ik.y = y; ik.single_level = true;
  ik.Lhi = Lhi;
  VW_TRY(inverse_impl<double>(c, ik));
  return ok();
}

extern "C" vw_status vw_modwt1_inverse_f64(vw_ctx* c, const double* approx, const double* detail, int64_t B,
                                           int64_t N, const double* lo, const double* hi, int L, int boundary,
                                           unsigned flags, double* y) {
  return modwt1_inverse(c, approx, detail, B, N, lo, hi, L, 0, boundary, flags, y);
}
extern "C" vw_status vw_modwt1_inverse_bi_f64(vw_ctx* c, const double* approx, const double* detail, int64_t B,
                                              int64_t N, const double* lo, int Llo, const double* hi, int Lhi,
                                              int boundary, unsigned flags, double* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt1_inverse(c, approx, detail, B, N, lo, hi, Llo, bank_hi(Llo, Lhi), boundary, flags, y);
}

// ------------------------------------------------------------------------------------------------
// com.morphiqlabs.financial (vw_fin.hip): FinancialAnalyzer's four metrics and FinancialWaveletAnalyzer's
// Sharpe ratios, one workgroup per row, one launch per call (the non-periodic wavelet Sharpe composes the
// single-level forward and inverse in ws2 first).

static vw_status fin_common(vw_ctx* c, const void* in, const void* out, int64_t B, unsigned flags) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!in || !out) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (flags & VW_FLAG_FMA)
    return fail(VW_ERR_ARG, "VW_FLAG_FMA is not supported by the financial calls (fused taps change the detail signs)");
  return VW_OK;
}

static vw_status fin_taps(const double* lo, const double* hi, int L, FinArgs* a) {
  if (!lo || !hi) return fail(VW_ERR_NULL, "null filter argument");
  if (L < 1 || L > kFinMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", L, kFinMaxTaps);
  const double s = 1.0 / std::sqrt(2.0);  // as copy_taps
  for (int i = 0; i < kFinMaxTaps; ++i) {
    a->lo[i] = i < L ? lo[i] * s : 0.0;
    a->hi[i] = i < L ? hi[i] * s : 0.0;
  }
  a->L = L;
  return VW_OK;
}

// the kernel's validation word -> status.  Bit 62: a return that overflowed between two finite prices
// (the reference's transform.forward rejects it); clear: a non-finite input element.
static vw_status fin_report(unsigned long long bad, int64_t N, bool prices) {
  if (bad == ~0ull) return VW_OK;
  const bool overflow = (bad >> 62) & 1ull;
  const unsigned long long flat = bad & ((1ull << 62) - 1);
  const long long i = (long long)(flat % (unsigned long long)N);
  const long long b = (long long)(flat / (unsigned long long)N) + (long long)t_signal_base;
  vw_status st;
  if (prices && !overflow)
    st = fail(VW_ERR_ARG, "Prices must contain only finite values (index %lld, signal %lld)", i, b);
  else
    st = fail(VW_ERR_NONFINITE, "%s contains non-finite value at index %lld (signal %lld)",
              prices ? "returns" : "signal", i, b);
  t_err_index = (int64_t)(b * (long long)N + i);
  return st;
}

static vw_status fin_launch(vw_ctx* c, const FinArgs& a, bool analyze, unsigned flags) {
  if (a.validate) VW_HIP(hipMemsetAsync(c->bad, 0xFF, sizeof(unsigned long long), c->stream));
  {
    LaunchTimer lt(c, "fin");
    hipError_t e = analyze ? launch_fin_analyze(a, c->stream) : launch_fin_sharpe(a, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  }
  if (a.validate) {
    unsigned long long bad = ~0ull;
    VW_TRY(read_bad(c, &bad));
    VW_TRY(fin_report(bad, a.N, analyze));
  }
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

extern "C" vw_status vw_fin_analyze_f64(vw_ctx* c, const double* prices, int64_t B, int64_t N, int64_t ld,
                                        const double* lo, const double* hi, int L, double anomaly_k, unsigned flags,
                                        double* out) {
  VW_TRY(fin_common(c, prices, out, B, flags));
  FinArgs a{};
  VW_TRY(fin_taps(lo, hi, L, &a));
  if (N < 2) return fail(VW_ERR_ARG, "Prices must contain at least 2 elements");
  if (ld < N) return fail(VW_ERR_ARG, "ld (%lld) < N (%lld)", (long long)ld, (long long)N);
  if (N - 1 > kFinMaxN)
    return fail(VW_ERR_UNSUPPORTED, "financial analysis keeps a row's coefficients in LDS: at most %d returns per row",
                kFinMaxN);
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(capture_guard(c, flags));
  a.B = B; a.N = (int)N; a.ld = ld; a.k = anomaly_k;
  a.tree = (flags & VW_FLAG_TREE_SUMS) ? 1 : 0;
  a.validate = (flags & VW_FLAG_VALIDATE) ? 1 : 0;
  a.bad = c->bad;
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dp, *dout;
    VW_TRY(s.in(prices, (size_t)(B - 1) * ld + N, &dp));
    VW_TRY(s.in<double>(nullptr, (size_t)5 * B, &dout));
    a.x = dp; a.out = dout;
    VW_TRY(fin_launch(c, a, true, 0));
    VW_TRY(s.out(out, dout, (size_t)5 * B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  a.x = prices; a.out = out;
  VW_TRY(fin_launch(c, a, true, flags));
  return ok();
}

static const char* const kSingleReturnMsg =
    "Cannot calculate Sharpe ratio with a single return value. "
    "At least 2 returns are required to calculate standard deviation (risk).";

static vw_status fin_sharpe_checks(int64_t N, int64_t ld) {
  if (N <= 0) return fail(VW_ERR_EMPTY, "Returns array cannot be empty");
  if (N == 1) return fail(VW_ERR_ARG, "%s", kSingleReturnMsg);
  if (ld < N) return fail(VW_ERR_ARG, "ld (%lld) < N (%lld)", (long long)ld, (long long)N);
  if (N > kFinMaxN)
    return fail(VW_ERR_UNSUPPORTED, "the Sharpe calls keep a row in LDS: at most %d returns per row", kFinMaxN);
  return VW_OK;
}

extern "C" vw_status vw_fin_sharpe_f64(vw_ctx* c, const double* returns, int64_t B, int64_t N, int64_t ld,
                                       double risk_free, unsigned flags, double* out) {
  VW_TRY(fin_common(c, returns, out, B, flags));
  VW_TRY(fin_sharpe_checks(N, ld));
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(capture_guard(c, flags));
  FinArgs a{};
  a.B = B; a.N = (int)N; a.ld = ld; a.k = risk_free;
  a.tree = (flags & VW_FLAG_TREE_SUMS) ? 1 : 0;
  a.bad = c->bad;  // (the reference's plain Sharpe ratio does not validate: VW_FLAG_VALIDATE checks nothing here)
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dr, *dout;
    VW_TRY(s.in(returns, (size_t)(B - 1) * ld + N, &dr));
    VW_TRY(s.in<double>(nullptr, (size_t)B, &dout));
    a.x = dr; a.out = dout;
    VW_TRY(fin_launch(c, a, false, 0));
    VW_TRY(s.out(out, dout, (size_t)B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  a.x = returns; a.out = out;
  VW_TRY(fin_launch(c, a, false, flags));
  return ok();
}

// device pointers in, device pointer out
static vw_status wavelet_sharpe_device(vw_ctx* c, FinArgs a, const double* lo, const double* hi, int boundary,
                                       unsigned flags) {
  if (boundary == VW_PERIODIC) {
    a.wavelet = 1;
    a.validate = (flags & VW_FLAG_VALIDATE) ? 1 : 0;
    return fin_launch(c, a, false, flags);
  }
  // ZERO_PADDING / SYMMETRIC: the existing single-level kernels, planes approx | detail | y in ws2
  const size_t plane = (size_t)a.B * (size_t)a.N;
  const size_t bytes = 3 * plane * sizeof(double);
  if (bytes > c->ws2_bytes) {
    if (c->capturing) return fail(VW_ERR_STATE, "workspace growth during capture: run the call once before capturing it");
    if (c->ws2) {
      hipDeviceSynchronize();
      ++c->ws_gen;
      hipFree(c->ws2);
      c->ws2 = nullptr;
      c->ws2_bytes = 0;
    }
    VW_HIP(hipMalloc(&c->ws2, bytes));
    c->ws2_bytes = bytes;
  }
  double* da = reinterpret_cast<double*>(c->ws2);
  double* dd = da + plane;
  double* dy = dd + plane;
  const unsigned tf = flags & (VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE);
  FwdCall<double> fk;
  fk.x = a.x; fk.B = a.B; fk.N = a.N; fk.ldx = a.ld; fk.lo = lo; fk.hi = hi; fk.L = a.L; fk.boundary = boundary;
  fk.J = 1; fk.flags = tf; fk.details = dd; fk.approx = da; fk.single_level = true;
  VW_TRY(forward_impl<double>(c, fk));
  VW_HIP(hipMemsetAsync(dd, 0, plane * sizeof(double), c->stream));  // `new double[detailCoeffs.length]`
  InvCall<double> ik;
  ik.details = dd; ik.approx = da; ik.B = a.B; ik.N = a.N; ik.lo = lo; ik.hi = hi; ik.L = a.L;
  ik.boundary = boundary; ik.J = 1; ik.detail_mask = 1u; ik.flags = tf & ~VW_FLAG_VALIDATE; ik.y = dy;
  ik.single_level = true;
  VW_TRY(inverse_impl<double>(c, ik));
  a.x = dy;
  a.ld = a.N;
  return fin_launch(c, a, false, flags);
}

extern "C" vw_status vw_fin_wavelet_sharpe_f64(vw_ctx* c, const double* returns, int64_t B, int64_t N, int64_t ld,
                                               const double* lo, const double* hi, int L, int boundary,
                                               double risk_free, unsigned flags, double* out) {
  VW_TRY(fin_common(c, returns, out, B, flags));
  FinArgs a{};
  VW_TRY(fin_taps(lo, hi, L, &a));
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING)
    return fail(VW_ERR_BOUNDARY, "MODWT only supports PERIODIC, ZERO_PADDING, and SYMMETRIC boundary modes");
  VW_TRY(fin_sharpe_checks(N, ld));
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(capture_guard(c, flags));
  a.B = B; a.N = (int)N; a.ld = ld; a.k = risk_free;
  a.tree = (flags & VW_FLAG_TREE_SUMS) ? 1 : 0;
  a.bad = c->bad;
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dr, *dout;
    VW_TRY(s.in(returns, (size_t)(B - 1) * ld + N, &dr));
    VW_TRY(s.in<double>(nullptr, (size_t)B, &dout));
    a.x = dr; a.out = dout;
    VW_TRY(wavelet_sharpe_device(c, a, lo, hi, boundary, flags & ~(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY)));
    VW_TRY(s.out(out, dout, (size_t)B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  a.x = returns; a.out = out;
  VW_TRY(wavelet_sharpe_device(c, a, lo, hi, boundary, flags));
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Wavelet energy per level (vw_energy.hip): MultiLevelMODWTResultImpl.getApproximationEnergy /
// getDetailEnergyAtLevel (:91-117, computeEnergy :211-216) per signal, out [J+1][B].
// Timing families: "energy_fused" (k_energy_fused), "energy_chain" (sequential plane sums), "energy_tree".

static vw_status ensure_ws2(vw_ctx* c, size_t bytes) {
  if (bytes <= c->ws2_bytes) return VW_OK;
  if (c->capturing) return fail(VW_ERR_STATE, "workspace growth during capture: run the call once before capturing it");
  if (c->ws2) {
    hipDeviceSynchronize();
    ++c->ws_gen;
    hipFree(c->ws2);
    c->ws2 = nullptr;
    c->ws2_bytes = 0;
  }
  VW_HIP(hipMalloc(&c->ws2, bytes));
  c->ws2_bytes = bytes;
  return VW_OK;
}

// device pointers in, device pointer out
static vw_status energy_planes_device(vw_ctx* c, const double* details, const double* approx, int64_t B, int64_t N,
                                      int J, unsigned flags, double* out) {
  EnergyPlanesArgs a{};
  a.approx = approx; a.details = details; a.B = B; a.N = (int)N; a.J = J; a.out = out;
  a.vec_io = (N % 2 == 0) && ((uintptr_t)approx & 15u) == 0 && ((uintptr_t)details & 15u) == 0;
  const bool tree = flags & VW_FLAG_TREE_SUMS;
  LaunchTimer lt(c, tree ? "energy_tree" : "energy_chain");
  hipError_t e = launch_energy_planes(a, tree, c->cus, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "energy launch failed: %s", hipGetErrorString(e));
  return VW_OK;
}

// device pointers in, device pointer out; arguments checked by the caller
static vw_status energy_device(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                               const double* hi, int L, int boundary, int J, unsigned flags, double* out) {
  VW_TRY(capture_guard(c, flags));
  FwdCall<double> fk;
  fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
  fk.flags = flags; fk.cus = c->cus;
  EnergyPlan p;
  plan_energy(c->tune, fk, &p);
  if (p.fused) {
    EnergyArgs a = p.args;
    a.x = x; a.out = out;
    copy_taps(a.lo, lo, L);
    copy_taps(a.hi, hi, L);
    LaunchTimer lt(c, "energy_fused");
    hipError_t e = launch_energy_fused(a, p.threads, p.lds, p.fma, p.nv, p.grid, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "energy launch failed: %s", hipGetErrorString(e));
  } else {
    // the forward's own plan and executor into the workspace (approx [B][N] | details [J][B][N]), then the plane sums
    const size_t plane = (size_t)B * (size_t)N;
    VW_TRY(ensure_ws2(c, ((size_t)J + 1) * plane * sizeof(double)));
    double* app = reinterpret_cast<double*>(c->ws2);
    double* det = app + plane;
    fk.flags = flags & ~(unsigned)VW_FLAG_SYNC; fk.details = det; fk.approx = app;
    VW_TRY(forward_impl<double>(c, fk));
    VW_TRY(energy_planes_device(c, det, app, B, N, J, flags, out));
  }
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

extern "C" vw_status vw_modwt_energy_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                         const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                         unsigned flags, double* out) {
  (void)wid;
  // vw_modwt_forward_f64's checks, in its order
  VW_TRY(check_common(c, x, out, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  VW_TRY(check_levels(N, L, J, flags));
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    if (c->capturing) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
    Staging s(c);
    double *dx, *dout;
    VW_TRY(s.in(x, (size_t)(B - 1) * ldx + N, &dx));  // (the last row's padding need not exist)
    VW_TRY(s.in<double>(nullptr, ((size_t)J + 1) * B, &dout));
    VW_TRY(energy_device(c, dx, B, N, ldx, lo, hi, L, boundary, J, flags & ~(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY), dout));
    VW_TRY(s.out(out, dout, ((size_t)J + 1) * B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(energy_device(c, x, B, N, ldx, lo, hi, L, boundary, J, flags, out));
  return ok();
}

extern "C" vw_status vw_energy_planes_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                          int64_t N, int J, unsigned flags, double* out) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!approx || !out || (!details && J > 0)) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (J < 0 || J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels must be in 0..%d", kMaxLevels);
  if (flags & ~(unsigned)(VW_FLAG_TREE_SUMS | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC))
    return fail(VW_ERR_ARG, "vw_energy_planes_f64 takes TREE_SUMS, HOST_MEMORY and SYNC only");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(capture_guard(c, flags));
  const size_t plane = (size_t)B * (size_t)N;
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *da, *dd = nullptr, *dout;
    VW_TRY(s.in(approx, plane, &da));
    if (J > 0) VW_TRY(s.in(details, (size_t)J * plane, &dd));
    VW_TRY(s.in<double>(nullptr, ((size_t)J + 1) * B, &dout));
    VW_TRY(energy_planes_device(c, dd, da, B, N, J, flags, dout));
    VW_TRY(s.out(out, dout, ((size_t)J + 1) * B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(energy_planes_device(c, details, approx, B, N, J, flags, out));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Multiresolution analysis (vw_mra.hip): out[c] = the inverse with detail_mask = c ? 1 << (c-1) : 0 and
// approx_zero = (c != 0) (VectorWaveSwtAdapter.extractLevel :576-598), every c in one call.
// Timing families: "mra" (k_mra); the loop path's launches count as "inverse" / "inverse_level".

// device pointers; k.y = out [J+1][B][N]; arguments checked by the caller
template <typename T>
static vw_status mra_planes_device(vw_ctx* c, InvCall<T> k) {
  VW_TRY(capture_guard(c, k.flags));
  k.cus = c->cus;
  MraPlan<T> p;
  plan_mra(c->tune, k, &p);
  if (p.fused) {
    MraArgs<T> a = p.args;
    a.details = k.details; a.approx = k.approx; a.out = k.y;
    copy_taps(a.lo, k.lo, k.L);
    copy_taps(a.hi, k.hi, k.L);
    LaunchTimer lt(c, "mra");
    hipError_t e = launch_mra<T>(a, p.threads, p.lds, p.fma, p.nv, p.grid, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "mra launch failed: %s", hipGetErrorString(e));
  } else {
    // the loop path: the J+1 masked inverses, each through its own plan
    const size_t plane = (size_t)k.B * (size_t)k.N;
    for (int comp = 0; comp <= k.J; ++comp) {
      InvCall<T> ik = k;
      ik.detail_mask = comp ? 1u << (comp - 1) : 0u;
      ik.approx_zero = comp != 0;
      ik.flags = k.flags & ~(unsigned)VW_FLAG_SYNC;
      ik.y = k.y + (size_t)comp * plane;
      VW_TRY(inverse_impl<T>(c, ik));
    }
  }
  if (k.flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

template <typename T>
static vw_status mra_planes(vw_ctx* c, const T* details, const T* approx, int64_t B, int64_t N, const double* lo,
                            const double* hi, int L, int wid, int boundary, int J, unsigned flags, T* out) {
  VW_TRY(check_inverse(c, details, approx, out, lo, hi, B, N, L, boundary, J, ~0u, 0, flags));
  if (flags & ~(unsigned)(VW_FLAG_CORE_LEVELS | VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC | VW_FLAG_VALIDATE |
                          VW_FLAG_REF_NONFINITE))
    return fail(VW_ERR_ARG, "vw_mra_planes takes CORE_LEVELS, FMA, HOST_MEMORY, SYNC, VALIDATE and REF_NONFINITE only");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  InvCall<T> ik;
  ik.details = details; ik.approx = approx; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.wid = wid;
  ik.boundary = boundary; ik.J = J; ik.flags = flags; ik.y = out;
  if (flags & VW_FLAG_HOST_MEMORY) {
    if (c->capturing) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
    const size_t plane = (size_t)B * (size_t)N;
    Staging s(c);
    T *dd, *da, *dout;
    VW_TRY(s.in(details, (size_t)J * plane, &dd));
    VW_TRY(s.in(approx, plane, &da));
    VW_TRY(s.in<T>(nullptr, ((size_t)J + 1) * plane, &dout));
    ik.details = dd; ik.approx = da; ik.y = dout;
    ik.flags = flags & ~(unsigned)(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY);
    VW_TRY(mra_planes_device<T>(c, ik));
    VW_TRY(s.out(out, dout, ((size_t)J + 1) * plane));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(mra_planes_device<T>(c, ik));
  return ok();
}

// device pointers; the forward's own plan and executor into the workspace (approx [B][N] | details [J][B][N]), then
// the planes call on those coefficients
template <typename T>
static vw_status mra_device(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const double* lo, const double* hi,
                            int L, int wid, int boundary, int J, unsigned flags, T* out) {
  VW_TRY(capture_guard(c, flags));
  const size_t plane = (size_t)B * (size_t)N;
  VW_TRY(ensure_ws2(c, ((size_t)J + 1) * plane * sizeof(T)));
  T* app = reinterpret_cast<T*>(c->ws2);
  T* det = app + plane;
  FwdCall<T> fk;
  fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
  fk.flags = flags & ~(unsigned)VW_FLAG_SYNC; fk.details = det; fk.approx = app;
  VW_TRY(forward_impl<T>(c, fk));
  InvCall<T> ik;
  ik.details = det; ik.approx = app; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.wid = wid;
  ik.boundary = boundary; ik.J = J; ik.flags = flags & ~(unsigned)VW_FLAG_FFT_SWITCH; ik.y = out;
  return mra_planes_device<T>(c, ik);
}

template <typename T>
static vw_status modwt_mra(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const double* lo, const double* hi,
                           int L, int wid, int boundary, int J, unsigned flags, T* out) {
  // vw_modwt_forward_*'s checks, in its order, then the inverse's
  VW_TRY(check_common(c, x, out, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  VW_TRY(check_levels(N, L, J, flags));
  VW_TRY(check_inverse(c, x, x, out, lo, hi, B, N, L, boundary, J, ~0u, 0, flags));
  if (flags & ~(unsigned)(VW_FLAG_CORE_LEVELS | VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC | VW_FLAG_VALIDATE |
                          VW_FLAG_REF_NONFINITE | VW_FLAG_FFT_SWITCH))
    return fail(VW_ERR_ARG, "vw_modwt_mra takes CORE_LEVELS, FFT_SWITCH, FMA, HOST_MEMORY, SYNC, VALIDATE and REF_NONFINITE only");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    if (c->capturing) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
    const size_t plane = (size_t)B * (size_t)N;
    Staging s(c);
    T *dx, *dout;
    VW_TRY(s.in(x, (size_t)(B - 1) * ldx + N, &dx));  // (the last row's padding need not exist)
    VW_TRY(s.in<T>(nullptr, ((size_t)J + 1) * plane, &dout));
    VW_TRY(mra_device<T>(c, dx, B, N, ldx, lo, hi, L, wid, boundary, J,
                         flags & ~(unsigned)(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY), dout));
    VW_TRY(s.out(out, dout, ((size_t)J + 1) * plane));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(mra_device<T>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, out));
  return ok();
}

extern "C" vw_status vw_mra_planes_f64(vw_ctx* c, const double* details, const double* approx, int64_t B, int64_t N,
                                       const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                       unsigned flags, double* out) {
  return mra_planes<double>(c, details, approx, B, N, lo, hi, L, wid, boundary, J, flags, out);
}
extern "C" vw_status vw_mra_planes_f32(vw_ctx* c, const float* details, const float* approx, int64_t B, int64_t N,
                                       const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                       unsigned flags, float* out) {
  return mra_planes<float>(c, details, approx, B, N, lo, hi, L, wid, boundary, J, flags, out);
}
extern "C" vw_status vw_modwt_mra_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                      const double* hi, int L, int wid, int boundary, int J, unsigned flags,
                                      double* out) {
  return modwt_mra<double>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, out);
}
extern "C" vw_status vw_modwt_mra_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                      const double* hi, int L, int wid, int boundary, int J, unsigned flags,
                                      float* out) {
  return modwt_mra<float>(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, flags, out);
}

// ------------------------------------------------------------------------------------------------
// Continuous wavelet transform (vw_cwt.hip): fixed-order correlations of each row with one table per scale, plan_cwt's
// launches heaviest scales first.  Timing family: "cwt".

// The call's device image: [CwtScaleDev x S, plan order][taps_re x ntaps][taps_im x ntaps], T-typed, 16-byte aligned
// parts.  Kept in the context: the same image again uploads nothing.  A new one bumps ws_gen (graphs recorded on
// the old tables are stale) and cannot be recorded.
template <typename T>
static vw_status cwt_upload(vw_ctx* c, const CwtPlan& p, const vw_cwt_scale* scales, int S, const double* taps_re,
                            const double* taps_im, int64_t ntaps, const CwtScaleDev<T>** sc, const T** dre,
                            const T** dim) {
  const size_t sc_bytes = align_up((size_t)S * sizeof(CwtScaleDev<T>), 16);
  const size_t tab_bytes = align_up((size_t)ntaps * sizeof(T), 16);
  const size_t bytes = sc_bytes + tab_bytes * (taps_im ? 2 : 1);
  std::vector<unsigned char> img(bytes + 2, 0);
  img[bytes] = (unsigned char)sizeof(T);  // the layout's own parameters close the image
  img[bytes + 1] = taps_im ? 1 : 0;
  CwtScaleDev<T>* hs = reinterpret_cast<CwtScaleDev<T>*>(img.data());
  for (int i = 0; i < S; ++i) {
    const vw_cwt_scale& d = scales[p.order[i].scale];
    CwtScaleDev<T> e;
    std::memset(&e, 0, sizeof(e));  // the image is compared byte for byte, padding included
    e.tap_begin = (int)d.tap_begin; e.taps = d.taps; e.window = d.window_begin; e.scale = p.order[i].scale;
    e.divisor = (T)d.divisor;
    std::memcpy(&hs[i], &e, sizeof(e));
  }
  T* hre = reinterpret_cast<T*>(img.data() + sc_bytes);
  for (int64_t i = 0; i < ntaps; ++i) hre[i] = (T)taps_re[i];
  if (taps_im) {
    T* him = reinterpret_cast<T*>(img.data() + sc_bytes + tab_bytes);
    for (int64_t i = 0; i < ntaps; ++i) him[i] = (T)taps_im[i];
  }
  if (img != c->cwt_img) {
    if (c->capturing) return fail(VW_ERR_STATE, "vw_cwt: new tables cannot be uploaded during a capture (run the call once first)");
    if (c->cwt_dev_bytes < bytes) {
      VW_HIP(hipStreamSynchronize(c->stream));
      if (c->cwt_dev) hipFree(c->cwt_dev);
      c->cwt_dev = nullptr; c->cwt_dev_bytes = 0; c->cwt_img.clear();
      VW_HIP(hipMalloc(&c->cwt_dev, bytes));
      c->cwt_dev_bytes = bytes;
    }
    c->cwt_img.clear();  // (not valid until the copy is enqueued)
    VW_HIP(hipMemcpyAsync(c->cwt_dev, img.data(), bytes, hipMemcpyHostToDevice, c->stream));
    VW_HIP(hipStreamSynchronize(c->stream));  // img is this call's
    c->cwt_img.swap(img);
    ++c->ws_gen;
  }
  const unsigned char* base = static_cast<const unsigned char*>(c->cwt_dev);
  *sc = reinterpret_cast<const CwtScaleDev<T>*>(base);
  *dre = reinterpret_cast<const T*>(base + sc_bytes);
  *dim = taps_im ? reinterpret_cast<const T*>(base + sc_bytes + tab_bytes) : nullptr;
  return VW_OK;
}

template <typename T>
static vw_status cwt_impl(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales, int S,
                          const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                          unsigned flags, T* out_re, T* out_im) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!x || !scales || !taps_re || !out_re || (taps_im && !out_im)) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (S <= 0) return fail(VW_ERR_EMPTY, "Scales cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  if (flags & ~(unsigned)(VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC))
    return fail(VW_ERR_ARG, "vw_cwt takes FMA, HOST_MEMORY and SYNC only");
  if (ext < VW_CWT_ZERO || ext > VW_CWT_WRAP_ZERO) return fail(VW_ERR_ARG, "unknown extension %d", ext);
  if (ext == VW_CWT_WRAP_ZERO && wrap < 1) return fail(VW_ERR_ARG, "VW_CWT_WRAP_ZERO needs wrap >= 1 (wrap=%lld)", (long long)wrap);
  if (ntaps < 1 || ntaps > (1LL << 30)) return fail(VW_ERR_ARG, "ntaps (%lld) outside 1..2^30", (long long)ntaps);
  std::vector<int> K((size_t)S);
  for (int s = 0; s < S; ++s) {
    const vw_cwt_scale& d = scales[s];
    if (d.taps < 1) return fail(VW_ERR_ARG, "scale %d has %d taps", s, (int)d.taps);
    if (d.tap_begin < 0 || d.tap_begin > ntaps - d.taps)
      return fail(VW_ERR_ARG, "scale %d reads taps [%lld, %lld) outside the table of %lld", s, (long long)d.tap_begin,
                  (long long)d.tap_begin + d.taps, (long long)ntaps);
    if (!(d.divisor > 0.0) || !((T)d.divisor > (T)0) || std::isinf((T)d.divisor))
      return fail(VW_ERR_ARG, "scale %d has divisor %g (must be positive and finite)", s, d.divisor);
    if (d.window_begin > (1 << 30) || d.window_begin < -(1 << 30))
      return fail(VW_ERR_ARG, "scale %d has window_begin %d outside +-2^30", s, (int)d.window_begin);
    K[s] = d.taps;
  }
  CwtCall k;
  k.B = B; k.N = N; k.S = S; k.taps = K.data(); k.elem_bytes = (int)sizeof(T); k.cplx = taps_im != nullptr; k.ext = ext;
  k.flags = flags;
  CwtPlan p;
  plan_cwt(k, &p);
  if (p.error != VW_OK) return fail((vw_status)p.error, "%s", p.msg);

  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  VW_TRY(capture_guard(c, flags));
  CwtArgs<T> a{};
  VW_TRY(cwt_upload<T>(c, p, scales, S, taps_re, taps_im, ntaps, &a.sc, &a.taps_re, &a.taps_im));
  const CwtScaleDev<T>* const sc0 = a.sc;
  a.ldx = ldx; a.B = B; a.N = (int)N; a.S = S; a.ntiles = p.ntiles; a.ext = ext; a.wrap = wrap > 0 ? wrap : 1;
  const size_t planes = (size_t)B * (size_t)S * (size_t)N;
  auto launches = [&]() -> vw_status {
    for (const CwtLaunch& l : p.launches) {
      a.sc = sc0 + l.first; a.nsc = l.count;
      LaunchTimer lt(c, "cwt");
      hipError_t e = launch_cwt<T>(a, p.threads, l.lds, p.cplx, p.fma, l.grid, c->stream);
      if (e != hipSuccess) return fail(VW_ERR_DEVICE, "cwt launch failed: %s", hipGetErrorString(e));
    }
    return VW_OK;
  };
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging stg(c);
    T *dx, *dre, *dim = nullptr;
    VW_TRY(stg.in(x, (size_t)(B - 1) * ldx + N, &dx));  // (the last row's padding need not exist)
    VW_TRY(stg.in<T>(nullptr, planes, &dre));
    if (taps_im) VW_TRY(stg.in<T>(nullptr, planes, &dim));
    a.x = dx; a.out_re = dre; a.out_im = dim;
    VW_TRY(launches());
    VW_TRY(stg.out(out_re, dre, planes));
    if (taps_im) VW_TRY(stg.out(out_im, dim, planes));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  a.x = x; a.out_re = out_re; a.out_im = taps_im ? out_im : nullptr;
  VW_TRY(launches());
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" vw_status vw_cwt_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales,
                                int S, const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                                unsigned flags, double* out_re, double* out_im) {
  return cwt_impl<double>(c, x, B, N, ldx, scales, S, taps_re, taps_im, ntaps, ext, wrap, flags, out_re, out_im);
}
extern "C" vw_status vw_cwt_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales,
                                int S, const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                                unsigned flags, float* out_re, float* out_im) {
  return cwt_impl<float>(c, x, B, N, ldx, scales, S, taps_re, taps_im, ntaps, ext, wrap, flags, out_re, out_im);
}

// ------------------------------------------------------------------------------------------------
// SWT denoise: fused forward -> per-signal exact median of |d_1| -> inverse with fused threshold.
extern "C" vw_status vw_noise_sigma_f64(vw_ctx* c, const double* coeffs, int64_t B, int64_t N, unsigned flags,
                                        double* sigma) {
  if (!c || !coeffs || !sigma) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "empty input");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dc, *ds;
    VW_TRY(s.in(coeffs, (size_t)B * N, &dc));
    VW_TRY(s.in<double>(nullptr, (size_t)B, &ds));
    hipError_t e = launch_noise_sigma(dc, N, B, (int)N, 0.0, ds, nullptr, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
    VW_TRY(s.out(sigma, ds, (size_t)B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  hipError_t e = launch_noise_sigma(coeffs, N, B, (int)N, 0.0, sigma, nullptr, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" vw_status vw_threshold_f64(vw_ctx* c, double* coeffs, int64_t B, int64_t N, const double* thr, int soft,
                                      unsigned flags) {
  if (!c || !coeffs || !thr) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "empty input");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dc, *dt;
    VW_TRY(s.in(coeffs, (size_t)B * N, &dc));
    VW_TRY(s.in(thr, (size_t)B, &dt));
    hipError_t e = launch_threshold<double>(dc, B, N, dt, soft, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
    VW_TRY(s.out(coeffs, dc, (size_t)B * N));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  hipError_t e = launch_threshold<double>(coeffs, B, N, thr, soft, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// out[c][r] = in[r][c] (rows x cols).  AoS [B][N] -> SoA [N][B] is (rows=B, cols=N); back is
// (rows=N, cols=B).  BatchSIMDMODWT.convertToSoA / convertFromSoA (BatchSIMDMODWT.java:282-308).
template <typename T>
static vw_status transpose_impl(vw_ctx* c, const T* in, int64_t rows, int64_t cols, unsigned flags, T* out) {
  if (!c || !in || !out) return fail(VW_ERR_NULL, "null argument");
  if (rows <= 0 || cols <= 0) return fail(VW_ERR_EMPTY, "empty input");
  if (in == out) return fail(VW_ERR_ARG, "transpose is out of place");
  if ((rows + 63) / 64 > 65535) return fail(VW_ERR_ARG, "rows %lld too large", (long long)rows);
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t n = (size_t)rows * (size_t)cols;
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    T *di, *dout;
    VW_TRY(s.in(in, n, &di));
    VW_TRY(s.in<T>(nullptr, n, &dout));
    hipError_t e = launch_transpose<T>(di, rows, cols, dout, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
    VW_TRY(s.out(out, dout, n));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  hipError_t e;
  {
    LaunchTimer lt(c, "transpose");
    e = launch_transpose<T>(in, rows, cols, out, c->stream);
  }
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" vw_status vw_transpose_f64(vw_ctx* c, const double* in, int64_t rows, int64_t cols, unsigned flags,
                                      double* out) {
  return transpose_impl<double>(c, in, rows, cols, flags, out);
}

extern "C" vw_status vw_transpose_f32(vw_ctx* c, const float* in, int64_t rows, int64_t cols, unsigned flags,
                                      float* out) {
  return transpose_impl<float>(c, in, rows, cols, flags, out);
}

static vw_status denoise_device(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                const double* hi, int L, int wid, int boundary, int J, double threshold, int soft,
                                unsigned flags, double* y, double* thr_out) {
  const size_t plane = (size_t)B * (size_t)N;
  // workspace: details [J][B][N] | approx [B][N] | thr [B]   (tiled levels use ws beyond, via a 2nd alloc)
  const size_t bytes = align_up(((size_t)J + 1) * plane * sizeof(double), 256) + align_up((size_t)B * 8, 256);
  if (bytes > c->ws2_bytes) {
    if (c->capturing) return fail(VW_ERR_STATE, "workspace growth during capture: run the call once before capturing it");
    if (c->ws2) {
      hipDeviceSynchronize();
      ++c->ws_gen;
      hipFree(c->ws2);
      c->ws2 = nullptr;
      c->ws2_bytes = 0;
    }
    VW_HIP(hipMalloc(&c->ws2, bytes));
    c->ws2_bytes = bytes;
  }
  void* buf = c->ws2;
  double* det = reinterpret_cast<double*>(buf);
  double* app = det + (size_t)J * plane;
  double* thr = reinterpret_cast<double*>(reinterpret_cast<char*>(buf) +
                                          align_up(((size_t)J + 1) * plane * sizeof(double), 256));
  FwdCall<double> fk;
  fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary; fk.J = J;
  fk.flags = flags & ~VW_FLAG_SYNC; fk.details = det; fk.approx = app;
  vw_status st = forward_impl<double>(c, fk);
  if (st == VW_OK) {
    hipError_t e = hipSuccess;
    if (threshold < 0) {
      // T = sigma * Math.sqrt(2 * Math.log(n))  core/swt/VectorWaveSwtAdapter.java:514
      const double scale_c = std::sqrt(2 * std::log((double)N));
      LaunchTimer lt(c, "sigma");
      e = launch_noise_sigma(det, N, B, (int)N, scale_c, nullptr, thr, c->stream);
    } else if (c->capturing) {
      st = fail(VW_ERR_STATE, "a fixed threshold cannot be captured");
    } else {
      std::vector<double> h((size_t)B, threshold);
      e = hipMemcpyAsync(thr, h.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) st = fail(VW_ERR_DEVICE, "threshold stage failed: %s", hipGetErrorString(e));
  }
  if (st == VW_OK) {
    InvCall<double> ik;
    ik.details = det; ik.approx = app; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.wid = wid;
    ik.boundary = boundary; ik.J = J; ik.flags = flags & ~VW_FLAG_SYNC; ik.y = y; ik.thr = thr; ik.soft = soft;
    st = inverse_impl<double>(c, ik);
  }
  if (st == VW_OK && thr_out) {
    hipError_t e = hipMemcpyAsync(thr_out, thr, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) st = fail(VW_ERR_DEVICE, "copy failed");
  }
  return st;
}

extern "C" vw_status vw_swt_denoise_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                        const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                        double threshold, int soft, unsigned flags, double* y,
                                        double* thresholds_out) {
  VW_TRY(check_common(c, x, y, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx < N");
  VW_TRY(check_levels(N, L, J, flags));
  if (vw_upsampled_length(L, J) > N && boundary != VW_PERIODIC)
    return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dx, *dy, *dt = nullptr;
    VW_TRY(s.in(x, (size_t)B * ldx, &dx));
    VW_TRY(s.in<double>(nullptr, (size_t)B * N, &dy));
    if (thresholds_out) VW_TRY(s.in<double>(nullptr, (size_t)B, &dt));
    VW_TRY(denoise_device(c, dx, B, N, ldx, lo, hi, L, wid, boundary, J, threshold, soft, flags, dy, dt));
    VW_TRY(s.out(y, dy, (size_t)B * N));
    if (thresholds_out) VW_TRY(s.out(thresholds_out, dt, (size_t)B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(denoise_device(c, x, B, N, ldx, lo, hi, L, wid, boundary, J, threshold, soft, flags, y, thresholds_out));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// ------------------------------------------------------------------------------------------------
// WaveletDenoiser (core/denoising/WaveletDenoiser.java): forward (single-level MODWTTransform for
// denoise()/denoiseFixed(), MultiLevelMODWTTransform for denoiseMultiLevel()), sigma = MAD of d_1,
// one threshold per (level, signal) by the method (vw_sigma.h), inverse with the per-level threshold
// fused into the detail staging.
static vw_status wavelet_denoise_device(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                        const double* lo, const double* hi, int L, int wid, int boundary, int levels,
                                        int method, double fixed, int soft, unsigned flags, double* y,
                                        double* thr_out) {
  const int J = levels > 0 ? levels : 1;
  const size_t plane = (size_t)B * (size_t)N;
  const size_t coef_bytes = align_up(((size_t)J + 1) * plane * sizeof(double), 256);
  const size_t bytes = coef_bytes + align_up((size_t)B * 8, 256) + align_up((size_t)J * B * 8, 256);
  if (bytes > c->ws2_bytes) {
    if (c->capturing) return fail(VW_ERR_STATE, "workspace growth during capture: run the call once before capturing it");
    if (c->ws2) {
      hipDeviceSynchronize();
      ++c->ws_gen;
      hipFree(c->ws2);
      c->ws2 = nullptr;
      c->ws2_bytes = 0;
    }
    VW_HIP(hipMalloc(&c->ws2, bytes));
    c->ws2_bytes = bytes;
  }
  double* det = reinterpret_cast<double*>(c->ws2);
  double* app = det + (size_t)J * plane;
  double* sig = reinterpret_cast<double*>(reinterpret_cast<char*>(c->ws2) + coef_bytes);
  double* thr = reinterpret_cast<double*>(reinterpret_cast<char*>(sig) + align_up((size_t)B * 8, 256));
  const unsigned fl = flags & ~VW_FLAG_SYNC;
  FwdCall<double> fk;
  fk.x = x; fk.B = B; fk.N = N; fk.ldx = ldx; fk.lo = lo; fk.hi = hi; fk.L = L; fk.boundary = boundary;
  fk.J = levels > 0 ? J : 1; fk.flags = levels > 0 ? fl : fl & ~VW_FLAG_FFT_SWITCH; fk.details = det; fk.approx = app;
  fk.single_level = levels <= 0;
  vw_status st = forward_impl<double>(c, fk);
  if (st != VW_OK) return st;
  hipError_t e = hipSuccess;
  if (method == kThrFixed) {
    if (c->capturing) return fail(VW_ERR_STATE, "a fixed threshold cannot be captured");
    std::vector<double> h((size_t)B, fixed);
    e = hipMemcpyAsync(thr, h.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  } else {
    DenoiseConsts k;
    memset(&k, 0, sizeof(k));
    for (int j = 1; j <= J; ++j) k.level_scale[j - 1] = levels > 0 ? std::sqrt((double)(1 << j)) : 1.0;
    k.univ_c = std::sqrt(2.0 * std::log((double)N));
    k.log_n = std::log((double)N);
    k.method = method;
    k.n = (int)N;
    {
      LaunchTimer lt(c, "sigma");
      e = launch_noise_sigma(det, N, B, (int)N, 0.0, sig, nullptr, c->stream);
    }
    if (e == hipSuccess) {
      LaunchTimer lt(c, "threshold");
      e = launch_level_threshold(det, (long long)plane, sig, k, B, J, thr, c->stream);
    }
  }
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "threshold stage failed: %s", hipGetErrorString(e));
  InvCall<double> ik;
  ik.details = det; ik.approx = app; ik.B = B; ik.N = N; ik.lo = lo; ik.hi = hi; ik.L = L; ik.boundary = boundary;
  ik.flags = fl; ik.y = y; ik.thr = thr; ik.soft = soft;
  if (levels > 0) {
    ik.wid = wid; ik.J = J; ik.thr_ld = B;
  } else {
    ik.J = 1; ik.detail_mask = 1u; ik.single_level = true;
  }
  st = inverse_impl<double>(c, ik);
  if (st == VW_OK && thr_out) {
    e = hipMemcpyAsync(thr_out, thr, (size_t)J * B * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) st = fail(VW_ERR_DEVICE, "copy failed");
  }
  return st;
}

extern "C" vw_status vw_wavelet_denoise_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                            const double* lo, const double* hi, int L, int wid, int boundary,
                                            int levels, int method, double fixed_threshold, int soft, unsigned flags,
                                            double* y, double* thresholds_out) {
  VW_TRY(check_common(c, x, y, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx < N");
  if (method < kThrUniversal || method > kThrFixed) return fail(VW_ERR_ARG, "Unknown threshold selection method");
  if (levels < 0) return fail(VW_ERR_LEVEL, "Invalid number of decomposition levels: %d", levels);
  if (levels > 0) {
    // calculateThreshold (:415-424): FIXED needs an explicit threshold (denoiseFixed is single-level)
    if (method == kThrFixed) return fail(VW_ERR_ARG, "Fixed threshold method requires explicit threshold value");
    VW_TRY(check_levels(N, L, levels, flags));
    if (vw_upsampled_length(L, levels) > N && boundary != VW_PERIODIC)
      return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  }
  if (method == kThrSure && N > kSureMaxN)
    return fail(VW_ERR_UNSUPPORTED, "SURE threshold on device supports N <= %d (got %lld)", kSureMaxN, (long long)N);
  const int J = levels > 0 ? levels : 1;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging s(c);
    double *dx, *dy, *dt = nullptr;
    VW_TRY(s.in(x, (size_t)B * ldx, &dx));
    VW_TRY(s.in<double>(nullptr, (size_t)B * N, &dy));
    if (thresholds_out) VW_TRY(s.in<double>(nullptr, (size_t)J * B, &dt));
    VW_TRY(wavelet_denoise_device(c, dx, B, N, ldx, lo, hi, L, wid, boundary, levels, method, fixed_threshold, soft,
                                  flags & ~VW_FLAG_HOST_MEMORY, dy, dt));
    VW_TRY(s.out(y, dy, (size_t)B * N));
    if (thresholds_out) VW_TRY(s.out(thresholds_out, dt, (size_t)J * B));
    VW_HIP(hipStreamSynchronize(c->stream));
    return ok();
  }
  VW_TRY(wavelet_denoise_device(c, x, B, N, ldx, lo, hi, L, wid, boundary, levels, method, fixed_threshold, soft, flags,
                                y, thresholds_out));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Statistics of MODWTStreamingDenoiser (core/modwt/streaming/MODWTStreamingDenoiser.java:133-272):
// MathUtils.median / medianAbsoluteDeviation / standardDeviation on device rows, and the noise-window
// ring update.  Device pointers only (the window lives on the device between blocks).
extern "C" vw_status vw_median_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, const double* center,
                                   unsigned flags, double* median_out) {
  if (!c || !x || !median_out) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "Array cannot be null or empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "row too long");
  if (flags & VW_FLAG_HOST_MEMORY) return fail(VW_ERR_UNSUPPORTED, "device pointers only");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  hipError_t e;
  if (center && N > kSigmaRegN) {
    // rows beyond the register-keyed centered path: deviations |x - center| into the workspace, then
    // the uncentered selection (any N) on them -- the same keys, the same exact order statistic
    if (B > 65535) return fail(VW_ERR_UNSUPPORTED, "centered median of more than 65535 long rows");
    const size_t need = (size_t)B * (size_t)N * sizeof(double);
    if (need > c->med_bytes) {
      if (c->capturing)
        return fail(VW_ERR_STATE, "median scratch growth during capture: run the call once before capturing it");
      if (c->med) {
        // the scratch may have been used on streams the context was bound to earlier, and graphs that
        // recorded a centred median hold its address: drain the device and make those graphs stale
        // (vw_graph_launch then refuses them with VW_ERR_STATE), as ensure_ws does for the workspace
        hipDeviceSynchronize();
        ++c->ws_gen;
        hipFree(c->med);
        c->med = nullptr;
        c->med_bytes = 0;
      }
      VW_HIP(hipMalloc(&c->med, need));
      c->med_bytes = need;
    }
    double* dev = reinterpret_cast<double*>(c->med);
    e = launch_abs_center(x, N, B, (int)N, center, dev, c->stream);
    if (e == hipSuccess) e = launch_median(dev, N, B, (int)N, nullptr, median_out, c->stream);
  } else {
    e = launch_median(x, N, B, (int)N, center, median_out, c->stream);
  }
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

extern "C" vw_status vw_stddev_f64(vw_ctx* c, const double* x, int64_t N, unsigned flags, double* out) {
  if (!c || !x || !out) return fail(VW_ERR_NULL, "null argument");
  if (N < 2) return fail(VW_ERR_ARG, "Need at least 2 values for standard deviation");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "too many values");
  if (flags & VW_FLAG_HOST_MEMORY) return fail(VW_ERR_UNSUPPORTED, "device pointers only");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  hipError_t e = launch_seq_std(x, (int)N, out, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// window[(start + k) % wsize] = |src[idx[k]]| for k < count; idx is a HOST array (the stratified
// sampling positions are integer bookkeeping, computed by the caller), staged to the device here.
extern "C" vw_status vw_window_gather_abs_f64(vw_ctx* c, const double* src, const int32_t* idx, int64_t count,
                                              double* window, int64_t wsize, int64_t start) {
  if (!c || !src || !window || (count > 0 && !idx)) return fail(VW_ERR_NULL, "null argument");
  if (wsize <= 0 || count < 0 || count > wsize || start < 0 || start >= wsize) return fail(VW_ERR_ARG, "bad window");
  if (count == 0) return ok();
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (c->capturing) return fail(VW_ERR_STATE, "cannot be captured");
  hipSetDevice(c->device);
  Staging s(c);
  int32_t* di = nullptr;
  VW_TRY(s.in(idx, (size_t)count, &di));
  hipError_t e = launch_gather_abs(src, di, (int)count, window, (int)wsize, (int)start, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return ok();  // Staging's destructor synchronizes before freeing the index copy
}

// ------------------------------------------------------------------------------------------------
// Streaming (BatchStreamingMODWT)
extern "C" vw_status vw_stream_create(vw_ctx* c, const double* lo, const double* hi, int L, int boundary, int levels,
                                      vw_stream** out) {
  if (!c || !lo || !hi || !out) return fail(VW_ERR_NULL, "null argument");
  if (levels < 1) return fail(VW_ERR_ARG, "levels must be >= 1");
  if (levels > kMaxLevels) return fail(VW_ERR_ARG, "levels too large");
  if (L < 1 || L > kMaxTaps) return fail(VW_ERR_ARG, "bad filter length");
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING) return fail(VW_ERR_BOUNDARY, "bad boundary");
  vw_stream* s = new vw_stream();
  s->ctx = c;
  s->lo.assign(lo, lo + L);
  s->hi.assign(hi, hi + L);
  s->L = L;
  s->boundary = boundary;
  s->levels = levels;
  s->hist.assign(levels, nullptr);
  s->snap.assign(levels, nullptr);
  s->hist_len.resize(levels);
  for (int j = 1; j <= levels; ++j) s->hist_len[j - 1] = (int)(vw_upsampled_length(L, j) - 1);
  *out = s;
  return ok();
}

static void free_hist(vw_stream* s) {
  for (auto* v : {&s->hist, &s->snap})
    for (auto& p : *v) {
      if (p) hipFree(p);
      p = nullptr;
    }
}

extern "C" vw_status vw_stream_destroy(vw_stream* s) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  free_hist(s);
  delete s;
  return ok();
}

extern "C" int64_t vw_stream_batch(vw_stream* s) { return s ? s->last_batch : -1; }

extern "C" int64_t vw_stream_history_length(vw_stream* s, int level) {
  if (!s || level < 1 || level > s->levels) return -1;
  return s->hist_len[level - 1];
}

static vw_status stream_run(vw_stream* s, const double* blk, int64_t B, int64_t n, unsigned flags, double* details,
                            double* approx, bool flush) {
  vw_ctx* c = s->ctx;
  if (s->boundary == VW_PERIODIC) {
    // processMultiLevel PERIODIC -> BatchMODWT.multiLevelAoS (no cap), BatchStreamingMODWT.java:115-116
    FwdCall<double> fk;
    fk.x = blk; fk.B = B; fk.N = n; fk.ldx = n; fk.lo = s->lo.data(); fk.hi = s->hi.data(); fk.L = s->L;
    fk.boundary = s->boundary; fk.J = s->levels; fk.flags = flags & ~VW_FLAG_SYNC; fk.details = details;
    fk.approx = approx;
    return forward_impl<double>(c, fk);
  }
  const bool first = !s->hist_init;
  const int mode = first ? -1 : kHaloHistory;
  FwdCall<double> fk;
  fk.x = blk; fk.B = B; fk.N = n; fk.ldx = n; fk.lo = s->lo.data(); fk.hi = s->hi.data(); fk.L = s->L;
  fk.boundary = s->boundary; fk.J = s->levels; fk.flags = flags & ~VW_FLAG_SYNC; fk.details = details;
  fk.approx = approx; fk.mode_override = mode; fk.hist = s->hist.data(); fk.hist_update = !flush;
  fk.hist_snap = s->snap[0] ? s->snap.data() : nullptr; fk.hist_first = first;
  return forward_impl<double>(c, fk);
}

extern "C" vw_status vw_stream_process_f64(vw_stream* s, const double* block, int64_t B, int64_t n, unsigned flags,
                                           double* details, double* approx) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  vw_ctx* c = s->ctx;
  VW_TRY(check_common(c, block, details, s->lo.data(), s->hi.data(), B, n, s->L, s->boundary));
  if (!approx) return fail(VW_ERR_NULL, "approx is null");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (s->boundary != VW_PERIODIC) {
    // ensureHistoryCapacity  BatchStreamingMODWT.java:310-324: batch change re-initialises history
    if (s->last_batch != B) {
      free_hist(s);
      for (int j = 0; j < s->levels; ++j)
        VW_HIP(hipMalloc(&s->hist[j], std::max<size_t>((size_t)B * s->hist_len[j] * sizeof(double), 16)));
      s->hist_init = false;
      s->last_batch = B;
    }
    if ((flags & VW_FLAG_REF_NONFINITE) && !s->snap[0])
      for (int j = 0; j < s->levels; ++j)
        VW_HIP(hipMalloc(&s->snap[j], std::max<size_t>((size_t)B * s->hist_len[j] * sizeof(double), 16)));
  }
  vw_status st;
  if (flags & VW_FLAG_HOST_MEMORY) {
    Staging sg(c);
    double *db, *dd, *da;
    VW_TRY(sg.in(block, (size_t)B * n, &db));
    VW_TRY(sg.in<double>(nullptr, (size_t)s->levels * B * n, &dd));
    VW_TRY(sg.in<double>(nullptr, (size_t)B * n, &da));
    st = stream_run(s, db, B, n, flags, dd, da, false);
    if (st != VW_OK) return st;
    VW_TRY(sg.out(details, dd, (size_t)s->levels * B * n));
    VW_TRY(sg.out(approx, da, (size_t)B * n));
    VW_HIP(hipStreamSynchronize(c->stream));
  } else {
    st = stream_run(s, block, B, n, flags, details, approx, false);
    if (st != VW_OK) return st;
    if (flags & VW_FLAG_SYNC) VW_HIP(hipStreamSynchronize(c->stream));
  }
  if (s->boundary != VW_PERIODIC) s->hist_init = true;
  return ok();
}

// flushMultiLevel  BatchStreamingMODWT.java:231-275: tail from level-1 history (ZERO: zeros;
// SYMMETRIC: hist[histLen-1-t]), run through every level's history without updating it.
extern "C" vw_status vw_stream_flush_f64(vw_stream* s, int64_t tail_len, unsigned flags, double* details,
                                         double* approx) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  vw_ctx* c = s->ctx;
  if (s->boundary == VW_PERIODIC) return fail(VW_ERR_UNSUPPORTED, "Flush is only applicable to ZERO_PADDING/SYMMETRIC");
  if (tail_len <= 0) return ok();
  if (!s->hist_init || s->last_batch <= 0) return fail(VW_ERR_STATE, "No prior blocks processed; cannot flush");
  int min_hist = s->hist_len[0];
  for (int j = 0; j < s->levels; ++j) min_hist = std::min(min_hist, s->hist_len[j]);
  if (tail_len > min_hist)
    return fail(VW_ERR_ARG, "tailLength (%lld) exceeds maximum allowed across levels (%d)", (long long)tail_len,
                min_hist);
  if (!details || !approx) return fail(VW_ERR_NULL, "null output");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (c->capturing) return fail(VW_ERR_STATE, "flush cannot be captured");
  hipSetDevice(c->device);
  const int64_t B = s->last_batch;
  const int h0 = s->hist_len[0];
  std::vector<double> hist((size_t)B * h0), tail((size_t)B * tail_len, 0.0);
  if (s->boundary == VW_SYMMETRIC) {
    VW_HIP(hipMemcpyAsync(hist.data(), s->hist[0], hist.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    VW_HIP(hipStreamSynchronize(c->stream));
    for (int64_t b = 0; b < B; ++b)
      for (int64_t t = 0; t < tail_len; ++t) tail[b * tail_len + t] = hist[b * h0 + (h0 - 1 - t)];
  }
  Staging sg(c);
  double *dt, *dd = nullptr, *da = nullptr;
  VW_TRY(sg.in(tail.data(), tail.size(), &dt));
  const bool host = flags & VW_FLAG_HOST_MEMORY;
  if (host) {
    VW_TRY(sg.in<double>(nullptr, (size_t)s->levels * B * tail_len, &dd));
    VW_TRY(sg.in<double>(nullptr, (size_t)B * tail_len, &da));
  }
  FwdCall<double> fk;
  fk.x = dt; fk.B = B; fk.N = tail_len; fk.ldx = tail_len; fk.lo = s->lo.data(); fk.hi = s->hi.data(); fk.L = s->L;
  fk.boundary = s->boundary; fk.J = s->levels; fk.flags = flags & ~VW_FLAG_SYNC; fk.details = host ? dd : details;
  fk.approx = host ? da : approx; fk.mode_override = kHaloHistory; fk.hist = s->hist.data();
  VW_TRY(forward_impl<double>(c, fk));
  if (host) {
    VW_TRY(sg.out(details, dd, (size_t)s->levels * B * tail_len));
    VW_TRY(sg.out(approx, da, (size_t)B * tail_len));
  }
  VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Device utilities
extern "C" vw_status vw_fill_uniform_f64(vw_ctx* c, double* x, int64_t count, uint64_t seed, int64_t offset) {
  if (!c || !x) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  hipError_t e = launch_fill_uniform<double>(x, count, seed, offset, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return ok();
}

extern "C" vw_status vw_fill_uniform_f32(vw_ctx* c, float* x, int64_t count, uint64_t seed, int64_t offset) {
  if (!c || !x) return fail(VW_ERR_NULL, "null argument");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  hipError_t e = launch_fill_uniform<float>(x, count, seed, offset, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return ok();
}

extern "C" vw_status vw_device_alloc(vw_ctx* c, int64_t bytes, void** out) {
  if (!c || !out) return fail(VW_ERR_NULL, "null argument");
  hipSetDevice(c->device);
  VW_HIP(hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16)));
  return ok();
}

extern "C" vw_status vw_device_free(vw_ctx* c, void* p) {
  if (!c) return fail(VW_ERR_NULL, "null argument");
  hipSetDevice(c->device);
  if (p) VW_HIP(hipFree(p));
  return ok();
}

extern "C" vw_status vw_memcpy(vw_ctx* c, void* dst, const void* src, int64_t bytes, int kind) {
  if (!c || !dst || !src) return fail(VW_ERR_NULL, "null argument");
  hipSetDevice(c->device);
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost
                                                                        : hipMemcpyDeviceToDevice;
  VW_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, k, c->stream));
  VW_HIP(hipStreamSynchronize(c->stream));
  return ok();
}
