// vw_ctx.cpp -- the state behind the C ABI (include/vectorwave_amd.h): the thread's error state, contexts and their
// streams, captured graphs, pipelines, launch timing, options, workspace growth, the staging pool of host-memory
// calls, and the device utilities.  The transforms are in vw_api_*.cpp, their executors in vw_exec.cpp.
#include "vw_host.h"

#include <cstdarg>
#include <cstdio>

using namespace vw;

// ------------------------------------------------------------------------------------------------
// Errors: the one definition of the thread-local state every unit of the host layer reports through
ErrState& vw::err_state() {
  static thread_local ErrState e;
  return e;
}

vw_status vw::fail(vw_status code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  ErrState& e = err_state();
  e.msg = buf;
  if (code != VW_ERR_NONFINITE) e.index = -1;
  return code;
}

vw_status vw::ok() {
  ErrState& e = err_state();
  e.msg.clear();
  e.index = -1;
  return VW_OK;
}

extern "C" const char* vw_last_error(void) { return err_state().msg.c_str(); }
extern "C" int64_t vw_last_error_index(void) { return err_state().index; }
extern "C" const char* vw_version(void) { return "vectorwave_amd 0.1.0 (gfx950)"; }
extern "C" void vw_set_signal_base(int64_t base) { err_state().signal_base = base; }

// Bookkeeping restated from the reference (vw_plan.cpp).
extern "C" int vw_max_levels(int64_t N, int L) { return max_levels(N, L); }
extern "C" int64_t vw_upsampled_length(int L, int level) { return upsampled_length(L, level); }

// ------------------------------------------------------------------------------------------------
// Launch timing
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

LaunchTimer::LaunchTimer(vw_ctx* ctx, const char* family) : c(ctx), on(ctx->timing) {
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

LaunchTimer::~LaunchTimer() {
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

// ------------------------------------------------------------------------------------------------
// Workspace growth
vw_status vw::grow_buffer(vw_ctx* c, void** buf, size_t* have, size_t bytes, size_t min_bytes, const char* what) {
  if (bytes <= *have) return VW_OK;
  if (c->capturing)
    return fail(VW_ERR_STATE, "%s growth during capture: run the call once before capturing it", what);
  if (*buf) {
    hipDeviceSynchronize();
    ++c->ws_gen;
    hipFree(*buf);
    *buf = nullptr;
    *have = 0;
  }
  const size_t want = std::max(bytes, min_bytes);
  VW_HIP(hipMalloc(buf, want));
  *have = want;
  return VW_OK;
}

// ------------------------------------------------------------------------------------------------
// The staged call (vw_host.h)
Staging::Staging(vw_ctx* ctx, unsigned flags) : c(ctx), fl(flags), lock(ctx->mu) { hipSetDevice(c->device); }

vw_status Staging::open() const {
  if (!c->capturing) return VW_OK;
  if (host()) return fail(VW_ERR_STATE, "host-memory calls cannot be captured (they synchronize)");
  return capture_guard(c, fl & VW_FLAG_SYNC);
}

// After the call's copies and kernels: keep only the largest block (the next call of the same
// shape allocates at most one block >= its whole need, and frees this one here), so the pool holds
// one block of about the largest call's size instead of every block it ever grew through.
Staging::~Staging() {
  if (!carved) return;
  if (!synced) hipStreamSynchronize(c->stream);
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

vw_status Staging::carve(size_t bytes, void** out) {
  carved = true;
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
  size_t total = bytes;
  for (size_t k = 0; k < used_block && k < c->stage.size(); ++k) total += c->stage[k].second;
  if (used_block < c->stage.size()) total += used_off;
  const size_t want = std::max(total, (size_t)4 << 20);
  void* p = nullptr;
  VW_HIP(hipMalloc(&p, want));
  c->stage.push_back({p, want});
  used_block = c->stage.size() - 1;
  used_off = bytes;
  *out = p;
  return VW_OK;
}

// `planes` packed device blocks of `bytes` <-> host blocks `host_stride` bytes apart
vw_status Staging::copy(void* dst, const void* src, size_t planes, size_t bytes, size_t host_stride,
                        hipMemcpyKind kind) {
  if (!bytes || !planes) return VW_OK;
  if (planes == 1) {
    VW_HIP(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
  } else {
    const bool up = kind == hipMemcpyHostToDevice;
    VW_HIP(hipMemcpy2DAsync(dst, up ? bytes : host_stride, src, up ? host_stride : bytes, bytes, planes, kind, c->stream));
  }
  return VW_OK;
}

vw_status Staging::copy_in(const void* host, size_t planes, size_t bytes, size_t host_stride, void** dev) {
  VW_TRY(carve(planes * bytes, dev));
  return copy(*dev, host, planes, bytes, host_stride, hipMemcpyHostToDevice);
}

vw_status Staging::reserve_out(void* host, size_t planes, size_t bytes, size_t host_stride, void** dev) {
  if (nouts == (int)(sizeof(outs) / sizeof(outs[0]))) return fail(VW_ERR_ARG, "too many staged outputs");
  VW_TRY(carve(planes * bytes, dev));
  outs[nouts++] = {host, *dev, planes, bytes, host_stride};
  return VW_OK;
}

vw_status Staging::finish() {
  for (int i = 0; i < nouts; ++i)
    VW_TRY(copy(outs[i].host, outs[i].dev, outs[i].planes, outs[i].bytes, outs[i].stride, hipMemcpyDeviceToHost));
  if (carved || (fl & VW_FLAG_SYNC)) {
    synced = true;
    VW_HIP(hipStreamSynchronize(c->stream));
  }
  return ok();
}

// ------------------------------------------------------------------------------------------------
// Context
static void kill_pipelines_of(vw_ctx* c);

// Frees the HIP objects of a graph (its context's device must be current).
static void release_graph(vw_graph* gr) {
  for (auto& t : gr->timed) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
  gr->timed.clear();
  if (gr->exec) hipGraphExecDestroy(gr->exec);
  if (gr->graph) hipGraphDestroy(gr->graph);
  gr->exec = nullptr;
  gr->graph = nullptr;
}

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
  if (c->icwt_dev) hipFree(c->icwt_dev);
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

// ------------------------------------------------------------------------------------------------
// Options, stream access, timing queries
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
// Device utilities
template <typename T>
static vw_status fill_uniform(vw_ctx* c, T* x, int64_t count, uint64_t seed, int64_t offset) {
  if (!c || !x) return fail(VW_ERR_NULL, "null argument");
  Staging s(c, 0);
  hipError_t e = launch_fill_uniform<T>(x, count, seed, offset, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}
extern "C" vw_status vw_fill_uniform_f64(vw_ctx* c, double* x, int64_t count, uint64_t seed, int64_t offset) {
  return fill_uniform(c, x, count, seed, offset);
}
extern "C" vw_status vw_fill_uniform_f32(vw_ctx* c, float* x, int64_t count, uint64_t seed, int64_t offset) {
  return fill_uniform(c, x, count, seed, offset);
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
