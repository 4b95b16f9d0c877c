// vw_exec.cpp -- the executors of the forward and inverse transforms.  Selection is vw_plan.cpp's: plan_forward /
// plan_inverse return which kernels run with what launch shape and layout, which buffers they read and write, and
// what must be reserved.  The code below adds the pointers and issues the launches; it decides nothing.
#include "vw_host.h"

using namespace vw;

vw_status vw::read_bad(vw_ctx* c, unsigned long long* out) {
  VW_HIP(hipMemcpyAsync(out, c->bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  VW_HIP(hipStreamSynchronize(c->stream));
  return VW_OK;
}

static vw_status report_bad(unsigned long long bad, int64_t N) {
  if (bad == ~0ull) return VW_OK;
  const bool out = (bad >> 62) & 1ull;
  const unsigned long long flat = bad & ((1ull << 62) - 1);
  const long long index = (long long)(flat % (unsigned long long)N);
  err_state().index = index;
  return fail(VW_ERR_NONFINITE, "%s contains non-finite value at index %lld (signal %lld)",
              out ? "coefficients" : "signal", index,
              (long long)(flat / (unsigned long long)N) + (long long)err_state().signal_base);
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
bool vw::pair_forward_shape(const FwdPlan<double>& p) {
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
void vw::pair_args(const FwdArgs<double>& f, const InvCall<double>& k, const InvPlan<double>& p, PairArgs<double>* a) {
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
vw_status vw::forward_impl(vw_ctx* c, FwdCall<T> k) {
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
vw_status vw::inverse_impl(vw_ctx* c, InvCall<T> k) {
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
  return VW_OK;
}

template vw_status vw::forward_impl<double>(vw_ctx*, FwdCall<double>);
template vw_status vw::forward_impl<float>(vw_ctx*, FwdCall<float>);
template vw_status vw::inverse_impl<double>(vw_ctx*, InvCall<double>);
template vw_status vw::inverse_impl<float>(vw_ctx*, InvCall<float>);
