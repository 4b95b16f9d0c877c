// TEST INFRASTRUCTURE: plan_cwt (vectorwave_amd/csrc/vw_plan.cpp, linked without anything from HIP) over tap counts
// {1, 2, 17, 64, 257, 1201, 8193, 8194, 40000}, row lengths {1, 16, 100, 4096, 65536, 2^20}, both element types, real
// and complex tables, every extension and two batch sizes -- each tap count alone and all placeable ones as one call
// -- checked against k_cwt's launch contract (vw_cwt.hip) and what vw_plan.h promises.  Prints nothing when all is
// well; otherwise one line per finding.  tests/test_plan_cwt_cpu.py fails on any output.
#include "../../vectorwave_amd/csrc/vw_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace vw;

static int g_findings = 0;
static long long g_placed = 0, g_refused = 0, g_multi_launch = 0;

static const int kKs[] = {1, 2, 17, 64, 257, 1201, 8193, 8194, 40000};
static const long long kNs[] = {1, 16, 100, 4096, 65536, 1 << 20};

struct Case {
  const char* dtype;
  long long N, B;
  int S, K0, cplx, ext;
};
static void finding(const Case& c, const char* rule, long long a = 0, long long b = 0) {
  if (++g_findings > 100) return;
  printf("%s N=%lld B=%lld S=%d K0=%d complex=%d ext=%d | %s (%lld, %lld)\n", c.dtype, c.N, c.B, c.S, c.K0, c.cplx, c.ext,
         rule, a, b);
}

static void one_case(const Case& c, int elem_bytes, const std::vector<int>& K, unsigned flags) {
  CwtCall k;
  k.B = c.B; k.N = c.N; k.S = (int)K.size(); k.taps = K.data(); k.elem_bytes = elem_bytes; k.cplx = c.cplx != 0;
  k.ext = c.ext; k.flags = flags;
  CwtPlan p;
  plan_cwt(k, &p);
  const int kmax = *std::max_element(K.begin(), K.end());
  if (p.error != VW_OK) {
    ++g_refused;
    if (p.error != VW_ERR_UNSUPPORTED) finding(c, "refusal is not VW_ERR_UNSUPPORTED", p.error);
    if (kmax <= kCwtMaxTaps) finding(c, "refused although every scale is within kCwtMaxTaps", kmax);
    if (!std::strstr(p.msg, "scale ")) finding(c, "the refusal does not name the scale");
    if (!p.order.empty() || !p.launches.empty()) finding(c, "a refused plan carries launches");
    return;
  }
  ++g_placed;
  if (kmax > kCwtMaxTaps) return finding(c, "placed a scale beyond kCwtMaxTaps", kmax);
  if ((bool)(flags & VW_FLAG_FMA) != p.fma || p.cplx != (c.cplx != 0)) finding(c, "FMA / complex not carried");
  // launch shape: whole waves, the kernel's bound, NV chunks of 32 bytes
  const int nv = kCwtChunkBytes / elem_bytes;
  if (p.nv != nv) finding(c, "NV is not 32 bytes of elements", p.nv);
  if (p.threads < 64 || p.threads % 64 != 0) finding(c, "threads are not whole waves", p.threads);
  if (p.threads > kCwtThreads || p.threads > kMaxThreads) finding(c, "threads beyond the kernel's bound", p.threads);
  if (p.tile != p.threads * p.nv) finding(c, "tile is not threads x NV", p.tile);
  // tiles cover [0, N) exactly once: tile t owns [t * tile, (t + 1) * tile) cut at N
  if ((long long)p.ntiles * p.tile < c.N) finding(c, "tiles short of the row", p.ntiles, p.tile);
  if ((long long)(p.ntiles - 1) * p.tile >= c.N) finding(c, "an empty last tile", p.ntiles, p.tile);
  if (p.threads > 64 && (long long)(p.threads - 64) * p.nv >= c.N && p.ntiles == 1) finding(c, "a whole wave without outputs", p.threads);
  // the order: a permutation of the scales, heaviest first, ties in the caller's order
  if (p.order.size() != K.size()) return finding(c, "order is not one entry per scale", (long long)p.order.size());
  std::vector<int> seen(K.size(), 0);
  for (size_t i = 0; i < p.order.size(); ++i) {
    const CwtScalePlan& s = p.order[i];
    if (s.scale < 0 || s.scale >= (int)K.size() || seen[s.scale]++) { finding(c, "order is not a permutation", s.scale); continue; }
    if (s.taps != K[s.scale]) finding(c, "tap count not carried", s.scale, s.taps);
    if (i && (p.order[i - 1].taps < s.taps || (p.order[i - 1].taps == s.taps && p.order[i - 1].scale > s.scale)))
      finding(c, "order is not heaviest first / stable", (long long)i);
    if (s.tile != p.tile || s.nv != p.nv || s.threads != p.threads) finding(c, "a scale's shape differs from the call's", s.scale);
    if (s.chunks != cwt_chunks(p.threads, s.taps, p.nv)) finding(c, "chunks differ from the kernel's rule", s.chunks);
    if (s.lds != s.chunks * kCwtChunkBytes) finding(c, "LDS is not chunks x 32 bytes", s.lds);
    if (s.lds > kLdsBytes) finding(c, "LDS beyond 160 KiB", s.lds);
    // the staged span [0, chunks * NV) covers every element every computed output reads: output j in [0, tile) reads
    // j + k, k in [0, K); and every chunk a thread loads: tid + k0 / NV + 1 with k0 <= K - 1
    const long long span = (long long)s.chunks * p.nv;
    if (span < (long long)p.tile + s.taps - 1) finding(c, "staged span short of the outputs' reach", span, s.taps);
    if (s.chunks <= p.threads - 1 + (s.taps - 1) / p.nv + 1) finding(c, "staged chunks short of the window loads", s.chunks, s.taps);
  }
  // the launches: a partition of the order into runs of one LDS class, LDS of the heaviest, a grid within bounds
  int next = 0;
  for (const CwtLaunch& l : p.launches) {
    if (l.first != next || l.count < 1) { finding(c, "launches do not partition the order", l.first, l.count); break; }
    next += l.count;
    if (next > (int)p.order.size()) { finding(c, "launches run past the order", next); break; }
    for (int i = l.first; i < l.first + l.count; ++i) {
      if (p.order[i].lds > l.lds) finding(c, "a launch's LDS is short of one of its scales", l.lds, p.order[i].lds);
      if (l.lds > 16 * 1024 && 2 * p.order[i].lds <= l.lds)
        finding(c, "a scale shares a launch with one needing more than twice its LDS", l.lds, p.order[i].lds);
    }
    if (l.lds > kLdsBytes) finding(c, "a launch's LDS beyond 160 KiB", l.lds);
    const long long work = (long long)l.count * p.ntiles * c.B;
    if (l.grid < 1 || l.grid > kCwtMaxGrid || l.grid > work) finding(c, "grid outside 1..min(work, kCwtMaxGrid)", l.grid, work);
    if (work <= kCwtMaxGrid && l.grid != work) finding(c, "grid short of the work where it fits", l.grid, work);
  }
  if (next != (int)p.order.size()) finding(c, "launches do not cover the order", next);
  if (p.launches.size() > 1) ++g_multi_launch;
}

static void walk(const char* dtype, int elem_bytes) {
  for (long long N : kNs)
    for (long long B : {1LL, 300LL})
      for (int cplx = 0; cplx < 2; ++cplx)
        for (int ext = kCwtZero; ext <= kCwtWrapZero; ++ext) {
          if (cplx && ext == kCwtWrapZero) continue;  // the FFT form is real
          for (unsigned flags : {0u, (unsigned)VW_FLAG_FMA}) {
            for (int K : kKs) one_case(Case{dtype, N, B, 1, K, cplx, ext}, elem_bytes, std::vector<int>{K}, flags);
            // all of them in one call, in an order that is neither ascending nor descending; then without the one
            // that cannot be placed
            std::vector<int> all = {257, 1, 8193, 17, 40000, 64, 2, 8194, 1201, 17};
            one_case(Case{dtype, N, B, (int)all.size(), all[0], cplx, ext}, elem_bytes, all, flags);
            all.erase(all.begin() + 4);
            one_case(Case{dtype, N, B, (int)all.size(), all[0], cplx, ext}, elem_bytes, all, flags);
          }
        }
}

// K = 8193 (Morlet at scale 1024) is placed, K = 40000 refused, in both element types
static void outcomes() {
  for (int elem_bytes : {8, 4}) {
    const Case c{elem_bytes == 8 ? "f64" : "f32", 1000, 1, 1, 8193, 1, kCwtReflect};
    int K = 8193;
    CwtCall k;
    k.B = 1; k.N = 1000; k.S = 1; k.taps = &K; k.elem_bytes = elem_bytes; k.cplx = true; k.ext = kCwtReflect;
    CwtPlan p;
    plan_cwt(k, &p);
    if (p.error != VW_OK || p.launches.size() != 1) finding(c, "K = 8193 is not placed", p.error);
    K = 40000;
    CwtPlan q;
    plan_cwt(k, &q);
    if (q.error != VW_ERR_UNSUPPORTED) finding(c, "K = 40000 is not refused", q.error);
  }
}

// Morlet, 32 log-spaced scales on [1, 128], 256 x 4096, fp64, REFLECT (tools/cwtbench.py): the plan, exactly.
static void pin() {
  // K_s = 2 (max(16, ceil(8 s)) / 2) + 1 for s = exp(i ln(128) / 31)
  const std::vector<int> K = {17, 17, 17, 17, 17, 19, 21, 25, 29, 33, 39, 45, 53, 63, 73, 85,
                              99, 115, 135, 157, 185, 215, 251, 293, 343, 401, 469, 549, 641, 749, 877, 1025};
  const Case c{"f64", 4096, 256, 32, 17, 1, kCwtReflect};
  CwtCall k;
  k.B = 256; k.N = 4096; k.S = 32; k.taps = K.data(); k.elem_bytes = 8; k.cplx = true; k.ext = kCwtReflect; k.flags = 0;
  CwtPlan p;
  plan_cwt(k, &p);
  if (p.error != VW_OK || p.fma || !p.cplx) return finding(c, "pinned flags", p.error);
  // 4096 outputs in chunks of 4 = 1024 threads wanted, 256 per workgroup: 4 tiles of 1024
  if (p.threads != 256 || p.nv != 4 || p.tile != 1024 || p.ntiles != 4) finding(c, "pinned launch shape", p.threads, p.tile);
  if (p.order.size() != 32) return finding(c, "pinned order size");
  // heaviest first: scales 31 .. 5 strictly descending, then the five K = 17 scales in the caller's order
  for (int i = 0; i < 32; ++i) {
    const int want = i < 27 ? 31 - i : i - 27;
    const CwtScalePlan& s = p.order[i];
    const int chunks = (256 + K[want] / 4 + 1) | 1;
    if (s.scale != want || s.taps != K[want] || s.chunks != chunks || s.lds != chunks * 32 || s.tile != 1024 || s.nv != 4 ||
        s.threads != 256)
      finding(c, "pinned scale", i, s.scale);
  }
  // K = 1025: 513 chunks, 16416 bytes, 32 over the first class -> a launch of its own; the other 31 share one at
  // the K = 877 scale's 477 chunks = 15264 bytes.  One workgroup per (row, tile, scale).
  if (p.launches.size() != 2) return finding(c, "pinned launch count", (long long)p.launches.size());
  const CwtLaunch &a = p.launches[0], &b = p.launches[1];
  if (a.first != 0 || a.count != 1 || a.lds != 16416 || a.grid != 1 * 4 * 256) finding(c, "pinned first launch", a.lds, a.grid);
  if (b.first != 1 || b.count != 31 || b.lds != 15264 || b.grid != 31 * 4 * 256) finding(c, "pinned second launch", b.lds, b.grid);
}

int main() {
  walk("f64", 8);
  walk("f32", 4);
  outcomes();
  pin();
  if (!g_placed || !g_refused || !g_multi_launch) {
    printf("the walk never %s\n", !g_placed ? "placed a call" : !g_refused ? "refused a call" : "split a call into launches");
    ++g_findings;
  }
  if (g_findings) printf("%d findings\n", g_findings);
  return g_findings ? 1 : 0;
}
