// TEST INFRASTRUCTURE: plan_icwt (vectorwave_amd/csrc/vw_plan.cpp, linked without anything from HIP) over row lengths
// {1, 63, 64, 127, 128, 200, 1024, 1025, 4096, 16384}, both element types, table lengths 1 .. 16384 (each alone, and
// mixed calls), two batch sizes, with and without FMA -- checked against k_icwt's launch contract (vw_icwt.hip) and
// what vw_plan.h promises.  Prints nothing when all is well; otherwise one line per finding.
// tests/test_plan_icwt_cpu.py fails on any output.
#include "../../vectorwave_amd/csrc/vw_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace vw;

static int g_findings = 0;
static long long g_placed = 0, g_refused = 0, g_strided = 0;

static const long long kNs[] = {1, 63, 64, 127, 128, 200, 1024, 1025, 4096, 16384};
static const int kKs[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 77, 256, 1023, 1024, 4096, 8193, 16383, 16384, 16385, 40000};

struct Case {
  const char* dtype;
  long long N, B;
  int nsc, K0;
};
static void finding(const Case& c, const char* rule, long long a = 0, long long b = 0) {
  if (++g_findings > 100) return;
  printf("%s N=%lld B=%lld nsc=%d K0=%d | %s (%lld, %lld)\n", c.dtype, c.N, c.B, c.nsc, c.K0, rule, a, b);
}

static void one_case(const Case& c, int elem_bytes, const std::vector<int>& K, unsigned flags) {
  IcwtCall k;
  k.B = c.B; k.N = c.N; k.nsc = (int)K.size(); k.taps = K.data(); k.elem_bytes = elem_bytes; k.flags = flags;
  IcwtPlan p;
  plan_icwt(k, &p);
  const int kmax = *std::max_element(K.begin(), K.end());
  if (p.error != VW_OK) {
    ++g_refused;
    if (p.error != VW_ERR_UNSUPPORTED) finding(c, "refusal is not VW_ERR_UNSUPPORTED", p.error);
    if (kmax <= kCwtMaxTaps) finding(c, "refused although every table is within kCwtMaxTaps", kmax);
    char want[32];
    const int first = (int)(std::find_if(K.begin(), K.end(), [](int v) { return v > kCwtMaxTaps; }) - K.begin());
    snprintf(want, sizeof(want), "scale %d ", first);
    if (!std::strstr(p.msg, want)) finding(c, "the refusal does not name the descriptor", first);
    return;
  }
  ++g_placed;
  if (kmax > kCwtMaxTaps) return finding(c, "placed a table beyond kCwtMaxTaps", kmax);
  if ((bool)(flags & VW_FLAG_FMA) != p.fma) finding(c, "FMA not carried");
  // launch shape: whole waves, the kernel's bound, NV chunks of 32 bytes
  const int nv = kCwtChunkBytes / elem_bytes;
  if (p.nv != nv) finding(c, "NV is not 32 bytes of elements", p.nv);
  if (p.threads < 64 || p.threads % 64 != 0) finding(c, "threads are not whole waves", p.threads);
  if (p.threads > kCwtThreads || p.threads > kMaxThreads) finding(c, "threads beyond the kernel's bound", p.threads);
  if (p.tile != p.threads * p.nv) finding(c, "tile is not threads x NV", p.tile);
  // every output covered exactly once: tile t owns [t * tile, (t + 1) * tile) cut at N, thread i of it NV outputs
  if ((long long)p.ntiles * p.tile < c.N) finding(c, "tiles short of the row", p.ntiles, p.tile);
  if ((long long)(p.ntiles - 1) * p.tile >= c.N) finding(c, "an empty last tile", p.ntiles, p.tile);
  if (p.threads > 64 && (long long)(p.threads - 64) * p.nv >= c.N && p.ntiles == 1) finding(c, "a whole wave without outputs", p.threads);
  std::vector<int> hits((size_t)c.N, 0);
  for (int t = 0; t < p.ntiles; ++t)
    for (int i = 0; i < p.threads; ++i)
      for (int v = 0; v < p.nv; ++v) {
        const long long tau = (long long)t * p.tile + (long long)i * p.nv + v;
        if (tau < c.N) ++hits[(size_t)tau];
      }
  for (long long tau = 0; tau < c.N; ++tau)
    if (hits[(size_t)tau] != 1) { finding(c, "an output not covered exactly once", tau, hits[(size_t)tau]); break; }
  // LDS: the longest table's chunks by the kernel's rule; every descriptor's own chunks fit in it and hold its window
  if (p.max_taps != kmax) finding(c, "max_taps is not the longest table", p.max_taps, kmax);
  if (p.chunks != cwt_chunks(p.threads, kmax, p.nv)) finding(c, "chunks differ from the kernel's rule", p.chunks);
  if (p.lds != p.chunks * kCwtChunkBytes) finding(c, "LDS is not chunks x 32 bytes", p.lds);
  if (p.lds > kLdsBytes) finding(c, "LDS beyond the device limit", p.lds);
  for (int Kj : K) {
    const int chunks = cwt_chunks(p.threads, Kj, p.nv);
    if (chunks > p.chunks) finding(c, "a descriptor's chunks beyond the launch's LDS", chunks, p.chunks);
    if ((long long)chunks * p.nv < (long long)p.tile + Kj - 1) finding(c, "staged span short of the outputs' reach", chunks, Kj);
    if (chunks <= p.threads - 1 + (Kj - 1) / p.nv + 1) finding(c, "staged chunks short of the window loads", chunks, Kj);
  }
  // the grid: one workgroup per (row, tile) where that fits, else the cap and the kernel's stride loop
  const long long work = (long long)p.ntiles * c.B;
  if (p.grid < 1 || p.grid > kCwtMaxGrid || p.grid > work) finding(c, "grid outside 1..min(work, kCwtMaxGrid)", p.grid, work);
  if (work <= kCwtMaxGrid && p.grid != work) finding(c, "grid short of the work where it fits", p.grid, work);
  if (work > kCwtMaxGrid) {
    ++g_strided;
    if (p.grid != kCwtMaxGrid) finding(c, "grid is not the cap where the work exceeds it", p.grid, work);
  }
}

static void walk(const char* dtype, int elem_bytes) {
  for (long long N : kNs)
    for (long long B : {1LL, 300LL, 5000000LL})
      for (unsigned flags : {0u, (unsigned)VW_FLAG_FMA}) {
        if (B > 300 && N > 64) continue;  // the stride loop's case needs no long coverage walk
        for (int K : kKs) one_case(Case{dtype, N, B, 1, K}, elem_bytes, std::vector<int>{K}, flags);
        std::vector<int> all = {77, 1, 8193, 17, 40000, 4096, 2, 16384, 1023, 17};
        one_case(Case{dtype, N, B, (int)all.size(), all[0]}, elem_bytes, all, flags);
        all.erase(all.begin() + 4);
        one_case(Case{dtype, N, B, (int)all.size(), all[0]}, elem_bytes, all, flags);
      }
  // every table length 1 .. 16384 at one row length
  for (int K = 1; K <= kCwtMaxTaps; ++K) one_case(Case{dtype, 1025, 3, 1, K}, elem_bytes, std::vector<int>{K}, 0u);
}

// Morlet, 32 log-spaced scales on [1, 128], 256 x 4096 (M = 4096), fp64 and fp32 (tools/icwtbench.py): the plan, exactly.
static void pin() {
  // the tables cut at their outermost non-zero entries, the upper six capped at M
  const std::vector<int> K = {77, 91, 105, 123, 145, 169, 197, 231, 271, 315, 369, 431, 505, 589, 689, 807,
                              943, 1103, 1287, 1505, 1761, 2059, 2409, 2815, 3293, 3851, 4096, 4096, 4096, 4096, 4096, 4096};
  IcwtCall k;
  k.B = 256; k.N = 4096; k.nsc = 32; k.taps = K.data(); k.elem_bytes = 8; k.flags = 0;
  IcwtPlan p;
  plan_icwt(k, &p);
  const Case c{"f64", 4096, 256, 32, 77};
  // 4096 outputs in chunks of 4: 256 threads per workgroup, 4 tiles of 1024; K = 4096: (256 + 1024 + 1) | 1 = 1281 chunks
  if (p.error != VW_OK || p.fma) finding(c, "pinned flags", p.error);
  if (p.threads != 256 || p.nv != 4 || p.tile != 1024 || p.ntiles != 4) finding(c, "pinned launch shape", p.threads, p.tile);
  if (p.max_taps != 4096 || p.chunks != 1281 || p.lds != 40992) finding(c, "pinned LDS", p.chunks, p.lds);
  if (p.grid != 4 * 256) finding(c, "pinned grid", p.grid);
  k.elem_bytes = 4; k.flags = VW_FLAG_FMA;
  IcwtPlan q;
  plan_icwt(k, &q);
  const Case d{"f32", 4096, 256, 32, 77};
  // chunks of 8: 512 threads wanted, 256 per workgroup, 2 tiles of 2048; (256 + 512 + 1) | 1 = 769 chunks
  if (q.error != VW_OK || !q.fma) finding(d, "pinned flags", q.error);
  if (q.threads != 256 || q.nv != 8 || q.tile != 2048 || q.ntiles != 2) finding(d, "pinned launch shape", q.threads, q.tile);
  if (q.max_taps != 4096 || q.chunks != 769 || q.lds != 24608) finding(d, "pinned LDS", q.chunks, q.lds);
  if (q.grid != 2 * 256) finding(d, "pinned grid", q.grid);
  // the longest table the planner places, fp64: (256 + 4096 + 1) | 1 = 4353 chunks = 139296 bytes
  const int kmax = kCwtMaxTaps;
  IcwtCall m;
  m.B = 1; m.N = 16384; m.nsc = 1; m.taps = &kmax; m.elem_bytes = 8;
  IcwtPlan r;
  plan_icwt(m, &r);
  if (r.error != VW_OK || r.chunks != 4353 || r.lds != 139296 || r.lds > kLdsBytes) finding(c, "pinned largest LDS", r.chunks, r.lds);
}

int main() {
  walk("f64", 8);
  walk("f32", 4);
  pin();
  if (!g_placed || !g_refused || !g_strided) {
    printf("the walk never %s\n", !g_placed ? "placed a call" : !g_refused ? "refused a call" : "met the grid cap");
    ++g_findings;
  }
  if (g_findings) printf("%d findings\n", g_findings);
  return g_findings ? 1 : 0;
}
