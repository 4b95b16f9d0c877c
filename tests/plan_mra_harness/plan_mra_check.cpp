// TEST INFRASTRUCTURE: plan_mra (vectorwave_amd/csrc/vw_plan.cpp, linked without anything from HIP) over filter
// lengths 1..64, both element types, the three boundaries, the nine signal lengths of tests/plan_harness and J from
// 1 to the level cap (and two levels past it, which only calls without CORE_LEVELS reach), under seven tunings, four
// flag sets and aligned / unaligned pointers -- checked against k_mra's launch contract (vw_mra.hip) and what
// vw_plan.h promises.  Prints nothing when all is well; otherwise one line per finding.
// tests/test_plan_mra_cpu.py fails on any output.
#include "../../vectorwave_amd/csrc/vw_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace vw;

static int g_findings = 0;
static long long g_fused = 0, g_loop = 0;

static const long long kNs[] = {7, 64, 512, 1000, 4096, 8192, 16384, 65536, 1 << 20};

struct Case {
  const char* dtype;
  const char* tune;
  long long N, B;
  int L, J, boundary, off;  // off: mask of the caller pointers one element off a 16-byte boundary (1 details, 2 approx, 4 y)
  unsigned flags;
};
static void finding(const Case& c, const char* rule, long long a = 0, long long b = 0) {
  if (++g_findings > 100) return;
  printf("%s N=%lld B=%lld L=%d J=%d boundary=%d flags=0x%x off=%d [%s] | %s (%lld, %lld)\n", c.dtype, c.N, c.B, c.L,
         c.J, c.boundary, c.flags, c.off, c.tune, rule, a, b);
}

template <typename T>
static void one_case(const Tuning& tu, const Case& c, bool single = false) {
  constexpr int V = 16 / (int)sizeof(T);
  alignas(16) static T dummy[8];
  InvCall<T> k;
  k.details = dummy + (c.off & 1); k.approx = dummy + ((c.off >> 1) & 1); k.y = dummy + ((c.off >> 2) & 1);  // never dereferenced by the planner
  const bool aligned = c.off == 0;
  k.B = c.B; k.N = c.N; k.L = c.L; k.boundary = c.boundary; k.J = c.J; k.flags = c.flags; k.cus = 256;
  k.single_level = single;
  MraPlan<T> p;
  plan_mra(tu, k, &p);
  const long long nvec = (c.N + V - 1) / V;
  const bool excluded = single || tu.force_tiled || tu.mra_fused == 0 ||
                        (c.flags & (VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE));
  // the class measured slower than the loop: the masked inverses would run tap-unrolled kernels (aligned full-slab
  // rows, a listed length) and k_mra has none for the length (past kMraUnrollMax); VW_MRA_FUSED=2 fuses there too
  const long long th4 = (nvec + 3) / 4, nv_want = th4 > 512 ? 8 : tu.nv;
  const long long th_want = ((nvec + nv_want - 1) / nv_want + 63) / 64 * 64;
  const bool slow = tu.mra_fused == 1 && aligned && c.N % V == 0 && (nv_want - 1) * th_want <= nvec &&
                    has_unrolled_taps(c.L) && c.L <= tu.unroll_max && c.L > kMraUnrollMax;
  if (!p.fused) {
    ++g_loop;
    // PERIODIC / ZERO_PADDING read t + i*s: no left halo, the right one (L-1)*s past the last vector.  Where two
    // such regions fit, only an exclusion keeps the call on the loop.
    if (!excluded && !slow && c.boundary != VW_SYMMETRIC) {
      const long long hr = (long long)(c.L - 1) * (1LL << (c.J - 1)) + (nvec * V - c.N);
      const long long region = (nvec * V + hr + V + V - 1) / V * V;
      if (2 * region * (long long)sizeof(T) <= kLdsBytes && (nvec + nv_want - 1) / nv_want <= kMaxThreads)
        finding(c, "loop path where two regions fit", region);
    }
    return;
  }
  ++g_fused;
  if (excluded) return finding(c, "fused under an excluded flag or option");
  if (slow) finding(c, "fused in the class measured slower than the loop");
  if ((bool)(c.flags & VW_FLAG_FMA) != p.fma) finding(c, "FMA flag not carried");
  const MraArgs<T>& a = p.args;
  if (p.nv != 4 && p.nv != 8) finding(c, "NV is neither 4 nor 8", p.nv);
  if (p.threads < 64 || p.threads % 64 != 0) finding(c, "threads are not whole waves", p.threads);
  if (p.threads > (p.nv <= 4 ? 512 : 1024)) finding(c, "threads beyond the kernel's bound", p.threads, p.nv);
  if ((long long)p.threads * p.nv < nvec) finding(c, "threads x NV short of the row", p.threads, p.nv);
  if (p.lds > kLdsBytes) finding(c, "LDS beyond 160 KiB", p.lds);
  if (p.grid < 1 || p.grid > c.B) finding(c, "grid outside 1..B", p.grid);
  if (a.N != c.N || a.B != c.B || a.J != c.J || a.taps != c.L) finding(c, "shape not carried");
  if (a.hlpad % V || a.region1 % V) finding(c, "region offsets not whole vectors", a.hlpad, a.region1);
  if ((long long)p.lds != 2LL * a.region1 * (long long)sizeof(T)) finding(c, "LDS is not two regions", p.lds, a.region1);
  const bool io = aligned && c.N % V == 0;  // k_mra reads the details and the approximation and writes y as vectors
  if ((a.vec_io != 0) != io) finding(c, "vec_io does not follow the alignment", a.vec_io);
  if (a.unrolled) {
    if (!io) finding(c, "unrolled on unaligned rows");
    if ((long long)(p.nv - 1) * p.threads > nvec) finding(c, "unrolled with a partial inner slab");
    if (!has_unrolled_taps(c.L) || c.L > kMraUnrollMax || c.L > tu.unroll_max) finding(c, "unrolled at an unlisted length");
  } else if (io && (long long)(p.nv - 1) * p.threads <= nvec && has_unrolled_taps(c.L) && c.L <= kMraUnrollMax &&
             c.L <= tu.unroll_max) {
    finding(c, "runtime-L body where the unrolled one applies");
  }
  int max_hl = 0, max_hr = 0;
  for (int j = 1; j <= c.J; ++j) {
    const LevelDesc& d = a.lv[j - 1];
    if (d.s != 1 << (j - 1)) finding(c, "level spacing", j, d.s);
    if (c.boundary != VW_SYMMETRIC && (d.dir_a != 1 || d.dir_d != 1 || d.off_a || d.off_d))
      finding(c, "orientation of a PERIODIC / ZERO_PADDING level", j);
    if (d.mode != ref_mode(c.boundary)) finding(c, "halo mode", j, d.mode);
    // halos cover the reach of L taps of both branches over every output the kernel computes: t in [0, nvec * V)
    for (int br = 0; br < 2; ++br) {
      const int dir = br ? d.dir_d : d.dir_a, off = br ? d.off_d : d.off_a;
      if (dir != 1 && dir != -1) finding(c, "branch direction", j, dir);
      const long long reach = (long long)(c.L - 1) * d.s, tmax = nvec * V - 1;
      const long long mn = dir > 0 ? off : off - reach, mx = tmax + (dir > 0 ? reach + off : off);
      if (d.hl < -mn) finding(c, "left halo short of a branch's reach", j, d.hl);
      if (d.hr < mx - (c.N - 1)) finding(c, "right halo short of a branch's reach", j, d.hr);
    }
    if (d.own && (d.hl > c.N || d.hr > c.N)) finding(c, "owner-written halo longer than the row", j);
    if (d.own && (d.vs > p.threads || (long long)d.ve < (long long)(p.nv - 1) * p.threads))
      finding(c, "owner-written halo outside the slabs that check it", j);
    max_hl = std::max(max_hl, d.hl);
    max_hr = std::max(max_hr, d.hr);
  }
  if (a.hlpad < max_hl) finding(c, "left pad short of the longest left halo", a.hlpad, max_hl);
  if ((long long)a.region1 < (long long)a.hlpad + nvec * V + max_hr) finding(c, "region short of row + halos", a.region1);
}

template <typename T>
static void walk(const char* dtype) {
  struct { const char* name; const char* key; int v; } tunings[] = {
      {"default", nullptr, 0}, {"VW_MRA_FUSED=0", "VW_MRA_FUSED", 0}, {"VW_FORCE_TILED=1", "VW_FORCE_TILED", 1},
      {"VW_NV=8", "VW_NV", 8}, {"VW_UNROLL_MAX=0", "VW_UNROLL_MAX", 0}, {"VW_LEVEL_CT=0", "VW_LEVEL_CT", 0},
      {"VW_MRA_FUSED=2", "VW_MRA_FUSED", 2}};
  for (const auto& ts : tunings) {
    Tuning tu;
    if (ts.key && !set_tuning(tu, ts.key, ts.v)) { printf("unknown tuning switch %s\n", ts.key); ++g_findings; }
    for (int L = 1; L <= kMaxTaps; ++L)
      for (int boundary : {VW_PERIODIC, VW_SYMMETRIC, VW_ZERO_PADDING})
        for (long long N : kNs) {
          const int cap = max_levels(N, L);
          for (int J = 1; J <= std::min(cap + 2, kMaxLevels); ++J)
            for (unsigned flags : {0u, (unsigned)VW_FLAG_FMA, (unsigned)VW_FLAG_VALIDATE, (unsigned)VW_FLAG_REF_NONFINITE})
              for (int off : {0, 1, 2, 4, 7}) {  // aligned, every pointer alone, all together
                const Case c{dtype, ts.name, N, (N & 1) ? 3 : 1031, L, J, boundary, off, flags};
                one_case<T>(tu, c);
                if (J == 1 && flags == 0 && off == 0) one_case<T>(tu, c, true);
              }
        }
  }
}

// db4, J = 6, 4096 x 4096, fp64, PERIODIC, 256 CUs: the headline shape's plan, exactly
static void pin() {
  alignas(16) static double dummy[4];
  InvCall<double> k;
  k.details = dummy; k.approx = dummy; k.y = dummy;
  k.B = 4096; k.N = 4096; k.L = 8; k.boundary = VW_PERIODIC; k.J = 6; k.flags = 0; k.cus = 256;
  MraPlan<double> p;
  plan_mra(Tuning(), k, &p);
  const Case c{"f64", "pin", 4096, 4096, 8, 6, VW_PERIODIC, 1, 0};
  const MraArgs<double>& a = p.args;
  // 2048 vectors / NV 4 = 512 threads; no left halo, right halo 7 * 32 = 224; region = 4096 + 224 + 2 doubles;
  // two regions = 69152 bytes -> two workgroups per CU by LDS (three by waves): grid 512
  if (!p.fused || p.fma || p.threads != 512 || p.nv != 4 || p.lds != 69152 || p.grid != 512)
    finding(c, "pinned launch shape", p.threads, p.lds);
  if (a.hlpad != 0 || a.region1 != 4322 || !a.vec_io || !a.unrolled || a.level_ct != 1 || a.taps != 8)
    finding(c, "pinned layout", a.hlpad, a.region1);
  for (int j = 1; j <= 6; ++j) {
    const LevelDesc& d = a.lv[j - 1];
    if (d.s != 1 << (j - 1) || d.hl != 0 || d.hr != 7 * d.s || d.mode != kHaloPeriodic || !d.own || d.dir_a != 1 ||
        d.dir_d != 1 || d.off_a || d.off_d || d.vs != (d.hr + 1) / 2 || d.ve != 2048)
      finding(c, "pinned level descriptor", j, d.hr);
  }
}

int main() {
  walk<double>("f64");
  walk<float>("f32");
  pin();
  if (!g_fused || !g_loop) { printf("the walk never took the %s path\n", g_fused ? "loop" : "fused"); ++g_findings; }
  if (g_findings) printf("%d findings\n", g_findings);
  return g_findings ? 1 : 0;
}
