// TEST INFRASTRUCTURE: the planner (vectorwave_amd/csrc/vw_plan.cpp, linked without anything from HIP) on banks
// with two filter lengths -- the 15 bior and 15 rbio length pairs, both directions, both element types, three
// boundaries, a list of N and seven tunings -- checked against what vw_plan.h promises for them.  Prints nothing
// when all is well; otherwise one line per finding.  tests/test_plan_bi_cpu.py fails on any output.
#include "../../vectorwave_amd/csrc/vw_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

using namespace vw;

static int g_findings = 0;

// (decomposition low-pass, reconstruction low-pass) lengths of BIOR1_1 .. BIOR6_8; the analysis pair is
// (dec, rec), the synthesis pair (rec, dec); RBIO swaps the sides.
static const int kBior[15][2] = {{2, 2},  {6, 2},  {10, 2}, {5, 3},  {9, 3},  {13, 3}, {17, 3}, {4, 4},
                                 {8, 4},  {12, 4}, {16, 4}, {20, 4}, {9, 7},  {12, 8}, {17, 16}};
static const long long kN[] = {64, 67, 256, 1000, 1024, 1500, 4096, 16384, 32768};

struct Case {
  const char* dir;
  const char* dtype;
  const char* tune;
  long long N;
  int Llo, Lhi, J, boundary;
  unsigned flags;
  int off = 0;  // mask of the caller pointers one element off a 16-byte boundary: forward 1 x, 2 details, 4 approx;
                // inverse 1 details, 2 approx, 4 y
};
static void finding(const Case& c, const char* rule, long long a = 0, long long b = 0) {
  if (++g_findings > 100) return;
  printf("%s %s N=%lld Llo=%d Lhi=%d J=%d boundary=%d flags=0x%x off=%d [%s] | %s (%lld, %lld)\n", c.dir, c.dtype, c.N, c.Llo,
         c.Lhi, c.J, c.boundary, c.flags, c.off, c.tune, rule, a, b);
}

// the tap count a bank of two lengths runs: the longer filter's, or one more where only that count is listed
static int bank_taps(const Tuning& tu, int Llo, int Lhi) {
  const int L = std::max(Llo, Lhi);
  return (Llo != Lhi && tu.bi_listed && !has_unrolled_taps(L) && has_unrolled_taps(L + 1)) ? L + 1 : L;
}

static long long tau(int L, int j) { return (long long)(L - 1) * (1LL << (j - 1)) / 2; }  // computeTauJ :795-806

// what every plan must satisfy, whichever path it takes
template <typename T, typename Args>
static void check_launch(const Case& c, const Plan<T, Args>& p) {
  if (p.fused) {
    if (p.kernel < kFwdFused || p.kernel > kInvMfma) finding(c, "no named fused kernel", p.kernel);
    if (p.lds > kLdsBytes) finding(c, "fused LDS beyond 160 KiB", p.lds);
    if (p.threads < 1 || p.threads > kMaxThreads) finding(c, "threads beyond 1024", p.threads);
  } else {
    if (p.steps.empty()) finding(c, "no steps");
    for (const auto& s : p.steps) {
      if (s.kind < kStepDeep || s.kind > kStepTile) finding(c, "no named step kernel", s.kind);
      if (s.lds > kLdsBytes) finding(c, "step LDS beyond 160 KiB", s.lds);
      const int taps = s.kind == kStepDeep ? s.deep.taps : s.kind == kStepMulti ? s.multi.taps : s.lvl.taps;
      if (taps != p.args.taps) finding(c, "a step runs another tap count than the plan's", taps, p.args.taps);
      if (s.kind != kStepTile && s.kind != kStepMulti && !has_unrolled_taps(taps))
        finding(c, "a listed-taps-only step kernel at an unlisted length", s.kind, taps);
    }
  }
}

template <typename T, typename Args>
static bool same_plan(const Plan<T, Args>& a, const Plan<T, Args>& b, int J) {
  if (a.error != b.error || a.fused != b.fused || a.kernel != b.kernel || a.threads != b.threads || a.nv != b.nv ||
      a.lds != b.lds || a.args.taps != b.args.taps || a.ref_nf != b.ref_nf || a.nf_probed != b.nf_probed ||
      a.res.ws_bytes != b.res.ws_bytes || a.steps.size() != b.steps.size())
    return false;
  if (memcmp(a.args.lv, b.args.lv, sizeof(LevelDesc) * J) != 0) return false;
  for (size_t k = 0; k < a.steps.size(); ++k)
    if (a.steps[k].kind != b.steps[k].kind || a.steps[k].lds != b.steps[k].lds || a.steps[k].jlo != b.steps[k].jlo ||
        a.steps[k].jhi != b.steps[k].jhi)
      return false;
  return true;
}

template <typename T>
static void forward_case(const Tuning& tu, Case c) {
  c.dir = "fwd";
  alignas(16) static T dummy[4];
  FwdCall<T> k;
  k.x = dummy + (c.off & 1); k.details = dummy + ((c.off >> 1) & 1); k.approx = dummy + ((c.off >> 2) & 1);  // never dereferenced by the planner
  k.B = 3; k.N = c.N; k.ldx = c.N; k.L = c.Llo; k.Lhi = c.Lhi; k.boundary = c.boundary; k.J = c.J; k.flags = c.flags;
  FwdPlan<T> p;
  plan_forward(tu, k, &p);
  int Lmax = bank_taps(tu, c.Llo, c.Lhi);
  // mixed FFT-switch levels, restated: behind the low-pass gate exactly one filter beyond N / 8
  int mixed = 0;
  const bool pow2 = (c.N & (c.N - 1)) == 0;
  for (int j = 1; j <= c.J && !mixed; ++j) {
    const long long llo = upsampled_length(c.Llo, j), lhi = upsampled_length(c.Lhi, j);
    if ((c.flags & VW_FLAG_FFT_SWITCH) && c.boundary == VW_PERIODIC && c.N >= 1024 && !pow2 && llo <= c.N / 2 &&
        ((double)llo > c.N / 8.0) != ((double)lhi > c.N / 8.0))
      mixed = j;
  }
  if (mixed) {
    char want[32];
    snprintf(want, sizeof(want), "level %d", mixed);
    if (p.error != VW_ERR_UNSUPPORTED || !strstr(p.msg, want)) finding(c, "mixed level not refused by name", p.error, mixed);
    return;
  }
  if (p.error != VW_OK) return finding(c, "unexpected plan error", p.error);
  // the fused kernels read x and write the details and the approximation at row + w * V: no vector form off alignment
  if (c.off && p.fused && (p.args.vec_io || p.args.unrolled)) finding(c, "vector I/O on a misaligned pointer", c.off);
  // the two-length route (VW_BI bit 0): the non-persistent fused forward at each filter's own count, halos for the longer
  const bool bi_route = p.args.taps_hi != p.args.taps;
  if (bi_route) {
    if (!(tu.bi & 1) || !p.fused || p.kernel != kFwdFused || p.nv == 2)
      finding(c, "two-length route outside its kernel", p.kernel, p.nv);
    if (p.args.taps != c.Llo || p.args.taps_hi != c.Lhi) finding(c, "two-length route tap counts", p.args.taps, p.args.taps_hi);
    if (p.args.unrolled && !has_unrolled_pair(c.Llo, c.Lhi)) finding(c, "unrolled two-length kernel at an unlisted pair");
    if (!(tu.bi & 4) && !p.args.unrolled && !c.off) finding(c, "runtime-L two-length forward without VW_BI bit 2");
    Lmax = std::max(c.Llo, c.Lhi);
  } else {
    if ((tu.bi & 1) && (tu.bi & 4) && c.Llo != c.Lhi && p.fused) finding(c, "padded route where the two-length forward fits", p.kernel);
    if (p.args.taps != Lmax) finding(c, "forward tap count is not the bank's", p.args.taps, Lmax);
  }
  check_launch(c, p);
  for (int j = 1; j <= c.J; ++j) {
    const LevelDesc& d = p.args.lv[j - 1];
    // the forward reads x[t - i*s] only, in every halo mode (FFT-pad included): all of its reach is to the left
    if (d.hl < (long long)(Lmax - 1) * d.s) finding(c, "left halo short of the longer filter's reach", j, d.hl);
    if (d.hr != 0) finding(c, "forward level with a right halo", j, d.hr);
    if (d.mode == kHaloFftPad && !((double)upsampled_length(c.Llo, j) > c.N / 8.0 && (double)upsampled_length(c.Lhi, j) > c.N / 8.0))
      finding(c, "FFT-pad level where a filter is outside the FFT region", j);
  }
  if (c.Llo == c.Lhi) {  // Lhi = L and Lhi = 0 are the equal-length call
    FwdCall<T> k0 = k;
    k0.Lhi = 0;
    FwdPlan<T> p0;
    plan_forward(tu, k0, &p0);
    if (!same_plan(p, p0, c.J)) finding(c, "Lhi = L plans differently from Lhi = 0");
  } else if (!bi_route) {  // the padded route: the plan of the equal-length call with the longer filter
    FwdCall<T> k0 = k;
    k0.L = Lmax; k0.Lhi = 0;
    FwdPlan<T> p0;
    plan_forward(tu, k0, &p0);
    bool fft_differs = false;  // the gate reads the low-pass length: only there may the two differ
    for (int j = 0; j < c.J; ++j) fft_differs = fft_differs || p.args.lv[j].mode != p0.args.lv[j].mode;
    if (!fft_differs && !same_plan(p, p0, c.J)) finding(c, "padded route plans differently from L = max(Llo, Lhi)");
  }
}

template <typename T>
static void inverse_case(const Tuning& tu, Case c, bool single) {
  c.dir = single ? "inv1" : "inv";
  alignas(16) static T dummy[4];
  InvCall<T> k;
  k.details = dummy + (c.off & 1); k.approx = dummy + ((c.off >> 1) & 1); k.y = dummy + ((c.off >> 2) & 1);
  k.B = 3; k.N = c.N; k.L = c.Llo; k.Lhi = c.Lhi; k.boundary = c.boundary; k.J = single ? 1 : c.J; k.flags = c.flags;
  k.single_level = single;
  if (single) k.detail_mask = 1u;
  InvPlan<T> p;
  plan_inverse(tu, k, &p);
  const bool pair = single || c.boundary == VW_ZERO_PADDING;
  if (pair && c.Lhi < c.Llo) {
    if (p.error != VW_ERR_UNSUPPORTED || !strstr(p.msg, "high-pass")) finding(c, "pairwise inverse with Lhi < Llo not refused", p.error);
    return;
  }
  if (p.error != VW_OK) return finding(c, "unexpected plan error", p.error);
  if (c.off && p.fused && (p.args.vec_io || p.args.unrolled || p.args.full)) finding(c, "vector I/O on a misaligned pointer", c.off);
  // the two-length route (VW_BI): the fused sequential-sum kernels, each branch at its own count, halos for the longer
  const bool bi_route = p.args.taps_hi != p.args.taps;
  if (bi_route) {
    if (!(tu.bi & 2) || pair || !p.fused || !(p.kernel == kInvSeq || p.kernel == kInvDb) || p.nv == 2 || p.args.blk)
      finding(c, "two-length route outside its kernels", p.kernel, p.nv);
    if (p.args.taps != c.Llo || p.args.taps_hi != c.Lhi) finding(c, "two-length route tap counts", p.args.taps, p.args.taps_hi);
    if (p.args.unrolled && !has_unrolled_pair(c.Llo, c.Lhi)) finding(c, "unrolled two-length kernel at an unlisted pair");
    if (!(tu.bi & 4) && !p.args.unrolled && !c.off) finding(c, "runtime-L two-length inverse without VW_BI bit 2");
  } else if ((tu.bi & 2) && (tu.bi & 4) && c.Llo != c.Lhi && !pair && p.fused && p.nv != 2 && (p.kernel == kInvSeq || p.kernel == kInvDb)) {
    finding(c, "padded route where the two-length route fits", p.kernel);
  }
  const int taps = pair ? c.Llo : bi_route ? std::max(c.Llo, c.Lhi) : bank_taps(tu, c.Llo, c.Lhi);
  if (!bi_route && p.args.taps != taps) finding(c, "inverse tap count", p.args.taps, taps);
  if (!bi_route && p.args.taps_hi != p.args.taps) finding(c, "taps_hi differs off the two-length route");
  if (pair && !(p.fused ? p.args.pair : p.steps[0].lvl.pair)) finding(c, "pairwise sums not planned");
  check_launch(c, p);
  // the equal-length plan of the low-pass length: same orientation, the detail shift moved by tau(Lhi) - tau(Llo)
  InvCall<T> k0 = k;
  k0.Lhi = 0;
  InvPlan<T> p0;
  plan_inverse(tu, k0, &p0);
  for (int j = 1; j <= k.J; ++j) {
    const LevelDesc& d = p.args.lv[j - 1];
    const LevelDesc& e = p0.args.lv[j - 1];
    if (d.dir_a != e.dir_a || d.dir_d != e.dir_d || d.off_a != e.off_a) finding(c, "alignment not keyed on the low-pass length", j);
    const long long shift = (c.boundary == VW_SYMMETRIC && !single) ? tau(c.Lhi, j) - tau(c.Llo, j) : 0;
    if (d.off_d - e.off_d != (d.dir_d > 0 ? -shift : shift)) finding(c, "detail shift is not tau(Lhi) + dG", j, d.off_d);
    // halos cover the reach of `taps` taps of both branches over t in [0, N)
    for (int br = 0; br < 2; ++br) {
      const int dir = br ? d.dir_d : d.dir_a, off = br ? d.off_d : d.off_a;
      const long long reach = (long long)(taps - 1) * d.s;
      const long long mn = dir > 0 ? off : off - reach, mx = (c.N - 1) + (dir > 0 ? reach + off : off);
      if (d.hl < -mn) finding(c, "left halo short of a branch's reach", j, d.hl);
      if (d.hr < mx - (c.N - 1)) finding(c, "right halo short of a branch's reach", j, d.hr);
    }
  }
  if (c.Llo == c.Lhi && !same_plan(p, p0, k.J)) finding(c, "Lhi = L plans differently from Lhi = 0");
}

template <typename T>
static void walk(const char* dtype) {
  struct { const char* name; const char* key; int v; } tunings[] = {
      {"default", nullptr, 0}, {"VW_BI=0", "VW_BI", 0}, {"VW_BI=1", "VW_BI", 1}, {"VW_BI=2", "VW_BI", 2}, {"VW_BI=7", "VW_BI", 7}, {"VW_FORCE_TILED=1", "VW_FORCE_TILED", 1}, {"VW_BI_LISTED=0", "VW_BI_LISTED", 0}};
  for (const auto& ts : tunings) {
    Tuning tu;
    if (ts.key && !set_tuning(tu, ts.key, ts.v)) { printf("unknown tuning switch %s\n", ts.key); ++g_findings; }
    for (int fam = 0; fam < 2; ++fam)       // 0: bior, 1: rbio
      for (const auto& pr : kBior)
        for (int side = 0; side < 2; ++side) {  // 0: analysis pair (forward), 1: synthesis pair (inverse)
          const int dec = fam ? pr[1] : pr[0], rec = fam ? pr[0] : pr[1];
          const int Llo = side ? rec : dec, Lhi = side ? dec : rec;
          for (int boundary : {VW_PERIODIC, VW_SYMMETRIC, VW_ZERO_PADDING})
            for (long long N : kN) {
              const int J = std::min(5, max_levels(N, std::max(Llo, Lhi)));
              if (J < 1) continue;
              for (unsigned flags : {0u, (unsigned)VW_FLAG_FMA, (unsigned)(VW_FLAG_REF_NONFINITE)}) {
                for (int off : {0, 1, 2, 4, 7}) {  // aligned, every caller pointer alone one element off, all together
                  if (off && flags == VW_FLAG_REF_NONFINITE) continue;
                  Case c{"", dtype, ts.name, N, Llo, Lhi, J, boundary, flags, off};
                  if (side == 0) forward_case<T>(tu, c);
                  else { inverse_case<T>(tu, c, false); if (flags == 0) inverse_case<T>(tu, c, true); }
                }
              }
              if (side == 0 && boundary == VW_PERIODIC) {  // the core decompose's flags, up to its level cap
                const int Jc = max_levels(N, Llo);
                for (int Jf = 1; Jf <= Jc; ++Jf) {
                  if (upsampled_length(std::max(Llo, Lhi), Jf) > N) break;  // the C ABI's VW_ERR_TOO_LARGE guard
                  Case c{"", dtype, ts.name, N, Llo, Lhi, Jf, boundary, VW_FLAG_CORE_LEVELS | VW_FLAG_FFT_SWITCH};
                  forward_case<T>(tu, c);
                }
              }
            }
        }
  }
}

int main() {
  walk<double>("f64");
  walk<float>("f32");
  if (g_findings) printf("%d findings\n", g_findings);
  return g_findings ? 1 : 0;
}
